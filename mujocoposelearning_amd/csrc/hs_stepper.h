// Stepper: one mj_step of MuJoCo 3.2.5 for one env on one half-wave, phase by phase -- mj_kinematics
// + mj_comPos, mj_collision, mj_crb, mj_comVel / mj_passive / mj_fwdActuation / mj_rne,
// mj_makeConstraint, the primal Newton solver (mj_solNewton) or PGS (mj_solPGS),
// mj_rnePostConstraint's contact part, mj_Euler (custom_env.py:121,160 call mj_step).
#pragma once
#include "hs_contacts.h"
#include "hs_dense.h"
#include "hs_lanes.h"
#include "hs_phase_clock.h"
#include "hs_scratch.h"

namespace hs {
namespace {

template <typename T, int NV, typename C>
struct Stepper {
  PhaseClock clk;
  MPtr<T> m;
  Scratch<T, C>& s;
  int sl, nb;
  bool up;        // upper half-wave (second env of the wave)
  T cd[6];        // cdof of this sub-lane's dof (registers)
  T Mr[NV];       // mass-matrix row of this sub-lane's dof
  T fsmooth;      // qfrc_smooth_i
  T fcon;         // qfrc_constraint_i
  T qacc;         // solver output qacc_i
  T qfa;          // qfrc_actuator_i (obs / kneeling reward)
  T damp;         // dof_damping_i, loaded with the constraint rows (Euler reads it)
  int niter;
  T* dbg = nullptr;   // stage-dump target (env 0 in debug mode only)

  __device__ Stepper(MPtr<T> mm, Scratch<T, C>& ss, int lane)
      : m(mm), s(ss), sl(lane & (HL - 1)), nb(mm->nbody), up(lane >= HL) {}

  // The Newton iterations rebuild H and factor it every time.  MuJoCo's rank-1 updates of the factor
  // (mju_cholUpdate) were built and measured slower on MI355X (DESIGN.md 3.1 "Incremental factor"):
  // each update is a serial 27-column chain, and the extra live state costs the queue kernel its last
  // registers.
  // the Newton factor as L D L' in the fp64 engine (unit lower L): the same elimination, but the
  // triangular solves lose one dependent multiply per column (fp64 0.740 -> 0.731 ms per configs[1]
  // launch; the Euler factorization and the fp32 engine measured the same either way and stay L L').
  static constexpr bool LDLF = sizeof(T) == 8;
  static constexpr bool LDLE = false;
  // the launch arguments (every step-kernel instance takes its KArgs at kernarg offset 0)
  __device__ __forceinline__ static KPtr<T> kargs() { return (KPtr<T>)__builtin_amdgcn_kernarg_segment_ptr(); }

  // start of a pipeline phase: nothing lane-invariant is carried over from the previous phase
  __device__ __forceinline__ void phase_begin() {
    m = opaque(m);
    sl = opaque_v(sl);
  }

  // mj_kinematics + mj_comPos
  __device__ __forceinline__ void kinematics() {
    phase_begin();
    if (sl == 0) {
      for (int k = 0; k < 3; k++) s.u.k.xpos[0][k] = 0;
      s.u.k.xquat[0][0] = 1; s.u.k.xquat[0][1] = s.u.k.xquat[0][2] = s.u.k.xquat[0][3] = 0;
      for (int k = 0; k < 9; k++) s.u.k.xmat[0][k] = (k % 4 == 0) ? T(1) : T(0);
    }
    // mj_kinematics, split so the serial level loop carries one frame composition per level:
    // (1) in parallel over bodies, the body's transform RELATIVE TO ITS PARENT (body_pos/quat
    //     followed by its hinges, each rotating about jnt_pos: p' = a - R(q qloc) jpos with the
    //     anchor a = p + R(q) jpos) and each hinge's anchor/axis in the parent frame;
    // (2) level by level: xquat = normalize(xquat_par * q_loc), xpos = xpos_par + xmat_par p_loc;
    // (3) in parallel again: xanchor = xpos_par + xmat_par a_loc, xaxis = xmat_par ax_loc.
    // Mathematically identical to MuJoCo's per-joint world-frame recursion (rounding differs).
    const int b = sl;
    const bool isb = b > 0 && b < nb;
    int depth = -1, par = 0, ja = 0, jn = 0, fqa = 0;
    bool isfree = false;
    T pl[3] = {0, 0, 0}, ql[4] = {1, 0, 0, 0};
    T anl[MAXJPB][3], axl[MAXJPB][3];
    if (isb) {
      depth = HS_LT(C, m).body_depth[b];
      par = HS_LT(C, m).body_parentid[b];
      ja = HS_LT(C, m).body_jntadr[b];
      jn = HS_LT(C, m).body_jntnum[b];
      isfree = jn == 1 && HS_LT(C, m).jnt_type[ja] == JNT_FREE;
      fqa = HS_LT(C, m).jnt_qposadr[ja];
      for (int k = 0; k < 3; k++) pl[k] = HS_LT(C, m).body_pos[b][k];
      for (int k = 0; k < 4; k++) ql[k] = HS_LT(C, m).body_quat[b][k];
    }
    if (isfree) {
      for (int k = 0; k < 3; k++) pl[k] = s.qpos[fqa + k];
      for (int k = 0; k < 4; k++) ql[k] = s.qpos[fqa + 3 + k];
    }
#pragma unroll
    for (int jj = 0; jj < MAXJPB; jj++) {
      const bool use = isb && !isfree && jj < jn;
      const int j = use ? ja + jj : 0;
      T jp[3], jx[3], ang = 0;
      for (int k = 0; k < 3; k++) { jp[k] = use ? m->jnt_pos[j][k] : T(0); jx[k] = use ? m->jnt_axis[j][k] : T(0); }
      if (use) {
        int qa = HS_LT(C, m).jnt_qposadr[j];
        ang = s.qpos[qa] - HS_LT(C, m).qpos0[qa];
      }
      T sn, cs;
      sincos_t(T(0.5) * ang, sn, cs);
      const T jr[4] = {cs, jx[0] * sn, jx[1] * sn, jx[2] * sn};
      T R[9];
      quat2mat(ql, R);
      mv3(R, jx, axl[jj]);
      mv3(R, jp, anl[jj]);
      for (int k = 0; k < 3; k++) anl[jj][k] += pl[k];
      if (use) {
        mulq(ql, jr, ql);
        quat2mat(ql, R);
        T v[3];
        mv3(R, jp, v);
        for (int k = 0; k < 3; k++) pl[k] = anl[jj][k] - v[k];
      }
    }
    WSYNC();
    for (int L = 1; L <= m->nlevel; L++) {
      if (depth == L) {
        T pos[3], q[4];
        if (isfree) {   // parent is the world: the free joint's qpos is the world frame
          for (int k = 0; k < 3; k++) pos[k] = pl[k];
          for (int k = 0; k < 4; k++) q[k] = ql[k];
        } else {
          mv3(s.u.k.xmat[par], pl, pos);
          for (int k = 0; k < 3; k++) pos[k] += s.u.k.xpos[par][k];
          T pq[4] = {s.u.k.xquat[par][0], s.u.k.xquat[par][1], s.u.k.xquat[par][2], s.u.k.xquat[par][3]};
          mulq(pq, ql, q);
        }
        normalize4(q);
        for (int k = 0; k < 4; k++) s.u.k.xquat[b][k] = q[k];
        for (int k = 0; k < 3; k++) s.u.k.xpos[b][k] = pos[k];
        quat2mat(q, s.u.k.xmat[b]);
      }
      WSYNC();
    }
    if (isb) {
      if (isfree) {
        for (int k = 0; k < 3; k++) { HS_KTAIL(s).xanchor[ja][k] = s.u.k.xpos[b][k]; HS_KTAIL(s).xaxis[ja][k] = m->jnt_axis[ja][k]; }
      } else {
        const T* Rp = s.u.k.xmat[par];
        const T* xp = s.u.k.xpos[par];
#pragma unroll
        for (int jj = 0; jj < MAXJPB; jj++) {
          if (jj < jn) {
            T an[3], ax[3];
            mv3(Rp, anl[jj], an);
            mv3(Rp, axl[jj], ax);
            for (int k = 0; k < 3; k++) { HS_KTAIL(s).xanchor[ja + jj][k] = xp[k] + an[k]; HS_KTAIL(s).xaxis[ja + jj][k] = ax[k]; }
          }
        }
      }
    }
    if (sl < m->ngeom) {
      int g = sl, gb = HS_LT(C, m).geom_bodyid[g];
      T gp[3] = {m->geom_pos[g][0], m->geom_pos[g][1], m->geom_pos[g][2]};
      T gz[3] = {m->geom_zaxis[g][0], m->geom_zaxis[g][1], m->geom_zaxis[g][2]};
      T w[3];
      mv3(s.u.k.xmat[gb], gp, w);
      for (int k = 0; k < 3; k++) HS_KTAIL(s).gpos[g][k] = s.u.k.xpos[gb][k] + w[k];
      mv3(s.u.k.xmat[gb], gz, HS_KTAIL(s).gax[g]);
    }
    T mx = 0, my = 0, mz = 0, xi[3] = {0, 0, 0};
    if (b > 0 && b < nb) {
      T ip[3] = {m->body_ipos[b][0], m->body_ipos[b][1], m->body_ipos[b][2]}, w[3];
      mv3(s.u.k.xmat[b], ip, w);
      for (int k = 0; k < 3; k++) xi[k] = s.u.k.xpos[b][k] + w[k];
      T mb = HS_LT(C, m).body_mass[b];
      mx = mb * xi[0]; my = mb * xi[1]; mz = mb * xi[2];
    }
    // mj_comPos: single kinematic tree -> subtree_com[root] == subtree_com[0] == whole-model COM
    T inv = T(1) / m->total_mass;
    T c0 = hsum(mx) * inv, c1 = hsum(my) * inv, c2 = hsum(mz) * inv;
    if (sl == 0) { s.com[0] = c0; s.com[1] = c1; s.com[2] = c2; }
    if (b > 0 && b < nb) {   // cinert (mju_inertCom)
      const T* R = s.u.k.xmat[b];
      CPtr<T> I6 = m->body_inert[b];
      T I[9] = {I6[0], I6[3], I6[4], I6[3], I6[1], I6[5], I6[4], I6[5], I6[2]};
      T A[9];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) A[3 * r + c] = R[3 * r] * I[c] + R[3 * r + 1] * I[3 + c] + R[3 * r + 2] * I[6 + c];
      T Ic[6];
      Ic[0] = A[0] * R[0] + A[1] * R[1] + A[2] * R[2];
      Ic[1] = A[3] * R[3] + A[4] * R[4] + A[5] * R[5];
      Ic[2] = A[6] * R[6] + A[7] * R[7] + A[8] * R[8];
      Ic[3] = A[0] * R[3] + A[1] * R[4] + A[2] * R[5];
      Ic[4] = A[0] * R[6] + A[1] * R[7] + A[2] * R[8];
      Ic[5] = A[3] * R[6] + A[4] * R[7] + A[5] * R[8];
      T d[3] = {xi[0] - c0, xi[1] - c1, xi[2] - c2};
      T mass = HS_LT(C, m).body_mass[b];
      T* ci = s.cinert[b];
      ci[0] = Ic[0] + mass * (d[1] * d[1] + d[2] * d[2]);
      ci[1] = Ic[1] + mass * (d[0] * d[0] + d[2] * d[2]);
      ci[2] = Ic[2] + mass * (d[0] * d[0] + d[1] * d[1]);
      ci[3] = Ic[3] - mass * d[0] * d[1];
      ci[4] = Ic[4] - mass * d[0] * d[2];
      ci[5] = Ic[5] - mass * d[1] * d[2];
      ci[6] = mass * d[0]; ci[7] = mass * d[1]; ci[8] = mass * d[2]; ci[9] = mass;
    }
    if (sl == 0)
      for (int k = 0; k < 10; k++) s.cinert[0][k] = 0;
    for (int k = 0; k < 6; k++) cd[k] = 0;
    if (sl < NV) {   // cdof (mju_dofCom)
      int j = HS_LT(C, m).dof_jntid[sl], db = HS_LT(C, m).dof_bodyid[sl];
      T off[3] = {c0 - HS_KTAIL(s).xanchor[j][0], c1 - HS_KTAIL(s).xanchor[j][1], c2 - HS_KTAIL(s).xanchor[j][2]};
      T ax[3];
      bool lin = false;
      if (HS_LT(C, m).jnt_type[j] == JNT_FREE) {
        int k = sl - HS_LT(C, m).jnt_dofadr[j];
        if (k < 3) {   // no dynamic indexing of register arrays (it would demote the Stepper to scratch)
          lin = true;
          cd[3] = k == 0 ? T(1) : T(0); cd[4] = k == 1 ? T(1) : T(0); cd[5] = k == 2 ? T(1) : T(0);
        } else {
          int c = k - 3;
          ax[0] = s.u.k.xmat[db][c]; ax[1] = s.u.k.xmat[db][3 + c]; ax[2] = s.u.k.xmat[db][6 + c];
        }
      } else {
        ax[0] = HS_KTAIL(s).xaxis[j][0]; ax[1] = HS_KTAIL(s).xaxis[j][1]; ax[2] = HS_KTAIL(s).xaxis[j][2];
      }
      if (!lin) {
        cd[0] = ax[0]; cd[1] = ax[1]; cd[2] = ax[2];
        cross3(ax, off, cd + 3);
      }
      for (int k = 0; k < 6; k++) s.cdof[sl][k] = cd[k];
    }
    WSYNC();
    if (dbg)    // stage dump (env 0, debug mode): xpos is phase-local, so dump it here
      for (int k = sl; k < MAXBODY * 3; k += HL) dbg[k] = s.u.k.xpos[k / 3][k % 3];
  }

  // mj_collision: one static pair per sub-lane per pass, ordered compaction into contacts
  __device__ __forceinline__ int collision() {
    phase_begin();
    int ncon = 0;
    const int npair = m->npair;
    // the next pass's pair records are loaded while this pass runs (their L1/L2 latency is otherwise
    // exposed at the top of every pass: one wave per SIMD in fp64)
    int4 info_n = make_int4(0, 0, 0, 0);
    T sz_n[4] = {0, 0, 0, 0};
    if (sl < npair) {
      info_n = make_int4(m->pair_info[sl][0], m->pair_info[sl][1], m->pair_info[sl][2], m->pair_info[sl][3]);
      for (int k = 0; k < 4; k++) sz_n[k] = m->pair_size[sl][k];
    }
    for (int base = 0; base < npair; base += HL) {
      int p = base + sl;
      Con<T> c0, c1;
      int n = 0;
      const int4 info = info_n;
      T sz[4] = {sz_n[0], sz_n[1], sz_n[2], sz_n[3]};
      if (p + HL < npair) {
        info_n = make_int4(m->pair_info[p + HL][0], m->pair_info[p + HL][1], m->pair_info[p + HL][2],
                           m->pair_info[p + HL][3]);
        for (int k = 0; k < 4; k++) sz_n[k] = m->pair_size[p + HL][k];
      }
      if (p < npair) n = collide_pair(s, info, sz, c0, c1);
      uint32_t m1 = hballot(n >= 1, up), m2 = hballot(n >= 2, up);
      int pre = below(m1, sl) + below(m2, sl);
      if (n >= 1) store_contact(m, s, ncon + pre, c0, p);
      if (n >= 2) store_contact(m, s, ncon + pre + 1, c1, p);
      ncon += __popc(m1) + __popc(m2);
    }
    int overflow = ncon > C::CON;
    if (overflow) ncon = C::CON;
    if (sl == 0) s.ncon = ncon;
    WSYNC();
    return overflow;
  }

  // mj_collision of the C::NEAR instances (physics_step picks it), the same contacts in the same slots as
  // collision().
  // A wave runs collide_pair's capsule-capsule branch (IEEE divides, a square root, make_frame) in every
  // pass where any of its 64 lanes holds a near pair, and a humanoid's ~26 near pairs lie scattered over
  // the five passes.  So a broad pass first compacts each env's near pairs, ascending, into a list in LDS
  // (Scratch::near_list), and the narrow phase runs ceil(max(near pairs of either half) / 32) passes over
  // the list: usually one.  Ascending pair order in the list keeps the contact slots in MuJoCo's order.
  __device__ __forceinline__ int collision_near() {
    phase_begin();
    const int npair = m->npair;
    uint32_t* const list = s.near_list();
    int nlo = 0, nhi = 0;       // near pairs of the wave's two envs so far (wave-uniform)
    int4 info_n = make_int4(0, 0, 0, 0);
    T sz_n[4] = {0, 0, 0, 0};
    if (sl < npair) {
      info_n = make_int4(m->pair_info[sl][0], m->pair_info[sl][1], m->pair_info[sl][2], m->pair_info[sl][3]);
      for (int k = 0; k < 4; k++) sz_n[k] = m->pair_size[sl][k];
    }
    for (int base = 0; base < npair; base += HL) {
      const int p = base + sl;
      const int4 info = info_n;
      const T sz[4] = {sz_n[0], sz_n[1], sz_n[2], sz_n[3]};
      if (p + HL < npair) {
        info_n = make_int4(m->pair_info[p + HL][0], m->pair_info[p + HL][1], m->pair_info[p + HL][2],
                           m->pair_info[p + HL][3]);
        for (int k = 0; k < 4; k++) sz_n[k] = m->pair_size[p + HL][k];
      }
      const int g1 = info.x, g2 = info.y, fn = info.z;
      bool near = false;
      if (p < npair) {
        const T* p1 = HS_KTAIL(s).gpos[g1];
        const T* p2 = HS_KTAIL(s).gpos[g2];
        const T* a1 = HS_KTAIL(s).gax[g1];
        const T d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
        // body pairs: collide_pair's own bounding-sphere test (it runs again there, on the same values).
        // plane pairs: the geom's centre above the plane by more than radius + half-length.  Exact: a
        // capsule's end spheres lie within h2 of its centre along a unit axis, so an end at cd_end <= r2
        // has the centre at cd <= r2 + h2.  The slack (1e-9 relative, 1e-12 absolute, far above the
        // rounding of these few operations) errs towards near only: a pair wrongly near costs a lane of
        // the narrow pass and yields no contact, a pair wrongly far would lose one.
        const T R = sz[0] + sz[1] + sz[2] + sz[3];
        const bool far_body = dot3(d, d) > R * R;
        const T reach = sz[2] + (fn == PAIR_PLANE_CAPSULE ? sz[3] : T(0));
        const bool far_plane = dot3(d, a1) > reach * T(1 + 1e-9) + T(1e-12);
        near = !(fn >= PAIR_SPHERE_SPHERE ? far_body : far_plane);
      }
      const uint64_t bm = __ballot(near);
      const uint32_t mk = up ? (uint32_t)(bm >> 32) : (uint32_t)bm;
      if (near) list[(up ? nhi : nlo) + below(mk, sl)] = near_entry(p, g1, g2, fn);
      nlo += __popc((uint32_t)bm);
      nhi += __popc((uint32_t)(bm >> 32));
    }
    const int nnear = up ? nhi : nlo;
    const int nmax = nlo > nhi ? nlo : nhi;
    WSYNC();
    int ncon = 0;
    for (int j0 = 0; j0 < nmax; j0 += HL) {
      const int j = j0 + sl;
      const bool on = j < nnear;
      const uint32_t e = on ? list[j] : 0u;     // (idle lanes load pair 0's records and run nothing)
      const int p = e & 0xff, g1 = (e >> 8) & 0xff, g2 = (e >> 16) & 0xff, fn = e >> 24;
      // everything the pass reads from the model at the pair's index, issued together
      const T sz[4] = {m->pair_size[p][0], m->pair_size[p][1], m->pair_size[p][2], m->pair_size[p][3]};
      const T mu = m->pair_mu[p];
      const int dim = m->pair_info[p][3];
      Con<T> c0, c1;
      int n = 0;
      if (on) n = collide_pair(s, make_int4(g1, g2, fn, dim), sz, c0, c1);
      uint32_t m1 = hballot(n >= 1, up), m2 = hballot(n >= 2, up);
      int pre = below(m1, sl) + below(m2, sl);
      if (n >= 1) store_contact_near(m, s, ncon + pre, c0, p, g1, g2, dim, mu);
      if (n >= 2) store_contact_near(m, s, ncon + pre + 1, c1, p, g1, g2, dim, mu);
      ncon += __popc(m1) + __popc(m2);
    }
    int overflow = ncon > C::CON;
    if (overflow) ncon = C::CON;
    if (sl == 0) s.ncon = ncon;
    WSYNC();
    return overflow;
  }

  // mj_crb -> Mr rows (registers)
  __device__ __forceinline__ void mass_matrix() {
    phase_begin();
    if (sl > 0 && sl < nb) {
      const uint32_t dm = HS_LT(C, m).body_descmask[sl] & ~1u & ((nb < 32 ? (1u << nb) : 0u) - 1u);
      T a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      HS_FOR_BITS(C, G_CRB, T)(dm, [&](int c) { Vals<T, 10> r; for (int k = 0; k < 10; k++) r.v[k] = s.cinert[c][k]; return r; },
                  [&](int, const Vals<T, 10>& r) { for (int k = 0; k < 10; k++) a[k] += r.v[k]; });   // the subtree's bodies, ascending
      for (int k = 0; k < 10; k++) s.u.c.crb[sl][k] = a[k];
    }
    WSYNC();
    T bf[6] = {0, 0, 0, 0, 0, 0};
    uint32_t anci = 0;
    T arm = 0;
    if (sl < NV) {
      mul_inert(s.u.c.crb[HS_LT(C, m).dof_bodyid[sl]], cd, bf);
      for (int k = 0; k < 6; k++) s.u.c.buf[sl][k] = bf[k];
      anci = HS_LT(C, m).dof_ancmask[sl];
      arm = HS_LT(C, m).dof_armature[sl];
    }
    WSYNC();
    // one column per scheduling group (2 or 3 measured the same)
    {
      // software-pipelined: column j+1's cdof / buf rows are read before column j's arithmetic, behind
      // the per-column scheduling fence, so each LDS round trip overlaps the previous column's FMAs
      // (A/B with the Hessian rows of solve(), fp64 ms per configs[1] launch: 0.681 -> CRB 0.674,
      // Hessian 0.661, both 0.659; the fp64 queue kernel drops from 510 to 482 unified registers)
      T cb2[2][12];
      auto load = [&](auto jc, T (&dst)[12]) {
        constexpr int j = decltype(jc)::value;
        for (int k = 0; k < 6; k++) { dst[k] = s.cdof[j][k]; dst[6 + k] = s.u.c.buf[j][k]; }
      };
      load(std::integral_constant<int, 0>{}, cb2[0]);
      static_for<0, NV>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if constexpr (j + 1 < NV) load(std::integral_constant<int, j + 1>{}, cb2[(j + 1) & 1]);
        SCHED_FENCE();
        const uint32_t ancj = m->dof_ancmask[j];
        const bool rel = (sl < NV) && (bit(anci, j) || bit(ancj, sl));
        const T* cj = cb2[j & 1];
        const T v = (j <= sl) ? dot6(cj, bf) : dot6(cd, cj + 6);
        Mr[j] = rel ? v + ((j == sl) ? arm : T(0)) : T(0);
      });
    }
    WSYNC();
  }

  // mj_comVel (cvel, cdof_dot), mj_passive, mj_fwdActuation, mj_rne -> fsmooth
  __device__ __forceinline__ void velocity_forces() {
    phase_begin();
    if (sl < nb) {
      T v[6] = {0, 0, 0, 0, 0, 0};
      if (sl > 0) {
        const uint32_t ch = HS_LT(C, m).body_chainmask[sl];
        HS_FOR_BITS(C, G_VEL, T)(ch, [&](int j) { ValsX<T, 6> r; r.x = s.qvel[j]; for (int k = 0; k < 6; k++) r.v[k] = s.cdof[j][k]; return r; },
                    [&](int, const ValsX<T, 6>& r) { for (int k = 0; k < 6; k++) v[k] = fma(r.v[k], r.x, v[k]); });   // the chain's dofs, ascending
      }
      for (int k = 0; k < 6; k++) s.cvel[sl][k] = v[k];
    }
    if (sl < NV) {
      const uint32_t dm = HS_LT(C, m).dof_dotmask[sl];
      T v[6] = {0, 0, 0, 0, 0, 0}, cdd[6];
      HS_FOR_BITS(C, G_VEL, T)(dm, [&](int j) { ValsX<T, 6> r; r.x = s.qvel[j]; for (int k = 0; k < 6; k++) r.v[k] = s.cdof[j][k]; return r; },
                  [&](int, const ValsX<T, 6>& r) { for (int k = 0; k < 6; k++) v[k] = fma(r.v[k], r.x, v[k]); });   // ascending, set bits only
      cross_motion(v, cd, cdd);
      for (int k = 0; k < 6; k++) s.u.r.cdofdot[sl][k] = cdd[k];
    }
    WSYNC();
    if (sl > 0 && sl < nb) {   // RNE: cacc, cfrc_body
      const uint32_t ch = HS_LT(C, m).body_chainmask[sl];
      T a[6] = {0, 0, 0, -m->gravity[0], -m->gravity[1], -m->gravity[2]};
      HS_FOR_BITS(C, G_VEL, T)(ch, [&](int j) { ValsX<T, 6> r; r.x = s.qvel[j]; for (int k = 0; k < 6; k++) r.v[k] = s.u.r.cdofdot[j][k]; return r; },
                  [&](int, const ValsX<T, 6>& r) { for (int k = 0; k < 6; k++) a[k] = fma(r.v[k], r.x, a[k]); });   // the chain's dofs, ascending
      T f[6], t[6], t2[6];
      mul_inert(s.cinert[sl], a, f);
      mul_inert(s.cinert[sl], s.cvel[sl], t);
      cross_force(s.cvel[sl], t, t2);
      for (int k = 0; k < 6; k++) s.u.r.cfrc[sl][k] = f[k] + t2[k];
    }
    WSYNC();
    if (sl > 0 && sl < nb) {   // subtree sums of cfrc_body
      const uint32_t dm = HS_LT(C, m).body_descmask[sl] & ~1u & ((nb < 32 ? (1u << nb) : 0u) - 1u);
      T a[6] = {0, 0, 0, 0, 0, 0};
      HS_FOR_BITS(C, G_VEL, T)(dm, [&](int c) { Vals<T, 6> r; for (int k = 0; k < 6; k++) r.v[k] = s.u.r.cfrc[c][k]; return r; },
                  [&](int, const Vals<T, 6>& r) { for (int k = 0; k < 6; k++) a[k] += r.v[k]; });   // the subtree's bodies, ascending
      for (int k = 0; k < 6; k++) s.u.r.csub[sl][k] = a[k];
    }
    WSYNC();
    fsmooth = 0;
    qfa = 0;
    if (sl < NV) {
      T bias = dot6(cd, s.u.r.csub[HS_LT(C, m).dof_bodyid[sl]]);
      int qa = HS_LT(C, m).dof_qposadr[sl];
      T pas = -HS_LT(C, m).dof_damping[sl] * s.qvel[sl];
      if (qa >= 0) pas -= HS_LT(C, m).dof_stiffness[sl] * (s.qpos[qa] - HS_LT(C, m).dof_springref[sl]);
      int u = HS_LT(C, m).dof_actuator[sl];
      if (u >= 0) {
        T c = s.ctrl[u];
        if (HS_LT(C, m).act_ctrllimited[u]) c = fmin(HS_LT(C, m).act_ctrlrange[u][1], fmax(HS_LT(C, m).act_ctrlrange[u][0], c));
        qfa = HS_LT(C, m).act_gear[u] * c;
      }
      fsmooth = pas - bias + qfa;
    }
    WSYNC();
  }

  // mj_makeConstraint + mj_makeImpedance + reference (aref); row q of this lane: r = sl + 32 q.
  // NEWTON (the Newton instances with C::WALKS): the rows' J x operands are read in one batch (rows_Jx), and the
  // chain walk behind J qvel also sums J xws (xws = qacc_warmstart, both known here), so that the initial
  // jar = J xws - aref of solve() comes out of this phase (jar0) and solve() walks no chain at its entry.
  // The PGS instances (NEWTON = false) keep the one-vector text.
  template <bool NEWTON>
  __device__ __forceinline__ int rows(T (&D)[C::RPL], T (&ar)[C::RPL], int (&rd)[C::RPL], T (&rc)[C::RPL], T xws,
                                      T (&jar0)[C::RPL]) {
    constexpr bool WK = C::WALKS && NEWTON;
    phase_begin();
    damp = sl < NV ? HS_LT(C, m).dof_damping[sl] : T(0);
    int overflow = 0;
    int ncon = s.ncon;
    int nrow = 0;
    {   // joint limits (lower side first, MuJoCo side = -1 then +1)
      bool lo = false, hi = false;
      if (sl < m->njnt && HS_LT(C, m).jnt_limited[sl]) {
        T q = s.qpos[HS_LT(C, m).jnt_qposadr[sl]];
        lo = (q - HS_LT(C, m).jnt_range[sl][0]) < HS_LT(C, m).jnt_margin[sl];
        hi = (HS_LT(C, m).jnt_range[sl][1] - q) < HS_LT(C, m).jnt_margin[sl];
      }
      uint32_t ml = hballot(lo, up), mh = hballot(hi, up);
      int pre = below(ml, sl) + below(mh, sl);
      if (lo) s.row_kid[pre] = (RK_JLO << 16) | sl;
      if (hi) s.row_kid[pre + lo] = (RK_JHI << 16) | sl;
      nrow = __popc(ml) + __popc(mh);
      s.lim_row[sl] = 0;                       // MAXDOF == HL: one slot per sub-lane
      if (lo || hi)
        s.lim_row[HS_LT(C, m).jnt_dofadr[sl]] = (uint16_t)((lo ? pre + 1 : 0) | (hi ? (pre + lo + 1) << 8 : 0));
    }
    const int njl = nrow;
    {   // tendon limits
      bool lo = false, hi = false;
      if (sl < m->ntendon && HS_LT(C, m).ten_limited[sl]) {
        T L = 0;
        for (int w = 0; w < HS_LT(C, m).ten_nwrap[sl]; w++) L += HS_LT(C, m).ten_wrapcoef[sl][w] * s.qpos[HS_LT(C, m).ten_wrapqadr[sl][w]];
        lo = (L - HS_LT(C, m).ten_range[sl][0]) < m->ten_margin[sl];
        hi = (HS_LT(C, m).ten_range[sl][1] - L) < m->ten_margin[sl];
      }
      uint32_t ml = hballot(lo, up), mh = hballot(hi, up);
      int pre = nrow + below(ml, sl) + below(mh, sl);
      if (lo) s.row_kid[pre] = (RK_TLO << 16) | sl;
      if (hi) s.row_kid[pre + lo] = (RK_THI << 16) | sl;
      nrow += __popc(ml) + __popc(mh);
    }
    int nlim = nrow;
    {   // contacts: 1 row (condim 1) or 4 pyramid rows (condim 3), in contact order
      int tot = 0;
#pragma unroll
      for (int cs = 0; cs < C::CON; cs += HL) {
        const int c = cs + sl;
        const bool isc = c < ncon;
        const bool pyr = isc && (s.con_bb[c] >> 16) == 3;
        tot += __popc(hballot(isc, up)) + 3 * __popc(hballot(pyr, up));
      }
      if (nrow + tot > C::EFC) {   // drop whole contacts that do not fit (counted as overflow)
        overflow = 1;
        int fit = 0, nr = nrow;
        for (int c = 0; c < ncon; c++) {
          int need = (s.con_bb[c] >> 16) == 3 ? 4 : 1;
          if (nr + need > C::EFC) break;
          nr += need;
          fit++;
        }
        ncon = fit;
      }
#pragma unroll
      for (int cs = 0; cs < C::CON; cs += HL) {
        const int c = cs + sl;
        const bool isc = c < ncon;
        const bool pyr = isc && (s.con_bb[c] >> 16) == 3;
        const uint32_t mc = hballot(isc, up), mp = hballot(pyr, up);
        const int pre = nrow + below(mc, sl) + 3 * below(mp, sl);
        if (isc) {
          s.con_adr[c] = pre;
          if (!pyr) s.row_kid[pre] = (RK_CN << 16) | c;
          else for (int q = 0; q < 4; q++) s.row_kid[pre + q] = ((RK_P0 + q) << 16) | c;
        }
        nrow += __popc(mc) + 3 * __popc(mp);
      }
    }
    if (sl == 0) { s.ncon = ncon; s.nefc = nrow; s.nlim = nlim; s.njl = njl; }
    if constexpr (WK) {
      if (sl < NV) s.vx[sl] = xws;      // s.vx = qacc_warmstart (solve() starts from it); J qvel reads s.qvel
      WSYNC();
      chain_vel2<NV>(s, sl, nb, chain_mask<C>(m, sl, nb));
      contact_vel(s, sl, s.u.n.bvel);                      // con_v of J qvel
    } else {
      if (sl < NV) s.vx[sl] = s.qvel[sl];
      WSYNC();
      map_vx<NV>(s, sl, nb, chain_mask<C>(m, sl, nb));     // row velocities J qvel for aref
    }
    // (WK) aref's operands, until the batch of J qvel is read
    [[maybe_unused]] T rB[WK ? C::RPL : 1], rKi[WK ? C::RPL : 1], rpm[WK ? C::RPL : 1];
#pragma unroll
    for (int q = 0; q < C::RPL; q++) {
      int r = sl + HL * q;
      D[q] = 0;
      if constexpr (WK) { rB[q] = 0; rKi[q] = 0; rpm[q] = 0; }
      ar[q] = 0;
      rd[q] = 0;
      rc[q] = 0;
      bool dense = false;
      if (r < nrow) {
        int kid = s.row_kid[r];
        int kind = rk_kind(kid), id = rk_id(kid);
        T pos, margin, dA, rscale = 1;
        CPtr<T> sr;
        CPtr<T> si;
        if (kind <= RK_JHI) {
          T qv = s.qpos[HS_LT(C, m).jnt_qposadr[id]];
          pos = kind == RK_JLO ? qv - HS_LT(C, m).jnt_range[id][0] : HS_LT(C, m).jnt_range[id][1] - qv;
          margin = HS_LT(C, m).jnt_margin[id];
          sr = m->jnt_solref[id]; si = m->jnt_solimp[id];
          int dof = HS_LT(C, m).jnt_dofadr[id];
          dA = HS_LT(C, m).dof_invweight0[dof];
          rd[q] = (kind << 16) | dof;
          rc[q] = kind == RK_JLO ? T(1) : T(-1);
        } else if (kind <= RK_THI) {
          T L = 0;
          for (int w = 0; w < HS_LT(C, m).ten_nwrap[id]; w++) L += HS_LT(C, m).ten_wrapcoef[id][w] * s.qpos[HS_LT(C, m).ten_wrapqadr[id][w]];
          pos = kind == RK_TLO ? L - HS_LT(C, m).ten_range[id][0] : HS_LT(C, m).ten_range[id][1] - L;
          margin = m->ten_margin[id];
          sr = m->ten_solref[id]; si = m->ten_solimp[id];
          dA = m->ten_invweight0[id];
          rd[q] = kid;
          rc[q] = kind == RK_TLO ? T(1) : T(-1);
          dense = true;
        } else {
          int p = s.con_pair[id];
          pos = s.con_dist[id];
          margin = m->pair_margin[p];
          sr = m->pair_solref[p]; si = m->pair_solimp[p];
          const uint32_t bb = s.con_bb[id];
          T tran = HS_LT(C, m).body_invweight_tran[bb & 0xff] + HS_LT(C, m).body_invweight_tran[(bb >> 8) & 0xff];
          T mu = s.con_mu[id];
          dA = kind == RK_CN ? tran : tran + mu * mu * tran;
          // pyramidal edges share one R: Rpy = 2 mu^2 R_edge / impratio (impratio = 1, enforced by the
          // compiler); pinned by the reference's recorded MuJoCo state, tests/test_reference_pin.py
          if (kind != RK_CN) rscale = 2 * mu * mu;
          rd[q] = kid;
          rc[q] = kind == RK_CN ? T(0) : (((kind - RK_P0) & 1) ? -mu : mu);
          dense = s.con_m1[id] != 0u;
        }
        T imp = impedance(si, pos, margin);
        T dmax = fmin(T(0.9999), fmax(T(0.0001), si[1]));
        T K, B;
        if (sr[0] > 0) {   // (reciprocals, not IEEE divides: ~1 ulp, and a shorter fp64 chain)
          T tc = fmax(sr[0], 2 * m->timestep), dr = sr[1];
          const T u = recip(dmax * tc), ud = u * recip(dr);
          K = ud * ud;
          B = 2 * u;
        } else {
          const T v = recip(dmax);
          K = -sr[0] * v * v;
          B = -sr[1] * v;
        }
        T R = rscale * fmax(T(1e-15), (1 - imp) * dA * recip(imp));
        D[q] = recip(R);
        s.row_D[r] = D[q];
        if constexpr (WK) { rB[q] = B; rKi[q] = K * imp; rpm[q] = pos - margin; }
        else ar[q] = -B * row_Jx(m, s, rd[q], rc[q]) - K * imp * (pos - margin);
      }
      uint32_t dm = hballot(dense, up);
      if (sl == 0) s.dense_mask[q] = dm;
    }
    if constexpr (WK) {
      bool vr[C::RPL];
      T jx[C::RPL];
#pragma unroll
      for (int q = 0; q < C::RPL; q++) vr[q] = sl + HL * q < nrow;
      rows_Jx(m, s, s.qvel, vr, rd, rc, jx);
#pragma unroll
      for (int q = 0; q < C::RPL; q++)
        if (vr[q]) ar[q] = -rB[q] * jx[q] - rKi[q] * rpm[q];
      WSYNC();
      contact_vel(s, sl, s.u.n.cfrc);                      // con_v of J qacc_warmstart
      rows_Jx(m, s, s.vx, vr, rd, rc, jx);
#pragma unroll
      for (int q = 0; q < C::RPL; q++) jar0[q] = vr[q] ? jx[q] - ar[q] : T(0);
    }
    WSYNC();
    return overflow;
  }

  // primal Newton (mj_solNewton semantics), warm-started; x = qacc
  // jar0: the initial jar = J xws - aref from rows<true>() where it sums two vectors per chain walk
  __device__ __forceinline__ void solve(T xws, int maxit, T tol, const T (&D)[C::RPL], const T (&ar)[C::RPL],
                                        const int (&rd)[C::RPL], const T (&rc)[C::RPL], const T (&jar0)[C::RPL]) {
    constexpr bool WK = C::WALKS;
    phase_begin();
    const int nefc = s.nefc;
    T x = sl < NV ? xws : T(0);
    bool vr[C::RPL];
#pragma unroll
    for (int q = 0; q < C::RPL; q++) vr[q] = sl + HL * q < nefc;
    const uint32_t anci = sl < NV ? HS_LT(C, m).dof_ancmask[sl] : 0u;
    const uint32_t bch = chain_mask<C>(m, sl, nb);     // loaded once per solve (map_vx per iteration)
    const T scale = m->newton_scale;
    if (sl < NV) s.vx[sl] = x;
    WSYNC();
    T Mx = matvec_lds(Mr, s.vx);     // kept current below (Mx += alpha M s)
    T jar[C::RPL], Js[C::RPL];
    if constexpr (WK) {
#pragma unroll
      for (int q = 0; q < C::RPL; q++) jar[q] = jar0[q];
    } else {
      map_vx<NV>(s, sl, nb, bch);
#pragma unroll
      for (int q = 0; q < C::RPL; q++) jar[q] = vr[q] ? row_Jx(m, s, rd[q], rc[q]) - ar[q] : T(0);
    }
    HS_STAMP(clk, 6);
    bool done = false;      // this half-wave's solver has converged
    int it = 0;
    if (sl == 0) s.niter = maxit;   // per env: the iteration at which this half converged
    for (; it < maxit; it++) {
      m = opaque(m);
      sl = opaque_v(sl);
      bool act[C::RPL];
#pragma unroll
      for (int q = 0; q < C::RPL; q++) {
        act[q] = vr[q] && jar[q] < 0;
        if (vr[q]) s.row_f[sl + HL * q] = act[q] ? -D[q] * jar[q] : T(0);
      }
      WSYNC();
      contact_aggregates(m, s, sl);
      HS_STAMP(clk, 7);
      // the contact terms of the Hessian come out of J'f's walk over the active contacts (WK), ahead of the
      // convergence test: on the converging iteration they are dropped (the walk costs, not the FMAs)
      T aug[6] = {0, 0, 0, 0, 0, 0};
      T jtf;
      if constexpr (WK) jtf = jtf_aug_lane(m, s, sl, cd, aug);
      else jtf = jtf_lane(m, s, sl, cd);
      T g = sl < NV ? Mx - fsmooth - jtf : T(0);
      const T gn2 = hsum(g * g);                 // |g| scale < tol, squared (no sqrt on the chain)
      const bool conv = scale * scale * gn2 < tol * tol;
      if (conv && !done && sl == 0) s.niter = it;
      done = done || conv;
      HS_STAMP(clk, 8);
      if (__ballot(!done) == 0) break;       // both envs of the wave converged
      T H[NV];
      T hdinv = 0, hdiag = 0;
      // Hessian lower rows: M + contact (tree form) + joint limits (diag) + dense rank-1 rows
      {
        T dadd = 0;
        struct CU { uint32_t m1, m2; T p[3], U[6]; };
        if constexpr (!WK) for_active_contacts_ld<T, C>(s.con_act, [&](int c) {
          CU v;
          v.m1 = s.con_m1[c]; v.m2 = s.con_m2[c];
          for (int k = 0; k < 3; k++) v.p[k] = s.con_pos[c][k];
          for (int k = 0; k < 6; k++) v.U[k] = s.con_U[c][k];
          return v;
        }, [&](int, const CU& v) {   // (contacts with U = 0 add exact zeros)
          if (v.m1 != 0u || !bit(v.m2, sl)) return;   // body-body: dense rank-1 rows below
          T r[3] = {v.p[0] - s.com[0], v.p[1] - s.com[1], v.p[2] - s.com[2]};
          T w[3];
          cross3(cd, r, w);
          T jp[3] = {cd[3] + w[0], cd[4] + w[1], cd[5] + w[2]};
          const T* U = v.U;
          T z[3] = {U[0] * jp[0] + U[3] * jp[1] + U[4] * jp[2], U[3] * jp[0] + U[1] * jp[1] + U[5] * jp[2],
                    U[4] * jp[0] + U[5] * jp[1] + U[2] * jp[2]};
          T rz[3];
          cross3(r, z, rz);
          for (int k = 0; k < 3; k++) { aug[k] += rz[k]; aug[3 + k] += z[k]; }
        });
        {   // active joint-limit rows of this dof (diagonal)
          int lr = s.lim_row[sl];
          int lo = (lr & 0xff) - 1, hi = (lr >> 8) - 1;
          if (lo >= 0 && s.row_f[lo] != T(0)) dadd += s.row_D[lo];
          if (hi >= 0 && s.row_f[hi] != T(0)) dadd += s.row_D[hi];
        }
        HS_STAMP(clk, 27);
        // HESS_G columns per scheduling group: their cdof rows are read from LDS together, so one
        // LDS round trip is exposed per group instead of per column (A/B, fp64 configs[1] ms per launch:
        // 2 columns 0.720 vs 1 column 0.724, 3 spill; the fp32 engine at 2 waves per SIMD has no
        // registers for a second column: 148 B/lane of scratch)
        constexpr int HESS_G = sizeof(T) == 8 ? 2 : 1;
        if constexpr (HESS_G == 1) {
#pragma unroll
          for (int j = 0; j < NV; j++) {
            T cj[6];
            for (int k = 0; k < 6; k++) cj[k] = s.cdof[j][k];
            H[j] = Mr[j] + (bit(anci, j) ? dot6(cj, aug) : T(0)) + ((j == sl) ? dadd : T(0));
            SCHED_FENCE();
          }
        } else {
          // software-pipelined: group g+1's cdof rows are read before group g's arithmetic (fenced),
          // so each group's LDS round trip overlaps the previous group's FMAs
          constexpr int NG = (NV + HESS_G - 1) / HESS_G;
          T cbuf[2][HESS_G][6];
          auto load = [&](auto gc, T (&dst)[HESS_G][6]) {
            constexpr int j0 = decltype(gc)::value * HESS_G;
            static_for<0, HESS_G>([&](auto tc) {
              constexpr int t = decltype(tc)::value;
              if constexpr (j0 + t < NV)
                for (int k = 0; k < 6; k++) dst[t][k] = s.cdof[j0 + t][k];
            });
          };
          load(std::integral_constant<int, 0>{}, cbuf[0]);
          static_for<0, NG>([&](auto gc) {
            constexpr int g = decltype(gc)::value, j0 = g * HESS_G;
            if constexpr (g + 1 < NG) load(std::integral_constant<int, g + 1>{}, cbuf[(g + 1) & 1]);
            SCHED_FENCE();
            static_for<0, HESS_G>([&](auto tc) {
              constexpr int t = decltype(tc)::value, j = j0 + t;
              if constexpr (j < NV)
                H[j] = Mr[j] + (bit(anci, j) ? dot6(cbuf[g & 1][t], aug) : T(0)) + ((j == sl) ? dadd : T(0));
            });
          });
        }
        HS_STAMP(clk, 28);
        // dense rank-1 rows (tendon limits, body-body contacts): only the rows flagged in
        // dense_mask; the loop runs max(#rows of either half) times (wave-uniform control)
        uint32_t dm[C::RPL];
#pragma unroll
        for (int q = 0; q < C::RPL; q++) dm[q] = s.dense_mask[q] & hballot(act[q], up);   // active ones only
        for (;;) {
          int r = -1;
#pragma unroll
          for (int q = C::RPL - 1; q >= 0; q--)
            if (dm[q]) r = HL * q + __builtin_ctz(dm[q]);
          if (__ballot(r >= 0) == 0) break;
          T jr = 0, Dr = 0;
          if (r >= 0) {
            dm[r / HL] &= dm[r / HL] - 1u;           // consume the row
            if (s.row_f[r] != T(0)) {
              int kid = s.row_kid[r];
              int kind = rk_kind(kid), id = rk_id(kid);
              Dr = s.row_D[r];
              if (kind == RK_TLO || kind == RK_THI) {
                for (int w = 0; w < HS_LT(C, m).ten_nwrap[id]; w++)
                  if (HS_LT(C, m).ten_wrapdof[id][w] == sl) jr += HS_LT(C, m).ten_wrapcoef[id][w];
                if (kind == RK_THI) jr = -jr;
              } else {
                int in2 = bit(s.con_m2[id], sl), in1 = bit(s.con_m1[id], sl);
                if (in1 != in2) {
                  T rr[3] = {s.con_pos[id][0] - s.com[0], s.con_pos[id][1] - s.com[1], s.con_pos[id][2] - s.com[2]};
                  T w[3], u[3];
                  cross3(cd, rr, w);
                  T jp[3] = {cd[3] + w[0], cd[4] + w[1], cd[5] + w[2]};
                  row_u(m, s, kind, id, u);
                  jr = in2 ? dot3(u, jp) : -dot3(u, jp);
                }
              }
            }
          }
          if (sl >= NV) jr = 0;
          T dj = Dr * jr;
          static_for<0, NV>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            H[j] += dj * bcast<j>(jr);
          });
        }
      }
      HS_STAMP(clk, 9);
      chol_rows<NV, T, LDLF>(H, hdinv, sl, s.u.n.cb, &hdiag);   // (LDLF: as L D L')
      HS_STAMP(clk, 15);
      T sdir = -chol_solve<NV, T, LDLF>(H, hdinv, g, sl);
      if (sl >= NV) sdir = 0;
      HS_STAMP(clk, 10);
      // exact line search along sdir (piecewise-quadratic cost)
      if (sl < NV) s.vx[sl] = sdir;
      WSYNC();
      T Ms = matvec_lds(Mr, s.vx);
      T A0 = hsum(sl < NV ? sdir * Ms : T(0));
      T B0 = hsum(sl < NV ? sdir * (Mx - fsmooth) : T(0));
      HS_STAMP(clk, 18);
      map_vx<NV>(s, sl, nb, bch);
      HS_STAMP(clk, 19);
      if constexpr (WK) {
        rows_Jx(m, s, s.vx, vr, rd, rc, Js);
      } else {
#pragma unroll
        for (int q = 0; q < C::RPL; q++) Js[q] = vr[q] ? row_Jx(m, s, rd[q], rc[q]) : T(0);
      }
      HS_STAMP(clk, 16);
      // alpha = 1 is exact when no row changes state on [0, 1] (jar is linear in alpha)
      bool same1 = true;
#pragma unroll
      for (int q = 0; q < C::RPL; q++) same1 = same1 && (!vr[q] || ((jar[q] + Js[q] < 0) == act[q]));
      bool lsdone = done || (hballot(!same1, up) == 0);
      T alpha = 1, lo = 0, hi = T(1e30);
      T d0 = 0;
      {
        T c = 0;
#pragma unroll
        for (int q = 0; q < C::RPL; q++) c += act[q] ? D[q] * jar[q] * Js[q] : T(0);
        d0 = B0 + hsum(c);
      }
      const T ltol = (sizeof(T) == 8 ? T(1e-10) : T(1e-5)) * fabs(d0);
      for (int ls = 0; ls < 30; ls++) {
        if (__ballot(!lsdone) == 0) break;
        T c1 = 0, c2 = 0;
#pragma unroll
        for (int q = 0; q < C::RPL; q++) {
          T jq = jar[q] + alpha * Js[q];
          bool a = vr[q] && jq < 0;
          c1 += a ? D[q] * jq * Js[q] : T(0);
          c2 += a ? D[q] * Js[q] * Js[q] : T(0);
        }
        T d1 = B0 + alpha * A0 + hsum(c1);
        T d2 = A0 + hsum(c2);
        if (!lsdone) {
          if (fabs(d1) <= ltol) {
            lsdone = true;
          } else {
            if (d1 < 0) lo = alpha; else hi = alpha;
            T an = d2 > 0 ? alpha - d1 * recip(d2) : T(-1);
            if (!(an > lo && an < hi)) an = hi < T(1e29) ? T(0.5) * (lo + hi) : T(2) * alpha;
            if (hi - lo <= (sizeof(T) == 8 ? T(1e-14) : T(1e-6)) * hi) lsdone = true;
            else alpha = an;
          }
        }
      }
      HS_STAMP(clk, 11);
      if (!done) {
        x += alpha * sdir;
        Mx += alpha * Ms;
        bool changed = false;
#pragma unroll
        for (int q = 0; q < C::RPL; q++) {
          T nj = jar[q] + alpha * Js[q];
          changed = changed || (vr[q] && ((nj < 0) != act[q]));
          jar[q] = nj;
        }
        if (hballot(changed, up) == 0 && fabs(alpha - T(1)) < T(1e-3)) {
          done = true;
          if (sl == 0) s.niter = it + 1;
        }
      }
      if (__ballot(!done) == 0) { it++; break; }
    }
    WSYNC();
    niter = s.niter;
    // final forces -> qfrc_constraint (recomputed after an exit at the loop's top too, where they are in LDS
    // already: skipping it there measured slower, profiles/newton_walks.md)
#pragma unroll
    for (int q = 0; q < C::RPL; q++)
      if (vr[q]) s.row_f[sl + HL * q] = jar[q] < 0 ? -D[q] * jar[q] : T(0);
    WSYNC();
    contact_aggregates(m, s, sl);
    fcon = sl < NV ? jtf_lane(m, s, sl, cd) : T(0);
    qacc = x;
    WSYNC();
    HS_STAMP(clk, 12);
  }

  // lane (dof) j's entry of constraint row r's Jacobian (the same per-row Jacobians row_Jx applies
  // through body velocities and the Newton Hessian's dense rank-1 terms use)
  __device__ __forceinline__ T row_J_lane(int r) {
    if (sl >= NV) return T(0);
    const int kid = s.row_kid[r];
    const int kind = rk_kind(kid), id = rk_id(kid);
    if (kind <= RK_JHI) return HS_LT(C, m).jnt_dofadr[id] == sl ? (kind == RK_JLO ? T(1) : T(-1)) : T(0);
    if (kind <= RK_THI) {
      T v = 0;
      for (int w = 0; w < HS_LT(C, m).ten_nwrap[id]; w++)
        if (HS_LT(C, m).ten_wrapdof[id][w] == sl) v += HS_LT(C, m).ten_wrapcoef[id][w];
      return kind == RK_TLO ? v : -v;
    }
    const int in2 = bit(s.con_m2[id], sl), in1 = bit(s.con_m1[id], sl);
    if (in1 == in2) return T(0);
    T rr[3] = {s.con_pos[id][0] - s.com[0], s.con_pos[id][1] - s.com[1], s.con_pos[id][2] - s.com[2]};
    T w[3], u[3];
    cross3(cd, rr, w);
    T jp[3] = {cd[3] + w[0], cd[4] + w[1], cd[5] + w[2]};
    row_u(m, s, kind, id, u);
    const T v = dot3(u, jp);
    return in2 ? v : -v;
  }

  // mj_solPGS (<option solver="PGS">), restating oracle/hsim_oracle.c solve_pgs: projected
  // Gauss-Seidel on the dual  min 0.5 f'AR f + f'b, f >= 0  (AR = J M^-1 J' + R, b = J qacc_smooth -
  // aref), rows swept in efc order, MuJoCo's stopping rule (a sweep's improvement * scale <
  // tolerance, or maxit sweeps).  Without forming AR (see PgsCache): with z = L' qacc = L^-1
  // (qfrc_smooth + J'f) kept per dof lane, row r's dual residual is  u_r . z + R_r f_r - aref_r  (z is
  // the NET acceleration in the factor's basis, so fp32 sums do not cancel two large terms) and its
  // update adds delta u_r to z.  The half-wave sum u_r . z runs PGS_LA rows ahead (see PGS_LA).
  // u_r = L^-1 J_r' of the cached rows comes from one multi-right-hand-side forward substitution per
  // substep.  Warm start: the forces of qacc_warmstart under the primal map, kept if their dual cost
  // is not positive.  z is re-anchored on the forces every 8 sweeps (fp32 rounding drift); the final
  // qacc = M^-1 (qfrc_smooth + J'f) comes from the final forces.
  __device__ __forceinline__ void solve_pgs(T xws, int maxit, const T (&D)[C::RPL], const T (&ar)[C::RPL],
                                            const int (&rd)[C::RPL], const T (&rc)[C::RPL], PgsCache<T, C>& pc) {
    phase_begin();
    const int nefc = s.nefc;
    const uint32_t bch = chain_mask<C>(m, sl, nb);
    const T fs = sl < NV ? fsmooth : T(0);
    constexpr int NC = PgsCache<T, C>::NC;
    constexpr int LA = PGS_LA;
    bool vr[C::RPL];
#pragma unroll
    for (int q = 0; q < C::RPL; q++) vr[q] = sl + HL * q < nefc;
    T L[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) L[j] = Mr[j];
    T dinv = 0;
    chol_rows<NV>(L, dinv, sl, s.u.n.cb);
    // warm start: f = -D (J xws - aref)_-;  per-row b_r = -aref_r, R_r
    if (sl < NV) s.vx[sl] = xws;
    WSYNC();
    map_vx<NV>(s, sl, nb, bch);
    T wc = 0;     // this lane's rows' part of the warm start's dual cost: sum f (0.5 R f - aref)
#pragma unroll
    for (int q = 0; q < C::RPL; q++) {
      const int r = sl + HL * q;
      if (vr[q]) {
        const T jar = row_Jx(m, s, rd[q], rc[q]) - ar[q];
        const T f = jar < 0 ? -D[q] * jar : T(0);
        const T R = recip(D[q]);
        s.row_f[r] = f;
        pc.row[r].b = -ar[q];
        pc.row[r].R = R;
        wc += f * (T(0.5) * R * f - ar[q]);
      }
    }
    WSYNC();
    // rows that exist in either half of the wave (wave-uniform loop bounds)
    int maxr = nefc;
    maxr = max(maxr, __shfl_xor(maxr, HL));
    // u_r of the cached rows (G right-hand sides per forward substitution)
    constexpr int G = sizeof(T) == 8 ? 4 : 8;
    const int ncache = maxr < NC ? maxr : NC;
    for (int r0 = 0; r0 < ncache; r0 += G) {
      T y[G];
      static_for<0, G>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        y[g] = r0 + g < nefc ? row_J_lane(r0 + g) : T(0);
      });
      chol_fwd_multi<NV, G>(L, dinv, y, sl);
      static_for<0, G>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if (r0 + g < NC) pc.u[r0 + g][sl] = sl < NV ? y[g] : T(0);   // MAXDOF == HL: a slot per sub-lane
      });
    }
    WSYNC();
    // u_r of any row (LDS cache, or rebuilt for rows past it; 0 past the half's rows)
    auto urow = [&](int r) -> T {
      if (r < NC) return pc.u[r][sl];
      T y = chol_fwd<NV>(L, dinv, r < nefc ? row_J_lane(r) : T(0), sl);
      return sl < NV ? y : T(0);
    };
    // AR_rr = |u_r|^2 + R_r and the lookahead Gram terms of every row
    {
      T uw[LA + 1];     // u_{r-LA} .. u_r
#pragma unroll
      for (int j = 0; j < LA; j++) uw[j] = 0;
      for (int r = 0; r < maxr; r++) {
        uw[LA] = urow(r);
        const T a = hsum(uw[LA] * uw[LA]);
        T gr[LA];
#pragma unroll
        for (int j = 1; j <= LA; j++) gr[j - 1] = hsum(uw[LA] * uw[LA - j]);
        if (r < nefc && sl == 0) {
          const T arr = a + pc.row[r].R;
          pc.row[r].ar = arr;
          pc.row[r].ai = recip(arr < T(1e-15) ? T(1e-15) : arr);
#pragma unroll
          for (int j = 0; j < LA; j++) pc.row[r].g[j] = gr[j];
        }
#pragma unroll
        for (int j = 0; j < LA; j++) uw[j] = uw[j + 1];
      }
    }
    WSYNC();
    // y0 = L^-1 qfrc_smooth and z = L^-1 (qfrc_smooth + J'f) of the warm-start forces
    contact_aggregates(m, s, sl);
    T z, y0;
    {
      T y2[2] = {fs, fs + (sl < NV ? jtf_lane(m, s, sl, cd) : T(0))};
      chol_fwd_multi<NV, 2>(L, dinv, y2, sl);
      y0 = sl < NV ? y2[0] : T(0);
      z = sl < NV ? y2[1] : T(0);
    }
    // keep the warm start only if its dual cost 0.5 f'AR f + f'b = 0.5 |z|^2 - 0.5 |y0|^2 +
    // sum f (0.5 R f - aref) is not positive
    if (hsum(wc + T(0.5) * (z * z - y0 * y0)) > T(0)) {
#pragma unroll
      for (int q = 0; q < C::RPL; q++)
        if (vr[q]) s.row_f[sl + HL * q] = 0;
      z = y0;
    }
    WSYNC();
    const T scale = m->newton_scale, tol = m->pgs_tol;
    bool done = false;
    int it = 0;
    for (int sweep = 0; sweep < maxit; sweep++) {
      m = opaque(m);
      sl = opaque_v(sl);
      T improvement = 0;
      // ring registers (slot = row mod RING, RING = LA + 1; the row loop is unrolled by RING so every
      // slot index is a compile-time constant and the pipeline shifts no registers):
      // U[slot] = u_row, S[slot] = u_row . z_{row-LA-1} (z with rows < row-LA applied),
      // Dl[slot] = delta_row.  At row r, z still lacks row r-1's update.  Positions past maxr are
      // phantom rows (u = 0, delta = 0).
      // LDS operands are loaded one row before their use (P/F: row r+1's scalars and force, un: u of
      // row r+LA+1), so no row waits on an LDS round trip (a wave issues in order: a load consumed
      // in the same row would stall it for the full LDS latency); loads are unconditional (clamped
      // index, masked value) so the row step has no divergent branch.
      // FAST: every row of both halves is in the u cache (the common case), no rebuild path.
      auto sweep_rows = [&](auto fastc) {
        constexpr bool FAST = decltype(fastc)::value;
        auto uget = [&](int r) -> T {
          if constexpr (FAST) return pc.u[r][sl];
          else return urow(r);
        };
        constexpr int RING = LA + 1;
        static_assert(RING % 2 == 0, "P/F double buffer alternates with the row parity");
        T U[RING], S[RING], Dl[RING];
#pragma unroll
        for (int i = 0; i < RING; i++) {
          U[i] = (i < LA && i < maxr) ? uget(i) : T(0);
          S[i] = i < LA ? hsum(U[i] * z) : T(0);
          Dl[i] = 0;
        }
        PgsRow<T> P[2];
        T F[2];
        P[0] = pc.row[0];
        F[0] = nefc > 0 ? s.row_f[0] : T(0);
        T unext = LA < maxr ? uget(LA) : T(0);
        for (int r0 = 0; r0 < maxr; r0 += RING) {
          static_for<0, RING>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            constexpr int prev = (i + RING - 1) % RING;   // slot of row r-1 (and of row r+LA)
            constexpr int cur = i & 1, nxt = cur ^ 1;
            const int r = r0 + i;
            {   // next row's operands
              const int rn = r + 1 < C::EFC ? r + 1 : C::EFC - 1;
              P[nxt] = pc.row[rn];
              const T fl = s.row_f[rn];
              F[nxt] = r + 1 < nefc ? fl : T(0);
            }
            const T un = unext;                          // u_{r+LA}
            unext = r + LA + 1 < maxr ? uget(r + LA + 1) : T(0);
            z = fma(Dl[prev], U[prev], z);               // z_{r-1}: rows < r applied
            const T Sn = hsum(un * z);                   // start row r+LA's sum on z_{r-1}
            const bool row = r < nefc;
            const bool live = row && !done;
            const PgsRow<T>& pr = P[cur];
            const T fr = F[cur];
            T dot = S[i];
            static_for<1, LA + 1>([&](auto jc) {         // corrections for rows r-1 .. r-LA
              constexpr int j = decltype(jc)::value;
              dot = fma(Dl[(i + RING - j) % RING], pr.g[j - 1], dot);
            });
            const T res = dot + (pr.b + pr.R * fr);
            T nf = fr - res * pr.ai;
            nf = nf < T(0) ? T(0) : nf;
            const T delta = live ? nf - fr : T(0);
            const T di = delta * res + T(0.5) * pr.ar * delta * delta;
            improvement -= row ? di : T(0);
            if (live && sl == 0) s.row_f[r] = nf;
            U[prev] = un;                                // row r+LA takes row r-1's slot
            S[prev] = Sn;
            Dl[i] = delta;
          });
        }
        z = fma(Dl[RING - 1], U[RING - 1], z);           // the last position's update (0 if phantom)
      };
      if (maxr <= NC) sweep_rows(std::true_type{});
      else sweep_rows(std::false_type{});
      if (!done) it++;
      done = done || (improvement * scale < tol);
      if (__ballot(!done) == 0) break;
      // re-anchor z on the current forces (fp32: every 8 sweeps; fp64 drifts ~1e-16 per update)
      if ((sweep & (sizeof(T) == 8 ? 31 : 7)) == (sizeof(T) == 8 ? 31 : 7)) {
        WSYNC();
        contact_aggregates(m, s, sl);
        const T zz = chol_fwd<NV>(L, dinv, fs + (sl < NV ? jtf_lane(m, s, sl, cd) : T(0)), sl);
        z = sl < NV ? zz : T(0);
      }
    }
    niter = it;
    WSYNC();
    contact_aggregates(m, s, sl);
    fcon = sl < NV ? jtf_lane(m, s, sl, cd) : T(0);
    const T qa = chol_solve<NV>(L, dinv, fs + fcon, sl);     // M^-1 (qfrc_smooth + J'f)
    qacc = sl < NV ? qa : T(0);
    WSYNC();
  }

  // full_state: contact part of mj_rnePostConstraint (cfrc_ext, at the root subtree com: body 2 of a
  // contact gets +[(p - com) x F, F], body 1 the opposite, world skipped) and mj_subtreeVel's linear
  // part (m v_com of every body = m lin + ang x (m d) from cvel / cinert, summed over subtrees).
  // Results stay in the Newton union (free after the solve) until obs / reward / commit read them.
  __device__ __forceinline__ void post_constraint() {
    phase_begin();
    const int b = sl;
    T cf[6] = {0, 0, 0, 0, 0, 0}, mv[3] = {0, 0, 0};
    if (b > 0 && b < nb) {
      for (int c = 0; c < s.ncon; c++) {
        const uint32_t bb = s.con_bb[c];
        const int b1 = bb & 0xff, b2 = (bb >> 8) & 0xff;
        if (b != b1 && b != b2) continue;
        const T sg = b == b2 ? T(1) : T(-1);
        T r[3] = {s.con_pos[c][0] - s.com[0], s.con_pos[c][1] - s.com[1], s.con_pos[c][2] - s.com[2]}, t[3];
        cross3(r, s.con_F[c], t);
        for (int k = 0; k < 3; k++) { cf[k] += sg * t[k]; cf[3 + k] += sg * s.con_F[c][k]; }
      }
      const T* ci = s.cinert[b];
      const T* cv = s.cvel[b];
      T w[3];
      cross3(cv, ci + 6, w);
      for (int k = 0; k < 3; k++) mv[k] = ci[9] * cv[3 + k] + w[k];
    }
    if (b < nb) {
      for (int k = 0; k < 6; k++) s.u.n.cfrc[b][k] = cf[k];
      for (int k = 0; k < 3; k++) s.u.n.mv[b][k] = mv[k];
    }
    WSYNC();
    if (b < nb) {
      const uint32_t dm = b == 0 ? ((1u << nb) - 2u) : HS_LT(C, m).body_descmask[b];
      T a[3] = {0, 0, 0}, ms = 0;
      if constexpr (C::GROUPS) {   // the same two sums over the subtree's bodies, ascending, a group per round trip
        for_bits_g<C, G_POST, T>(dm & ~1u & ((nb < 32 ? (1u << nb) : 0u) - 1u),
                   [&](int c) { Vals<T, 4> r; for (int k = 0; k < 3; k++) r.v[k] = s.u.n.mv[c][k]; r.v[3] = s.cinert[c][9]; return r; },
                   [&](int, const Vals<T, 4>& r) { for (int k = 0; k < 3; k++) a[k] += r.v[k]; ms += r.v[3]; });
      } else {
        for (int c = 1; c < nb; c++)
          if (bit(dm, c)) {
            for (int k = 0; k < 3; k++) a[k] += s.u.n.mv[c][k];
            ms += s.cinert[c][9];
          }
      }
      const T inv = T(1) / (ms > T(1e-15) ? ms : T(1e-15));
      for (int k = 0; k < 3; k++) s.u.n.linv[b][k] = a[k] * inv;
    }
    WSYNC();
  }

  // mj_Euler with implicit damping, mj_integratePos
  __device__ __forceinline__ void euler(T& time) {
    phase_begin();
    T h = m->timestep;
    T He[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) He[j] = Mr[j] + ((j == sl) ? h * damp : T(0));
    HS_STAMP(clk, 20);
    T edinv = 0, ediag = 0;
    chol_rows<NV, T, LDLE>(He, edinv, sl, s.u.n.cb, &ediag);
    HS_STAMP(clk, 21);
    T a = chol_solve<NV, T, LDLE>(He, edinv, fsmooth + fcon, sl);
    HS_STAMP(clk, 17);
    if (sl < NV) s.qvel[sl] += h * a;
    WSYNC();
    if (sl < m->njnt) {
      int qa = HS_LT(C, m).jnt_qposadr[sl], da = HS_LT(C, m).jnt_dofadr[sl];
      if (HS_LT(C, m).jnt_type[sl] == JNT_FREE) {
        for (int k = 0; k < 3; k++) s.qpos[qa + k] += h * s.qvel[da + k];
        T w[3] = {s.qvel[da + 3], s.qvel[da + 4], s.qvel[da + 5]};
        T ang = h * normalize3(w);
        T sn, cs;
        sincos_t(T(0.5) * ang, sn, cs);
        T qr[4] = {cs, w[0] * sn, w[1] * sn, w[2] * sn};
        T q[4] = {s.qpos[qa + 3], s.qpos[qa + 4], s.qpos[qa + 5], s.qpos[qa + 6]};
        normalize4(q);
        mulq(q, qr, q);
        for (int k = 0; k < 4; k++) s.qpos[qa + 3 + k] = q[k];
      } else {
        s.qpos[qa] += h * s.qvel[da];
      }
    }
    time += h;
    WSYNC();
  }
};

}  // namespace
}  // namespace hs
