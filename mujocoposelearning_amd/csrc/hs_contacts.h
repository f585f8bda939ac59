// Contacts and constraint rows: the narrow phase (mjc_PlaneSphere / PlaneCapsule / SphereSphere /
// SphereCapsule / CapsuleCapsule, mju_makeFrame), solimp impedance (mj_makeImpedance), J x for all
// rows through body velocities, per-contact force aggregates and J' f (mj_mulJacVec / mj_mulJacTVec
// in the tree-structured form).
#pragma once
#include "hs_lanes.h"
#include "hs_scratch.h"

namespace hs {
namespace {

// ------------------------------------------------------------------ narrow phase
template <typename T>
struct Con {
  T pos[3], n[3], t1[3], dist;
};

template <typename T>
__device__ __forceinline__ bool plane_sphere(const T* pp, const T* pn, const T* c, T r, Con<T>& o) {
  T d[3] = {c[0] - pp[0], c[1] - pp[1], c[2] - pp[2]};
  T cd = dot3(d, pn);
  if (cd > r) return false;
  o.dist = cd - r;
  for (int k = 0; k < 3; k++) { o.n[k] = pn[k]; o.pos[k] = c[k] - pn[k] * (o.dist * T(0.5) + r); o.t1[k] = 0; }
  return true;
}
template <typename T>
__device__ __forceinline__ bool sphere_sphere(const T* p1, T r1, const T* p2, T r2, Con<T>& o) {
  T d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  T len = sqrt(dot3(d, d));
  T dist = len - r1 - r2;
  if (dist > 0) return false;
  o.dist = dist;
  if (len < T(1e-15)) { o.n[0] = 1; o.n[1] = 0; o.n[2] = 0; }
  else { T i = recip(len); for (int k = 0; k < 3; k++) o.n[k] = d[k] * i; }
  for (int k = 0; k < 3; k++) { o.pos[k] = p1[k] + o.n[k] * (r1 + dist * T(0.5)); o.t1[k] = 0; }
  return true;
}
// mju_makeFrame: complete (n, t1 hint) -> orthonormal t1
template <typename T>
__device__ __forceinline__ void make_frame(Con<T>& c) {
  normalize3(c.n);
  if (sqrt(dot3(c.t1, c.t1)) < T(0.5)) {
    if (fabs(c.n[1]) < T(0.5)) { c.t1[0] = 0; c.t1[1] = 1; c.t1[2] = 0; }
    else { c.t1[0] = 0; c.t1[1] = 0; c.t1[2] = 1; }
  }
  T d = dot3(c.n, c.t1);
  for (int k = 0; k < 3; k++) c.t1[k] -= c.n[k] * d;
  normalize3(c.t1);
}

// number of contacts (0..2) for static pair p (mjc_* primitives)
template <typename T, typename C>
__device__ __forceinline__ int collide_pair(const Scratch<T, C>& s, const int4 info, const T (&sz)[4], Con<T>& c0,
                                           Con<T>& c1) {
  const int g1 = info.x, g2 = info.y, fn = info.z;
  const T* p1 = HS_KTAIL(s).gpos[g1];
  const T* p2 = HS_KTAIL(s).gpos[g2];
  const T* a1 = HS_KTAIL(s).gax[g1];
  const T* a2 = HS_KTAIL(s).gax[g2];
  const T r1 = sz[0], h1 = sz[1], r2 = sz[2], h2 = sz[3];
  int n = 0;
  if (fn >= PAIR_SPHERE_SPHERE) {
    // bounding spheres (radius + half-length, MuJoCo's geom_rbound) apart: no contact.  Exact (a
    // contact needs dist <= 0 between the geoms, inside both bounds), so only a shortcut -- and when
    // no lane of the wave holds a near pair, the wave skips the capsule-capsule branch altogether
    const T d[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
    const T R = r1 + h1 + r2 + h2;
    if (dot3(d, d) > R * R) return 0;
  }
  if (fn == PAIR_PLANE_SPHERE) {
    n = plane_sphere(p1, a1, p2, r2, c0) ? 1 : 0;
  } else if (fn == PAIR_PLANE_CAPSULE) {
    T e[3];
    for (int k = 0; k < 3; k++) e[k] = p2[k] + h2 * a2[k];
    Con<T> t;
    if (plane_sphere(p1, a1, e, r2, t)) { for (int k = 0; k < 3; k++) t.t1[k] = a2[k]; c0 = t; n = 1; }
    for (int k = 0; k < 3; k++) e[k] = p2[k] - h2 * a2[k];
    if (plane_sphere(p1, a1, e, r2, t)) {
      for (int k = 0; k < 3; k++) t.t1[k] = a2[k];
      if (n == 0) c0 = t; else c1 = t;
      n++;
    }
  } else if (fn == PAIR_SPHERE_SPHERE) {
    n = sphere_sphere(p1, r1, p2, r2, c0) ? 1 : 0;
  } else if (fn == PAIR_SPHERE_CAPSULE) {
    T d[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
    T x = dot3(a2, d);
    x = x > h2 ? h2 : (x < -h2 ? -h2 : x);
    T v[3] = {p2[0] + x * a2[0], p2[1] + x * a2[1], p2[2] + x * a2[2]};
    n = sphere_sphere(p1, r1, v, r2, c0) ? 1 : 0;
  } else {   // capsule-capsule (mjc_CapsuleCapsule)
    T ax1[3] = {a1[0] * h1, a1[1] * h1, a1[2] * h1}, ax2[3] = {a2[0] * h2, a2[1] * h2, a2[2] * h2};
    T dif[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
    T ma = dot3(ax1, ax1), mb = -dot3(ax1, ax2), mc = dot3(ax2, ax2), u = -dot3(ax1, dif), v = dot3(ax2, dif);
    T det = ma * mc - mb * mb;
    T v1[3], v2[3];
    if (fabs(det) >= T(1e-15)) {
      T x1 = (mc * u - mb * v) / det, x2 = (ma * v - mb * u) / det;
      if (x1 > 1) { x1 = 1; x2 = (v - mb) / mc; }
      else if (x1 < -1) { x1 = -1; x2 = (v + mb) / mc; }
      if (x2 > 1) { x2 = 1; x1 = (u - mb) / ma; x1 = x1 > 1 ? 1 : (x1 < -1 ? -1 : x1); }
      else if (x2 < -1) { x2 = -1; x1 = (u + mb) / ma; x1 = x1 > 1 ? 1 : (x1 < -1 ? -1 : x1); }
      for (int k = 0; k < 3; k++) { v1[k] = p1[k] + x1 * ax1[k]; v2[k] = p2[k] + x2 * ax2[k]; }
      n = sphere_sphere(v1, r1, v2, r2, c0) ? 1 : 0;
    } else {
      for (int side = 1; side >= -1; side -= 2) {
        T x2 = (v - side * mb) / mc;
        x2 = x2 > 1 ? 1 : (x2 < -1 ? -1 : x2);
        for (int k = 0; k < 3; k++) { v1[k] = p1[k] + side * ax1[k]; v2[k] = p2[k] + x2 * ax2[k]; }
        Con<T> t;
        if (sphere_sphere(v1, r1, v2, r2, t)) { if (n == 0) c0 = t; else c1 = t; n++; }
      }
    }
  }
  if (n > 0) make_frame(c0);
  if (n > 1) make_frame(c1);
  return n;
}

template <typename T, typename C>
__device__ __forceinline__ void store_contact(MPtr<T> m, Scratch<T, C>& s, int slot, const Con<T>& c, int p) {
  if (slot >= C::CON) return;
  for (int k = 0; k < 3; k++) { s.con_pos[slot][k] = c.pos[k]; s.con_n[slot][k] = c.n[k]; s.con_t1[slot][k] = c.t1[k]; }
  s.con_dist[slot] = c.dist;
  s.con_pair[slot] = p;
  const int b1 = m->pair_b1[p], b2 = m->pair_b2[p];
  s.con_bb[slot] = (uint32_t)b1 | (uint32_t)b2 << 8 | (uint32_t)m->pair_dim[p] << 16;
  s.con_m1[slot] = b1 ? HS_LT(C, m).body_chainmask[b1] : 0u;
  s.con_m2[slot] = HS_LT(C, m).body_chainmask[b2];
  s.con_mu[slot] = m->pair_mu[p];
}

// Near-pair list entry of the C::NEAR collision: pair | g1 << 8 | g2 << 16 | fn << 24.
static_assert(MAXPAIR <= 256 && MAXGEOM <= 256 && PAIR_CAPSULE_CAPSULE < 256, "near-pair entry: one byte per field");
__device__ __forceinline__ uint32_t near_entry(int p, int g1, int g2, int fn) {
  return (uint32_t)p | (uint32_t)g1 << 8 | (uint32_t)g2 << 16 | (uint32_t)fn << 24;
}
// store_contact for a lane that holds its pair's geoms, condim and friction already: the pair's bodies are
// its geoms' (pair_b1 / pair_b2 are geom_bodyid[g1] / [g2], mjcf.cpp), read from the lane table
template <typename T, typename C>
__device__ __forceinline__ void store_contact_near(MPtr<T> m, Scratch<T, C>& s, int slot, const Con<T>& c, int p,
                                                   int g1, int g2, int dim, T mu) {
  if (slot >= C::CON) return;
  for (int k = 0; k < 3; k++) { s.con_pos[slot][k] = c.pos[k]; s.con_n[slot][k] = c.n[k]; s.con_t1[slot][k] = c.t1[k]; }
  s.con_dist[slot] = c.dist;
  s.con_pair[slot] = p;
  const int b1 = lanes<C>(m).geom_bodyid[g1], b2 = lanes<C>(m).geom_bodyid[g2];
  s.con_bb[slot] = (uint32_t)b1 | (uint32_t)b2 << 8 | (uint32_t)dim << 16;
  s.con_m1[slot] = b1 ? lanes<C>(m).body_chainmask[b1] : 0u;
  s.con_m2[slot] = lanes<C>(m).body_chainmask[b2];
  s.con_mu[slot] = mu;
}

// impedance (mj_makeImpedance getimpedance), MuJoCo clamps d0/dmax to [1e-4, 0.9999].  The sigmoid
// y = x^p / mid^(p-1) (x <= mid) or 1 - (1-x)^p / (1-mid)^(p-1) takes its constant denominators from
// the model (si[5..7], fill_solimp) and one pow, skipped for the default power 2.
template <typename T>
__device__ __forceinline__ T impedance(CPtr<T> si, T pos, T margin) {
  T s0 = fmin(T(0.9999), fmax(T(0.0001), si[0])), s1 = fmin(T(0.9999), fmax(T(0.0001), si[1]));
  if (s0 == s1 || si[2] <= T(1e-15)) return T(0.5) * (s0 + s1);
  T x = (pos - margin) * si[5];
  if (x < 0) x = -x;
  if (x >= 1 || x <= 0) return x >= 1 ? s1 : s0;
  const T p = si[4];
  T y = x;
  if (p != T(1)) {
    const bool lo = x <= si[3];
    const T base = lo ? x : 1 - x;
    T pw = base * base;
    if (p != T(2)) pw = pow(base, p);
    y = lo ? pw * si[6] : 1 - pw * si[7];
  }
  return s0 + y * (s1 - s0);
}

// ------------------------------------------------------------------ J x for all rows
// s.vx (generalized vector) -> body spatial velocities -> contact frame velocities
// ch: this body lane's dof chain mask (body_chainmask, 0 for the world), loaded by the caller
template <typename C, typename T>
__device__ __forceinline__ uint32_t chain_mask(MPtr<T> m, int sl, int nb) {
  return (sl > 0 && sl < nb) ? HS_LT(C, m).body_chainmask[sl] : 0u;
}
// contact-frame velocities con_v of this lane's contact slots from the body spatial velocities bv
template <typename T, typename C>
__device__ __forceinline__ void contact_vel(Scratch<T, C>& s, int sl, const T (*bv)[6]) {
#pragma unroll
  for (int cs = 0; cs < C::CON; cs += HL) {   // contact slots of this lane (one per lane in the resident tier)
    const int c = cs + sl;
    if (c < s.ncon) {
      const uint32_t bb = s.con_bb[c];
      const int b1 = bb & 0xff, b2 = (bb >> 8) & 0xff;
      T r[3] = {s.con_pos[c][0] - s.com[0], s.con_pos[c][1] - s.com[1], s.con_pos[c][2] - s.com[2]};
      T w[3], v1[3], v2[3];
      cross3(bv[b2], r, w);
      for (int k = 0; k < 3; k++) v2[k] = bv[b2][3 + k] + w[k];
      cross3(bv[b1], r, w);
      for (int k = 0; k < 3; k++) v1[k] = bv[b1][3 + k] + w[k];
      T dv[3] = {v2[0] - v1[0], v2[1] - v1[1], v2[2] - v1[2]};
      T t2[3];
      cross3(s.con_n[c], s.con_t1[c], t2);
      s.con_v[c][0] = dot3(s.con_n[c], dv);
      s.con_v[c][1] = dot3(s.con_t1[c], dv);
      s.con_v[c][2] = dot3(t2, dv);
    }
  }
  WSYNC();
}
template <int NV, typename T, typename C>
__device__ __forceinline__ void map_vx(Scratch<T, C>& s, int sl, int nb, uint32_t ch) {
  if (sl < nb) {   // body spatial velocity = sum over the body's dof chain of cdof_j x_j
    T v[6] = {0, 0, 0, 0, 0, 0};
    // the chain's dofs only, ascending: the same sum as over all dofs (the skipped terms are exact
    // zeros), ~half the fp64 FMAs (fp64 0.866 -> 0.812 ms per launch)
    HS_FOR_BITS(C, G_VX, T)(ch, [&](int j) { ValsX<T, 6> r; r.x = s.vx[j]; for (int k = 0; k < 6; k++) r.v[k] = s.cdof[j][k]; return r; },
                [&](int, const ValsX<T, 6>& r) {
#pragma unroll
                  for (int k = 0; k < 6; k++) v[k] = fma(r.v[k], r.x, v[k]);
                });
    for (int k = 0; k < 6; k++) s.u.n.bvel[sl][k] = v[k];
  }
  WSYNC();
  contact_vel(s, sl, s.u.n.bvel);
}
// map_vx's first stage for two generalized vectors in one walk of the chain (rows() of the C::WALKS instances):
// s.qvel -> u.n.bvel and s.vx -> u.n.cfrc, each cdof row read once, each sum with map_vx's ascending FMAs.
// u.n.cfrc has bvel's shape and is dead here: post_constraint writes it after the solve (hs_scratch.h).
template <int NV, typename T, typename C>
__device__ __forceinline__ void chain_vel2(Scratch<T, C>& s, int sl, int nb, uint32_t ch) {
  struct V2 { T x, y; T v[6]; };
  if (sl < nb) {
    T v[6] = {0, 0, 0, 0, 0, 0}, u[6] = {0, 0, 0, 0, 0, 0};
    for_bits_g<C, G_VX, T>(ch, [&](int j) { V2 r; r.x = s.qvel[j]; r.y = s.vx[j]; for (int k = 0; k < 6; k++) r.v[k] = s.cdof[j][k]; return r; },
                           [&](int, const V2& r) {
#pragma unroll
                             for (int k = 0; k < 6; k++) { v[k] = fma(r.v[k], r.x, v[k]); u[k] = fma(r.v[k], r.y, u[k]); }
                           });
    for (int k = 0; k < 6; k++) { s.u.n.bvel[sl][k] = v[k]; s.u.n.cfrc[sl][k] = u[k]; }
  }
  WSYNC();
}

// Row descriptor kept in registers by the row's lane for the whole solve (no LDS / model
// lookups per use): desc = kind << 16 | j with j = dof (joint limits), tendon id or contact id;
// coef = +-1 (limits), +-mu (pyramid rows), 0 (frictionless contact normal).
template <typename T, typename C>
__device__ __forceinline__ T row_Jx(MPtr<T> m, const Scratch<T, C>& s, int desc, T coef) {
  int kind = rk_kind(desc), j = rk_id(desc);
  if (kind <= RK_JHI) return coef * s.vx[j];
  if (kind <= RK_THI) {
    T v = 0;
    for (int w = 0; w < HS_LT(C, m).ten_nwrap[j]; w++) v += HS_LT(C, m).ten_wrapcoef[j][w] * s.vx[HS_LT(C, m).ten_wrapdof[j][w]];
    return coef * v;
  }
  int comp = kind == RK_CN ? 1 : 1 + ((kind - RK_P0) >> 1);
  return s.con_v[j][0] + coef * s.con_v[j][comp];
}

// row_Jx for all of a lane's row slots at once (the C::WALKS instances): every slot's two LDS operands are
// read first -- xv[j] twice for a joint row, con_v[j][0] and con_v[j][comp] for a contact row -- behind one
// scheduling fence, then each slot's value is formed from them by its kind's expression of row_Jx, so the
// slots share one LDS round trip where the calls one after the other wait for one each.  Tendon rows keep
// row_Jx's loop under a wave-uniform test (no lane of humanoid.xml's usual step holds one).  xv: the
// generalized vector the body velocities behind con_v were summed from (s.vx, or s.qvel in rows()).
template <typename T, typename C>
__device__ __forceinline__ void rows_Jx(MPtr<T> m, const Scratch<T, C>& s, const T* xv, const bool (&vr)[C::RPL],
                                        const int (&rd)[C::RPL], const T (&rc)[C::RPL], T (&out)[C::RPL]) {
  T a[C::RPL], b[C::RPL];
  bool ten = false;
#pragma unroll
  for (int q = 0; q < C::RPL; q++) {
    const int kind = rk_kind(rd[q]), j = rk_id(rd[q]);
    const bool con = kind >= RK_CN;
    const int comp = kind == RK_CN ? 1 : 1 + ((kind - RK_P0) >> 1);
    const T* p0 = con ? &s.con_v[j][0] : &xv[j];     // (a tendon or an empty slot reads xv[id]: in bounds, unused)
    const T* p1 = con ? &s.con_v[j][comp] : p0;
    a[q] = *p0;
    b[q] = *p1;
    ten = ten || (vr[q] && kind >= RK_TLO && kind <= RK_THI);
  }
  SCHED_FENCE();
#pragma unroll
  for (int q = 0; q < C::RPL; q++) {
    const T cv = fma(rc[q], b[q], a[q]), jv = rc[q] * a[q];
    out[q] = vr[q] ? (rk_kind(rd[q]) >= RK_CN ? cv : jv) : T(0);
  }
  if (__ballot(ten) != 0) {
#pragma unroll
    for (int q = 0; q < C::RPL; q++) {
      const int kind = rk_kind(rd[q]), j = rk_id(rd[q]);
      if (vr[q] && kind >= RK_TLO && kind <= RK_THI) {
        T v = 0;
        for (int w = 0; w < HS_LT(C, m).ten_nwrap[j]; w++) v += HS_LT(C, m).ten_wrapcoef[j][w] * xv[HS_LT(C, m).ten_wrapdof[j][w]];
        out[q] = rc[q] * v;
      }
    }
  }
}

// world-frame force direction u of a contact row
template <typename T, typename C>
__device__ __forceinline__ void row_u(MPtr<T> m, const Scratch<T, C>& s, int kind, int c, T* u) {
  if (kind == RK_CN) { for (int k = 0; k < 3; k++) u[k] = s.con_n[c][k]; return; }
  int sub = kind - RK_P0;
  T mu = s.con_mu[c];
  T sg = (sub & 1) ? -mu : mu;
  T t[3];
  if (sub >> 1) cross3(s.con_n[c], s.con_t1[c], t);
  else { t[0] = s.con_t1[c][0]; t[1] = s.con_t1[c][1]; t[2] = s.con_t1[c][2]; }
  for (int k = 0; k < 3; k++) u[k] = s.con_n[c][k] + sg * t[k];
}

// per-contact aggregates from current row forces: U = sum D u u' (active rows), F = sum f u
// and the mask of contacts whose force is nonzero (the others add exact zeros to J'f and the Newton
// Hessian, so those loops skip them)
template <typename T, typename C>
__device__ __forceinline__ void contact_aggregates(MPtr<T> m, Scratch<T, C>& s, int sl) {
  const bool up = threadIdx.x >= HL;
#pragma unroll
  for (int cs = 0; cs < C::CON; cs += HL) {
    const int c = cs + sl;
    bool act = false;
    if (c < s.ncon) {
      int adr = s.con_adr[c];
      int nr = (s.con_bb[c] >> 16) == 1 ? 1 : 4;
      T U[6] = {0, 0, 0, 0, 0, 0}, F[3] = {0, 0, 0};
      // straight-line over the (at most 4) rows: every LDS operand is read up front (one round trip),
      // then the same sums in the same order as a row loop whose every iteration waits on its own reads
      // (fp64 0.662 -> 0.634 ms per configs[1] launch)
      const bool pyr = nr == 4;
      T f4[4], D4[4], nn[3], t1[3], t2[3];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const bool on = q == 0 || pyr;
        f4[q] = on ? s.row_f[adr + q] : T(0);
        D4[q] = on ? s.row_D[adr + q] : T(0);
      }
      for (int k = 0; k < 3; k++) { nn[k] = s.con_n[c][k]; t1[k] = s.con_t1[c][k]; }
      const T mu = s.con_mu[c];
      cross3(nn, t1, t2);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const T f = f4[q];
        if (f != T(0)) {
          T u[3];
          if (!pyr) {
            for (int k = 0; k < 3; k++) u[k] = nn[k];
          } else {
            const T sg = (q & 1) ? -mu : mu;
            for (int k = 0; k < 3; k++) u[k] = nn[k] + sg * ((q >> 1) ? t2[k] : t1[k]);
          }
          const T D = D4[q];
          U[0] += D * u[0] * u[0]; U[1] += D * u[1] * u[1]; U[2] += D * u[2] * u[2];
          U[3] += D * u[0] * u[1]; U[4] += D * u[0] * u[2]; U[5] += D * u[1] * u[2];
          for (int k = 0; k < 3; k++) F[k] += f * u[k];
        }
      }
      for (int k = 0; k < 6; k++) s.con_U[c][k] = U[k];
      for (int k = 0; k < 3; k++) s.con_F[c][k] = F[k];
      act = F[0] != T(0) || F[1] != T(0) || F[2] != T(0) || U[0] != T(0) || U[1] != T(0) || U[2] != T(0);
    }
    const uint32_t mk = hballot(act, up);
    if (sl == 0) s.con_act[cs / HL] = mk;
  }
  WSYNC();
}
// for each contact c with a nonzero force, in contact order: f(c)
template <typename C, typename F>
__device__ __forceinline__ void for_active_contacts(const uint32_t* act, F&& f) {
#pragma unroll
  for (int w = 0; w < (C::CON + HL - 1) / HL; w++)
    for (uint32_t mk = act[w]; mk; mk &= mk - 1u) f(w * HL + __builtin_ctz(mk));
}

// the same with every per-contact LDS operand read by ld(c) in one batch (one round trip per
// contact instead of a read, a branch on it and dependent reads; HS_CONTACT_FLAT) and the next
// contact's reads issued before the current contact's arithmetic (HS_CONTACT_AHEAD): J'f and the
// Hessian's contact terms.  A/B, fp64 ms per configs[1] launch: 0.635 -> flat 0.634 -> + ahead 0.632.
template <typename T, typename C, typename LD, typename F>
__device__ __forceinline__ void for_active_contacts_ld(const uint32_t* act, LD&& ld, F&& f) {
#pragma unroll
  for (int w = 0; w < (C::CON + HL - 1) / HL; w++)
    for_bits<T, true>(
        act[w], [&](int j) { return ld(w * HL + j); }, [&](int j, const auto& v) { f(w * HL + j, v); });
}

// the joint-limit and tendon-limit terms of (J' f)_i, added to the contacts' acc: the dof's limit-row slots
// and rows [njl, nlim)
template <typename T, typename C>
__device__ __forceinline__ T jtf_tail(MPtr<T> m, const Scratch<T, C>& s, int sl, T acc) {
  if (sl < MAXDOF) {
    int lr = s.lim_row[sl];
    int lo = (lr & 0xff) - 1, hi = (lr >> 8) - 1;
    if (lo >= 0) acc += s.row_f[lo];
    if (hi >= 0) acc -= s.row_f[hi];
  }
  for (int r = s.njl; r < s.nlim; r++) {
    int id = rk_id(s.row_kid[r]);
    T f = rk_kind(s.row_kid[r]) == RK_TLO ? s.row_f[r] : -s.row_f[r];
    for (int w = 0; w < HS_LT(C, m).ten_nwrap[id]; w++)
      if (HS_LT(C, m).ten_wrapdof[id][w] == sl) acc += f * HS_LT(C, m).ten_wrapcoef[id][w];
  }
  return acc;
}

// (J' f)_i for dof sub-lane i: contacts via point Jacobians, then jtf_tail.  AUG (the C::WALKS instances' Newton
// iteration): the same walk over the active contacts also adds the contact terms of the Newton Hessian to aug
// (Stepper::solve).  Both read con_m1 / con_m2 / con_pos and form the same r = pos - com, w = cd x r and
// jp = cd[3:] + w, so a contact's operands are read once and its round trip is paid once.  Each accumulator keeps
// the guard and the operation order it has in a loop of its own: J'f takes every contact with in1 != in2, the
// Hessian those of them with m1 == 0 (then in1 = 0 and in2 = bit(m2, sl) = 1).
template <typename T>
struct ConF { uint32_t m1, m2; T p[3], f[3]; };
template <typename T>
struct ConFU { uint32_t m1, m2; T p[3], f[3], U[6]; };
template <bool AUG, typename T, typename C>
__device__ __forceinline__ T jtf_walk(MPtr<T> m, const Scratch<T, C>& s, int sl, const T* cd, T* aug) {
  T acc = 0;
  using CV = std::conditional_t<AUG, ConFU<T>, ConF<T>>;
  for_active_contacts_ld<T, C>(s.con_act, [&](int c) {
    CV v;
    v.m1 = s.con_m1[c]; v.m2 = s.con_m2[c];
    for (int k = 0; k < 3; k++) { v.p[k] = s.con_pos[c][k]; v.f[k] = s.con_F[c][k]; }
    if constexpr (AUG)
      for (int k = 0; k < 6; k++) v.U[k] = s.con_U[c][k];
    return v;
  }, [&](int, const CV& v) {
    const int in2 = bit(v.m2, sl), in1 = bit(v.m1, sl);
    if (in1 != in2) {
      T r[3] = {v.p[0] - s.com[0], v.p[1] - s.com[1], v.p[2] - s.com[2]};
      T w[3];
      cross3(cd, r, w);
      T jp[3] = {cd[3] + w[0], cd[4] + w[1], cd[5] + w[2]};
      T x = dot3(jp, v.f);
      acc += in2 ? x : -x;
      if constexpr (AUG) {
        if (v.m1 == 0u) {   // plane contacts; body-body ones enter the Hessian as dense rank-1 rows
          const T* U = v.U;
          T z[3] = {U[0] * jp[0] + U[3] * jp[1] + U[4] * jp[2], U[3] * jp[0] + U[1] * jp[1] + U[5] * jp[2],
                    U[4] * jp[0] + U[5] * jp[1] + U[2] * jp[2]};
          T rz[3];
          cross3(r, z, rz);
          for (int k = 0; k < 3; k++) { aug[k] += rz[k]; aug[3 + k] += z[k]; }
        }
      }
    }
  });
  return jtf_tail(m, s, sl, acc);
}
template <typename T, typename C>
__device__ __forceinline__ T jtf_lane(MPtr<T> m, const Scratch<T, C>& s, int sl, const T* cd) {
  return jtf_walk<false>(m, s, sl, cd, (T*)nullptr);
}
template <typename T, typename C>
__device__ __forceinline__ T jtf_aug_lane(MPtr<T> m, const Scratch<T, C>& s, int sl, const T* cd, T (&aug)[6]) {
  return jtf_walk<true>(m, s, sl, cd, aug);
}

}  // namespace
}  // namespace hs
