// Per-env LDS layouts: Scratch (the mjData fields one mj_step needs, phase-local arrays aliased in a
// union so a wave's two envs fit 20 KB) and the PGS instance's row cache.
#pragma once
#include <cstdint>

#include "hs_lanes.h"
#include "hs_model.h"

namespace hs {
namespace {

enum RowKind { RK_JLO = 0, RK_JHI = 1, RK_TLO = 2, RK_THI = 3, RK_CN = 4, RK_P0 = 5 };   // P0..P0+3: pyramid
__device__ __forceinline__ int rk_kind(int kid) { return kid >> 16; }
__device__ __forceinline__ int rk_id(int kid) { return kid & 0xffff; }

// kinematics' joint anchors / axes and geom frames (read until the end of collision)
template <typename T>
struct KinTail { T xanchor[MAXJNT][3]; T xaxis[MAXJNT][3]; T gpos[MAXGEOM][3]; T gax[MAXGEOM][3]; };

template <typename T, typename C>
struct Scratch {
  T qpos[MAXQ];
  T qvel[MAXDOF];
  T ctrl[MAXU];
  alignas(16) T vx[MAXDOF];   // generalized vector for J x; Cholesky column buffer
  T com[4];
  T cinert[MAXBODY][10];
  T cdof[MAXDOF][6];
  T cvel[MAXBODY][6];
  T con_pos[C::CON][3];
  T con_n[C::CON][3];
  T con_t1[C::CON][3];
  T con_dist[C::CON];
  T con_v[C::CON][3];
  T con_U[C::CON][6];
  T con_F[C::CON][3];
  int con_pair[C::CON];
  int con_adr[C::CON];
  uint32_t con_bb[C::CON];    // b1 | b2 << 8 | condim << 16 of the contact's pair (no model lookups per use)
  uint32_t con_m1[C::CON];    // dof chain masks of the contact's bodies (m1 = 0: world)
  uint32_t con_m2[C::CON];
  T con_mu[C::CON];
  uint32_t con_act[(C::CON + HL - 1) / HL];   // contacts with a nonzero force (contact_aggregates)
  uint16_t lim_row[MAXDOF];   // joint-limit rows of a dof: (lo row + 1) | (hi row + 1) << 8
  uint32_t dense_mask[C::RPL];   // rows added as dense rank-1 Hessian terms (tendons, body-body)
  int row_kid[C::EFC];
  T row_D[C::EFC];
  T row_f[C::EFC];
  int ncon, nefc, nlim, njl;   // njl: joint-limit rows (tendon rows are [njl, nlim))
  int niter;                   // this env's Newton iterations (the wave's loop runs for the slower env)
  // Instances with the lane table in LDS (C::LANES) make room for it: their KinTail lies over con_v /
  // con_U / con_F, which are first written in rows() (map_vx) and the solve (contact_aggregates), after
  // collision's last read of the tail, and last read in post_constraint, before the next substep's
  // kinematics (store_contact writes none of them).  The union's largest member is then the RNE one.
  // (In fp64 the tail fills con_v and con_U exactly and ends where con_F begins: near_list() below.)
  struct KinHead { T xpos[MAXBODY][3]; T xmat[MAXBODY][9]; T xquat[MAXBODY][4]; };
  struct KinFull { T xpos[MAXBODY][3]; T xmat[MAXBODY][9]; T xquat[MAXBODY][4]; T xanchor[MAXJNT][3];
                   T xaxis[MAXJNT][3]; T gpos[MAXGEOM][3]; T gax[MAXGEOM][3]; };
  using Kin = std::conditional_t<C::LANES, KinHead, KinFull>;
  static_assert(!C::LANES || sizeof(KinTail<T>) <= sizeof(T) * C::CON * 12, "KinTail fits con_v, con_U, con_F");
  // xanchor, xaxis, gpos, gax: wherever the instance keeps them
  __device__ __forceinline__ decltype(auto) ktail() {
    if constexpr (C::LANES) return (*reinterpret_cast<KinTail<T>*>(&con_v[0][0]));
    else return (u.k);
  }
  __device__ __forceinline__ decltype(auto) ktail() const {
    if constexpr (C::LANES) return (*reinterpret_cast<const KinTail<T>*>(&con_v[0][0]));
    else return (u.k);
  }
  // The near-pair list of the C::NEAR instances' collision (one word per pair, hs_contacts.h near_entry) lies over
  // con_F, where those instances' KinTail ends.  con_F is dead for the whole of collision: its last writer
  // before it is contact_aggregates at the end of the previous substep's solve, its readers are jtf_lane
  // (inside the solve, after that write) and post_constraint (full_state, right after the solve), and its
  // first writer after collision is contact_aggregates in this substep's solve -- a write, so nothing ever
  // reads list words as forces.  dump_debug reads no con_F, commit(full) reads the union's cfrc / linv
  // (post_constraint's outputs, taken from con_F before the next substep's kinematics); the acceleration
  // check's second attempt restarts at kinematics and rebuilds the list.  store_contact writes none of
  // con_v / con_U / con_F, so the list and the tail both outlive the narrow passes.
  static_assert(!C::NEAR || (C::LANES && sizeof(uint32_t) * MAXPAIR <= sizeof(T) * C::CON * 3 &&
                             sizeof(KinTail<T>) <= sizeof(T) * C::CON * 9),
                "the near-pair list fits con_F, past the KinTail over con_v / con_U");
  __device__ __forceinline__ uint32_t* near_list() { return reinterpret_cast<uint32_t*>(&con_F[0][0]); }
  // The second body-velocity set of the C::WALKS instances' rows() (chain_vel2, hs_contacts.h: J qacc_warmstart
  // beside J qvel in u.n.bvel) lies in u.n.cfrc, which has bvel's shape.  u.n.cfrc is dead for the whole of
  // rows(): its only writer is post_constraint, after the solve, and its readers (obs / reward / commit with
  // full_state) run after the last substep's post_constraint and before the next kinematics, which overwrites
  // the union anyway (u.k).  The RNE member u.r lies over the same bytes and is last read at the end of
  // velocity_forces (csub -> qfrc_smooth), before rows(); u.n.cb (the Cholesky column pairs, between bvel and
  // cfrc) is first written in the solve.  rows() reads the set back (contact_vel) before it returns, so nothing
  // of it is live when the solve starts.  No LDS is added.
  union {   // phase-local arrays (aliased)
    Kin k;                                                        // kinematics + collision
    struct { T crb[MAXBODY][10]; T buf[MAXDOF][6]; } c;          // composite rigid body
    struct { T cdofdot[MAXDOF][6]; T cfrc[MAXBODY][6]; T csub[MAXBODY][6]; } r;   // RNE
    struct { T bvel[MAXBODY][6];                                  // J x mapping (rows, Newton)
             alignas(16) T cb[MAXDOF][2];                         // Cholesky column pairs
             T cfrc[MAXBODY][6], linv[MAXBODY][3], mv[MAXBODY][3]; } n;   // full_state (after solve)
    // fused rollout's policy forward (fp64 engine only: inside the union's 4 KB there; the fp32
    // engine's union is smaller and must not grow, so its member is a stub)
    struct { alignas(16) float x[sizeof(T) == 8 ? 512 : 4]; alignas(16) float h[sizeof(T) == 8 ? 256 : 4]; } pol;
  } u;
};

// PGS solver scratch (the <option solver="PGS"> kernel instance only; the Newton instance never
// allocates it).  With M = L L', row r's u_r = L^-1 J_r' (one nv-vector per row) gives the whole dual:
// AR = J M^-1 J' + R has AR_ik = u_i . u_k + R_i [i == k], and J_r qacc = u_r . (L' qacc).  Rows
// [0, NC) keep u_r in LDS (later rows rebuild it per use); every row keeps b_r = -aref_r, R_r, AR_rr,
// 1 / AR_rr and its lookahead Gram terms.
// Row sweep lookahead: row r's residual u_r . z is started PGS_LA rows early, on a z that still lacks the
// updates of rows r-PGS_LA .. r-1, and corrected with delta_{r-j} (u_r . u_{r-j}) when row r's turn
// comes (the Gram terms G_rj are computed once per substep).  The half-wave sum thus leaves the
// serial chain, which shrinks to a few scalar FMAs per row.
constexpr int PGS_LA = 3;
// cached rows: 40 in fp32 keep the resident PGS instance at 4 workgroups per CU; fp64 (48) runs at 2
template <typename T>
constexpr int pgs_cache_rows() { return sizeof(T) == 4 ? 40 : 48; }
template <typename T>
struct alignas(4 * sizeof(T)) PgsRow {
  T b, R, ar, ai;                 // -aref_r, R_r, AR_rr, 1 / max(AR_rr, MINVAL)
  T g[4];                         // G_rj = u_r . u_{r-j}, j = 1..PGS_LA (0 past the first row)
};
template <typename T, typename C>
struct PgsCache {
  static constexpr int NC = pgs_cache_rows<T>();
  T u[NC][MAXDOF];
  PgsRow<T> row[C::EFC];
};

}  // namespace
}  // namespace hs
