// Lane-level primitives of the step kernel (two envs per wavefront, 32 lanes each): capacity
// tiers, scheduling / LDS fences, DPP broadcasts and half-wave sums, the opaque() launderers, the
// launch-argument block (KArgs) and the 3-vector / spatial algebra (mju_* helpers of MuJoCo's
// engine_util_blas / engine_util_spatial) every later phase uses.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "hs_kernels.h"
#include "hs_model.h"
#include "hs_bits.h"

namespace hs {
namespace {

constexpr int WAVE = 64;
constexpr int HL = 32;            // lanes per env
static_assert(MAXDOF == HL, "one dof per sub-lane (lim_row slots, dof masks)");

// Per-env contact / constraint-row capacity of a kernel instance (hs_model.h): the resident tier
// every launch runs with and the wide tier that re-runs the (rare) envs overflowing it.
template <int NCON, int NEFC, bool W = false, bool LT = false>
struct Cap {
  static constexpr int CON = NCON;        // contacts (at most one slot per lane per HL-slot pass)
  static constexpr int EFC = NEFC;        // constraint rows
  static constexpr int RPL = NEFC / HL;   // rows per lane (kept in registers by the row's lane)
  static constexpr bool WIDE = W;         // the wide (re-run) tier
  static constexpr bool LANES = LT;       // the model's per-lane constants are read from LDS (lanes() below)
  // collision compacts the near pairs before the narrow phase (Stepper::collision_near).  A flag of its own
  // for the phases to test, but no template parameter of its own: it holds for exactly the instances with
  // the lane table (the list lies over con_F, where their kinematics tail ends, and store_contact_near
  // reads the table), and another parameter would rename every fp32 function that carries its Cap.
  static constexpr bool NEAR = LT;
  // the chain / subtree sums read their operands a group of bits at a time (for_bits_g below): the same
  // instances again, and a constant of its own for the same reason
  static constexpr bool GROUPS = LT;
  // the Newton solve walks the active contacts once per iteration for J'f and the Hessian's contact terms
  // (jtf_aug_lane), and the row slots' J x operands are read in one batch (rows_Jx, hs_contacts.h): the same
  // instances again (profiles/newton_walks.md)
  static constexpr bool WALKS = LT;
  static_assert((NCON % HL == 0 || HL % NCON == 0) && NEFC % HL == 0, "capacity in whole half-waves");
};
// resident tier per precision (hs_model.h).  The fp64 instances keep the lane table in LDS: at one wave
// per SIMD nothing hides the latency of its reads through vector memory.  The fp32 engine (its direct
// kernel fills LDS: 8 workgroups of 20,480 B per CU) and the wide tier read the model as before.
// The same instances run the collision narrow phase over a compacted list of near pairs (NEAR): their
// capsule-capsule branch is fp64-heavy and a wave executes it in every pass where any lane holds a near
// pair; the fp32 engine and the wide tier keep the five-pass loop.
template <typename T>
using Resident = std::conditional_t<sizeof(T) == 8, Cap<MAXCON_F64, MAXEFC_F64, false, true>, Cap<MAXCON, MAXEFC>>;
using Wide = Cap<MAXCON_WIDE, MAXEFC_WIDE, true>;

// scheduling fence: keeps the machine scheduler from hoisting loads across iterations of fully
// unrolled loops (which otherwise inflates VGPR pressure far past the occupancy target; without the
// per-loop fences the Cholesky / CRB loops cost 1136 / 564 B/lane of scratch)
#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

// single-wave workgroup: LDS ops of a wave execute in order, so a compiler-only barrier suffices to
// keep LDS accesses from moving across phase boundaries (no s_barrier, and no s_waitcnt that a
// workgroup-scope fence would add).
#define WSYNC() asm volatile("" ::: "memory")

// ------------------------------------------------------------------ cross-lane helpers
// compile-time loop: f(std::integral_constant<int, i>) for i in [B, E)
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}
// bound_ctrl set: every pattern used here reads in-bounds lanes only, and with it the DPP combiner
// folds the move into its consumer (hsum's adds become single v_add_f32_dpp instructions)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
// v_permlane16_swap(v, v): .first = rows {0,0,2,2}, .second = rows {1,1,3,3} (row = 16 lanes),
// i.e. every lane of a 32-lane half sees the half's low row in .first and its high row in .second.
struct RowPair { uint32_t lo, hi; };
__device__ __forceinline__ RowPair rowswap(uint32_t v) {
  auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  return {r[0], r[1]};
}
// value of sub-lane K (compile-time) of the caller's 32-lane half: DPP row_newbcast + one
// permlane16 swap -- 3 VALU ops, no SGPR round trip, and bcast<K> / bcast<K+16> share both ops.
template <int K>
__device__ __forceinline__ uint32_t bcast32(uint32_t v) {
  RowPair r = rowswap(dpp32<0x150 + (K & 15)>(v));
  return K < 16 ? r.lo : r.hi;
}
template <int K>
__device__ __forceinline__ float bcast(float v) {
  return __uint_as_float(bcast32<K>(__float_as_uint(v)));
}
template <int K>
__device__ __forceinline__ double bcast(double v) {
  uint64_t x = (uint64_t)__double_as_longlong(v);
  uint64_t lo = bcast32<K>((uint32_t)x), hi = bcast32<K>((uint32_t)(x >> 32));
  return __longlong_as_double((long long)((hi << 32) | lo));
}
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __uint_as_float(dpp32<CTRL>(__float_as_uint(v)));
}
template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
  uint64_t x = (uint64_t)__double_as_longlong(v);
  uint64_t lo = dpp32<CTRL>((uint32_t)x), hi = dpp32<CTRL>((uint32_t)(x >> 32));
  return __longlong_as_double((long long)((hi << 32) | lo));
}
__device__ __forceinline__ float rows_sum(float v) {
  RowPair r = rowswap(__float_as_uint(v));
  return __uint_as_float(r.lo) + __uint_as_float(r.hi);
}
__device__ __forceinline__ double rows_sum(double v) {
  uint64_t x = (uint64_t)__double_as_longlong(v);
  RowPair l = rowswap((uint32_t)x), h = rowswap((uint32_t)(x >> 32));
  return __longlong_as_double((long long)(((uint64_t)h.lo << 32) | l.lo)) +
         __longlong_as_double((long long)(((uint64_t)h.hi << 32) | l.hi));
}
// the value of the same position in the half's high 16-lane row (valid on the low row's lanes)
__device__ __forceinline__ float up_row(float v) { return __uint_as_float(rowswap(__float_as_uint(v)).hi); }
__device__ __forceinline__ double up_row(double v) {
  uint64_t x = (uint64_t)__double_as_longlong(v);
  const uint64_t lo = rowswap((uint32_t)x).hi, hi = rowswap((uint32_t)(x >> 32)).hi;
  return __longlong_as_double((long long)((hi << 32) | lo));
}
// sum over each 32-lane half (result in every lane of the half); all-VALU, no LDS permute
template <typename T>
__device__ __forceinline__ T hsum(T v) {
  v += dpp<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp<0x141>(v);   // row_half_mirror
  v += dpp<0x140>(v);   // row_mirror
  return rows_sum(v);   // + the other 16-lane row of the half
}
__device__ __forceinline__ uint32_t hballot(bool p, bool upper) {
  uint64_t m = __ballot(p);
  return upper ? (uint32_t)(m >> 32) : (uint32_t)m;
}
// f(j, ld(j)) for each set bit j of mk, ascending (the chain / subtree sums).  AHEAD: the loads of the
// next bit's operands are issued before the current bit's arithmetic, so one LDS round trip overlaps
// the FMAs (the same operations in the same order) -- the contact loops take it.  For the chain /
// subtree sums it measured slower in both engines (fp64 0.697 vs 0.691 ms, fp32 0.411 vs 0.408 ms
// per configs[1] launch): it keeps one round trip per bit, hides it behind ~10 adds only
// and pays 14-20 register copies per bit for that.  Those sums take for_bits_g below instead, which
// reads a group of bits per round trip (profiles/chain_sums.md).
template <typename T, bool AHEAD = false, typename LD, typename F>
__device__ __forceinline__ void for_bits(uint32_t mk, LD&& ld, F&& f) {
  if constexpr (AHEAD) {
    if (mk == 0u) return;
    int j = __builtin_ctz(mk);
    mk &= mk - 1u;
    auto cur = ld(j);
    for (; mk; mk &= mk - 1u) {
      const int jn = __builtin_ctz(mk);
      auto nxt = ld(jn);
      f(j, cur);
      cur = nxt;
      j = jn;
    }
    f(j, cur);
  } else {
    for (; mk; mk &= mk - 1u) {
      const int j = __builtin_ctz(mk);
      f(j, ld(j));
    }
  }
}
// The chain / subtree sums' walk: G bits per round (for_bit_groups, hs_bits.h) in the instances with
// Cap::GROUPS, the bit-by-bit walk in every other.  At one wave per SIMD nothing hides an LDS round trip,
// and the bit-by-bit walk pays one per set bit of the wave's longest mask (15 dofs for a foot's chain,
// 16 bodies for the root's subtree on humanoid.xml); the fp32 engine runs two waves per SIMD and has no
// registers for a second set of operands.  Group sizes per call site: profiles/chain_sums.md.
template <typename C, int G, typename T, typename LD, typename F>
__device__ __forceinline__ void for_bits_g(uint32_t mk, LD&& ld, F&& f) {
  if constexpr (C::GROUPS && G > 1) for_bit_groups<G>(mk, ld, f, [] { SCHED_FENCE(); });
  else for_bits<T>(mk, ld, f);
}
// The phases spell the call HS_FOR_BITS(C, G, T)(mask, ld, f); in the fp32 pass it is the for_bits call it
// replaces (as HS_LT below: the fp32 code object stays byte for byte what it is without the groups).
#ifdef HS_ONLY_F32
#define HS_FOR_BITS(C, G, T) for_bits<T>
#else
#define HS_FOR_BITS(C, G, T) for_bits_g<C, G, T>
#endif
// Bits per round.  A/B among {2, 3, 4} on the configs[1] launch (profiles/chain_sums.md): the 10-value subtree sum of
// mass_matrix (20 VGPRs per bit in flight) takes 2; the four sums of velocity_forces were measured together, not one
// by one, and share 3 (14 VGPRs per bit, 12 for the cfrc subtree sum); map_vx takes 3.  4 everywhere measured no
// faster than the bit-by-bit walk.  post_constraint runs only with full_state, which that launch does not set: its 3
// follows the other 6-value sums and was not measured on its own.
constexpr int G_CRB = 2, G_VEL = 3, G_VX = 3, G_POST = 3;
template <typename T, int N>
struct Vals { T v[N]; };
template <typename T, int N>
struct ValsX { T x; T v[N]; };

// Hide a (uniform) pointer's value from the optimiser.  The model pointer is const __restrict__,
// so without this LICM hoists every per-lane model load (m->dof_bodyid[sl], ...) out of the
// substep / Newton loops and keeps each one live in a VGPR for the whole kernel.
// (The value is wave-uniform by construction; readfirstlane only tells the uniformity analysis so,
// where control flow hides it -- e.g. across the chunk-queue loop -- and folds away otherwise.)
template <typename P>
__device__ __forceinline__ P opaque(P p) {
  uint64_t v = (uint64_t)p;
  uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  v = ((uint64_t)hi << 32) | lo;
  asm volatile("" : "+s"(v));
  return (P)v;
}
// The model lives in the constant address space: it is never written by the kernel, so reads at
// a wave-uniform index become scalar loads (s_load via the scalar cache) even through an
// opaque()-laundered pointer; lane-varying reads stay vector loads.
template <typename T>
using MPtr = const __attribute__((address_space(4))) DevModel<T>*;
template <typename T>
using CPtr = const __attribute__((address_space(4))) T*;      // pointer into the model
// The wave's LDS copy of the model's lane table (hs_model.h LaneTable; one workgroup = one wave, both
// halves step envs of the same model).  A function-scope static: only the kernels whose instances
// call lanes() below with C::LANES allocate it, and every access is an LDS instruction at a constant
// address (no pointer to launder or keep live).
template <typename T>
__device__ __forceinline__ LaneTable<T>& lane_table() {
  __shared__ LaneTable<T> tab;
  return tab;
}
// Once per launch, before the wave's first item: every lane copies 16-byte pieces, all loads in flight
// before the first store (one wait).
template <typename T>
__device__ __forceinline__ void load_lane_table(MPtr<T> m) {
  constexpr int N = (int)(sizeof(LaneTable<T>) / 16), PER = (N + WAVE - 1) / WAVE;
  static_assert(sizeof(LaneTable<T>) % 16 == 0 && alignof(LaneTable<T>) == 16, "16-byte pieces");
  typedef uint32_t Piece __attribute__((ext_vector_type(4)));
  CPtr<Piece> src = (CPtr<Piece>)&m->lanes;
  Piece* dst = reinterpret_cast<Piece*>(&lane_table<T>());
  const int lane = threadIdx.x;
  Piece v[PER];
#pragma unroll
  for (int i = 0; i < PER; i++) {
    const int k = lane + i * WAVE;
    v[i] = src[k < N ? k : N - 1];
  }
#pragma unroll
  for (int i = 0; i < PER; i++) {
    const int k = lane + i * WAVE;
    if (k < N) dst[k] = v[i];
  }
  asm volatile("" ::: "memory");
}
// Where an instance reads the model's per-lane constants: lanes<C>(m).field[i] is the LDS copy for
// C::LANES and m->field[i] otherwise (LaneTable and DevModel name the fields alike).
template <typename C, typename T>
__device__ __forceinline__ decltype(auto) lanes(MPtr<T> m) {
  if constexpr (C::LANES) return (lane_table<T>());
  else return (*m);
}
// The phases spell these reads HS_LT(C, m).field[i].  The fp32 pass over the kernels (HS_ONLY_F32) has
// no instance with a lane table, and there the macro is the plain member access it replaces, so that
// the fp32 code object stays byte for byte what it is without the table (the compiler's register
// allocation for the fp32 direct kernel turns on less).  HS_KTAIL(s): the same for Scratch::ktail().
#ifdef HS_ONLY_F32
#define HS_LT(C, m) (*(m))
#define HS_KTAIL(s) (s).u.k
#else
#define HS_LT(C, m) lanes<C>(m)
#define HS_KTAIL(s) (s).ktail()
#endif
// All launch arguments travel as ONE by-value struct, so it sits at offset 0 of the kernarg
// segment.  The kernel reads it through an opaque()-laundered constant-address-space pointer to
// that segment: every use is a fresh scalar load (scalar cache) instead of ~80 SGPRs kept live
// for the whole kernel (which spill to VGPR lanes, and the per-lane buffer addresses derived
// from them to scratch -- 150 B/lane of spill traffic written back to HBM every launch).
template <typename T>
struct KArgs {
  MPtr<T> m;
  EnvBuffers<T> b;
  const float* actions;       // [N][nu] f32 (null in MODE_RESET)
  const uint8_t* reset_mask;  // [N] or null
  const T* nz_q;              // [N][nq] host reset noise or null (device RNG)
  const T* nz_v;              // [N][nv] or null
  StepParams p;
  int nenv;
  TapeOut<T> tape;            // per-step outputs of a tape launch (p.nsteps > 1), or all null
  RolloutArgs ro;             // fused rollout (ro.obs != null): actions from the policy, see hs_kernels.h
  EvalArgs ev;                // fused evaluation (the EVAL instance only; after ro, so every other offset stays)
  NormArgs nm;                // obs normalisation of the fused policy (the NORM instances only; last, as above)
  TermArgs tm;                // built-in termination condition (the TERM instances only; last, as above)
  InitArgs<T> in;             // bank of initial states the reset pass draws from (K = 0: none; last, as above)
};
template <typename T>
using KPtr = const __attribute__((address_space(4))) KArgs<T>*;
// Same for a per-lane value: stops lane-invariant compare masks (j <= sl, bit(mask, sl), ...)
// being hoisted out of the loops as dozens of 64-bit SGPR masks (which then spill).
__device__ __forceinline__ int opaque_v(int x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ int below(uint32_t m, int sl) { return __popc(m & ((1u << sl) - 1u)); }
__device__ __forceinline__ bool bit(uint32_t mask, int i) { return i < 32 && ((mask >> i) & 1u); }
template <typename T>
__device__ __forceinline__ bool isbad(T x) {
  return !(x <= T(1e10) && x >= T(-1e10));   // NaN or |x| > mjMAXVAL
}

// Chunk-queue hand-off rows (b.mid, uncached) are written and read at agent scope.  A row is rewritten
// by one CU and read by another, and a tape launch reads env e's row once per env step, often on a CU
// whose vector L1 still holds the line from an earlier step: plain loads could return that stale line
// (measured: tape launches were nondeterministic with plain loads, tests/test_gpu_tape.py).
template <typename T>
__device__ __forceinline__ T row_ld(const T* p) {
  return __hip_atomic_load(const_cast<T*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void row_st(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ small algebra
// sin/cos: fp64 libm for the parity mode; the fp32 engine uses the hardware v_sin/v_cos
// (|error| ~1e-6 on the half joint angles, inside the fp32 tolerance)
__device__ __forceinline__ void sincos_t(double x, double& s, double& c) { sincos(x, &s, &c); }
__device__ __forceinline__ void sincos_t(float x, float& s, float& c) { s = __sinf(x); c = __cosf(x); }
template <typename T>
__device__ __forceinline__ void quat2mat(const T* q, T* R) {
  T w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}
template <typename T>
__device__ __forceinline__ void mulq(const T* a, const T* b, T* r) {
  T t0 = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  T t1 = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  T t2 = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  T t3 = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = t0; r[1] = t1; r[2] = t2; r[3] = t3;
}
template <typename T>
__device__ __forceinline__ void mv3(const T* R, const T* v, T* r) {
  T a = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
  T b = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
  T c = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
  r[0] = a; r[1] = b; r[2] = c;
}
template <typename T>
__device__ __forceinline__ void cross3(const T* a, const T* b, T* r) {
  T x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
template <typename T>
__device__ __forceinline__ T dot3(const T* a, const T* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
template <typename T>
__device__ __forceinline__ T dot6(const T* a, const T* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}
template <typename T>
__device__ __forceinline__ T rsqrt_t(T x);
template <>
__device__ __forceinline__ float rsqrt_t<float>(float x) { return __builtin_amdgcn_rsqf(x); }
// fp64: below recip()
// 1/x: fp32 is v_rcp_f32 under -fno-hip-fp32-correctly-rounded-divide-sqrt; fp64 is v_rcp_f64 +
// one cubic correction (e + e^2) instead of two Newton steps: 4 dependent operations instead of 5,
// the same ~1 ulp for normal nonzero x (fp64 0.662 -> 0.656 ms per configs[1] launch).
// Domain of recip(double): normal, nonzero x whose reciprocal is normal too; 0 and denormals give NaN
// by construction (v_rcp_f64 returns +-inf there and e = 1 - x * inf is NaN), no class check.
__device__ __forceinline__ float recip(float x) { return 1.0f / x; }
__device__ __forceinline__ double recip(double x) {
  double y = __builtin_amdgcn_rcp(x);
  // y (1 + e + e^2) with e = 1 - x y: relative error cubed in one step (4 dependent operations)
  const double e = fma(-x, y, 1.0);
  return fma(fma(e, e, e), y, y);
}
// fp64 1/sqrt(x), x >= 1e-30 at every call site (the Cholesky pivots are clamped to it, the
// normalizations branch below it), so no denormal scaling or zero / infinity class check:
// v_rsq_f64, one Goldschmidt step (h ~ 1/(2 sqrt x)), one Newton step on y = 2h -- within ~1 ulp,
// 7 dependent operations.  A/B, fp64 ms per configs[1] launch (with the DPP pivots of chol_rows):
// recip(sqrt(x)) (18 operations) 0.714, the library sqrt sequence without its scaling / class check
// then recip() (13) 0.701, this 0.690.  (Round 2 measured a v_rsq_f64 + two-Newton-step variant
// slower, 305k vs 298k cycles per env substep, under the default machine scheduler.)
template <>
__device__ __forceinline__ double rsqrt_t<double>(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double r = fma(-h, g, 0.5);
  h = fma(h, r, h);
  const double y1 = h + h;
  const double e = fma(-(x * y1), y1, 1.0);
  return fma(h, e, y1);
}
template <typename T>
__device__ __forceinline__ T normalize3(T* v) {
  const T n2 = dot3(v, v);
  if (n2 < T(1e-30)) { v[0] = 1; v[1] = 0; v[2] = 0; return sqrt(n2); }
  const T i = rsqrt_t(n2);
  v[0] *= i; v[1] *= i; v[2] *= i;
  return n2 * i;
}
template <typename T>
__device__ __forceinline__ void normalize4(T* q) {
  const T n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (n2 < T(1e-30)) { q[0] = 1; q[1] = q[2] = q[3] = 0; }
  else { const T i = rsqrt_t(n2); q[0] *= i; q[1] *= i; q[2] *= i; q[3] *= i; }
}
// spatial inertia (10-param cinert layout) times motion vector (mju_mulInertVec)
template <typename T>
__device__ __forceinline__ void mul_inert(const T* i, const T* v, T* r) {
  r[0] = i[0] * v[0] + i[3] * v[1] + i[4] * v[2] - i[8] * v[4] + i[7] * v[5];
  r[1] = i[3] * v[0] + i[1] * v[1] + i[5] * v[2] + i[8] * v[3] - i[6] * v[5];
  r[2] = i[4] * v[0] + i[5] * v[1] + i[2] * v[2] - i[7] * v[3] + i[6] * v[4];
  r[3] = i[8] * v[1] - i[7] * v[2] + i[9] * v[3];
  r[4] = i[6] * v[2] - i[8] * v[0] + i[9] * v[4];
  r[5] = i[7] * v[0] - i[6] * v[1] + i[9] * v[5];
}
template <typename T>
__device__ __forceinline__ void cross_motion(const T* v, const T* m, T* r) {
  r[0] = -v[2] * m[1] + v[1] * m[2];
  r[1] = v[2] * m[0] - v[0] * m[2];
  r[2] = -v[1] * m[0] + v[0] * m[1];
  r[3] = -v[2] * m[4] + v[1] * m[5] - v[5] * m[1] + v[4] * m[2];
  r[4] = v[2] * m[3] - v[0] * m[5] + v[5] * m[0] - v[3] * m[2];
  r[5] = -v[1] * m[3] + v[0] * m[4] - v[4] * m[0] + v[3] * m[1];
}
template <typename T>
__device__ __forceinline__ void cross_force(const T* v, const T* f, T* r) {
  r[0] = -v[2] * f[1] + v[1] * f[2] - v[5] * f[4] + v[4] * f[5];
  r[1] = v[2] * f[0] - v[0] * f[2] + v[5] * f[3] - v[3] * f[5];
  r[2] = -v[1] * f[0] + v[0] * f[1] - v[4] * f[3] + v[3] * f[4];
  r[3] = -v[2] * f[4] + v[1] * f[5];
  r[4] = v[2] * f[3] - v[0] * f[5];
  r[5] = -v[1] * f[3] + v[0] * f[4];
}

}  // namespace
}  // namespace hs
