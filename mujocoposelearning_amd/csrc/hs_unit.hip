// Unit harness of the step kernels' device primitives (libhsim_unit.so).  TEST CODE: never linked into
// libhsim.so, never loaded by the package, nothing of it in include/hsim.h.
//
// Thin __global__ wrappers that call the functions of hs_lanes.h, hs_dense.h and hs_contacts.h, unchanged,
// on inputs a test constructs (tests/unit_kernels.py), so a defect in one of them shows at that function
// and not as a qacc mismatch at the far end of the pipeline.  Compiled twice like hs_kernels.hip
// (HS_ONLY_F32 / HS_ONLY_F64, each with its engine's flags), so the primitives get each engine's code
// generation; the pass exports hsu_<name>_f32 or hsu_<name>_f64(device pointers..., n, stream).
//
// Every entry point returns HSU_EARG (and launches nothing) on a null pointer or n < 1, otherwise the
// hipError_t of the launch.  Every kernel runs 64-thread blocks (WSYNC() and the cross-lane helpers are
// valid for single-wave workgroups only), executes the cross-lane code with all 64 lanes active and
// bounds-checks every global access against n: an item past n (the ghost half of an odd count) computes
// on zeros and stores nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hs_contacts.h"
#include "hs_dense.h"
#include "hs_lanes.h"
#include "hs_scratch.h"

#if defined(HS_ONLY_F32) == defined(HS_ONLY_F64)
#error "hs_unit.hip: compile with exactly one of -DHS_ONLY_F32 / -DHS_ONLY_F64"
#endif
#ifdef HS_ONLY_F32
typedef float HT;
#define HSU(name) hsu_##name##_f32
#else
typedef double HT;
#define HSU(name) hsu_##name##_f64
#endif

namespace hs {
namespace {

constexpr int NV = 27;                              // the only instantiated size (humanoid.xml)
constexpr int GE = sizeof(HT) == 8 ? 4 : 8;         // right-hand sides per chol_fwd_multi call of the PGS instance
constexpr int NPL = MAXGEOM / 2;                    // narrow-phase cases per half-wave: two geoms each

// ------------------------------------------------------------------ math, element-wise
__global__ __launch_bounds__(64) void k_rsqrt(const HT* x, HT* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) out[i] = rsqrt_t<HT>(x[i]);
}
__global__ __launch_bounds__(64) void k_recip(const HT* x, HT* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) out[i] = recip(x[i]);
}
__global__ __launch_bounds__(64) void k_sincos(const HT* x, HT* s, HT* c, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) sincos_t(x[i], s[i], c[i]);
}
// v [n][3] -> out [n][3] (normalized), len [n] (the returned norm)
__global__ __launch_bounds__(64) void k_normalize3(const HT* v, HT* out, HT* len, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  HT w[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
  len[i] = normalize3(w);
  for (int k = 0; k < 3; k++) out[3 * i + k] = w[k];
}
__global__ __launch_bounds__(64) void k_normalize4(const HT* q, HT* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  HT w[4] = {q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]};
  normalize4(w);
  for (int k = 0; k < 4; k++) out[4 * i + k] = w[k];
}

// ------------------------------------------------------------------ lanes
// item = one 32-lane half (the two halves of a wave hold different items).  x [n][32] ->
// sum, rows, up [n][32]; bc [n][32][32] (bc[item][K][lane] = bcast<K>); ballot [n][32] of x > 0.
__global__ __launch_bounds__(64) void k_lanes(const HT* x, HT* sum, HT* rows, HT* up, HT* bc, uint32_t* ballot, int n) {
  const bool upper = threadIdx.x >= HL;
  const int sl = threadIdx.x & (HL - 1), it = 2 * blockIdx.x + (upper ? 1 : 0);
  const bool on = it < n;
  const HT v = on ? x[(size_t)it * HL + sl] : HT(0);
  const HT s = hsum(v), r = rows_sum(v), u = up_row(v);
  const uint32_t bal = hballot(v > HT(0), upper);
  if (on) {
    const size_t o = (size_t)it * HL + sl;
    sum[o] = s; rows[o] = r; up[o] = u; ballot[o] = bal;
  }
  static_for<0, HL>([&](auto kc) {
    constexpr int K = decltype(kc)::value;
    const HT b = bcast<K>(v);
    if (on) bc[((size_t)it * HL + K) * HL + sl] = b;
  });
}

// ------------------------------------------------------------------ dense, NV = 27
// item = one half: A [n][27][27] row-major, b [n][27] -> L [n][27][27] (what chol_rows leaves in the rows),
// dinv, diag, xs [n][32] (xs = chol_solve of b with the factor; diag only written by the L D L' form).
template <bool LDL>
__global__ __launch_bounds__(64) void k_chol(const HT* A, const HT* b, HT* L, HT* dinv, HT* diag, HT* xs, int n) {
  __shared__ alignas(16) HT cb[2][MAXDOF][2];
  const bool upper = threadIdx.x >= HL;
  const int sl = threadIdx.x & (HL - 1), it = 2 * blockIdx.x + (upper ? 1 : 0);
  const bool row = it < n && sl < NV;
  HT R[NV];
#pragma unroll
  for (int j = 0; j < NV; j++) R[j] = row ? A[((size_t)it * NV + sl) * NV + j] : HT(0);
  const HT rhs = row ? b[(size_t)it * NV + sl] : HT(0);
  HT di = 0, dg = 0;
  chol_rows<NV, HT, LDL>(R, di, sl, cb[upper ? 1 : 0], &dg);
  WSYNC();
  const HT x = chol_solve<NV, HT, LDL>(R, di, rhs, sl);
  if (row) {
#pragma unroll
    for (int j = 0; j < NV; j++) L[((size_t)it * NV + sl) * NV + j] = R[j];
  }
  if (it < n) {
    const size_t o = (size_t)it * HL + sl;
    dinv[o] = di; diag[o] = dg; xs[o] = x;
  }
}
// forward substitutions with a given L L' factor: L [n][27][27] (strictly lower part read), dinv [n][32],
// b [n][GE][27] -> y1 [n][32] (chol_fwd of b[0]), y2 [n][2][32] (chol_fwd_multi<2> of b[0..1]),
// yg [n][GE][32] (chol_fwd_multi<GE>)
__global__ __launch_bounds__(64) void k_fwd(const HT* L, const HT* dinv, const HT* b, HT* y1, HT* y2, HT* yg, int n) {
  const bool upper = threadIdx.x >= HL;
  const int sl = threadIdx.x & (HL - 1), it = 2 * blockIdx.x + (upper ? 1 : 0);
  const bool row = it < n && sl < NV;
  HT R[NV];
#pragma unroll
  for (int j = 0; j < NV; j++) R[j] = (row && j < sl) ? L[((size_t)it * NV + sl) * NV + j] : HT(0);
  const HT di = row ? dinv[(size_t)it * HL + sl] : HT(0);
  HT bg[GE];
#pragma unroll
  for (int g = 0; g < GE; g++) bg[g] = row ? b[((size_t)it * GE + g) * NV + sl] : HT(0);
  const HT a1 = chol_fwd<NV>(R, di, bg[0], sl);
  HT b2[2] = {bg[0], bg[1]};
  chol_fwd_multi<NV, 2>(R, di, b2, sl);
  chol_fwd_multi<NV, GE>(R, di, bg, sl);
  if (it < n) {
    y1[(size_t)it * HL + sl] = a1;
#pragma unroll
    for (int g = 0; g < 2; g++) y2[((size_t)it * 2 + g) * HL + sl] = b2[g];
#pragma unroll
    for (int g = 0; g < GE; g++) yg[((size_t)it * GE + g) * HL + sl] = bg[g];
  }
}
// A [n][27][27], v [n][27] -> out [n][32] = A v (v through LDS, as the Newton loop reads s.vx)
__global__ __launch_bounds__(64) void k_matvec(const HT* A, const HT* v, HT* out, int n) {
  __shared__ alignas(16) HT vs[2][MAXDOF];
  const bool upper = threadIdx.x >= HL;
  const int sl = threadIdx.x & (HL - 1), it = 2 * blockIdx.x + (upper ? 1 : 0);
  const bool row = it < n && sl < NV;
  HT R[NV];
#pragma unroll
  for (int j = 0; j < NV; j++) R[j] = row ? A[((size_t)it * NV + sl) * NV + j] : HT(0);
  vs[upper ? 1 : 0][sl] = row ? v[(size_t)it * NV + sl] : HT(0);
  WSYNC();
  const HT r = matvec_lds<NV>(R, vs[upper ? 1 : 0]);
  if (it < n) out[(size_t)it * HL + sl] = r;
}

// ------------------------------------------------------------------ narrow phase
// case i: geoms (pos, axis) g [n][2][6], sizes sz [n][4] = {r1, h1, r2, h2}, pair function fn [n] ->
// cnt [n] (contacts, 0..2), con [n][2][10] = {pos, n, t1, dist} per contact (zeros past cnt).
// A block holds 2 * NPL cases: sub-lane l < NPL of a half writes its case's geoms to slots 2l, 2l + 1 of
// the half's Scratch (where kinematics leaves them) and calls collide_pair on them.
__global__ __launch_bounds__(64) void k_collide(const HT* g, const HT* sz, const int* fn, int* cnt, HT* con, int n) {
  __shared__ Scratch<HT, Resident<HT>> smem[2];
  const bool upper = threadIdx.x >= HL;
  const int sl = threadIdx.x & (HL - 1);
  const int i = (2 * blockIdx.x + (upper ? 1 : 0)) * NPL + sl;
  const bool on = sl < NPL && i < n;
  Scratch<HT, Resident<HT>>& s = smem[upper ? 1 : 0];
  if (on) {
    for (int q = 0; q < 2; q++)
      for (int k = 0; k < 3; k++) {
        HS_KTAIL(s).gpos[2 * sl + q][k] = g[((size_t)i * 2 + q) * 6 + k];
        HS_KTAIL(s).gax[2 * sl + q][k] = g[((size_t)i * 2 + q) * 6 + 3 + k];
      }
  }
  WSYNC();
  if (!on) return;
  const int f = fn[i];
  if (f < PAIR_PLANE_SPHERE || f > PAIR_CAPSULE_CAPSULE) { cnt[i] = -1; return; }
  const HT size[4] = {sz[4 * (size_t)i], sz[4 * (size_t)i + 1], sz[4 * (size_t)i + 2], sz[4 * (size_t)i + 3]};
  Con<HT> c[2];
  for (int q = 0; q < 2; q++) {
    for (int k = 0; k < 3; k++) c[q].pos[k] = c[q].n[k] = c[q].t1[k] = 0;
    c[q].dist = 0;
  }
  const int nc = collide_pair(s, make_int4(2 * sl, 2 * sl + 1, f, 3), size, c[0], c[1]);
  cnt[i] = nc;
  for (int q = 0; q < 2; q++) {
    HT* o = con + ((size_t)i * 2 + q) * 10;
    const bool w = q < nc;
    for (int k = 0; k < 3; k++) {
      o[k] = w ? c[q].pos[k] : HT(0);
      o[3 + k] = w ? c[q].n[k] : HT(0);
      o[6 + k] = w ? c[q].t1[k] : HT(0);
    }
    o[9] = w ? c[q].dist : HT(0);
  }
}
// f [n][6] = (n, t1 hint) -> out [n][6] = (n, t1) of make_frame
__global__ __launch_bounds__(64) void k_make_frame(const HT* f, HT* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Con<HT> c;
  for (int k = 0; k < 3; k++) { c.pos[k] = 0; c.n[k] = f[6 * (size_t)i + k]; c.t1[k] = f[6 * (size_t)i + 3 + k]; }
  c.dist = 0;
  make_frame(c);
  for (int k = 0; k < 3; k++) { out[6 * (size_t)i + k] = c.n[k]; out[6 * (size_t)i + 3 + k] = c.t1[k]; }
}
// si [n][SOLIMP] (the device record: solimp + the derived constants of fill_solimp), pos, margin [n] -> out [n].
// The record is read through the constant address space, as the model is.
__global__ __launch_bounds__(64) void k_impedance(const HT* si, const HT* pos, const HT* margin, HT* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  out[i] = impedance<HT>((CPtr<HT>)(si + (size_t)SOLIMP * i), pos[i], margin[i]);
}

constexpr int HSU_EARG = -1;
__host__ int blocks_of(int n, int per) { return (n + per - 1) / per; }
__host__ int launched() { return (int)hipGetLastError(); }

}  // namespace
}  // namespace hs

using namespace hs;

#define HSU_ARGS(cond) \
  if (!(cond) || n < 1) return HSU_EARG
#define HSU_GO(kernel, per, ...)                                                                     \
  hipLaunchKernelGGL(kernel, dim3(blocks_of(n, per)), dim3(64), 0, (hipStream_t)stream, __VA_ARGS__); \
  return launched()

extern "C" {
int HSU(rsqrt)(const HT* x, HT* out, int n, void* stream) { HSU_ARGS(x && out); HSU_GO(k_rsqrt, 64, x, out, n); }
int HSU(recip)(const HT* x, HT* out, int n, void* stream) { HSU_ARGS(x && out); HSU_GO(k_recip, 64, x, out, n); }
int HSU(sincos)(const HT* x, HT* s, HT* c, int n, void* stream) { HSU_ARGS(x && s && c); HSU_GO(k_sincos, 64, x, s, c, n); }
int HSU(normalize3)(const HT* v, HT* out, HT* len, int n, void* stream) {
  HSU_ARGS(v && out && len);
  HSU_GO(k_normalize3, 64, v, out, len, n);
}
int HSU(normalize4)(const HT* q, HT* out, int n, void* stream) { HSU_ARGS(q && out); HSU_GO(k_normalize4, 64, q, out, n); }
int HSU(lanes)(const HT* x, HT* sum, HT* rows, HT* up, HT* bc, uint32_t* ballot, int n, void* stream) {
  HSU_ARGS(x && sum && rows && up && bc && ballot);
  HSU_GO(k_lanes, 2, x, sum, rows, up, bc, ballot, n);
}
int HSU(chol)(const HT* A, const HT* b, HT* L, HT* dinv, HT* diag, HT* xs, int ldl, int n, void* stream) {
  HSU_ARGS(A && b && L && dinv && diag && xs);
  if (ldl) { HSU_GO(k_chol<true>, 2, A, b, L, dinv, diag, xs, n); }
  HSU_GO(k_chol<false>, 2, A, b, L, dinv, diag, xs, n);
}
int HSU(fwd)(const HT* L, const HT* dinv, const HT* b, HT* y1, HT* y2, HT* yg, int n, void* stream) {
  HSU_ARGS(L && dinv && b && y1 && y2 && yg);
  HSU_GO(k_fwd, 2, L, dinv, b, y1, y2, yg, n);
}
int HSU(fwd_group)(void) { return GE; }
int HSU(matvec)(const HT* A, const HT* v, HT* out, int n, void* stream) { HSU_ARGS(A && v && out); HSU_GO(k_matvec, 2, A, v, out, n); }
int HSU(collide)(const HT* g, const HT* sz, const int* fn, int* cnt, HT* con, int n, void* stream) {
  HSU_ARGS(g && sz && fn && cnt && con);
  HSU_GO(k_collide, 2 * NPL, g, sz, fn, cnt, con, n);
}
int HSU(make_frame)(const HT* f, HT* out, int n, void* stream) { HSU_ARGS(f && out); HSU_GO(k_make_frame, 64, f, out, n); }
int HSU(impedance)(const HT* si, const HT* pos, const HT* margin, HT* out, int n, void* stream) {
  HSU_ARGS(si && pos && margin && out);
  HSU_GO(k_impedance, 64, si, pos, margin, out, n);
}
}
