// hsim policy-net kernels for gfx950 (MI355X): the fused MLP forward and the input-gradient +
// activation-backward pass of the PPO update.  PRODUCT CODE.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hs_act.h"
#include "hs_kernels.h"
#include "ppo_launch.h"

namespace hs {
namespace {

// ------------------------------------------------------------------ fused 2-hidden-layer MLP forward
// out = act(act(X W1' + b1) W2' + b2) W3' + b3 (act = ReLU or Tanh, hs_act.h) for one policy net (PPO rollout: the pi net's mean per
// env step, the vf net's values once per rollout).  The weights come as nn.Linear stores them,
// [out][in] row-major (W1 [H][ld1], W2 [H][ld2], W3 [A][ld3]): the reduction index k is
// contiguous, so one 16-byte load fetches a lane's B operand for four v_mfma_f32_16x16x4_f32 steps.
// Within each group of 16 k the MFMA steps run over a permuted k (step j of lane group ak takes
// k = 16 q + 4 ak + j) so that A (from LDS) and B (from global) are both one b128 per lane per
// group -- the sum over k is the same, only its order differs from the GEMM's.
// The hidden width H (64, 128 or 256) and the activation ACT are template parameters.
// One workgroup per 16 RB rows, H / 32 waves (8 at H = 256): wave w owns output columns
// [32 w, 32 w + 32) of a hidden layer for all the rows (RB row blocks x 2 column tiles of
// accumulators).  Its weight rows are read by no other wave, so they stream straight into VGPRs (the MI355X guide's GEMV rule: no LDS round
// trip), MLP_PF groups ahead of the MFMAs in a register ring, and each 16-byte weight load feeds RB
// row blocks; the input tile and the hidden activations live in LDS (dynamic: sized to D).
// RB = 1 for the per-step pi forward (4096 rows: 256 workgroups, every CU busy), RB = 2 for the
// rollout-buffer vf pass (half the weight traffic per row).
// Replaces three library GEMM launches and their two [N][H] HBM round trips.
// MLP_TPB: the threads of the H = 256 instance (and of dgrad_mask_mfma_kernel, which shares the tiles)
constexpr int MLP_WAVES = 8, MLP_TPB = 64 * MLP_WAVES, MLP_MAXD = 512, MLP_PF = 4;
// above this many rows two row blocks per wave (A/B with each forced, tools/probes/gpu_mlp2_fwd.py,
// profiles/r5i: 4096 rows 23.5 vs 26.6 us, 8192 rows 40.2 vs 26.4 us).  Measured at H = 256 only;
// the H = 64 and 128 instances keep the rule, not re-measured.
constexpr int MLP_RB2_ROWS = 6144;
// LDS row stride (floats) of the hidden tiles: 16-byte aligned rows
__host__ __device__ constexpr int mlp_sh(int H) { return H + 4; }
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__device__ __forceinline__ f32x4 mlp_ld4(const float* __restrict__ p) {
  if constexpr (VEC) return *reinterpret_cast<const f32x4*>(p);
  else return f32x4{p[0], p[1], p[2], p[3]};
}

// acc[rb][t] += A_rb[16 x 16] . B_t[16 x 16] for k-group g: a = LDS base of this lane's A row in
// row block 0 (+ 4 ak), sa = the row-block stride (16 rows) in floats
template <int RB>
__device__ __forceinline__ void mlp_group(const float* a, int sa, int g, const f32x4& b0, const f32x4& b1,
                                          f32x4 (&acc)[RB][2]) {
  f32x4 x[RB];
#pragma unroll
  for (int rb = 0; rb < RB; rb++) x[rb] = *reinterpret_cast<const f32x4*>(a + rb * sa + 16 * g);
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int rb = 0; rb < RB; rb++) {
      acc[rb][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[rb][s], b0[s], acc[rb][0], 0, 0, 0);
      acc[rb][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[rb][s], b1[s], acc[rb][1], 0, 0, 0);
    }
}
// the full k-groups [0, G) of one wave's two column tiles; w0 / w1 = this lane's weight rows (+ 4 ak).
// Every ring refill is unconditional (the group index clamped to G - 1: the last refills re-read
// it) and follows the MFMAs that consumed the slot, so the compiler's wait before a slot's use
// counts only the loads issued after it and the ring needs no register copies.
template <bool VEC, int RB>
__device__ __forceinline__ void mlp_groups(const float* a, int sa, const float* __restrict__ w0,
                                           const float* __restrict__ w1, int G, f32x4 (&acc)[RB][2]) {
  if (G <= 0) return;
  f32x4 bq[MLP_PF][2];
#pragma unroll
  for (int j = 0; j < MLP_PF; j++) {
    const int g = j < G - 1 ? j : G - 1;
    bq[j][0] = mlp_ld4<VEC>(w0 + 16 * g);
    bq[j][1] = mlp_ld4<VEC>(w1 + 16 * g);
  }
  const int Gm = G - G % MLP_PF;
  for (int g0 = 0; g0 < Gm; g0 += MLP_PF) {
#pragma unroll
    for (int j = 0; j < MLP_PF; j++) {
      const int g = g0 + j;
      mlp_group<RB>(a, sa, g, bq[j][0], bq[j][1], acc);
      const int gn = g + MLP_PF < G - 1 ? g + MLP_PF : G - 1;
      bq[j][0] = mlp_ld4<VEC>(w0 + 16 * gn);
      bq[j][1] = mlp_ld4<VEC>(w1 + 16 * gn);
      __builtin_amdgcn_sched_barrier(0);   // keep each refill in its group (the scheduler would batch them)
    }
  }
#pragma unroll
  for (int j = 0; j < MLP_PF - 1; j++)   // the last G % MLP_PF groups, already in slots 0..
    if (Gm + j < G) mlp_group<RB>(a, sa, Gm + j, bq[j][0], bq[j][1], acc);
}

// dynamic LDS of one workgroup: the input tile (row stride roundup16(D) + 4), later layer 2's output
// (stride mlp_sh(H)), then layer 1's output
__host__ __device__ constexpr int mlp_xs_stride(int D, int H) {
  return ((D + 15) & ~15) + 4 > mlp_sh(H) ? ((D + 15) & ~15) + 4 : mlp_sh(H);
}
__host__ __device__ constexpr size_t mlp_lds_bytes(int RB, int D, int H) {
  return (size_t)16 * RB * (mlp_xs_stride(D, H) + mlp_sh(H)) * 4;
}

template <bool VEC, int RB, int H, int ACT>
__global__ __launch_bounds__(2 * H) void mlp2_fwd_kernel(const float* __restrict__ X, int ldx, int D, int N,
                                                           const float* __restrict__ W1, int ld1,
                                                           const float* __restrict__ b1,
                                                           const float* __restrict__ W2, int ld2,
                                                           const float* __restrict__ b2,
                                                           const float* __restrict__ W3, int ld3,
                                                           const float* __restrict__ b3, int A,
                                                           float* __restrict__ out, int ldo) {
  static_assert(H == 64 || H == 128 || H == 256, "hidden width");
  constexpr int R = 16 * RB, TPB = 2 * H, SH = mlp_sh(H), KQ = H / 64;   // H / 32 waves; KQ head k-slices of 64
  extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
  const int sx = mlp_xs_stride(D, H);
  float* xs = mlp_lds;                 // X tile, then layer 2's output
  float* hs = mlp_lds + R * sx;        // layer 1's output, then the head's partial sums
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ar = lane & 15, ak = lane >> 4;   // A: row ar, k 4 ak..; B: column ar, k 4 ak..; C: rows 4 ak.., column ar
  const int row0 = blockIdx.x * R;
  const int Gf = D >> 4, Dp = (D + 15) & ~15;
  if ((D & 3) == 0 && (ldx & 3) == 0 && ((uintptr_t)X & 15) == 0) {   // 16-byte staging: 32 threads per row
    for (int r = threadIdx.x >> 5; r < R; r += TPB / 32) {
      const bool live = row0 + r < N;
      const float* xr = X + (size_t)(live ? row0 + r : 0) * ldx;
      for (int c = 4 * (threadIdx.x & 31); c < Dp; c += 128) {
        const f32x4 v = (live && c < D) ? *reinterpret_cast<const f32x4*>(xr + c) : f32x4{0, 0, 0, 0};
        *reinterpret_cast<f32x4*>(xs + r * sx + c) = v;
      }
    }
  } else {
    for (int e = threadIdx.x; e < R * Dp; e += TPB) {
      const int r = e / Dp, c = e - r * Dp;
      xs[r * sx + c] = (row0 + r < N && c < D) ? X[(size_t)(row0 + r) * ldx + c] : 0.f;
    }
  }
  __syncthreads();
  const int c0 = wave * 32 + ar;   // this lane's column of tile 0 (tile 1: + 16)
  auto epilogue = [&](const f32x4 (&acc)[RB][2], const float* __restrict__ bias, float* dst) {
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const float bb = bias[c0 + 16 * t];
#pragma unroll
      for (int rb = 0; rb < RB; rb++)
#pragma unroll
        for (int r = 0; r < 4; r++)
          dst[(16 * rb + 4 * ak + r) * SH + c0 + 16 * t] = hs_act<ACT>(acc[rb][t][r] + bb);
    }
  };
  {   // layer 1: K = D (full groups pipelined, a partial last group with masked loads)
    f32x4 acc[RB][2] = {};
    const float* w0 = W1 + (size_t)c0 * ld1 + 4 * ak;
    const float* w1 = w0 + (size_t)16 * ld1;
    const float* a = xs + ar * sx + 4 * ak;
    mlp_groups<VEC, RB>(a, 16 * sx, w0, w1, Gf, acc);
    if (D & 15) {
      const int kb = 16 * Gf + 4 * ak;
      f32x4 b0, b1v;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        b0[i] = kb + i < D ? w0[16 * Gf + i] : 0.f;
        b1v[i] = kb + i < D ? w1[16 * Gf + i] : 0.f;
      }
      mlp_group<RB>(a, 16 * sx, Gf, b0, b1v, acc);
    }
    epilogue(acc, b1, hs);
  }
  __syncthreads();
  {   // layer 2: K = H, into xs (the X tile is dead)
    f32x4 acc[RB][2] = {};
    const float* w0 = W2 + (size_t)c0 * ld2 + 4 * ak;
    mlp_groups<VEC, RB>(hs + ar * SH + 4 * ak, 16 * SH, w0, w0 + (size_t)16 * ld2, H / 16, acc);
    epilogue(acc, b2, xs);
  }
  __syncthreads();
  // head: A <= 32 columns = 2 tiles x KQ = H / 64 slices of 64 k over the H / 32 waves (every wave's 4
  // weight loads in flight at once), the slices' partial sums added through LDS (hs is free after
  // layer 2); a lane whose column is >= A reads row A - 1 and multiplies zeros
  {
    const int t = wave & 1, kq = wave >> 1, col = 16 * t + ar;
    if (16 * t < A) {
      const float* w = W3 + (size_t)(col < A ? col : A - 1) * ld3 + 4 * ak + 64 * kq;
      const float keep = col < A ? 1.f : 0.f;
      const float* a = xs + ar * SH + 4 * ak + 64 * kq;
      f32x4 bw[4];
#pragma unroll
      for (int g = 0; g < 4; g++) bw[g] = mlp_ld4<VEC>(w + 16 * g) * keep;
      f32x4 acc[RB] = {};
#pragma unroll
      for (int g = 0; g < 4; g++)
#pragma unroll
        for (int rb = 0; rb < RB; rb++) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(a + 16 * rb * SH + 16 * g);
#pragma unroll
          for (int s = 0; s < 4; s++) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[s], bw[g][s], acc[rb], 0, 0, 0);
        }
#pragma unroll
      for (int rb = 0; rb < RB; rb++)
#pragma unroll
        for (int r = 0; r < 4; r++) hs[(kq * R + 16 * rb + 4 * ak + r) * 32 + col] = acc[rb][r];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < R * A; e += TPB) {
    const int r = e / A, c = e - r * A;
    if (row0 + r >= N) continue;
    float s = hs[r * 32 + c];
    if constexpr (KQ == 2) s += hs[(R + r) * 32 + c];
    if constexpr (KQ == 4) s = (s + hs[(R + r) * 32 + c]) + (hs[(2 * R + r) * 32 + c] + hs[(3 * R + r) * 32 + c]);
    out[(size_t)(row0 + r) * ldo + c] = b3[c] + s;
  }
}

// ------------------------------------------------------------------ input gradient + activation backward
// The backward of a Linear layer whose input x is the previous layer's activation output:
//   GX = (G W) ⊙ act'(X),  partial[wg][n] = sum of GX over the workgroup's rows
// with act' from the activation's output (hs_act_grad): X > 0 for ReLU, 1 - X^2 for Tanh.
// G [B][K] (ldg) is the layer's output gradient, W [K][N] its nn.Linear weight ([out][in]), X [B][N]
// (ldx) its input.  The mask is the previous layer's ReLU backward and the partial sums its bias
// gradient's first pass, so that layer needs no separate pass over [B][N] (autograd writes G W,
// then threshold_backward reads it with X and writes it again, then the bias sum reads it).
// N = 256 (the hidden width).
// K % 16 == 0 (hidden layers, K = 256): the MFMA tiles of mlp2_fwd_kernel on Wt = W' ([N][K], k
// contiguous: dg_transpose_kernel, once per call) so that a lane's B operand of a k-group is one
// 16-byte load; the accumulators go through LDS so that the mask read of X, the GX store and the
// column sums run on whole rows (16-byte accesses) instead of the MFMA's 64-byte column slivers.
// K <= 32 (the heads: 21 actions, 1 value): VALU, the G tile in LDS, a float4 of columns per thread.
constexpr int DG_N = 256, DG_RB4_ROWS = 16384;

// Wt[n][k] = W[k][n] (W [K][ldw], Wt [N][K]): 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void dg_transpose_kernel(const float* __restrict__ W, int ldw, int K, int N,
                                                           float* __restrict__ Wt) {
  __shared__ float t[32][33];
  const int k0 = blockIdx.y * 32, n0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8)
    if (k0 + r < K && n0 + tx < N) t[r][tx] = W[(size_t)(k0 + r) * ldw + n0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (n0 + r < N && k0 + tx < K) Wt[(size_t)(n0 + r) * K + k0 + tx] = t[tx][r];
}

// mask, store and column-sum an [R][DG_N] gradient tile held in LDS (row stride st): thread t owns
// columns 4 (t % 64) .. + 3 of rows t / 64 + TPB / 64 i; the per-thread sums reduce through `red`
// ([TPB / 64][64] float4, may alias the tile after the barrier)
template <int R, int TPB, bool XVEC, int ACT>
__device__ __forceinline__ void dg_finish(const float* tile, int st, const float* __restrict__ X, int ldx, int B,
                                          int row0, float* __restrict__ GX, float* __restrict__ part, f32x4* red) {
  constexpr int P = TPB / 64;
  const int c4 = threadIdx.x & 63, rp = threadIdx.x >> 6;
  f32x4 xv[R / P], gv[R / P];
#pragma unroll
  for (int i = 0; i < R / P; i++) {   // every X load of the thread in flight at once
    const int row = row0 + rp + P * i;
    const float* xr = X + (size_t)(row < B ? row : 0) * ldx + 4 * c4;
    xv[i] = mlp_ld4<XVEC>(xr);
    gv[i] = *reinterpret_cast<const f32x4*>(tile + (rp + P * i) * st + 4 * c4);
  }
  f32x4 cs = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < R / P; i++) {
    const int row = row0 + rp + P * i;
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; q++) v[q] = hs_act_grad<ACT>(gv[i][q], xv[i][q]);
    if (row < B) {
      *reinterpret_cast<f32x4*>(GX + (size_t)row * DG_N + 4 * c4) = v;
      cs += v;
    }
  }
  __syncthreads();   // the tile is read: red may alias it
  red[rp * 64 + c4] = cs;
  __syncthreads();
  if (rp == 0) {
    f32x4 tsum = red[c4];
#pragma unroll
    for (int p = 1; p < P; p++) tsum += red[p * 64 + c4];
    *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * DG_N + 4 * c4) = tsum;
  }
}

__host__ __device__ constexpr int dg_stride(int K) { return (K > DG_N ? K : DG_N) + 4; }

template <int RB, bool XVEC, int ACT>
__global__ __launch_bounds__(MLP_TPB) void dgrad_mask_mfma_kernel(const float* __restrict__ G, int ldg, int K,
                                                                  const float* __restrict__ Wt,
                                                                  const float* __restrict__ X, int ldx, int B,
                                                                  float* __restrict__ GX, float* __restrict__ part) {
  constexpr int R = 16 * RB;
  extern __shared__ __attribute__((aligned(16))) float dg_lds[];
  const int sg = dg_stride(K);                // G tile, then the output tile: 16-byte aligned rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ar = lane & 15, ak = lane >> 4;
  const int row0 = blockIdx.x * R;
  for (int r = threadIdx.x >> 5; r < R; r += MLP_TPB / 32) {   // 32 threads per row, 16-byte loads
    const bool live = row0 + r < B;
    const float* gr = G + (size_t)(live ? row0 + r : 0) * ldg;
    for (int c = 4 * (threadIdx.x & 31); c < K; c += 128)
      *reinterpret_cast<f32x4*>(dg_lds + r * sg + c) = live ? *reinterpret_cast<const f32x4*>(gr + c)
                                                            : f32x4{0, 0, 0, 0};
  }
  __syncthreads();
  const int c0 = wave * 32 + ar;
  f32x4 acc[RB][2] = {};
  const float* w0 = Wt + (size_t)c0 * K + 4 * ak;
  mlp_groups<true, RB>(dg_lds + ar * sg + 4 * ak, 16 * sg, w0, w0 + (size_t)16 * K, K >> 4, acc);
  __syncthreads();   // every wave is done with the G tile
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
      for (int r = 0; r < 4; r++) dg_lds[(16 * rb + 4 * ak + r) * sg + c0 + 16 * t] = acc[rb][t][r];
  __syncthreads();
  dg_finish<R, MLP_TPB, XVEC, ACT>(dg_lds, sg, X, ldx, B, row0, GX, part, reinterpret_cast<f32x4*>(dg_lds));
}

// K <= 32: 32 rows per workgroup; the G tile in LDS (each wave's row of it read as a broadcast),
// W[k][4 c4 .. + 3] one load per k, k outer over the thread's 8 rows
constexpr int DG_SMALL_K = 32, DG_SMALL_R = 32, DG_SMALL_TPB = 256;
template <bool XVEC, int ACT>
__global__ __launch_bounds__(DG_SMALL_TPB) void dgrad_mask_small_kernel(const float* __restrict__ G, int ldg, int K,
                                                                        const float* __restrict__ W, int ldw,
                                                                        const float* __restrict__ X, int ldx, int B,
                                                                        float* __restrict__ GX,
                                                                        float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float gs[DG_SMALL_R][DG_SMALL_K + 1];
  __shared__ __attribute__((aligned(16))) f32x4 tile[DG_SMALL_R * 64];   // [R][256] floats, row stride 256
  const int c4 = threadIdx.x & 63, rp = threadIdx.x >> 6;
  const int row0 = blockIdx.x * DG_SMALL_R;
  for (int e = threadIdx.x; e < DG_SMALL_R * K; e += DG_SMALL_TPB) {
    const int r = e / K, k = e - r * K;
    gs[r][k] = row0 + r < B ? G[(size_t)(row0 + r) * ldg + k] : 0.f;
  }
  __syncthreads();
  constexpr int P = DG_SMALL_TPB / 64, RR = DG_SMALL_R / P;
  f32x4 v[RR] = {};
  for (int k = 0; k < K; k++) {
    const f32x4 w = mlp_ld4<XVEC>(W + (size_t)k * ldw + 4 * c4);
#pragma unroll
    for (int i = 0; i < RR; i++) v[i] += gs[rp + P * i][k] * w;
  }
#pragma unroll
  for (int i = 0; i < RR; i++) tile[(rp + P * i) * 64 + c4] = v[i];
  __syncthreads();
  dg_finish<DG_SMALL_R, DG_SMALL_TPB, XVEC, ACT>(reinterpret_cast<const float*>(tile), DG_N, X, ldx, B, row0, GX, part,
                                            tile);
}

}  // namespace

hipError_t launch_mlp2_fwd(const float* X, int ldx, int D, int N, int H, int act, const float* W1, int ld1,
                           const float* b1, const float* W2, int ld2, const float* b2, const float* W3, int ld3,
                           const float* b3, int A, float* out, int ldo, hipStream_t stream) {
  if ((act != ACT_RELU && act != ACT_TANH) || (H != 64 && H != 128 && H != 256) || D < 1 || D > MLP_MAXD || A < 1 || A > 32 || N < 0 || ld1 < D || ld2 < H ||
      ld3 < H || ldx < D || ldo < A)
    return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  // 16-byte weight loads when every weight row starts 16-byte aligned; two row blocks per wave for
  // large row counts (half the weight traffic; one-block workgroups keep every CU busy below)
  auto al = [](const float* p, int ld) { return ((uintptr_t)p & 15) == 0 && (ld & 3) == 0; };
  const bool vec = al(W1, ld1) && al(W2, ld2) && al(W3, ld3);
  const int RB = N > MLP_RB2_ROWS ? 2 : 1;
  const dim3 grid((N + 16 * RB - 1) / (16 * RB));
  const size_t lds = mlp_lds_bytes(RB, D, H);
  // dynamic LDS above 64 KiB needs the per-kernel opt-in (once per instance)
  return with_int<256, 128, 64>(H, [&](auto h) {
    return with_bool(vec, [&](auto v) {
      return with_int<2, 1>(RB, [&](auto rb) {
        return with_act(act, [&](auto ac) {
          constexpr int HH = decltype(h)::value, B = decltype(rb)::value;
          constexpr auto kernel = &mlp2_fwd_kernel<decltype(v)::value, B, HH, decltype(ac)::value>;
          const hipError_t attr = allow_dynamic_lds<kernel>((int)mlp_lds_bytes(B, MLP_MAXD, HH));
          if (attr != hipSuccess) return attr;
          kernel<<<grid, 2 * HH, lds, stream>>>(X, ldx, D, N, W1, ld1, b1, W2, ld2, b2, W3, ld3, b3, A, out, ldo);
          return hipGetLastError();
        });
      });
    });
  });
}

// row blocks per workgroup of the MFMA instance: 16 rows below MLP_RB2_ROWS, 32 to DG_RB4_ROWS,
// 64 above (each workgroup streams all of Wt: more rows per workgroup, less L2 traffic per row)
static int dg_rb(int B) { return B > DG_RB4_ROWS ? 4 : B > MLP_RB2_ROWS ? 2 : 1; }

size_t dgrad_mask_partial_rows(int B, int K) {
  if (B <= 0) return 0;
  const int R = K <= DG_SMALL_K ? DG_SMALL_R : 16 * dg_rb(B);
  return (size_t)((B + R - 1) / R);
}

size_t dgrad_mask_workspace(int K) { return K <= DG_SMALL_K ? 0 : (size_t)DG_N * K; }

hipError_t launch_dgrad_mask(const float* G, int ldg, int K, const float* W, int ldw, const float* X, int ldx, int B,
                             int N, int act, float* GX, float* partial, float* workspace, hipStream_t stream) {
  if ((act != ACT_RELU && act != ACT_TANH) || B < 0 || N != DG_N || K < 1 || (K > DG_SMALL_K && (K % 16 != 0 || K > MLP_MAXD)) || ldg < K || ldw < N ||
      ldx < N)
    return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const bool xvec = ((uintptr_t)X & 15) == 0 && (ldx & 3) == 0;
  if (K <= DG_SMALL_K) {
    const bool vec = xvec && ((uintptr_t)W & 15) == 0 && (ldw & 3) == 0;   // X and W rows 16-byte aligned
    return with_bool(vec, [&](auto v) {
      return with_act(act, [&](auto ac) {
        hipLaunchKernelGGL((dgrad_mask_small_kernel<decltype(v)::value, decltype(ac)::value>),
                           dim3((B + DG_SMALL_R - 1) / DG_SMALL_R), dim3(DG_SMALL_TPB), 0, stream, G, ldg, K, W, ldw, X,
                           ldx, B, GX, partial);
        return hipGetLastError();
      });
    });
  }
  if (((uintptr_t)G & 15) || (ldg & 3) || !workspace) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dg_transpose_kernel, dim3(DG_N / 32, (K + 31) / 32), dim3(256), 0, stream, W, ldw, K, N, workspace);
  const int RB = dg_rb(B);
  const size_t lds = (size_t)16 * RB * dg_stride(K) * 4;
  return with_int<4, 2, 1>(RB, [&](auto rb) {
    return with_bool(xvec, [&](auto xv) {
      return with_act(act, [&](auto ac) {
        constexpr int BB = decltype(rb)::value;
        constexpr auto kernel = &dgrad_mask_mfma_kernel<BB, decltype(xv)::value, decltype(ac)::value>;
        const hipError_t attr = allow_dynamic_lds<kernel>((int)((size_t)16 * BB * dg_stride(MLP_MAXD) * 4));
        if (attr != hipSuccess) return attr;
        kernel<<<dim3((B + 16 * BB - 1) / (16 * BB)), MLP_TPB, lds, stream>>>(G, ldg, K, workspace, X, ldx, B, GX,
                                                                             partial);
        return hipGetLastError();
      });
    });
  });
}

}  // namespace hs
