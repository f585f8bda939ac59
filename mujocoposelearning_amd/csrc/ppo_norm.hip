// hsim VecNormalize kernels for gfx950 (MI355X): running-moment normalisation of observations and
// rewards (SB3 2.3.2 common/running_mean_std.py, common/vec_env/vec_normalize.py).  PRODUCT CODE.
//
// * obs_norm: one pass over [R][D] float32 rows that writes clamp((x - mean) inv_std, +-clip)
//   (hs_norm.h, the function the fused policy's obs load calls) and, optionally, accumulates the raw
//   rows' column moments in float64.  The moments are taken about a shift, the rows' own first row (a
//   sample lies within a few standard deviations of the mean, so sum d^2 - (sum d)^2 / n loses a few
//   bits where the plain sum of squares loses ten digits at offset 1e3 / std 1e-2).  Every workgroup
//   owns a chunk of rows and writes its (sum d, sum d^2) per column; a second launch adds the chunks in
//   a fixed order.  No atomics: two runs are bitwise equal.
// * rms_merge: Chan's merge of batch moment sets into the running (mean, var, count), float64, in
//   RunningMeanStd.update_from_moments' operation order, and the fp32 mean / inv_std the consumers read.
// * return_moments / reward_scale: VecNormalize's reward path as a post-pass over a rollout's [T][N]
//   rewards and dones.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "hs_kernels.h"
#include "hs_norm.h"
#include "ppo_launch.h"

namespace hs {
namespace {

constexpr int ON_THREADS = 512;     // most threads of an obs_norm workgroup (scalar path: one per column)
constexpr int ON_TARGET = 256;      // threads a workgroup aims at: column groups x row phases
constexpr int ON_MAX_CHUNKS = 1024; // row chunks (workgroups per column tile)
constexpr int ON_FIN_COLS = 64, ON_FIN_PHASES = 16;

template <int W>
__device__ __forceinline__ void ld_vec(const float* p, float (&v)[W]) {
  if constexpr (W == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = p[0];
  }
}
template <int W>
__device__ __forceinline__ void st_vec(float* p, const float (&v)[W]) {
  if constexpr (W == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else p[0] = v[0];
}

// the shift of the moments: the first raw row, copied before the (possibly in-place) pass rewrites it
__global__ void obs_shift_kernel(const float* __restrict__ x, int D, float* __restrict__ shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < D) shift[c] = x[c];
}

// Workgroup: nvc column groups of W floats x PH row phases (nvc PH <= ON_THREADS threads, consecutive
// threads on consecutive addresses of a row); blockIdx.x: the chunk of rows [r0, r1).
// MOM: part[chunk][2][D] gets the chunk's sum d and sum d^2 (d = x - shift) per column, the phases
// combined in ascending order.
template <int W, bool MOM>
__global__ __launch_bounds__(ON_THREADS) void obs_norm_kernel(const float* x, size_t ldx, size_t R, int D, int nvc,
                                                              int PH, size_t rows_per_chunk,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ inv_std, float clip,
                                                              float* out, size_t ldo,
                                                              const float* __restrict__ shift,
                                                              double* __restrict__ part) {
  extern __shared__ double on_lds[];   // MOM: [PH][nvc][2 W]
  const int t = threadIdx.x, vc = t % nvc, ph = t / nvc, c = vc * W;
  const size_t r0 = (size_t)blockIdx.x * rows_per_chunk;
  const size_t r1 = r0 + rows_per_chunk < R ? r0 + rows_per_chunk : R;
  float m[W], s[W], sh[W];
  ld_vec<W>(mean + c, m);
  ld_vec<W>(inv_std + c, s);
  double s1[W], s2[W];
#pragma unroll
  for (int j = 0; j < W; j++) s1[j] = s2[j] = 0.0;
  if constexpr (MOM) ld_vec<W>(shift + c, sh);
  auto row = [&](size_t r, const float (&v)[W]) {
    float y[W];
#pragma unroll
    for (int j = 0; j < W; j++) {
      y[j] = hs_obs_normalize(v[j], m[j], s[j], clip);
      if constexpr (MOM) {
        const double d = (double)v[j] - (double)sh[j];
        s1[j] += d;
        s2[j] += d * d;
      }
    }
    st_vec<W>(out + r * ldo + c, y);
  };
  size_t r = r0 + ph;
  // four rows in flight per thread (x and out may be the same rows, so the loads are issued by hand
  // ahead of the stores); rows are still accumulated in ascending order
  for (; r + 3 * (size_t)PH < r1; r += 4 * (size_t)PH) {
    float v0[W], v1[W], v2[W], v3[W];
    ld_vec<W>(x + r * ldx + c, v0);
    ld_vec<W>(x + (r + PH) * ldx + c, v1);
    ld_vec<W>(x + (r + 2 * (size_t)PH) * ldx + c, v2);
    ld_vec<W>(x + (r + 3 * (size_t)PH) * ldx + c, v3);
    row(r, v0);
    row(r + PH, v1);
    row(r + 2 * (size_t)PH, v2);
    row(r + 3 * (size_t)PH, v3);
  }
  for (; r < r1; r += PH) {
    float v[W];
    ld_vec<W>(x + r * ldx + c, v);
    row(r, v);
  }
  if constexpr (MOM) {
    double* mine = on_lds + ((size_t)ph * nvc + vc) * 2 * W;
#pragma unroll
    for (int j = 0; j < W; j++) {
      mine[j] = s1[j];
      mine[W + j] = s2[j];
    }
    __syncthreads();
    if (ph == 0) {
      for (int k = 1; k < PH; k++) {
        const double* o = on_lds + ((size_t)k * nvc + vc) * 2 * W;
#pragma unroll
        for (int j = 0; j < W; j++) {
          s1[j] += o[j];
          s2[j] += o[W + j];
        }
      }
      double* p = part + (size_t)blockIdx.x * 2 * D;
#pragma unroll
      for (int j = 0; j < W; j++) {
        p[c + j] = s1[j];
        p[D + c + j] = s2[j];
      }
    }
  }
}

// moments[0] = R, moments[1 + c] = mean, moments[1 + D + c] = M2 of column c from the chunk sums: phase
// ph adds chunks ph, ph + 16, ... in ascending order, the 16 phases are then added in ascending order
__global__ __launch_bounds__(ON_FIN_COLS* ON_FIN_PHASES) void obs_moments_finish_kernel(
    const double* __restrict__ part, int chunks, int D, size_t R, const float* __restrict__ shift,
    double* __restrict__ moments) {
  __shared__ double a1[ON_FIN_PHASES][ON_FIN_COLS], a2[ON_FIN_PHASES][ON_FIN_COLS];
  const int lane = threadIdx.x, ph = threadIdx.y, c = blockIdx.x * ON_FIN_COLS + lane;
  double s1 = 0.0, s2 = 0.0;
  if (c < D) {
#pragma unroll 4
    for (int k = ph; k < chunks; k += ON_FIN_PHASES) {
      s1 += part[(size_t)k * 2 * D + c];
      s2 += part[(size_t)k * 2 * D + D + c];
    }
  }
  a1[ph][lane] = s1;
  a2[ph][lane] = s2;
  __syncthreads();
  if (ph == 0 && c < D) {
    s1 = s2 = 0.0;
#pragma unroll
    for (int k = 0; k < ON_FIN_PHASES; k++) {
      s1 += a1[k][lane];
      s2 += a2[k][lane];
    }
    const double n = (double)R;
    const double m2 = s2 - s1 * s1 / n;
    moments[1 + c] = (double)shift[c] + s1 / n;
    moments[1 + D + c] = m2 > 0.0 ? m2 : 0.0;
    if (c == 0) moments[0] = n;
  }
}

// RunningMeanStd.update_from_moments (running_mean_std.py), set by set in ascending order; a set is
// (count, mean[D], M2[D]) -- batch_var * batch_count is M2 -- and one with count 0 is skipped.
// state: (count, mean[D], var[D]).  One workgroup; thread 0 writes the count after every thread read it.
__global__ __launch_bounds__(256) void rms_merge_kernel(double* state, int D, const double* __restrict__ sets,
                                                        int nsets, size_t set_stride, double eps,
                                                        float* __restrict__ mean32, float* __restrict__ inv_std32) {
  const double count0 = state[0];
  double count = count0;
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    double mean = state[1 + c], var = state[1 + D + c];
    count = count0;
    for (int k = 0; k < nsets; k++) {
      const double* b = sets + (size_t)k * set_stride;
      const double bn = b[0];
      if (!(bn > 0.0)) continue;
      const double delta = b[1 + c] - mean;
      const double tot = count + bn;
      const double new_mean = mean + delta * bn / tot;
      const double m_a = var * count;
      const double m_b = b[1 + D + c];
      const double m2 = m_a + m_b + delta * delta * count * bn / tot;
      mean = new_mean;
      var = m2 / tot;
      count = tot;
    }
    state[1 + c] = mean;
    state[1 + D + c] = var;
    if (mean32) mean32[c] = (float)mean;
    if (inv_std32) inv_std32[c] = (float)(1.0 / sqrt(var + eps));
  }
  if (threadIdx.x == 0 && D > 0) state[0] = count;   // D <= blockDim.x or not, thread 0 owns column 0
}

// VecNormalize.step_wait's self.returns = self.returns * gamma + reward over a rollout: one thread per env
// scans t = 0 .. T - 1, writes the step's returns (before the done envs are zeroed, as ret_rms sees them)
// to ret[t][n] and leaves the carry for the next rollout
__global__ void return_scan_kernel(const float* __restrict__ rew, const uint8_t* __restrict__ done, int T, int N,
                                   double gamma, double* __restrict__ carry, double* __restrict__ ret) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double r = carry[n];
  for (int t = 0; t < T; t++) {
    const size_t i = (size_t)t * N + n;
    r = r * gamma + (double)rew[i];
    ret[i] = r;
    if (done[i]) r = 0.0;
  }
  carry[n] = r;
}

// fixed-order workgroup sum: thread partials combined in ascending thread order by thread 0
__device__ __forceinline__ double block_sum_256(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x < 64) {   // 64 partial sums of 4, then one thread: two short fixed-order stages
    s = (lds[4 * threadIdx.x] + lds[4 * threadIdx.x + 1]) + (lds[4 * threadIdx.x + 2] + lds[4 * threadIdx.x + 3]);
  }
  __syncthreads();
  if (threadIdx.x < 64) lds[threadIdx.x] = s;
  __syncthreads();
  s = 0.0;
  for (int k = 0; k < 64; k++) s += lds[k];   // every thread: the same order, the same result
  __syncthreads();
  return s;
}

// out[t] = (N, mean, M2) of ret[t][0 .. N): two passes (mean, then squared deviations), workgroup t
__global__ __launch_bounds__(256) void return_moments_kernel(const double* __restrict__ ret, int N,
                                                             double* __restrict__ out) {
  __shared__ double lds[256];
  const double* row = ret + (size_t)blockIdx.x * N;
  double s = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) s += row[n];
  const double mean = block_sum_256(s, lds) / (double)N;
  double q = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) {
    const double d = row[n] - mean;
    q += d * d;
  }
  const double m2 = block_sum_256(q, lds);
  if (threadIdx.x == 0) {
    double* o = out + (size_t)blockIdx.x * 3;
    o[0] = (double)N;
    o[1] = mean;
    o[2] = m2;
  }
}

// ret_rms.update(self.returns) step by step (one thread): step t's batch is the union of the nsets sets
// sets[k][t] (one per rank, merged in ascending k), merged into state = (count, mean, var); scale[t] =
// sqrt(var + eps) with the variance AFTER step t's merge, as VecNormalize.step_wait normalises
__global__ void ret_merge_kernel(double* state, const double* __restrict__ sets, int nsets, size_t set_stride, int T,
                                 double eps, double* __restrict__ scale) {
  if (blockIdx.x || threadIdx.x) return;
  double count = state[0], mean = state[1], var = state[2];
  for (int t = 0; t < T; t++) {
    double bn = 0.0, bm = 0.0, bq = 0.0;
    for (int k = 0; k < nsets; k++) {
      const double* b = sets + (size_t)k * set_stride + (size_t)t * 3;
      if (!(b[0] > 0.0)) continue;
      if (bn == 0.0) {
        bn = b[0]; bm = b[1]; bq = b[2];
        continue;
      }
      const double delta = b[1] - bm, tot = bn + b[0];
      bq = bq + b[2] + delta * delta * bn * b[0] / tot;
      bm = bm + delta * b[0] / tot;
      bn = tot;
    }
    if (bn > 0.0) {
      const double delta = bm - mean, tot = count + bn;
      const double new_mean = mean + delta * bn / tot;
      const double m2 = var * count + bq + delta * delta * count * bn / tot;
      mean = new_mean;
      var = m2 / tot;
      count = tot;
    }
    scale[t] = sqrt(var + eps);
  }
  state[0] = count;
  state[1] = mean;
  state[2] = var;
}

// rew[t][n] = clip(rew[t][n] / sqrt(var_t + eps), +-clip) (normalize_reward), the quotient in float64
__global__ void reward_scale_kernel(float* __restrict__ rew, const double* __restrict__ scale, int T, int N,
                                    double clip) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)T * N) return;
  const double y = (double)rew[i] / scale[i / N];
  rew[i] = (float)fmin(fmax(y, -clip), clip);
}

struct ObsNormPlan {
  int W, nvc, PH, chunks;
  size_t rpc;
};
ObsNormPlan obs_norm_plan(const float* x, size_t ldx, float* out, size_t ldo, size_t R, int D, const float* mean,
                          const float* inv_std) {
  ObsNormPlan p;
  const bool vec = D % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 &&
                   !(((uintptr_t)x | (uintptr_t)out | (uintptr_t)mean | (uintptr_t)inv_std) & 15);
  p.W = vec ? 4 : 1;
  p.nvc = D / p.W;
  p.PH = ON_TARGET / p.nvc < 1 ? 1 : ON_TARGET / p.nvc;
  // chunks of >= 4 rows per phase, at most ON_MAX_CHUNKS of them
  size_t chunks = (R + (size_t)4 * p.PH - 1) / ((size_t)4 * p.PH);
  if (chunks > ON_MAX_CHUNKS) chunks = ON_MAX_CHUNKS;
  if (chunks < 1) chunks = 1;
  p.rpc = (R + chunks - 1) / chunks;
  p.chunks = (int)((R + p.rpc - 1) / p.rpc);
  return p;
}

}  // namespace

size_t obs_norm_workspace(size_t R, int D) {
  // the shift row (D floats, padded to doubles) + ON_MAX_CHUNKS chunk sums of 2 D doubles
  (void)R;
  return ((size_t)(D + 1) / 2 + (size_t)ON_MAX_CHUNKS * 2 * D) * sizeof(double);
}

hipError_t launch_obs_norm(const float* x, size_t ldx, size_t R, int D, const float* mean, const float* inv_std,
                           float clip, float* out, size_t ldo, double* moments, void* workspace, hipStream_t stream) {
  if (R == 0 || D <= 0) return hipSuccess;
  if (D > ON_THREADS) return hipErrorInvalidValue;
  const ObsNormPlan p = obs_norm_plan(x, ldx, out, ldo, R, D, mean, inv_std);
  if (p.nvc > ON_THREADS) return hipErrorInvalidValue;
  float* shift = (float*)workspace;
  double* part = (double*)workspace + (D + 1) / 2;
  const dim3 grid(p.chunks), block(p.nvc * p.PH);
  const size_t lds = moments ? (size_t)p.PH * p.nvc * 2 * p.W * sizeof(double) : 0;
  if (moments) hipLaunchKernelGGL(obs_shift_kernel, dim3((D + 255) / 256), dim3(256), 0, stream, x, D, shift);
  const hipError_t rc = with_bool(p.W == 4, [&](auto vec) {
    constexpr int W = decltype(vec)::value ? 4 : 1;
    return with_bool(moments != nullptr, [&](auto mom) {
      hipLaunchKernelGGL((obs_norm_kernel<W, decltype(mom)::value>), grid, block, lds, stream, x, ldx, R, D, p.nvc,
                         p.PH, p.rpc, mean, inv_std, clip, out, ldo, (const float*)shift, part);
      return hipGetLastError();
    });
  });
  if (rc != hipSuccess || !moments) return rc;
  hipLaunchKernelGGL(obs_moments_finish_kernel, dim3((D + ON_FIN_COLS - 1) / ON_FIN_COLS),
                     dim3(ON_FIN_COLS, ON_FIN_PHASES), 0, stream, (const double*)part, p.chunks, D, R,
                     (const float*)shift, moments);
  return hipGetLastError();
}

hipError_t launch_rms_merge(double* state, int D, const double* sets, int nsets, size_t set_stride, double eps,
                            float* mean32, float* inv_std32, hipStream_t stream) {
  if (D <= 0) return hipSuccess;
  hipLaunchKernelGGL(rms_merge_kernel, dim3(1), dim3(256), 0, stream, state, D, sets, nsets, set_stride, eps, mean32,
                     inv_std32);
  return hipGetLastError();
}

hipError_t launch_return_moments(const float* rew, const uint8_t* done, int T, int N, double gamma, double* carry,
                                 double* ret_ws, double* out, hipStream_t stream) {
  if (T <= 0 || N <= 0) return hipSuccess;
  hipLaunchKernelGGL(return_scan_kernel, dim3((N + 127) / 128), dim3(128), 0, stream, rew, done, T, N, gamma, carry,
                     ret_ws);
  hipLaunchKernelGGL(return_moments_kernel, dim3(T), dim3(256), 0, stream, (const double*)ret_ws, N, out);
  return hipGetLastError();
}

hipError_t launch_reward_scale(float* rew, int T, int N, double* state, const double* sets, int nsets,
                               size_t set_stride, double eps, double clip, double* scale_ws, hipStream_t stream) {
  if (T <= 0 || N <= 0) return hipSuccess;
  hipLaunchKernelGGL(ret_merge_kernel, dim3(1), dim3(1), 0, stream, state, sets, nsets, set_stride, T, eps, scale_ws);
  const size_t tot = (size_t)T * N;
  hipLaunchKernelGGL(reward_scale_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, rew,
                     (const double*)scale_ws, T, N, clip);
  return hipGetLastError();
}

}  // namespace hs
