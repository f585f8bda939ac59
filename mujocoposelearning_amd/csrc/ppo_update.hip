// hsim PPO update kernels for gfx950 (MI355X): the minibatch loss, the KL stop and Adam.  PRODUCT CODE.
//
// SB3 PPO.train's per-minibatch loss terms (stable_baselines3 2.3.2 ppo/ppo.py) over a minibatch
// gathered by idx from the rollout arrays (the torch restatement is ~25 small kernels):
//   a     = adv[idx];  a_n = (a - mean(a)) / (std(a) + 1e-8)       (std unbiased; skipped if B = 1)
//   r     = exp(logp - old_logp[idx])
//   pg    = -mean(min(a_n r, a_n clamp(r, 1 - clip, 1 + clip)))
//   vf    = mean((ret[idx] - v)^2)
// Backward (torch's derivative conventions: min splits ties, clamp passes its closed interval):
//   dpg/dlogp_i = -(1/B) r_i dmin_i,  dmin_i = a_n [s1 < s2] + a_n [r in range] [s1 > s2] + ties / 2
//   dvf/dv_i    = 2 (v_i - ret_i) / B
// The random gathers bound the work (each lane of a gather touches its own cache line), so they
// are spread over LOSS_BLOCKS-wide grids: loss_gather writes the gathered a / old_logp / ret
// compactly (the backward reads those coalesced) with per-block sums of a - a_0 and (a - a_0)^2
// (shifted by the minibatch's first advantage against cancellation); loss_terms reduces those
// partials in a fixed order (deterministic) and forms per-block surrogate / MSE sums; loss_final
// writes the two scalars.  Workspace: 3 B + 4 blocks floats + 2 stats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "hs_kernels.h"

namespace hs {
namespace {

constexpr int LOSS_TPB = 256;

// The _ex forms (hs_ppo_loss_ex, include/hsim.h) read clip_range / clip_range_vf from the device
// hyperparameter block `hp` (HP_*), gather the rollout values when value clipping is on
//   v_c = old_v + clamp(v - old_v, -clip_vf, clip_vf),  vf = mean((ret - v_c)^2),
//   dvf/dv_i = 2 (v_c - ret_i) / B inside the closed interval, 0 outside (torch's clamp)
// and reduce, in the same block order as pg and vf, the sums of (r - 1) - d (SB3's approx_kl,
// d = logp - old_logp) and of [|r - 1| > clip] (its clip_fraction): one more gathered array and
// two more partials per block (workspace 4 B + 6 blocks + 2).  EX = false is hs_ppo_loss unchanged.
template <bool EX> __host__ __device__ constexpr int loss_ng() { return EX ? 4 : 3; }   // gathered arrays
template <bool EX> __host__ __device__ constexpr int loss_ps() { return EX ? 6 : 4; }   // partials per block

// sum over the 64 lanes of a wave, in every lane (a fixed xor tree)
__device__ inline float wave_sum(float v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ inline float block_sum256(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <bool EX>
__global__ __launch_bounds__(LOSS_TPB) void loss_gather_kernel(const int64_t* __restrict__ idx,
                                                               const float* __restrict__ adv,
                                                               const float* __restrict__ ret,
                                                               const float* __restrict__ old_logp,
                                                               const float* __restrict__ old_v,
                                                               const float* __restrict__ hp, int B,
                                                               float* __restrict__ ws) {
  __shared__ float red[LOSS_TPB / 64];
  constexpr int PS = loss_ps<EX>();
  const int i = blockIdx.x * LOSS_TPB + threadIdx.x;
  float* a_g = ws;
  float* old_g = ws + B;
  float* ret_g = ws + 2 * (size_t)B;
  float* part = ws + loss_ng<EX>() * (size_t)B;   // [blocks][PS]: sum d, sum d^2, sum pg, sum vf (, sum kl, clipped)
  const float a0 = adv[idx[0]];
  float d = 0.f;
  if (i < B) {
    const int64_t j = idx[i];
    const float a = adv[j];
    a_g[i] = a;
    old_g[i] = old_logp[j];
    ret_g[i] = ret[j];
    if constexpr (EX)
      if (hp[HP_CLIP_VF] >= 0.f) ws[3 * (size_t)B + i] = old_v[j];
    d = a - a0;
  }
  const float s1 = block_sum256(d, red);
  const float s2 = block_sum256(d * d, red);
  if (threadIdx.x == 0) {
    part[PS * blockIdx.x + 0] = s1;
    part[PS * blockIdx.x + 1] = s2;
  }
}

// sum over blocks of part[PS k + c], by one full wave (lane-strided, then a fixed xor tree: the
// same order in every block and every run)
template <int PS = 4>
__device__ inline float wave_part_sum(const float* part, int nblk, int c) {
  const int l = threadIdx.x & 63;
  float t = 0.f;
  for (int k = l; k < nblk; k += 64) t += part[PS * k + c];
  return wave_sum(t);
}

// mean and 1 / (std + 1e-8) from the per-block shifted sums (called by a whole wave)
// (norm == 0: SB3's normalize_advantage=False -- mean 0, scale 1)
template <bool EX>
__device__ inline void loss_stats(const float* ws, int B, int nblk, float a0, int norm, float& mean, float& inv) {
  const float* part = ws + loss_ng<EX>() * (size_t)B;
  const float s1 = wave_part_sum<loss_ps<EX>()>(part, nblk, 0), s2 = wave_part_sum<loss_ps<EX>()>(part, nblk, 1);
  if (B > 1 && norm) {
    mean = a0 + s1 / (float)B;
    float var = (s2 - s1 * s1 / (float)B) / (float)(B - 1);
    inv = 1.f / (sqrtf(fmaxf(var, 0.f)) + 1e-8f);
  } else {
    mean = 0.f;
    inv = 1.f;
  }
}

template <bool EX>
__global__ __launch_bounds__(LOSS_TPB) void loss_terms_kernel(const float* __restrict__ logp,
                                                              const float* __restrict__ v, int B, float clip_arg,
                                                              const float* __restrict__ hp, int norm,
                                                              float* __restrict__ ws, int nblk) {
  __shared__ float red[LOSS_TPB / 64];
  __shared__ float st[2];
  constexpr int PS = loss_ps<EX>();
  const float* a_g = ws;
  const float* old_g = ws + B;
  const float* ret_g = ws + 2 * (size_t)B;
  float* part = ws + loss_ng<EX>() * (size_t)B;
  if (threadIdx.x < 64) {
    float mu, iv;
    loss_stats<EX>(ws, B, nblk, a_g[0], norm, mu, iv);
    if (threadIdx.x == 0) { st[0] = mu; st[1] = iv; }
  }
  __syncthreads();
  const float mean = st[0], inv = st[1];
  float clip = clip_arg;
  if constexpr (EX) clip = hp[HP_CLIP];
  const int i = blockIdx.x * LOSS_TPB + threadIdx.x;
  float pg = 0.f, vf = 0.f, kl = 0.f, cnt = 0.f;
  if (i < B) {
    const float an = (a_g[i] - mean) * inv;
    const float d = logp[i] - old_g[i];
    const float r = expf(d);
    const float rc = fminf(fmaxf(r, 1.f - clip), 1.f + clip);
    pg = fminf(an * r, an * rc);
    float vp = v[i];
    if constexpr (EX) {
      kl = (r - 1.f) - d;
      cnt = fabsf(r - 1.f) > clip ? 1.f : 0.f;
      const float cv = hp[HP_CLIP_VF];
      if (cv >= 0.f) {
        const float ov = ws[3 * (size_t)B + i];
        vp = ov + fminf(fmaxf(vp - ov, -cv), cv);
      }
    }
    const float e = ret_g[i] - vp;
    vf = e * e;
  }
  pg = block_sum256(pg, red);
  vf = block_sum256(vf, red);
  if constexpr (EX) {
    kl = block_sum256(kl, red);
    cnt = block_sum256(cnt, red);    // whole numbers <= 256 per block, < 2^24 in all: exact
  }
  if (threadIdx.x == 0) {
    part[PS * blockIdx.x + 2] = pg;
    part[PS * blockIdx.x + 3] = vf;
    if constexpr (EX) {
      part[PS * blockIdx.x + 4] = kl;
      part[PS * blockIdx.x + 5] = cnt;
    }
    if (blockIdx.x == 0) {                    // stats for the backward
      float* stats = part + PS * nblk;
      stats[0] = mean;
      stats[1] = inv;
    }
  }
}

__global__ void loss_final_kernel(const float* __restrict__ ws, int B, int nblk, float* __restrict__ pg_out,
                                  float* __restrict__ vf_out) {
  const float* part = ws + 3 * (size_t)B;
  const float pg = wave_part_sum(part, nblk, 2), vf = wave_part_sum(part, nblk, 3);
  if (threadIdx.x != 0) return;
  pg_out[0] = -pg / (float)B;
  vf_out[0] = vf / (float)B;
}

// SB3's `if target_kl is not None and approx_kl_div > 1.5 * target_kl: break`, on the device: the
// minibatch's approx_kl goes into the slot of the current epoch (ctl[CTL_EPOCH], bumped by the host
// between epochs) and, above the threshold hp[HP_KL_STOP] (< 0: no target_kl), sets the stop word
// ctl[CTL_STOP], which hs_adam_clip_ex and every later loss_final_ex read.  One thread.
__device__ inline void kl_decide(float akl, const float* hp, float* stats, int n_epochs, int* ctl) {
  int e = ctl[CTL_EPOCH];
  e = e < 0 ? 0 : (e >= n_epochs ? n_epochs - 1 : e);
  stats[ST_KL + 2 * e] += akl;
  stats[ST_KL + 2 * e + 1] += 1.f;
  stats[ST_KL_LAST] = akl;
  const float thr = hp[HP_KL_STOP];
  if (thr >= 0.f && akl > thr) ctl[CTL_STOP] = 1;
}

// one wave: the two loss scalars and, unless an earlier minibatch of this train() set the stop
// word, this minibatch's SB3 train statistics added to the stats block (ST_*; the tripping
// minibatch is recorded, SB3 appends before it checks).  kl_out != NULL: the approx_kl is only
// written there (world > 1: the decision is hs_ppo_kl_stop's, from the all-reduced value).
__global__ void loss_final_ex_kernel(const float* __restrict__ ws, int B, int nblk, PpoLossEx x,
                                     float* __restrict__ pg_out, float* __restrict__ vf_out) {
  const float* part = ws + 4 * (size_t)B;
  const float pg = wave_part_sum<6>(part, nblk, 2), vf = wave_part_sum<6>(part, nblk, 3);
  const float kl = wave_part_sum<6>(part, nblk, 4), cnt = wave_part_sum<6>(part, nblk, 5);
  // DiagGaussian entropy sum_j (1/2 + log(sqrt(2 pi)) + log_std[j]), A <= 32
  float ent = (int)threadIdx.x < x.A ? 1.41893853320467274f + x.log_std[threadIdx.x] : 0.f;
  ent = wave_sum(ent);
  if (threadIdx.x != 0) return;
  const float pgv = -pg / (float)B, vfv = vf / (float)B, akl = kl / (float)B;
  pg_out[0] = pgv;
  vf_out[0] = vfv;
  if (x.kl_out) x.kl_out[0] = akl;
  if (x.ctl[CTL_STOP] != 0) return;
  const float loss = pgv + x.vf_coef * vfv - x.ent_coef * ent;
  float* st = x.stats;
  st[ST_PG] += pgv;
  st[ST_VF] += vfv;
  st[ST_CLIPFRAC] += cnt / (float)B;
  st[ST_ENT] += ent;
  st[ST_LOSS] += loss;
  st[ST_LOSS_LAST] = loss;
  st[ST_COUNT] += 1.f;
  if (!x.kl_out) kl_decide(akl, x.hp, st, x.n_epochs, x.ctl);
}

__global__ void kl_stop_kernel(const float* __restrict__ kl, const float* __restrict__ hp, float* __restrict__ stats,
                               int n_epochs, int* __restrict__ ctl) {
  if (threadIdx.x != 0 || ctl[CTL_STOP] != 0) return;
  kl_decide(kl[0], hp, stats, n_epochs, ctl);
}

template <bool EX>
__global__ __launch_bounds__(256) void ppo_loss_bwd_kernel(const float* __restrict__ logp,
                                                           const float* __restrict__ v, int B, float clip_arg,
                                                           const float* __restrict__ hp,
                                                           const float* __restrict__ ws, int nblk,
                                                           const float* __restrict__ g_pg,
                                                           const float* __restrict__ g_vf,
                                                           float* __restrict__ g_logp, float* __restrict__ g_v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float* a_g = ws;
  const float* old_g = ws + B;
  const float* ret_g = ws + 2 * (size_t)B;
  const float* stats = ws + loss_ng<EX>() * (size_t)B + loss_ps<EX>() * nblk;
  float clip = clip_arg;
  if constexpr (EX) clip = hp[HP_CLIP];
  const float an = (a_g[i] - stats[0]) * stats[1];
  const float r = expf(logp[i] - old_g[i]);
  const float lo = 1.f - clip, hi = 1.f + clip;
  const float rc = fminf(fmaxf(r, lo), hi);
  const float s1 = an * r, s2 = an * rc;
  const float d1 = an, d2 = (r >= lo && r <= hi) ? an : 0.f;
  const float dmin = s1 < s2 ? d1 : (s1 > s2 ? d2 : 0.5f * (d1 + d2));
  g_logp[i] = g_pg[0] * (-1.f / (float)B) * dmin * r;
  if constexpr (EX) {
    const float cv = hp[HP_CLIP_VF];
    if (cv >= 0.f) {
      const float ov = ws[3 * (size_t)B + i];
      const float dv = v[i] - ov;
      const float vp = ov + fminf(fmaxf(dv, -cv), cv);
      g_v[i] = (dv >= -cv && dv <= cv) ? g_vf[0] * 2.f * (vp - ret_g[i]) / (float)B : 0.f;
      return;
    }
  }
  g_v[i] = g_vf[0] * 2.f * (v[i] - ret_g[i]) / (float)B;
}

// clip_grad_norm_(max_norm) + Adam (torch.optim.Adam, capturable/fused formula) over up to
// ADAM_MAXT parameter tensors per chunk in three launches (torch: a multi-tensor norm, stack, norm, clamp,
// foreach mul and the fused Adam kernel):
//   adam_sqsum   per-block sums of g^2 over the concatenated gradients (fixed order)
//   adam_update  every block reduces those partials (same order) to the clip coefficient
//                min(1, max_norm / (||g|| + 1e-6)), then updates its chunk:
//                  m = b1 m + (1-b1) g c;  v = b2 v + (1-b2) (g c)^2
//                  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),  t = step + 1
//   adam_step    step[i] = t for every tensor (after all blocks have read the old step)
// All tensors take the same number of steps (one optimizer), so tensor 0's step is the clock.
constexpr int ADAM_MAXT = 16, ADAM_TPB = 256, ADAM_PER = 4;
constexpr int ADAM_MAXCHUNK = 64;   // launch_adam_clip handles up to ADAM_MAXT * ADAM_MAXCHUNK tensors

struct AdamArgs {
  float* p[ADAM_MAXT];
  const float* g[ADAM_MAXT];
  float* m[ADAM_MAXT];
  float* v[ADAM_MAXT];
  float* step[ADAM_MAXT];
  long long start[ADAM_MAXT + 1];   // prefix offsets of the tensors in the concatenation
  int nt;
};

__device__ inline int adam_tensor(const AdamArgs& a, long long e) {
  int t = 0;
  while (t + 1 < a.nt && e >= a.start[t + 1]) t++;
  return t;
}

__global__ __launch_bounds__(ADAM_TPB) void adam_sqsum_kernel(AdamArgs a, float* __restrict__ part) {
  __shared__ float red[ADAM_TPB / 64];
  float acc = 0.f;
  const long long base = (long long)blockIdx.x * ADAM_TPB * ADAM_PER;
  for (int k = 0; k < ADAM_PER; k++) {
    const long long e = base + (long long)k * ADAM_TPB + threadIdx.x;
    if (e < a.start[a.nt]) {
      const int t = adam_tensor(a, e);
      const float g = a.g[t][e - a.start[t]];
      acc += g * g;
    }
  }
  // wave_sum, spelled out: through the call this kernel's instructions come out in another order
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// hp / skip (hs_adam_clip_ex; both NULL in hs_adam_clip): lr = hp[HP_LR] from the device block, and
// *skip != 0 (the stop word of the KL early stop) leaves p, m, v and step as they are
__global__ __launch_bounds__(ADAM_TPB) void adam_update_kernel(AdamArgs a, const float* __restrict__ part, int nblk,
                                                               float max_norm, float lr, float b1, float b2,
                                                               float omb1, float omb2, float eps,
                                                               const float* __restrict__ hp,
                                                               const int* __restrict__ skip) {
  __shared__ float coef_s;
  if (skip && *skip != 0) return;   // the whole grid alike: nothing writes the word meanwhile
  if (hp) lr = hp[HP_LR];
  if (threadIdx.x < 64) {
    float t = 0.f;
    for (int k = threadIdx.x; k < nblk; k += 64) t += part[k];
    t = wave_sum(t);
    if (threadIdx.x == 0) coef_s = max_norm > 0.f ? fminf(1.f, max_norm / (sqrtf(t) + 1e-6f)) : 1.f;
  }
  __syncthreads();
  const float c = coef_s;
  const float step = a.step[0][0] + 1.f;
  const float bc1 = 1.f - powf(b1, step), bc2s = sqrtf(1.f - powf(b2, step));
  const float step_size = lr / bc1;
  const long long base = (long long)blockIdx.x * ADAM_TPB * ADAM_PER;
  for (int k = 0; k < ADAM_PER; k++) {
    const long long e = base + (long long)k * ADAM_TPB + threadIdx.x;
    if (e >= a.start[a.nt]) break;
    const int t = adam_tensor(a, e);
    const long long i = e - a.start[t];
    const float g = a.g[t][i] * c;
    const float m = b1 * a.m[t][i] + omb1 * g;        // omb = 1 - beta, rounded once from double
    const float v = b2 * a.v[t][i] + omb2 * g * g;
    a.m[t][i] = m;
    a.v[t][i] = v;
    a.p[t][i] -= step_size * m / (sqrtf(v) / bc2s + eps);
  }
}

__global__ void adam_step_kernel(AdamArgs a, const int* __restrict__ skip) {
  if (skip && *skip != 0) return;
  const float step = a.step[0][0] + 1.f;
  __syncthreads();
  if ((int)threadIdx.x < a.nt) a.step[threadIdx.x][0] = step;
}

}  // namespace

size_t ppo_loss_workspace(int B) {
  const size_t nblk = B > 0 ? ((size_t)B + LOSS_TPB - 1) / LOSS_TPB : 0;
  return 3 * (size_t)B + 4 * nblk + 2;
}

size_t ppo_loss_workspace_ex(int B) {
  const size_t nblk = B > 0 ? ((size_t)B + LOSS_TPB - 1) / LOSS_TPB : 0;
  return 4 * (size_t)B + 6 * nblk + 2;
}

hipError_t launch_ppo_loss_fwd(const float* logp, const float* v, const int64_t* idx, const float* adv,
                               const float* ret, const float* old_logp, int B, float clip, int normalize, float* pg,
                               float* vf, float* ws, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const int nblk = (B + LOSS_TPB - 1) / LOSS_TPB;
  hipLaunchKernelGGL(loss_gather_kernel<false>, dim3(nblk), dim3(LOSS_TPB), 0, stream, idx, adv, ret, old_logp,
                     (const float*)nullptr, (const float*)nullptr, B, ws);
  hipLaunchKernelGGL(loss_terms_kernel<false>, dim3(nblk), dim3(LOSS_TPB), 0, stream, logp, v, B, clip,
                     (const float*)nullptr, normalize, ws, nblk);
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, stream, (const float*)ws, B, nblk, pg, vf);
  return hipGetLastError();
}

hipError_t launch_ppo_loss_bwd(const float* logp, const float* v, int B, float clip, const float* ws,
                               const float* g_pg, const float* g_vf, float* g_logp, float* g_v, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const int nblk = (B + LOSS_TPB - 1) / LOSS_TPB;
  hipLaunchKernelGGL(ppo_loss_bwd_kernel<false>, dim3(nblk), dim3(256), 0, stream, logp, v, B, clip,
                     (const float*)nullptr, ws, nblk, g_pg, g_vf, g_logp, g_v);
  return hipGetLastError();
}

// the same three launches with the hyperparameters read from x.hp, the SB3 diagnostics reduced
// beside pg / vf and the stats / stop-word bookkeeping in the final single-wave kernel
hipError_t launch_ppo_loss_fwd_ex(const float* logp, const float* v, const int64_t* idx, const float* adv,
                                  const float* ret, const float* old_logp, const float* old_v, int B, int normalize,
                                  const PpoLossEx& x, float* pg, float* vf, float* ws, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const int nblk = (B + LOSS_TPB - 1) / LOSS_TPB;
  hipLaunchKernelGGL(loss_gather_kernel<true>, dim3(nblk), dim3(LOSS_TPB), 0, stream, idx, adv, ret, old_logp, old_v,
                     x.hp, B, ws);
  hipLaunchKernelGGL(loss_terms_kernel<true>, dim3(nblk), dim3(LOSS_TPB), 0, stream, logp, v, B, 0.f, x.hp, normalize,
                     ws, nblk);
  hipLaunchKernelGGL(loss_final_ex_kernel, dim3(1), dim3(64), 0, stream, (const float*)ws, B, nblk, x, pg, vf);
  return hipGetLastError();
}

hipError_t launch_ppo_loss_bwd_ex(const float* logp, const float* v, int B, const float* hp, const float* ws,
                                  const float* g_pg, const float* g_vf, float* g_logp, float* g_v,
                                  hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const int nblk = (B + LOSS_TPB - 1) / LOSS_TPB;
  hipLaunchKernelGGL(ppo_loss_bwd_kernel<true>, dim3(nblk), dim3(256), 0, stream, logp, v, B, 0.f, hp, ws, nblk, g_pg,
                     g_vf, g_logp, g_v);
  return hipGetLastError();
}

hipError_t launch_ppo_kl_stop(const float* kl, const float* hp, float* stats, int n_epochs, int* ctl,
                              hipStream_t stream) {
  hipLaunchKernelGGL(kl_stop_kernel, dim3(1), dim3(64), 0, stream, kl, hp, stats, n_epochs, ctl);
  return hipGetLastError();
}

// partial sums of the squared-gradient pass: one per ADAM_TPB * ADAM_PER elements of each chunk of
// ADAM_MAXT tensors (the per-chunk rounding adds at most one partial per chunk)
int adam_partials(long long total) {
  return (int)((total + (long long)ADAM_TPB * ADAM_PER - 1) / ((long long)ADAM_TPB * ADAM_PER)) + ADAM_MAXCHUNK;
}

// Any number of tensors (<= ADAM_MAXT * ADAM_MAXCHUNK): chunks of ADAM_MAXT share one partials
// array, so every update block reduces the partials of ALL chunks to the same clip coefficient;
// the step counters advance after every chunk's update has read them.  hp / skip non-NULL
// (hs_adam_clip_ex): lr from the device block, and no chunk writes anything when *skip != 0.
hipError_t launch_adam_clip(int nt, float* const* p, const float* const* g, float* const* m, float* const* v,
                            float* const* step, const long long* numel, float* part, float max_norm, double lr,
                            double b1, double b2, double eps, hipStream_t stream, const float* hp, const int* skip) {
  if (nt <= 0 || nt > ADAM_MAXT * ADAM_MAXCHUNK) return hipErrorInvalidValue;
  const int nchunk = (nt + ADAM_MAXT - 1) / ADAM_MAXT;
  AdamArgs a[ADAM_MAXCHUNK];
  int nblk[ADAM_MAXCHUNK], off[ADAM_MAXCHUNK + 1];
  off[0] = 0;
  for (int c = 0; c < nchunk; c++) {
    a[c] = AdamArgs{};
    a[c].nt = std::min(ADAM_MAXT, nt - c * ADAM_MAXT);
    a[c].start[0] = 0;
    for (int j = 0; j < a[c].nt; j++) {
      const int t = c * ADAM_MAXT + j;
      a[c].p[j] = p[t];
      a[c].g[j] = g[t];
      a[c].m[j] = m[t];
      a[c].v[j] = v[t];
      a[c].step[j] = step[t];
      a[c].start[j + 1] = a[c].start[j] + numel[t];
    }
    nblk[c] = (int)((a[c].start[a[c].nt] + (long long)ADAM_TPB * ADAM_PER - 1) / ((long long)ADAM_TPB * ADAM_PER));
    off[c + 1] = off[c] + nblk[c];
  }
  if (off[nchunk] <= 0) return hipSuccess;
  for (int c = 0; c < nchunk; c++)
    if (nblk[c]) hipLaunchKernelGGL(adam_sqsum_kernel, dim3(nblk[c]), dim3(ADAM_TPB), 0, stream, a[c], part + off[c]);
  for (int c = 0; c < nchunk; c++)
    if (nblk[c])
      hipLaunchKernelGGL(adam_update_kernel, dim3(nblk[c]), dim3(ADAM_TPB), 0, stream, a[c], (const float*)part,
                         off[nchunk], max_norm, (float)lr, (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2),
                         (float)eps, hp, skip);
  for (int c = 0; c < nchunk; c++) hipLaunchKernelGGL(adam_step_kernel, dim3(1), dim3(64), 0, stream, a[c], skip);
  return hipGetLastError();
}

}  // namespace hs
