// hsim PPO rollout kernels for gfx950 (MI355X).  PRODUCT CODE.
//
// The per-step bookkeeping of SB3 2.3.2 PPO.collect_rollouts (stable_baselines3/common/
// on_policy_algorithm.py), which the reference's PPO.learn runs n_steps times per rollout
// (train_sb3.py:229), as two launches per env step around the policy GEMMs and the env kernel:
//
//   ppo_act_kernel   ActorCriticPolicy.forward's DiagGaussianDistribution.sample() + log_prob()
//                    (common/distributions.py) on the policy heads, the clip of the actions to
//                    the action space (on_policy_algorithm.py: np.clip(actions, low, high)) and
//                    the rollout-buffer writes of step t (actions, values, log_probs,
//                    episode_starts; common/buffers.py RolloutBuffer.add)
//   ppo_post_kernel  the step's reward bookkeeping: time-limit bootstrap
//                    r += gamma V(terminal_obs) for envs with TimeLimit.truncated (or, deferred,
//                    the boot flags and terminal-obs rows for one batched V at rollout end)
//                    (on_policy_algorithm.py: infos[idx]["TimeLimit.truncated"]), dones,
//                    episode-return accumulation, the new episode_starts, and the copy of the
//                    next observation into the rollout buffer's slot t+1
//
// Both are HBM/launch-bound elementwise work (no GEMM shape), so they are laid out for
// coalescing: ppo_act maps a half-wave (32 lanes) onto one env's action vector (A <= 32), so
// a wave touches two consecutive 84 B head rows and the log-prob sum is a 5-step DPP/swizzle
// reduction within the half-wave; ppo_post moves the [N][D] observation copy as 16 B vectors.
//
// Noise: Philox4x32-10 (Salmon et al., SC'11) keyed by the 64-bit seed, counter =
// (env * 32 + action index, rollout-step counter), and a Box-Muller transform of two of its
// words: a counter-based stream, so every (env, step, action) draw is independent of the
// launch shape and reproducible from (seed, counter).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hs_kernels.h"
#include "hs_philox.h"

namespace hs {
namespace {

__global__ __launch_bounds__(256) void ppo_act_kernel(const float* __restrict__ mean, int mean_ld,
                                                      const float* __restrict__ value, int value_ld,
                                                      const float* __restrict__ log_std,
                                                      const float* __restrict__ episode_start, uint32_t k0,
                                                      uint32_t k1, uint64_t counter,
                                                      const uint64_t* __restrict__ counter_base, int deterministic,
                                                      float* __restrict__ act, float* __restrict__ act_clip,
                                                      float* __restrict__ logp, float* __restrict__ val,
                                                      float* __restrict__ start_out, int N, int A) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = gid >> 5, j = gid & 31;
  if (n >= N) return;                         // whole half-waves exit together (N*32 lanes)
  float term = 0.f;
  if (j < A) {
    const float m = mean[(size_t)n * mean_ld + j];
    const float ls = log_std[j];
    float z = 0.f;
    if (!deterministic) {
      const uint64_t c = counter + (counter_base ? *counter_base : 0ull);
      z = policy_noise((uint32_t)n, (uint32_t)j, c, k0, k1);   // counter block (env * 32 + j, env >> 27, c)
    }
    const float a = m + __expf(ls) * z;
    const size_t i = (size_t)n * A + j;
    act[i] = a;
    act_clip[i] = fminf(fmaxf(a, -1.0f), 1.0f);
    // DiagGaussian log_prob: sum_j -((a-m)^2 / (2 sigma^2)) - log sigma - log(sqrt(2 pi))
    term = -0.5f * z * z - ls - 0.91893853320467274f;
  }
  const float lp = half_sum(term);
  if (j == 0) {
    logp[n] = lp;
    val[n] = value[(size_t)n * value_ld];
    start_out[n] = episode_start[n];
  }
}

__global__ __launch_bounds__(256) void ppo_post_kernel(const float* __restrict__ reward,
                                                       const uint8_t* __restrict__ terminated,
                                                       const uint8_t* __restrict__ truncated,
                                                       const float* __restrict__ terminal_value,
                                                       const float* __restrict__ terminal_obs,
                                                       float* __restrict__ boot_obs_out,
                                                       uint8_t* __restrict__ boot_out, float gamma,
                                                       const float* __restrict__ obs, float* __restrict__ obs_out,
                                                       size_t obs_n, int vec4, float* __restrict__ reward_out,
                                                       uint8_t* __restrict__ done_out, double* __restrict__ ep_acc,
                                                       double* __restrict__ ep_return_out,
                                                       float* __restrict__ episode_start, int N, int obs_dim) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (vec4) {   // 16 B-aligned pointers, obs_n = floats / 4
    const float4* __restrict__ src = reinterpret_cast<const float4*>(obs);
    float4* __restrict__ dst = reinterpret_cast<float4*>(obs_out);
    for (size_t i = gid; i < obs_n; i += stride) dst[i] = src[i];
  } else {
    for (size_t i = gid; i < obs_n; i += stride) obs_out[i] = obs[i];
  }
  if (gid < (size_t)N) {
    const bool term = terminated[gid] != 0, trunc = truncated[gid] != 0;
    const float r = reward[gid];
    // TimeLimit.truncated = truncated and not terminated: bootstrap from V(terminal obs), now
    // (terminal_value given) or deferred to the end of the rollout (boot flag + the terminal obs
    // row kept in boot_obs_out; rows are copied only for the rare boot envs)
    const bool boot = trunc && !term;
    if (terminal_value) {
      reward_out[gid] = boot ? r + gamma * terminal_value[gid] : r;
    } else {
      reward_out[gid] = r;
      boot_out[gid] = boot;
      if (boot)
        for (int k = 0; k < obs_dim; k++)
          boot_obs_out[gid * obs_dim + k] = terminal_obs[gid * obs_dim + k];
    }
    const bool done = term || trunc;
    const double acc = ep_acc[gid] + (double)r;
    done_out[gid] = done;
    ep_return_out[gid] = acc;
    ep_acc[gid] = done ? 0.0 : acc;
    episode_start[gid] = done ? 1.0f : 0.0f;
  }
}

// DiagGaussianDistribution.log_prob of given actions (SB3 common/distributions.py), the PPO
// update's evaluate_actions, and its backward: with z = (a - mean) / sigma and upstream g = dL/dlogp,
//   logp       = sum_j (-z_j^2 / 2 - log sigma_j) - A log(sqrt(2 pi))
//   dL/dmean_j = g z_j / sigma_j
//   dL/dlog sigma_j = sum_rows g (z_j^2 - 1)     (the per-row terms are written to `gls_rows`;
//                                                the batch sum is colsum_kernel's)
// Half-wave per row (A <= 32), as ppo_act_kernel.
__global__ __launch_bounds__(256) void gauss_logp_kernel(const float* __restrict__ mean, int mean_ld,
                                                         const float* __restrict__ act,
                                                         const float* __restrict__ log_std,
                                                         float* __restrict__ logp, int N, int A) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = gid >> 5, j = gid & 31;
  if (n >= N) return;
  float term = 0.f;
  if (j < A) {
    const float ls = log_std[j];
    const float z = (act[(size_t)n * A + j] - mean[(size_t)n * mean_ld + j]) * __expf(-ls);
    term = -0.5f * z * z - ls - 0.91893853320467274f;
  }
  const float lp = half_sum(term);
  if (j == 0) logp[n] = lp;
}

__global__ __launch_bounds__(256) void gauss_logp_grad_kernel(const float* __restrict__ mean, int mean_ld,
                                                              const float* __restrict__ act,
                                                              const float* __restrict__ log_std,
                                                              const float* __restrict__ g_logp,
                                                              float* __restrict__ g_mean,
                                                              float* __restrict__ gls_rows, int N, int A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // element of [N][A]
  if (i >= (size_t)N * A) return;
  const size_t n = i / A;
  const int j = (int)(i - n * A);
  const float ls = log_std[j];
  const float inv = __expf(-ls);
  const float z = (act[i] - mean[n * mean_ld + j]) * inv;
  const float g = g_logp[n];
  g_mean[i] = g * z * inv;
  gls_rows[i] = g * (z * z - 1.0f);
}

}  // namespace

hipError_t launch_ppo_act(const float* mean, int mean_ld, const float* value, int value_ld, const float* log_std,
                          const float* episode_start, uint64_t seed, uint64_t counter, const uint64_t* counter_base,
                          int deterministic, float* act,
                          float* act_clip, float* logp, float* val, float* start_out, int N, int A,
                          hipStream_t stream) {
  if (N <= 0) return hipSuccess;
  const size_t threads = (size_t)N * 32;
  const int block = 256;
  const dim3 grid((unsigned)((threads + block - 1) / block));
  hipLaunchKernelGGL(ppo_act_kernel, grid, dim3(block), 0, stream, mean, mean_ld, value, value_ld, log_std,
                     episode_start, (uint32_t)seed, (uint32_t)(seed >> 32), counter, counter_base, deterministic, act,
                     act_clip, logp, val, start_out, N, A);
  return hipGetLastError();
}

hipError_t launch_ppo_post(const float* reward, const uint8_t* terminated, const uint8_t* truncated,
                           const float* terminal_value, const float* terminal_obs, float* boot_obs_out,
                           uint8_t* boot_out, int obs_dim, float gamma, const float* obs, float* obs_out,
                           size_t obs_floats, float* reward_out, uint8_t* done_out, double* ep_acc,
                           double* ep_return_out, float* episode_start, int N, hipStream_t stream) {
  if (N <= 0) return hipSuccess;
  const int vec4 = obs_floats % 4 == 0 && ((uintptr_t)obs | (uintptr_t)obs_out) % 16 == 0;
  const size_t obs_n = vec4 ? obs_floats / 4 : obs_floats;
  const size_t work = obs_n > (size_t)N ? obs_n : (size_t)N;
  const int block = 256;
  // one 16 B vector per lane per pass, at most 8 passes' worth of workgroups resident
  size_t blocks = (work + block - 1) / block;
  if (blocks > 2048) blocks = 2048;
  if (blocks * block < (size_t)N) blocks = ((size_t)N + block - 1) / block;
  hipLaunchKernelGGL(ppo_post_kernel, dim3((unsigned)blocks), dim3(block), 0, stream, reward, terminated, truncated,
                     terminal_value, terminal_obs, boot_obs_out, boot_out, gamma, obs, obs_out, obs_n, vec4,
                     reward_out, done_out, ep_acc, ep_return_out, episode_start, N, obs_dim);
  return hipGetLastError();
}

hipError_t launch_gauss_logp(const float* mean, int mean_ld, const float* act, const float* log_std, float* logp, int N,
                             int A, hipStream_t stream) {
  if (N <= 0) return hipSuccess;
  const size_t threads = (size_t)N * 32;
  hipLaunchKernelGGL(gauss_logp_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, mean, mean_ld,
                     act, log_std, logp, N, A);
  return hipGetLastError();
}

hipError_t launch_gauss_logp_grad(const float* mean, int mean_ld, const float* act, const float* log_std,
                                  const float* g_logp, float* g_mean, float* gls_rows, int N, int A,
                                  hipStream_t stream) {
  if (N <= 0) return hipSuccess;
  const size_t el = (size_t)N * A;
  hipLaunchKernelGGL(gauss_logp_grad_kernel, dim3((unsigned)((el + 255) / 256)), dim3(256), 0, stream, mean, mean_ld,
                     act, log_std, g_logp, g_mean, gls_rows, N, A);
  return hipGetLastError();
}

}  // namespace hs
