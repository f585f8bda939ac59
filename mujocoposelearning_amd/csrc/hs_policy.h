// The fused rollout's and the fused evaluation's policy forward: the SB3 MlpPolicy's pi net on the two
// envs of a wave, inside the step kernel (step_pair's next_action, hs_env_step.h).
#pragma once
#include <cstddef>

#include "hs_act.h"
#include "hs_lanes.h"
#include "hs_norm.h"
#include "hs_scratch.h"

namespace hs {
namespace {

// Fused rollout: the SB3 MlpPolicy's pi net (mlp_extractor.policy_net + action_net, fp32 as SB3's
// policy) on the wave's two envs at once (the lower half-wave's env and the upper's; a ghost half
// mirrors its partner).  Two hidden layers of H = 64 R (R = 1, 2, 4: RolloutArgs::H = 64, 128, 256) with
// the activation ACT (RolloutArgs::hact: ReLU or Tanh, hs_act.h -- the function of mlp2_fwd_kernel):
// lane L (of 64) owns outputs R L .. R L + R - 1 for BOTH envs, so each input costs one 4 R-byte weight
// load per lane (coalesced: the wave reads each weight row once) and two LDS broadcasts (the two envs'
// inputs).  Every output sums its inputs in ascending index, whatever R.  The head: sub-lane sl < A of
// each half owns action sl of its half's env.  The obs rows and hidden activations are staged in each
// half's scratch union (free after the env step; x[512] / h[256] hold every width).  Returns the action
// mean of (this half's env, sub-lane sl), 0 for sl >= A.
// unroll of the hidden layers' loads (groups of 4 rows) and of the head's: measured 1 / 2 / 4 / 8 in
// profiles/ab/ab_r4u_policy_unroll.log (4 and 8 tie), a rolling 16-row ring in ab_r4ae_policy_ring.log
// -- at H = 256 only; the narrower nets (latency-bound: a 256- or 512-byte row per wave) keep them
constexpr int kPolUnroll = 4, kPolHeadUnroll = 16;
// R consecutive floats as one load of 4 R bytes (p is 4 R-byte aligned)
template <int R>
__device__ __forceinline__ void pol_load(const float* p, float (&u)[R]) {
  static_assert(R == 1 || R == 2 || R == 4, "hidden width 64, 128 or 256");
  if constexpr (R == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    u[0] = v.x; u[1] = v.y; u[2] = v.z; u[3] = v.w;
  } else if constexpr (R == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    u[0] = v.x; u[1] = v.y;
  } else {
    u[0] = p[0];
  }
}
// UC: the obs row is the fused evaluation's staging row (uncached memory, rewritten every env step): read
// at agent scope, as the hand-off rows (row_ld)
// NORM: the launch carries VecNormalize's moments (KArgs::nm): each obs value is normalised as it is staged
// (hs_obs_normalize, the function hs_obs_norm runs over the buffer rows), the row in memory stays raw
template <int R, int ACT, bool UC = false, bool NORM = false, typename T, typename C>
__device__ __forceinline__ float policy_mean_body(KPtr<T> k, const float* obs, Scratch<T, C>* smem, int lane) {
  constexpr int H = 64 * R;
  const bool up = lane >= HL;
  const int sl = lane & (HL - 1);
  float* xa = smem[0].u.pol.x;   // lower half's env
  float* xb = smem[1].u.pol.x;   // upper half's env
  float* ha = smem[0].u.pol.h;
  float* hb = smem[1].u.pol.h;
  const int D = k->ro.D, A = k->ro.A, ld1 = k->ro.ld1;
  float* xo = up ? xb : xa;
  if constexpr (NORM) {
    const float* nmean = k->nm.mean;
    const float* nscale = k->nm.inv_std;
    const float nclip = k->nm.clip;
    for (int i = sl; i < D; i += HL) {
      float v;
      if constexpr (UC) v = row_ld(obs + i);
      else v = obs[i];
      xo[i] = hs_obs_normalize(v, nmean[i], nscale[i], nclip);
    }
  } else if constexpr (UC) {
    for (int i = sl; i < D; i += HL) xo[i] = row_ld(obs + i);
  } else {
    for (int i = sl; i < D; i += HL) xo[i] = obs[i];
  }
  WSYNC();
  auto layer = [&](const float* w, int ld, const float* b, const float* ina, const float* inb, int n, float* outa,
                   float* outb) {
    float a[R], c[R];
    pol_load<R>(b + R * lane, a);
#pragma unroll
    for (int j = 0; j < R; j++) c[j] = a[j];
    const float* wl = w + R * lane;
#pragma unroll kPolUnroll
    for (int i = 0; i < n; i += 4) {
      const float4 va = *reinterpret_cast<const float4*>(ina + i);
      const float4 vb = *reinterpret_cast<const float4*>(inb + i);
      const float xs[4] = {va.x, va.y, va.z, va.w}, ys[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
      for (int ii = 0; ii < 4; ii++) {
        float u[R];
        pol_load<R>(wl + (size_t)(i + ii) * ld, u);
#pragma unroll
        for (int j = 0; j < R; j++) a[j] += xs[ii] * u[j];
#pragma unroll
        for (int j = 0; j < R; j++) c[j] += ys[ii] * u[j];
      }
    }
    WSYNC();   // every lane has read the inputs (the outputs may alias them)
#pragma unroll
    for (int j = 0; j < R; j++) {
      outa[R * lane + j] = hs_act<ACT>(a[j]);
      outb[R * lane + j] = hs_act<ACT>(c[j]);
    }
    WSYNC();
  };
  layer(k->ro.w1, ld1, k->ro.b1, xa, xb, D, ha, hb);        // obs -> h1
  layer(k->ro.w2, H, k->ro.b2, ha, hb, H, xa, xb);          // h1 -> h2 (into the obs slots)
  float mean = 0.f;
  if (sl < A) {
    mean = k->ro.b3[sl];
    const float* w3 = k->ro.w3 + sl;
#pragma unroll kPolHeadUnroll
    for (int i = 0; i < H; i++) mean += xo[i] * w3[(size_t)i * A];
  }
  return mean;
}
// The narrow instances are calls, not inlined: inlined beside the 256 ones they cost the rollout kernel
// registers (4 AGPRs more, profiles/rollout_widths.md), and a call per env step is noise next to the step.
// The two 256-wide bodies (ReLU and Tanh) are inlined: together they leave every figure of the kernel
// where it was, and as a call the Tanh one ran the rollout 5 % slower (profiles/tanh_policy.md).
template <int R, int ACT, bool UC = false, bool NORM = false, typename T, typename C>
__device__ __noinline__ float policy_mean_call(KPtr<T> k, const float* obs, Scratch<T, C>* smem, int lane) {
  return policy_mean_body<R, ACT, UC, NORM>(k, obs, smem, lane);
}
// one wave-uniform dispatch on the hidden width and the activation (hs_rollout_act admits 64, 128 and 256,
// ReLU and Tanh only)
template <bool UC = false, bool NORM = false, typename T, typename C>
__device__ __forceinline__ float policy_mean(KPtr<T> k, const float* obs, Scratch<T, C>* smem, int lane) {
  const int H = k->ro.H;
  if (k->ro.hact == ACT_TANH) {
    if (H == 256) return policy_mean_body<4, ACT_TANH, UC, NORM>(k, obs, smem, lane);
    if (H == 128) return policy_mean_call<2, ACT_TANH, UC, NORM>(k, obs, smem, lane);
    return policy_mean_call<1, ACT_TANH, UC, NORM>(k, obs, smem, lane);
  }
  if (H == 256) return policy_mean_body<4, ACT_RELU, UC, NORM>(k, obs, smem, lane);
  if (H == 128) return policy_mean_call<2, ACT_RELU, UC, NORM>(k, obs, smem, lane);
  return policy_mean_call<1, ACT_RELU, UC, NORM>(k, obs, smem, lane);
}

}  // namespace
}  // namespace hs
