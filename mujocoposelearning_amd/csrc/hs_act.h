// Hidden-layer activation of the policy nets (product): ReLU or Tanh, the two an SB3 MlpPolicy is
// built with (activation_fn = nn.ReLU in the reference's config, nn.Tanh by SB3's default).  Shared
// by the fused MLP forward / backward kernels (ppo_mlp.hip, ppo_reduce.hip) and the fused rollout's in-kernel pi net
// (hs_policy.h policy_mean_body), so every path evaluates bitwise the same tanh.
#pragma once
#include <hip/hip_runtime.h>

namespace hs {

// hsim.h's HS_ACT_RELU / HS_ACT_TANH
constexpr int ACT_RELU = 0, ACT_TANH = 1;

// tanh(x) = sign(x) (1 - 2 / (exp(2 |x|) + 1)) on the transcendental unit: one v_exp_f32 and one
// v_rcp_f32 (quarter rate, but only H of them per layer per row).
// * odd by construction (computed on |x|, the sign copied back), exact at 0 (exp2(0) = 1, rcp(2) = 1/2);
// * |x| is clamped at 16, where the fp32 result is 1 already (1 - tanh(16) = 2.5e-14), so exp never
//   overflows and every finite input gives a finite result, +-1 beyond; a NaN stays a NaN;
// * 2 |x| log2(e) is formed as a head and a tail (the product's rounding error, up to 2^-20 at the
//   clamp, would otherwise be an equal relative error of the exponential); the tail enters to first
//   order, e (1 + tail ln 2).
// Absolute error against the exact tanh <= ~2^-23: v_exp_f32's and v_rcp_f32's 1 ulp at the scale of
// 2 / (e + 1) <= 1, and the roundings of e + 1 and of the final fma.
__device__ __forceinline__ float hs_tanh(float x) {
  constexpr float C = 2.8853900817779268f;                // 2 log2(e), rounded to fp32
  constexpr float CL = (float)(2.8853900817779268 - (double)C);
  const float ax = fminf(fabsf(x), 16.0f);
  const float y = ax * C;
  const float yl = fmaf(ax, CL, fmaf(ax, C, -y));
  float e = __builtin_amdgcn_exp2f(y);
  e = fmaf(e, yl * 0.69314718055994531f, e);
  const float t = fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
  return x != x ? x : copysignf(t, x);
}

template <int ACT>
__device__ __forceinline__ float hs_act(float v) {
  static_assert(ACT == ACT_RELU || ACT == ACT_TANH, "activation");
  if constexpr (ACT == ACT_TANH) return hs_tanh(v);
  else return fmaxf(v, 0.f);
}

// the activation's derivative applied to an upstream gradient g, from the activation's OUTPUT y
// (ReLU: y > 0; Tanh: 1 - y^2 -- nothing but the layer's output needs to be kept for the backward)
template <int ACT>
__device__ __forceinline__ float hs_act_grad(float g, float y) {
  static_assert(ACT == ACT_RELU || ACT == ACT_TANH, "activation");
  if constexpr (ACT == ACT_TANH) return g * fmaf(-y, y, 1.0f);
  else return y > 0.f ? g : 0.f;
}

}  // namespace hs
