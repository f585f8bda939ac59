// The reward plug-ins (reward_functions.py:66-261) on the device: their gathered inputs, the formulas,
// numpy's summation order for the two sums they read, and the step kernel's gather from an env's
// scratch.  reward_eval_kernel (hs_kernels.hip) runs the same formulas on caller-supplied fields.
#pragma once
#include <cmath>

#include "hs_lanes.h"
#include "hs_scratch.h"

namespace hs {
namespace {

// sum |cfrc_ext| of the last two bodies ("feet", reward_functions.py:121-122,176-177)
template <typename T, typename C>
__device__ __forceinline__ void foot_forces(MPtr<T> m, const Scratch<T, C>& s, T& lf, T& rf) {
  const int nb = m->nbody;
  lf = 0;
  rf = 0;
  for (int k = 0; k < 6; k++) { lf += fabs(s.u.n.cfrc[nb - 2][k]); rf += fabs(s.u.n.cfrc[nb - 1][k]); }
}

// The reward plug-ins' inputs, gathered per env.  The step kernel fills them from its scratch
// (compute_reward below); hs_reward_eval (reward_eval_kernel) from caller-supplied fields.  Both run
// the same reward_formula, so the device formulas are pinned directly by the reference's golden vectors.
template <typename T>
struct RewardIn {
  T h, qw, qx, qy, qz;   // qpos[2], qpos[3:7]
  T vx;                  // qvel[0]
  T time;
  T com0, com1;          // subtree_com[0][0:2]
  T comv;                // sum(subtree_linvel[0]^2), numpy order (sequential: 3 < 8 terms)
  T lf, rf;              // sum |cfrc_ext[-2]|, sum |cfrc_ext[-1]| (numpy order: sequential over 6)
  T energy;              // sum((qfrc_actuator[-nj:] * qvel[6:])^2), numpy's pairwise order (np_sum_half)
  T ctrl_sq;             // sum(ctrl^2), numpy's pairwise order
};

// reward_functions.py:66-261 + utils.py:3-21, each expression in the reference's own association
// and without FMA contraction, so the only difference to numpy is the device libm (exp / atan2 / asin).
// The reference's Python min(a, b) is `b if b < a else a` (a NaN first operand is returned as is).
template <typename T, typename KP>
__device__ __forceinline__ T reward_formula(int reward_id, KP kn, const RewardIn<T>& in) {
#pragma clang fp contract(off)
  const T w = in.qw, x = in.qx, y = in.qy, z = in.qz;
  const T roll = atan2(T(2) * (w * x + y * z), T(1) - T(2) * (x * x + y * y));
  const T pitch = asin(T(2) * (w * y - z * x));   // not clamped: |sinp| > 1 -> NaN, as np.arcsin
  const T h = in.h;
  auto pymin = [](T a, T b) { return b < a ? b : a; };
  if (reward_id == REWARD_STAND || reward_id == REWARD_WALK) {
    const T hd = h - T(1.282);
    const T height_reward = exp(T(-2.0) * (hd * hd));
    const T orientation_reward = exp(T(-3.0) * (roll * roll + pitch * pitch));
    const T posture = T(0.5) * height_reward + T(0.5) * orientation_reward;
    const T torque = exp(T(-0.05) * in.ctrl_sq);
    if (reward_id == REWARD_STAND) {                       // :156-211
      if (h < T(0.8)) return T(0);
      const T vd = in.vx - T(1.0);
      const T vr = exp(T(-2.0) * (vd * vd));
      const T total = in.lf + in.rf + T(1e-8);
      const T foot = T(1.0) - pymin(in.lf, in.rf) / total;
      return T(0.4) * vr + T(0.3) * posture + T(0.2) * foot + T(0.1) * torque;
    }
    if (h < T(0.8)) return T(0.1) * h / T(0.8);           // :213-261
    const T vd = in.vx - T(10.0);
    const T vr = exp(T(-0.5) * (vd * vd));
    return vr + posture * torque;
  }
  if (reward_id == REWARD_KNEELING) {                      // :66-154
    // kn: target_height, min_height, max_roll_pitch, com_radius, energy_w, posture_w, com_w, foot_w, alive_w
    if (h < T(kn[1])) return h * h;
    const T mrp = T(kn[2]);
    const T orientation_error = (roll * roll + pitch * pitch) / (mrp * mrp);
    const T posture_reward = exp(T(-5.0) * orientation_error);
    const T hd = h - T(kn[0]);
    const T height_reward = exp(T(-5.0) * (hd * hd));
    const T posture = T(0.7) * posture_reward + T(0.3) * height_reward;
    const T dist = sqrt(in.com0 * in.com0 + in.com1 * in.com1);
    const T com = T(0.7) * exp(T(-10.0) * (dist / T(kn[3]))) + T(0.3) * exp(T(-0.1) * in.comv);
    const T total = in.lf + in.rf + T(1e-8);
    const T foot = pymin(in.lf, in.rf) / total;
    const T energy = exp(T(-0.01) * in.energy);
    const T alive = T(1.0) - exp(T(-0.5) * in.time);
    return T(kn[5]) * posture + T(kn[6]) * com + T(kn[7]) * foot + T(kn[4]) * energy + T(kn[8]) * alive;
  }
  return T(0);
}

// the step kernel's reward: inputs from the env's scratch.  cfrc_ext and subtree_linvel are never
// computed by mj_step without sensors (lazy), so the reference's reward reads zeros for them; with
// full_state, the real wrenches / velocity of post_constraint.
template <typename T, typename C>
__device__ __forceinline__ T compute_reward(MPtr<T> m, const Scratch<T, C>& s, KPtr<T> k, T time,
                                            T energy_sum, T ctrl_sq) {
  RewardIn<T> in;
  in.h = s.qpos[2];
  in.qw = s.qpos[3];
  in.qx = s.qpos[4];
  in.qy = s.qpos[5];
  in.qz = s.qpos[6];
  in.vx = s.qvel[0];
  in.time = time;
  in.com0 = s.com[0];
  in.com1 = s.com[1];
  in.comv = T(0);
  in.lf = T(0);
  in.rf = T(0);
  if (k->p.full_state) {
#pragma clang fp contract(off)
    for (int q = 0; q < 3; q++) in.comv += s.u.n.linv[0][q] * s.u.n.linv[0][q];
    foot_forces(m, s, in.lf, in.rf);
  }
  in.energy = energy_sum;
  in.ctrl_sq = ctrl_sq;
  return reward_formula(k->p.reward_id, k->p.kneel, in);
}

// np.sum's order (numpy pairwise_sum, n <= 128) over the values x_i held by sub-lanes off + i,
// i < n, of each 32-lane half: n < 8 -> ((0 + x0) + x1) + ...; else eight accumulators r_j = x_j +
// x_{j+8} + ... over the whole blocks of 8, combined ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)),
// then the rest added in order.  The block stage and the tree are DPP (row_ror:8, permlane16 swap,
// the quad / half-mirror steps of hsum); the tail is a few lane reads.  off + n <= 32; the result is
// in every lane of the half.  (hsum's butterfly order differs from numpy's by an ulp of the sum,
// which the exp() of a reward term can amplify to several ulp of the reward.)
template <typename T>
__device__ __forceinline__ T np_sum_half(T v, int off, int n, int lane) {
#pragma clang fp contract(off)
  const int base = (lane & HL) + off;
  auto at = [&](int i) { return __shfl(v, base + i, WAVE); };
  T res;
  int i;
  if (n < 8) {
    res = T(0);
    i = 0;
  } else {
    T x = off == 0 ? v : __shfl(v, base + (lane & (HL - 1)), WAVE);   // x_j on sub-lane j
    const int nb = n - n % 8;
    T r = x;
    const T x8 = dpp<0x128>(x);                           // row_ror:8 -> x_{j+8} on sub-lanes 0..7
    if (nb >= 16) r += x8;
    if (nb >= 24) { const T t = x; r += up_row(t); }       // x_{j+16}
    if (nb >= 32) r += up_row(x8);                         // x_{j+24}
    r += dpp<0xB1>(r);                                     // r0 + r1, r2 + r3, ...
    r += dpp<0x4E>(r);                                     // (r0 + r1) + (r2 + r3), ...
    r += dpp<0x141>(r);                                    // ... + ((r4 + r5) + (r6 + r7)) on sub-lane 0
    res = bcast<0>(r);
    i = nb;
  }
  for (; i < n; i++) res += at(i);
  return res;
}

}  // namespace
}  // namespace hs
