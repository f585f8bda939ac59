// The observation normalisation of VecNormalize (SB3 2.3.2 common/vec_env/vec_normalize.py normalize_obs):
// ONE function for every kernel that normalises an obs value -- hs_obs_norm over buffer rows and the fused
// policy's obs load -- so the obs a policy saw during a rollout and the obs the update trains on are
// bitwise equal.  y = clamp((x - m) s, -c, c) in fp32, s = 1 / sqrt(var + eps) precomputed in float64 and
// rounded once (hs_rms_merge).  The subtraction and the product are explicit round-to-nearest operations,
// so no call site can contract them into an FMA.
#pragma once
#include <hip/hip_runtime.h>

namespace hs {

__device__ __forceinline__ float hs_obs_normalize(float x, float m, float s, float c) {
  const float y = __fmul_rn(__fsub_rn(x, m), s);
  return fminf(fmaxf(y, -c), c);
}

}  // namespace hs
