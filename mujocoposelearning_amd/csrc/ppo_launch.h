// Host-side instance dispatch of the templated PPO kernels (product): a launcher turns its runtime
// choices (vector loads or not, row blocks per workgroup, hidden width, activation) into template
// constants by handing each to a generic lambda as a std::integral_constant, and opts an instance
// in to large dynamic LDS through one helper.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hs_act.h"

namespace hs {

// f(std::integral_constant<int, V>) for the V of V0, Vs... that equals v; the last one listed also
// takes every other v (the launchers validate before they dispatch)
template <int V0, int... Vs, typename F>
inline hipError_t with_int(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
  else return v == V0 ? f(std::integral_constant<int, V0>{}) : with_int<Vs...>(v, f);
}

template <typename F>
inline hipError_t with_bool(bool v, F&& f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}

template <typename F>
inline hipError_t with_act(int act, F&& f) {
  return with_int<ACT_TANH, ACT_RELU>(act, f);
}

// dynamic LDS above 64 KiB needs the per-kernel opt-in: set once per kernel instance K and
// process, on first use
template <auto K>
inline hipError_t allow_dynamic_lds(int bytes) {
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return attr;
}

}  // namespace hs
