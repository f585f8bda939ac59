// Diagnostic per-phase clock of the HS_TIMING build (libhsim_timing.so, never the product):
// PhaseClock, HS_STAMP and HS_FLUSH -- s_memtime stamps accumulated per phase and summed over waves
// into dbg[8000 + slot].  The product build compiles all three to nothing.
#pragma once
#include <cstdint>

#include "hs_lanes.h"

namespace hs {
namespace {

#ifdef HS_TIMING
constexpr int NSLOT = 29;
struct PhaseClock {
  uint64_t acc[NSLOT] = {0};
  uint64_t prev = 0, t0 = 0, rt0 = 0;   // rt0: s_memrealtime (100 MHz, one clock for all XCDs)
  __device__ __forceinline__ void start() { prev = t0 = __builtin_amdgcn_s_memtime(); rt0 = __builtin_amdgcn_s_memrealtime(); }
  __device__ __forceinline__ void stamp(int slot) {
    uint64_t now = __builtin_amdgcn_s_memtime();
    uint64_t d = now - prev;
    asm volatile("" : "+v"(d));   // accumulate in VGPRs (stamps sit in divergent regions too)
    acc[slot] += d;
    prev = now;
  }
};
#define HS_STAMP(clk, slot) (clk).stamp(slot)
// flushed once, inside the substep loop at its exits: a per-lane accumulator live past the loop
// trips an isel bug ("illegal VGPR to SGPR copy") in this compiler.  Expands inside step_pair
// (hs_env_step.h) and names its locals.
#define HS_FLUSH()                                                                              \
  do {                                                                                           \
    T* dbg_ = opaque(ka)->b.dbg;                                                                 \
    if (dbg_ && !WIDE) {                                                                         \
      if (sl == 0)                                                                               \
        for (int q = 0; q < NSLOT; q++) { atomicAdd(&dbg_[8000 + q], (T)st.clk.acc[q]); st.clk.acc[q] = 0; } \
      if (sl == 0) atomicAdd(&dbg_[8030], (T)tot_iter);                                          \
      if (lane == 0 && blockIdx.x < 2048) dbg_[9000 + blockIdx.x] = (T)(st.clk.prev - st.clk.t0);  \
      if (lane == 0 && blockIdx.x < 2048) {                                                      \
        dbg_[16384 + blockIdx.x] = (T)(uint32_t)(st.clk.rt0 & 0xFFFFFFu);                          \
        dbg_[18432 + blockIdx.x] = (T)(uint32_t)(__builtin_amdgcn_s_memrealtime() & 0xFFFFFFu);    \
      }                                                                                          \
      if (sl == 0 && blockIdx.x < 2048) dbg_[11100 + 2 * blockIdx.x + (up ? 1 : 0)] = (T)tot_iter;  \
      if (lane == 0 && titem >= 0 && titem < 4096) {   /* queued items: realtime start / end */  \
        dbg_[20480 + 2 * titem] = (T)(uint32_t)(st.clk.rt0 & 0xFFFFFFu);                            \
        dbg_[20480 + 2 * titem + 1] = (T)(uint32_t)(__builtin_amdgcn_s_memrealtime() & 0xFFFFFFu);  \
      }                                                                                          \
      tot_iter = 0;                                                                              \
    }                                                                                            \
  } while (0)
#else
#define HS_FLUSH() ((void)0)
struct PhaseClock {
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void stamp(int) {}
};
#define HS_STAMP(clk, slot) ((void)0)
#endif

}  // namespace
}  // namespace hs
