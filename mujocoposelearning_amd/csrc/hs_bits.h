// Bit walking of the chain / subtree sums in groups (for_bits_g, hs_lanes.h).  No device intrinsic
// beyond __builtin_ctz, so a host compiler builds it too: tools/for_bits_check.cpp walks it under
// the sanitizers (tests/test_for_bits_groups.py).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HS_BITS_FN __device__ __forceinline__
#define HS_BITS_UNROLL _Pragma("unroll")
#else
#define HS_BITS_FN inline
#define HS_BITS_UNROLL
#endif

namespace hs {

// One round: the lowest G set bits of a mask, ascending.
template <int G>
struct BitGroup {
  int j[G];   // slot g's bit; a slot at or past n repeats slot 0's bit, so a read at it stays in bounds
  int n;      // slots in use: min(G, popcount), 0 only for an empty mask
};
// takes the round's bits out of mk
template <int G>
HS_BITS_FN BitGroup<G> take_bits(uint32_t& mk) {
  BitGroup<G> r;
  r.n = 0;
  HS_BITS_UNROLL
  for (int g = 0; g < G; g++) {
    const bool on = mk != 0u;
    r.j[g] = on ? __builtin_ctz(mk) : (g ? r.j[0] : 0);
    r.n += on ? 1 : 0;
    mk &= mk - 1u;   // (0 stays 0)
  }
  return r;
}

// f(j, ld(j)) for each set bit j of mk, ascending, G bits per round: the round's G reads are issued
// together, then its bodies run in ascending bit order, so a round costs one read latency where the
// bit-by-bit walk pays one per bit.  A lane whose mask runs out inside a round reads slot 0's operands
// again for the idle slots and runs no body for them (no zero term is added: -0 + +0 would change a
// sign).  Every lane does the operations of the bit-by-bit walk in its order.  fence() runs between a round's
// reads and its bodies: the kernels pass the scheduling fence that keeps the reads together (without it the
// grouped walk measured slower than the bit-by-bit one, profiles/chain_sums.md), the host check a counter.
template <int G, typename LD, typename F, typename FENCE>
HS_BITS_FN void for_bit_groups(uint32_t mk, LD&& ld, F&& f, FENCE&& fence) {
  static_assert(G >= 1 && G <= 8, "group size");
  while (mk) {
    const BitGroup<G> b = take_bits<G>(mk);
    decltype(ld(0)) v[G];
    HS_BITS_UNROLL
    for (int g = 0; g < G; g++) v[g] = ld(b.j[g]);
    fence();
    HS_BITS_UNROLL
    for (int g = 0; g < G; g++)
      if (g < b.n) f(b.j[g], v[g]);
  }
}

}  // namespace hs
