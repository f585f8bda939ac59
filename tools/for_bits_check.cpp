// Stand-alone check of the grouped bit walk of the chain / subtree sums (csrc/hs_bits.h), built with
// -fsanitize=address,undefined (make asan-for-bits) and run by tests/test_for_bits_groups.py.
//   for_bits_check            -> one line per check, "ok ..." or "FAIL ...", exit status 0 / 1
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hs_bits.h"

namespace {

int fails = 0;
void fail(const char* what, int G, uint32_t mk) {
  if (fails++ < 10) std::printf("FAIL %s G=%d mask=0x%08x\n", what, G, mk);
}

// the bit-by-bit walk of for_bits (hs_lanes.h)
std::vector<int> plain_walk(uint32_t mk) {
  std::vector<int> js;
  for (; mk; mk &= mk - 1u) js.push_back(__builtin_ctz(mk));
  return js;
}
int popcount(uint32_t mk) { return (int)plain_walk(mk).size(); }

struct Val { int j; uint32_t tag; };

// one mask through for_bit_groups<G>: the calls of f are the plain walk's, every read is at a set bit of the
// mask, and f gets the value read at its own bit
template <int G>
void check_mask(uint32_t mk) {
  std::vector<int> calls, reads;
  bool value_ok = true;
  int fences = 0;
  hs::for_bit_groups<G>(
      mk,
      [&](int j) { reads.push_back(j); return Val{j, 0xabcd0000u + (uint32_t)j}; },
      [&](int j, const Val& v) { calls.push_back(j); value_ok = value_ok && v.j == j && v.tag == 0xabcd0000u + (uint32_t)j; },
      [&] { fences++; });
  if (calls != plain_walk(mk)) fail("call sequence", G, mk);
  if (!value_ok) fail("value of another bit", G, mk);
  for (int j : reads)
    if (j < 0 || j > 31 || !((mk >> j) & 1u)) fail("read off the mask", G, mk);
  const int rounds = (popcount(mk) + G - 1) / G;
  if ((int)reads.size() != rounds * G) fail("reads per round", G, mk);
  if (fences != rounds) fail("one fence per round", G, mk);
}

template <int G>
long check_all_masks() {
  long n = 0;
  for (uint32_t lo = 0; lo < 0x10000u; lo++) {
    check_mask<G>(lo);
    check_mask<G>(lo | 0x80000000u);
    n += 2;
  }
  const uint32_t more[] = {0xffffffffu, 0x80000000u, 0xc0000000u, 0xffff0000u, 0x80000001u, 0xaaaaaaaau, 0x55555555u,
                           0xfffffffeu, 0x7fffffffu};
  for (uint32_t mk : more) { check_mask<G>(mk); n++; }
  return n;
}

// 64 lanes in lockstep, as a wavefront runs the loop: a round is executed while any lane has bits left, and only
// by the lanes that have; it ends after ceil(max popcount / G) rounds, every lane has made its popcount calls in
// ascending order, and a lane makes no call in a slot past its last bit or in a round after it
template <int G>
long check_waves(int nwaves) {
  uint32_t rng = 12345u + (uint32_t)G;
  auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng; };
  for (int w = 0; w < nwaves; w++) {
    uint32_t mk[64], mk0[64];
    int maxpop = 0;
    for (int l = 0; l < 64; l++) {
      uint32_t x = next() ^ (next() >> 7);
      switch ((w + l) % 5) {   // chains of mixed lengths, the empty mask (the world body's lane) among them
        case 0: x = 0u; break;
        case 1: x &= next(); x &= next(); break;
        case 2: x &= 0xffffu; break;
        case 3: x |= 0x80000000u; break;
        default: break;
      }
      if (w == 0) x = l < 32 ? (l == 0 ? 0u : (1u << l) - 1u) : (0xffffffffu >> (l - 32));   // popcounts 0..32
      mk[l] = mk0[l] = x;
      if (popcount(x) > maxpop) maxpop = popcount(x);
    }
    std::vector<int> calls[64];
    int rounds = 0;
    for (;;) {
      bool any = false;
      for (int l = 0; l < 64; l++) any = any || mk[l] != 0u;
      if (!any) break;
      rounds++;
      for (int l = 0; l < 64; l++) {
        if (mk[l] == 0u) continue;   // the lane has left the loop
        const int before = popcount(mk[l]);
        const hs::BitGroup<G> b = hs::take_bits<G>(mk[l]);
        if (b.n != (before < G ? before : G)) fail("slots in use", G, mk0[l]);
        for (int g = 0; g < G; g++) {
          if (g < b.n) calls[l].push_back(b.j[g]);
          else if (b.j[g] != b.j[0]) fail("idle slot's bit", G, mk0[l]);
        }
      }
    }
    if (rounds != (maxpop + G - 1) / G) fail("round count", G, (uint32_t)rounds);
    for (int l = 0; l < 64; l++)
      if (calls[l] != plain_walk(mk0[l])) fail("lane's calls", G, mk0[l]);
    uint32_t zero = 0u;
    if (hs::take_bits<G>(zero).n != 0 || zero != 0u) fail("empty mask", G, 0u);
  }
  return nwaves;
}

template <int G>
void run() {
  const long n = check_all_masks<G>();
  const long w = check_waves<G>(200);
  std::printf("%s G=%d masks=%ld waves=%ld\n", fails ? "FAIL" : "ok", G, n, w);
}

}  // namespace

int main() {
  run<1>();
  run<2>();
  run<3>();
  run<4>();
  return fails ? 1 : 0;
}
