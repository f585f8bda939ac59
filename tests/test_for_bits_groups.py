"""The grouped bit walk of the fp64 chain / subtree sums (csrc/hs_bits.h: take_bits, for_bit_groups) on the host.

tools/for_bits_check.cpp is a stand-alone program built with -fsanitize=address,undefined (make asan-for-bits).
For G in {1, 2, 3, 4} it walks every 16-bit mask, each of them again with bit 31 set and a few full-width masks:
the calls f(j) are the bit-by-bit walk's, in its order, each with the value read at its own bit, every read is
at a set bit of the mask (an idle slot repeats the round's first bit), and a round issues G reads.  Then 200
wavefronts of 64 lanes with different masks (popcounts 0 to 32, the empty mask among them) in lockstep: a wave
ends after ceil(max popcount / G) rounds, every lane has made exactly its own calls, and a lane whose bits run
out inside a round makes no further call.  No GPU needed.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grouped_walk_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mujocoposelearning_amd", "csrc"), "asan-for-bits"])
    exe = os.path.join(ROOT, "build", "asan", "for_bits_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines == [f"ok G={g} masks=131081 waves=200" for g in (1, 2, 3, 4)], r.stdout
