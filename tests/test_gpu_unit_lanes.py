"""Cross-lane helpers of hs_lanes.h (hsum, rows_sum, up_row, bcast<K> for every K, hballot), called directly.

Inputs are integers, so every sum is exact and the results are bitwise those of numpy, per 32-lane half.  The two
halves of a wave hold different data, so a value leaking across the half boundary shows; the item count is odd, so
the last wave has a ghost half.
"""
import numpy as np
import pytest

import unit_kernels as uk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_half_wave_primitives_are_bitwise_numpy(prec):
    dt = uk.DT[prec]
    n = 2049
    rng = np.random.default_rng(3)
    x = rng.integers(-1000, 1001, (n, 32)).astype(dt)
    x[0], x[1], x[2] = 0, 1, -1                    # ballots of none, all, none
    x[3, :16], x[3, 16:] = 7, 0                    # rows that differ as a whole
    x[4] = np.arange(32)                           # every lane its own index
    s, rows, up, bc, ballot = uk.dev(prec, "lanes", [x], [((n, 32), dt)] * 3 + [((n, 32, 32), dt), ((n, 32), np.int32)], n)
    assert np.array_equal(s, np.repeat(x.sum(1, keepdims=True), 32, 1)), "hsum"
    two = x[:, :16] + x[:, 16:]
    assert np.array_equal(rows, np.concatenate([two, two], 1)), "rows_sum"
    assert np.array_equal(up[:, :16], x[:, 16:]), "up_row (valid on the low row's lanes)"
    assert np.array_equal(bc, np.repeat(x[:, :, None], 32, 2)), "bcast<K>: sub-lane K's value in every lane of the half"
    mask = ((x > 0).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
    assert np.array_equal(ballot.view(np.uint32), np.repeat(mask[:, None], 32, 1)), "hballot"
