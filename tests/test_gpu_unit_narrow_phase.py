"""collide_pair (all five pair functions), make_frame and impedance of hs_contacts.h, called directly on
constructed inputs, so every branch is reached on purpose and counted, not met by chance in a humanoid state.

References (tests/unit_kernels.py): the geometric one -- the true closest points of two segments, of a point and a
segment, of a plane and a sphere, in longdouble, valid where the closest pair is unique -- and the oracle's
conventions (contact count, slot order, the two-contact parallel case, the tangent) through orc_collide_pairs.
The bar is the harness's: kernel error against the geometric truth <= max(4 x the error of the mjc_* sequence
written plainly in the working precision, 4 ulp of the coordinates' scale).

Classes, each with a census from the reference alone and a floor (tests/test_unit_references.py asserts the same):
the nine (x1, x2) clamp regions of capsule-capsule and the second x1 clamp; exactly parallel axes (overlapping:
two contacts; partly overlapping; apart; collinear with coincident closest points); axes at 1e-9 .. 1e-5 rad on
both sides of the |det| < 1e-15 switch; sphere-sphere with coincident centres; sphere-capsule at both ends and the
middle; plane-capsule with 0, 1, 2 ends touching, lying flat, upright; both default tangents of make_frame; pairs
just inside and just outside the bounding-sphere shortcut.

fp32: the determinant of nearly parallel axes is rounding noise (1e-7 h^4 against the 1e-15 switch), so the
geometric reference skips sin^2 < 1e-3, and the classes with oblique parallel or nearly parallel axes assert only
counts in range, finite outputs and orthonormal frames there.  Measured: profiles/unit_kernels.md.
"""
import numpy as np
import pytest

import unit_kernels as uk

pytestmark = pytest.mark.gpu
PRECS = ["fp64", "fp32"]


@pytest.mark.parametrize("prec", PRECS)
def test_collide_pair(prec):
    fails, census = uk.narrow_check(prec, uk.narrow_device_run(prec))
    for k, v in census.items():
        print(f"UNIT {prec} census {k}: {v}")
    assert not fails, fails


@pytest.mark.parametrize("prec", PRECS)
def test_make_frame(prec):
    f = uk.frame_inputs(prec).astype(uk.DT[prec])
    (got,) = uk.dev(prec, "make_frame", [f], [(f.shape, f.dtype)], len(f))
    fails, census = uk.frame_check(prec, got)
    print(f"UNIT {prec} census {census}")
    assert not fails, fails


@pytest.mark.parametrize("prec", PRECS)
def test_impedance(prec):
    _, rec, pos, mar = uk.impedance_cases(prec)
    dt = uk.DT[prec]
    (got,) = uk.dev(prec, "impedance", [rec, pos.astype(dt), mar.astype(dt)], [((len(rec),), dt)], len(rec))
    fails = uk.impedance_check(prec, got)
    assert not fails, fails
