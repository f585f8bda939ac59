"""Device math primitives of hs_lanes.h, called directly (libhsim_unit.so) and held to the code's own claims:

  * rsqrt_t<double>, recip(double): <= 2 ulp (their comments say ~1 ulp), on [1e-30, 1e300] and on
    1e-300 <= |x| <= 1e300, truth at 50 digits;
  * fp32 recip / rsqrt_t: <= 2.5 ulp (the Makefile's figure for v_rcp / v_rsq), truth in float64;
  * fp32 sincos_t: <= 2e-6 absolute on |x| <= 1.6 (the comment says ~1e-6 on half joint angles); fp64 sincos_t is
    the device libm, held to the 4 ulp that OpenCL's full profile allows sin and cos and that ROCm's device
    library is built to;
  * normalize3 / normalize4: the harness's bar (tests/unit_kernels.py) against v / sqrt(v . v) in the working
    precision, and the exact fallback (1, 0, ..) below |v|^2 = 1e-30.

Measured on the MI355X: profiles/unit_kernels.md.
"""
import ctypes as C

import mpmath
import numpy as np
import pytest

import unit_kernels as uk

pytestmark = pytest.mark.gpu
PRECS = ["fp64", "fp32"]


@pytest.mark.parametrize("prec", PRECS)
def test_entry_points_reject_null_pointers_and_empty_counts(prec):
    import torch
    x = torch.ones(64, dtype=torch.float64 if prec == "fp64" else torch.float32, device="cuda")
    p, null = C.c_void_p(x.data_ptr()), C.c_void_p(None)
    for name, nptr in (("rsqrt", 2), ("recip", 2), ("sincos", 3), ("normalize3", 3), ("normalize4", 2), ("lanes", 6),
                       ("fwd", 6), ("matvec", 3), ("collide", 5), ("make_frame", 2), ("impedance", 4)):
        f = uk.entry(name, prec)
        assert f(*([p] * nptr), C.c_int(0), null) < 0, name
        assert f(*([p] * nptr), C.c_int(-3), null) < 0, name
        for k in range(nptr):
            args = [p] * nptr
            args[k] = null
            assert f(*args, C.c_int(1), null) < 0, (name, k)
    f = uk.entry("chol", prec)
    assert f(*([p] * 6), C.c_int(0), C.c_int(0), null) < 0
    assert f(*([p] * 5), null, C.c_int(1), C.c_int(1), null) < 0
    torch.cuda.synchronize()
    assert (x == 1).all()


@pytest.mark.parametrize("prec", PRECS)
def test_rsqrt(prec):
    x = uk.math_inputs("rsqrt", prec)
    (got,) = uk.dev(prec, "rsqrt", [x], [(x.shape, x.dtype)], len(x))
    worst, mean, _ = uk.ulp_err(got, (lambda t: 1 / mpmath.sqrt(t)) if prec == "fp64" else (lambda t: 1 / np.sqrt(t)), x, prec)
    print(f"UNIT {prec} rsqrt_t: max {worst:.3f} ulp, mean {mean:.3f} ulp over {len(x)} values")
    assert worst <= (2.0 if prec == "fp64" else 2.5)


@pytest.mark.parametrize("prec", PRECS)
def test_recip(prec):
    x = uk.math_inputs("recip", prec)
    (got,) = uk.dev(prec, "recip", [x], [(x.shape, x.dtype)], len(x))
    worst, mean, _ = uk.ulp_err(got, lambda t: 1 / t, x, prec)
    print(f"UNIT {prec} recip: max {worst:.3f} ulp, mean {mean:.3f} ulp over {len(x)} values")
    assert worst <= (2.0 if prec == "fp64" else 2.5)


@pytest.mark.parametrize("prec", PRECS)
def test_sincos(prec):
    x = uk.math_inputs("sincos", prec)
    s, c = uk.dev(prec, "sincos", [x], [(x.shape, x.dtype)] * 2, len(x))
    if prec == "fp32":
        es = np.abs(s.astype(np.float64) - np.sin(x.astype(np.float64))).max()
        ec = np.abs(c.astype(np.float64) - np.cos(x.astype(np.float64))).max()
        print(f"UNIT fp32 sincos_t: max |error| sin {es:.3e}, cos {ec:.3e} on |x| <= 1.6")
        assert max(es, ec) <= 2e-6
    else:
        nz = x != 0
        es, ms, _ = uk.ulp_err(s[nz], mpmath.sin, x[nz], prec)
        ec, mc, _ = uk.ulp_err(c, mpmath.cos, x, prec)
        print(f"UNIT fp64 sincos_t: max sin {es:.3f} ulp, cos {ec:.3f} ulp on |x| <= 7")
        assert (s[~nz] == 0).all() and max(es, ec) <= 4.0


@pytest.mark.parametrize("dim", [3, 4])
@pytest.mark.parametrize("prec", PRECS)
def test_normalize(prec, dim):
    v = uk.normalize_inputs(dim, prec)
    n = len(v)
    if dim == 3:
        unit, nrm = uk.dev(prec, "normalize3", [v], [((n, 3), v.dtype), ((n,), v.dtype)], n)
    else:
        (unit,) = uk.dev(prec, "normalize4", [v], [((n, 4), v.dtype)], n)
    tu, tn = uk.normalize_truth(v)
    bu, bn = uk.normalize_textbook(v, prec)
    small = (v.astype(np.float64) ** 2).sum(1) < 1e-30
    assert small.sum() >= 100 and (~small).sum() >= 1000
    assert np.array_equal(unit[small], bu[small]), "below |v|^2 = 1e-30 the result is (1, 0, ..) exactly"
    ok = uk.bar_ok(f"{prec} normalize{dim} components", np.abs(unit[~small].astype(uk.LD) - tu[~small]).max(),
                   np.abs(bu[~small].astype(uk.LD) - tu[~small]).max(), uk.BAR * uk.EPS[prec])
    if dim == 3:
        rel = lambda a: np.abs(a[~small].astype(uk.LD) / tn[~small] - 1).max()    # noqa: E731
        ok &= uk.bar_ok(f"{prec} normalize3 returned norm", rel(nrm), rel(bn), uk.BAR * uk.EPS[prec])
        # the fallback returns sqrt(|v|^2) of the working precision's own sum of squares
        # (fp32: |v|^2 below the least normal float, 1.2e-38, may be flushed to zero: sqrt of it is 1.1e-19)
        slack = 4 * uk.EPS[prec] * 1e-15 + (1.1e-19 if prec == "fp32" else 0.0)
        assert np.abs(nrm[small].astype(np.float64) - bn[small].astype(np.float64)).max() <= slack
    assert ok
