"""Register-resident dense algebra of hs_dense.h at NV = 27, called directly: chol_rows as L L' and as L D L',
chol_solve (UNIT false / true), chol_fwd, chol_fwd_multi<27, 2> and <27, G of the engine>, matvec_lds.

The Newton loop absorbs a factor that is subtly less accurate than it should be (it converges to 1e-13 with a
few more iterations), so the pipeline's parity tests do not see one.  Here each operation is measured
against truth (mpmath at 50 digits for fp64, float64 for fp32) and held to the harness's bar, class by class:
    kernel error <= max(4 x the textbook's error in the working precision, 4 ulp)      (tests/unit_kernels.py)
with the factor's error max |L - L_true| / max |L_true|, the solve's normwise backward error
|b - A x| / (|A| |x| + |b|), and |A - L D L'| / |A| for the L D L' form.

Classes: a_H, a_M -- the Hessians H = M + J' D J and mass matrices of the oracle on the 48 parity states and 8 lying
states (cond 4e3 .. 2e5); b_* -- Q diag(lambda) Q' with cond 1e2, 1e4, 1e6 and 2e7 (100 x the oracle's largest),
plain and with every 2x2 pivot block of the elimination ill-conditioned; c -- semi-definite matrices, for which
only the documented clamp (pivot -> 1e-30) and finite outputs are asserted.  Each wave factors two different
matrices; the item count is odd.  Measured ratios: profiles/unit_kernels.md.
"""
import numpy as np
import pytest

import unit_kernels as uk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_dense_operations_meet_the_bar(prec):
    fails = uk.dense_check(prec, uk.dense_device_run(prec))
    assert not fails, fails


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_semidefinite_pivots_are_clamped(prec):
    dt = uk.DT[prec]
    A = uk.dense_classes()["c_semidefinite"].astype(dt)
    b = uk.dense_rhs(len(A)).astype(dt)
    run = uk.dense_device_run(prec)
    L, dinv, _, x = run["chol"](A, b, False)
    assert np.isfinite(L).all() and np.isfinite(dinv).all() and np.isfinite(x).all()
    L2, dinv2, diag, x2 = run["chol"](A, b, True)
    assert np.isfinite(L2).all() and np.isfinite(dinv2).all() and np.isfinite(diag).all() and np.isfinite(x2).all()
    assert (diag >= dt(1e-30)).all(), "every pivot is at least the clamp"
    for i, rows in enumerate(uk.C_ZERO_ROWS):
        assert (diag[i, rows] == dt(1e-30)).all(), "a zero pivot becomes 1e-30"
        assert np.allclose(1 / dinv[i, rows].astype(np.float64) ** 2, 1e-30, rtol=64 * uk.EPS[prec]), "1 / L_kk = rsqrt(1e-30)"
        assert np.allclose(1 / dinv2[i, rows].astype(np.float64), 1e-30, rtol=64 * uk.EPS[prec])
        assert (L[i, rows] == 0).all() and (L2[i, rows] == 0).all(), "a zero row stays zero"
        keep = np.setdiff1d(np.arange(uk.NV), rows)
        assert (diag[i, keep] > dt(1e-3)).all(), "the definite part keeps its pivots"
