"""The unit harness's references and input classes, checked without a GPU (tests/unit_kernels.py), so the CPU
and GPU suites assert the same input conditions:

  * the geometric narrow-phase reference agrees with the oracle's own contacts to 1e-12 on every contact of the
    oracle's parity and lying states, and orc_collide_pairs reproduces those contacts bit for bit;
  * the census floors of every input class hold and the skipped shares stay within their caps;
  * the textbook references meet their expected error against truth (the backward-error bounds of Cholesky and
    of the triangular solves, Higham, Accuracy and Stability of Numerical Algorithms, theorems 10.3, 10.4, 8.5);
  * the checks pass on the textbook's own results and notice a 1e-10 pivot error, a swapped clamp and a tangent
    from the wrong default.
"""
import numpy as np
import pytest

import unit_kernels as uk

PRECS = ["fp64", "fp32"]


def test_geometric_reference_agrees_with_the_oracle_on_its_own_states():
    from oracle.oracle import collide_pairs
    _, _, pairs = uk.harvest()
    assert len(pairs) >= 150
    fn = np.array([p[0] for p in pairs], np.int32)
    print("pairs by function:", np.bincount(fn, minlength=5))
    g = np.array([p[1] for p in pairs])
    sz = np.array([p[2] for p in pairs], dtype=np.float64)
    cnt, con = collide_pairs(fn, g, sz)
    ref = uk.geo_reference(fn, g, sz, "fp64")
    worst = 0.0
    for i, p in enumerate(pairs):
        assert cnt[i] == len(p[3]), "orc_collide_pairs finds the contacts the oracle's collision() found"
        assert np.array_equal(con[i, :cnt[i]], p[3]), "and the same values, bit for bit"
        if ref["valid"][i]:
            assert ref["cnt"][i] == cnt[i]
            worst = max(worst, float(np.abs(ref["con"][i, :cnt[i]] - con[i, :cnt[i]]).max()))
    assert ref["valid"].mean() >= 0.98
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("prec", PRECS)
def test_census_floors_and_skipped_shares(prec):
    census, ref = uk.narrow_census(prec)          # asserts the floors and the caps itself
    assert len(ref) == len(uk.narrow_classes(prec)) and census
    f = uk.frame_inputs(prec).astype(uk.LD)
    n_t, t_t, *_ = uk.frame_truth(f[:, :3], f[:, 3:])
    fails, frames = uk.frame_check(prec, np.concatenate([n_t, t_t], 1).astype(uk.DT[prec]))    # asserts its floors too
    assert not fails and frames


@pytest.mark.parametrize("prec", PRECS)
def test_dense_textbook_meets_its_backward_error_bounds(prec):
    eps, n = uk.EPS[prec] / 2, uk.NV               # unit roundoff
    for name, As in uk.dense_classes().items():
        if name.startswith("c_") or (prec == "fp32" and name.startswith(("b_1e+06", "b_2e+07"))):
            continue                                # fp32 at cond >= 1e6: n eps cond > 1, no bound applies
        A = As.astype(uk.DT[prec])
        b = uk.dense_rhs(len(A)).astype(uk.DT[prec])
        L = uk.chol_textbook(A, prec)
        x = uk.solve_textbook(L, b, prec)
        # |A - L L'| <= gamma_{n+1} |L| |L'| (10.3) and | |L| |L'| |_F <= n |A|_2; the solve adds gamma_{3n+1} (10.4)
        rec = np.array([np.linalg.norm(l.astype(np.float64) @ l.astype(np.float64).T - a.astype(np.float64)) / np.linalg.norm(a.astype(np.float64))
                        for l, a in zip(L, A)])
        assert rec.max() <= (n + 1) * eps * n, (name, rec.max())
        assert uk.backward_err(A, x, b, prec).max() <= (3 * n + 1) * eps * n, name
    Ms, Hs, _ = uk.harvest()
    if prec == "fp64":
        # the conditioning the classes were sized on, and the textbook factor's distance from the 50-digit one
        assert 1e3 < np.linalg.cond(Ms).min() and np.linalg.cond(Hs).max() < 1e6
        e = uk.factor_err(uk.chol_textbook(Hs, prec), uk.chol_truth(prec)["a_H"])
        assert e.max() <= 1e-13, e.max()


@pytest.mark.parametrize("prec", PRECS)
def test_dense_checks_pass_on_the_textbook_and_notice_a_pivot_error(prec):
    run = uk.dense_textbook_run(prec)
    assert not uk.dense_check(prec, run)

    def off(A, b, ldl):                             # a 1e-10 relative error in one pivot of the L L' factor
        L, dinv, diag, x = run["chol"](A, b, ldl)
        if not ldl:
            dinv = dinv.copy()
            dinv[:, 6] *= 1 + (1e-10 if prec == "fp64" else 1e-4)
        return L, dinv, diag, x
    fails = uk.dense_check(prec, dict(run, chol=off))
    assert any(f.startswith("chol_rows LL' factor a_") for f in fails) and not any("LDL'" in f for f in fails)


@pytest.mark.parametrize("prec", PRECS)
def test_narrow_phase_checks_pass_on_the_textbook_and_notice_a_swapped_clamp(prec):
    fails, _ = uk.narrow_check(prec, lambda fn, g, sz: uk.narrow_textbook(fn, g, sz, prec))
    assert not fails, fails

    def swapped(fn, g, sz):                          # capsule-capsule with the roles of the two clamps exchanged
        cnt, con = uk.narrow_textbook(fn, g[:, ::-1], sz[:, [2, 3, 0, 1]], prec)
        con = con.copy()
        con[:, :, 3:6] *= -1                         # the normal points from geom 1 to geom 2 again
        k = fn == uk.PAIR_CAPSULE_CAPSULE
        c0, o0 = uk.narrow_textbook(fn, g, sz, prec)
        c0[k], o0[k] = cnt[k], con[k]
        return c0, o0
    fails, _ = uk.narrow_check(prec, swapped)
    assert any(f.startswith("cc_") for f in fails), "clamping x2 first gives other contacts for parallel axes"


def test_narrow_textbook_is_the_oracles_sequence():
    """The fp64 textbook and the oracle's C differ by rounding only (no decision flips away from the ties)."""
    from oracle.oracle import collide_pairs
    names, fn, g, sz, sl = uk.narrow_all("fp64")
    cnt, con = uk.narrow_textbook(fn, g, sz, "fp64")
    ocnt, ocon = collide_pairs(fn, g, sz)
    near = sl["cc_near_parallel"]
    keep = np.ones(len(fn), bool)
    keep[near] = False
    keep &= np.concatenate([uk.narrow_census("fp64")[1][n]["valid"] | (n.startswith("cc_parallel") or n == "ss_coincident") for n in names])
    assert (cnt[keep] == ocnt[keep]).all()
    up = sl["pc_upright"]
    d = np.abs(con - ocon)
    d[up, :, 6:9] = 0                                # upright capsules: the tangent is rounding noise
    assert d[keep].max() <= 1e-9, d[keep].max()      # (1 / sin^2 >= 1e-6 times a few ulp)


@pytest.mark.parametrize("prec", PRECS)
def test_impedance_references(prec):
    si, rec, pos, mar = uk.impedance_cases(prec)
    tb = uk.impedance_textbook(si, pos, mar, prec)
    assert not uk.impedance_check(prec, tb)
    e = np.abs(tb.astype(uk.LD) - uk.impedance_truth(si, pos, mar)).max()
    assert e <= 8 * uk.EPS[prec], e                  # a division, two pow (<= 1 ulp each in libm), four more roundings
    wrong = tb.copy()
    x = np.abs(pos - mar) / np.where(si[:, 2] > 0, si[:, 2], 1)
    k = (si[:, 4] == 3.0) & (si[:, 2] > 1e-15) & (x > 0) & (x < si[:, 3]) & (np.clip(si[:, 0], 1e-4, 0.9999) != np.clip(si[:, 1], 1e-4, 0.9999))
    wrong[k] = tb[k] * (1 + 64 * uk.EPS[prec])
    assert uk.impedance_check(prec, wrong) == ["sigmoid power 3"]


@pytest.mark.parametrize("prec", PRECS)
def test_math_inputs_cover_their_domains(prec):
    x = uk.math_inputs("rsqrt", prec).astype(np.float64)
    assert x.min() >= 1e-30 and x.max() > (1e299 if prec == "fp64" else 1e37) and len(x) <= 8000
    m, _ = np.frexp(x)
    assert (m == 0.5).sum() >= 200, "powers of two"
    x = uk.math_inputs("recip", prec).astype(np.float64)
    assert (x > 0).sum() > 1000 and (x < 0).sum() > 1000 and np.isfinite(1 / x).all()
    for dim in (3, 4):
        v = uk.normalize_inputs(dim, prec).astype(np.float64)
        n2 = (v ** 2).sum(1)
        assert (n2 < 1e-30).sum() >= 100 and not ((n2 > 2.5e-31) & (n2 < 4e-30)).any()
