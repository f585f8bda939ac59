"""Unit harness of the step kernels' device primitives: inputs, references and the bar.

``mujocoposelearning_amd/libhsim_unit.so`` (csrc/hs_unit.hip, test code) calls the device functions of
hs_lanes.h / hs_dense.h / hs_contacts.h directly; this module builds the inputs, the references and the checks
that tests/test_gpu_unit_*.py (device) and tests/test_unit_references.py (CPU) share, so both assert the same
input conditions.  A plain helper module: no fixtures, no conftest.

Two references per operation:
  * truth: mpmath at 50 digits for the fp64 kernels, numpy float64 for the fp32 kernels (geometry: numpy
    longdouble, 64-bit mantissa, for both).  Truth factors are carried as numpy longdouble (an mpmath value split
    into two doubles: 2^-64 relative, 1/2000 of an fp64 ulp).  The L D L' reconstruction of fp64 results is
    accumulated in longdouble: 27 * 2^-64 = 1.5e-18 of the matrix's scale, under 2 % of the 4-ulp floor;
  * textbook: the same operation written naively in the working precision (the column Cholesky of
    oracle/hsim_oracle.c chol(), the formula of getimpedance, the mjc_* sequences).

The bar, the same rule everywhere (``bar_ok``): on each input class
    kernel error against truth <= max(4 * textbook error against the same truth, 4 ulp of the result's scale).
The factor 4 covers the different association order (2x2 block elimination, FMAs) and the ~1-ulp rsqrt_t.
"""
import ctypes as C
import functools
import os

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "mujocoposelearning_amd", "assets", "humanoid.xml")
LIB_PATH = os.environ.get("HSIM_UNIT_LIB", os.path.join(ROOT, "mujocoposelearning_amd", "libhsim_unit.so"))   # as HSIM_LIB

mpmath.mp.dps = 50
LD = np.longdouble
NV = 27
DT = {"fp32": np.float32, "fp64": np.float64}
EPS = {"fp32": 2.0 ** -23, "fp64": 2.0 ** -52}       # one ulp at 1
MANT = {"fp32": 24, "fp64": 53}
BAR = 4.0
PAIR_PLANE_SPHERE, PAIR_PLANE_CAPSULE, PAIR_SPHERE_SPHERE, PAIR_SPHERE_CAPSULE, PAIR_CAPSULE_CAPSULE = range(5)


# ------------------------------------------------------------------ the bar
def bar_ok(label, kernel_err, ref_err, floor, rows=None):
    """Print one line of the table and return whether kernel_err <= max(4 ref_err, floor) (floor = 4 ulp of the
    result's scale).  A NaN kernel error fails; a NaN / inf textbook error (the naive code broke down) leaves the
    kernel only the requirement of a finite error."""
    ke, re = float(kernel_err), float(ref_err)
    bound = np.inf if not np.isfinite(re) else max(BAR * re, float(floor))
    ok = bool(np.isfinite(ke) and ke <= bound)
    ratio = ke / re if re > 0 and np.isfinite(re) else float("nan")
    line = f"UNIT {label:<44s} kernel {ke:9.3e}  textbook {re:9.3e}  ratio {ratio:6.2f}  bar {bound:9.3e}  {'ok' if ok else 'FAIL'}"
    print(line)
    if rows is not None:
        rows.append((label, ke, re, ratio, bound, ok))
    return ok


# ------------------------------------------------------------------ device plumbing
_LIB = None


def unit_lib():
    """libhsim_unit.so (built by the default make target); a missing library is an error."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run make in mujocoposelearning_amd/csrc")
        _LIB = C.CDLL(LIB_PATH)
    return _LIB


def entry(name, prec):
    f = getattr(unit_lib(), f"hsu_{name}_{'f32' if prec == 'fp32' else 'f64'}")
    f.restype = C.c_int
    return f


def dev(prec, name, ins, outs, n, ints=()):
    """One launch: ins (numpy arrays, copied to the device), outs [(shape, numpy dtype)] (zero-filled), then the
    integer arguments, n and the stream.  Returns the outputs as numpy arrays."""
    import torch
    tin = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ins]
    tout = [torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda") for shape, dt in outs]
    args = [C.c_void_p(t.data_ptr()) for t in tin + tout] + [C.c_int(int(i)) for i in ints]
    rc = entry(name, prec)(*args, C.c_int(int(n)), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, f"hsu_{name} ({prec}) returned {rc}"
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tout]


# ------------------------------------------------------------------ ulps
def ulp_at(t, prec):
    """Size of one ulp of the working format at |t| (float64 array, t != 0)."""
    _, e = np.frexp(np.abs(np.asarray(t, dtype=np.float64)))
    return np.ldexp(1.0, e - MANT[prec])


def ulp_err(got, truth_fn, x, prec):
    """max and mean |got - truth| in ulps of the truth.  fp64: truth_fn(mpf) at 50 digits per element;
    fp32: truth_fn on the float64 array."""
    got = np.asarray(got, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if prec == "fp32":
        t = truth_fn(x)
        e = np.abs(got - t) / ulp_at(t, prec)
    else:
        e = np.empty(len(x))
        for i, (xi, gi) in enumerate(zip(x, got)):
            t = truth_fn(mpmath.mpf(float(xi)))
            if not np.isfinite(gi):
                e[i] = np.inf
                continue
            _, ex = mpmath.frexp(t)
            e[i] = float(abs(mpmath.mpf(float(gi)) - t) / mpmath.ldexp(1, int(ex) - MANT[prec]))
    return float(e.max()), float(e.mean()), e


def mp_to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


# ------------------------------------------------------------------ math inputs
def math_inputs(kind, prec, seed=0):
    """rsqrt: [1e-30, 1e300] log-uniform (fp32: up to 1e38, its range), powers of 2 (so of 4) and their +-1 ulp
    neighbours.  recip: 1e-300 <= |x| <= 1e300, both signs (fp32: 1e-37 .. 1e37, where x and 1/x are normal)."""
    rng = np.random.default_rng(seed)
    dt = DT[prec]
    if kind == "rsqrt":
        lo, hi = (-30.0, 300.0) if prec == "fp64" else (-30.0, 38.0)
        x = (10.0 ** rng.uniform(lo, hi, 3000)).astype(dt)
        k = np.arange(-99, 996 if prec == "fp64" else 127)
        p2 = np.ldexp(1.0, k).astype(dt)
        x = np.concatenate([x, p2, np.nextafter(p2, dt(0)), np.nextafter(p2, dt(np.inf))])
        return x[(x >= dt(1e-30))]
    if kind == "recip":
        lim = 300.0 if prec == "fp64" else 37.0
        x = (10.0 ** rng.uniform(-lim, lim, 3000)).astype(dt) * rng.choice([-1, 1], 3000).astype(dt)
        k = np.arange(-990 if prec == "fp64" else -120, 991 if prec == "fp64" else 121, 7 if prec == "fp64" else 1)
        p2 = np.ldexp(1.0, k).astype(dt)
        return np.concatenate([x, p2, -p2, np.nextafter(p2, dt(0)), np.nextafter(p2, dt(np.inf))])
    if kind == "sincos":
        lim = 1.6 if prec == "fp32" else 7.0
        return np.concatenate([rng.uniform(-lim, lim, 3000), [0.0, lim, -lim, 1e-8, -1e-8], 10.0 ** rng.uniform(-12, 0, 200)]).astype(dt)
    raise KeyError(kind)


def normalize_inputs(dim, prec, seed=1):
    """Vectors of every scale the branch at |v|^2 < 1e-30 separates (a factor 4 away from it), and zeros."""
    rng = np.random.default_rng(seed + dim)
    dt = DT[prec]
    v = rng.normal(size=(1500, dim))
    big = v * 10.0 ** rng.uniform(-10, (10 if prec == "fp32" else 100), (1500, 1))
    small = v[:300] / np.linalg.norm(v[:300], axis=1, keepdims=True) * 10.0 ** rng.uniform(-22, -15.4, (300, 1))
    out = np.concatenate([big, small, np.zeros((3, dim))]).astype(dt)
    n2 = (out.astype(np.float64) ** 2).sum(1)
    return out[(n2 < 2.5e-31) | (n2 > 4e-30)]


def normalize_truth(v):
    """(v / |v|, |v|) in longdouble for |v|^2 >= 1e-30, ((1, 0, ..), |v|) below (normalize3 / normalize4)."""
    w = v.astype(LD)
    n2 = (w * w).sum(1)
    nrm = np.sqrt(n2)
    unit = np.zeros_like(w)
    unit[:, 0] = 1
    ok = n2 >= LD(1e-30)
    unit[ok] = w[ok] / nrm[ok, None]
    return unit, nrm


def normalize_textbook(v, prec):
    dt = DT[prec]
    w = v.astype(dt)
    n2 = (w * w).sum(1, dtype=dt)
    nrm = np.sqrt(n2)
    unit = np.zeros_like(w)
    unit[:, 0] = 1
    ok = n2 >= dt(1e-30)
    unit[ok] = w[ok] / nrm[ok, None]
    return unit, nrm


# ------------------------------------------------------------------ dense inputs
def oracle_states():
    """The 56 states whose conditioning the harness was sized on: the 48 of test_gpu_parity._states(M, 48, 7) and 8
    lying states (test_gpu_contacts.lying_states, inside the resident tier)."""
    from oracle.oracle import Oracle
    from test_gpu_contacts import lying_states
    from test_gpu_parity import _states
    o = Oracle(XML)
    st = list(_states(o.M, 48, seed=7))
    for q in lying_states(o, 8, seed=2, overflow=False):
        st.append((q, np.zeros(27), np.zeros(21, np.float32)))
    return o, st


@functools.lru_cache(maxsize=None)
def harvest():
    """Per oracle state: M (qM), H = M + J' D J over the active rows of the converged solve, and the state's
    contact pairs as narrow-phase cases."""
    o, st = oracle_states()
    Ms, Hs, pairs = [], [], []
    gt = np.asarray(o.M["geom_type"])
    gs = np.asarray(o.M["geom_size"]).reshape(-1, 3)
    fn_of = {(0, 2): 0, (0, 3): 1, (2, 2): 2, (2, 3): 3, (3, 3): 4}
    for q, v, c in st:
        o.reset_data()
        o.qpos[:] = q
        o.qvel[:] = v
        o.ctrl[:] = c
        o.forward()
        M = o.get("qM")
        ne = o.d.nefc
        J = np.ctypeslib.as_array(o.d.efc_J)[:ne, :NV]
        D = np.ctypeslib.as_array(o.d.efc_D)[:ne]
        act = np.ctypeslib.as_array(o.d.efc_force)[:ne] != 0
        Ms.append(M)
        Hs.append(M + J[act].T @ (D[act, None] * J[act]))
        xp, xm = o.get("geom_xpos"), o.get("geom_xmat")
        seen = {}
        for con in o.contacts():
            seen.setdefault(con["geom"], []).append(con)
        for (g1, g2), cons in seen.items():
            gg = np.array([np.r_[xp[g], xm[g][[2, 5, 8]]] for g in (g1, g2)])
            h = [gs[g][1] if gt[g] == 3 else 0.0 for g in (g1, g2)]
            pairs.append((fn_of[(gt[g1], gt[g2])], gg, [gs[g1][0], h[0], gs[g2][0], h[1]],
                          np.array([np.r_[k["pos"], k["frame"][:6], k["dist"]] for k in cons])))
    return np.array(Ms), np.array(Hs), pairs


def _spd(rng, cond, pivot):
    """Q diag(lambda) Q' with lambda log-spaced over [1, cond].  pivot: the 13 smallest eigenvalues belong to the
    eigenvectors (e_2k - e_2k+1) / sqrt 2, so every 2x2 pivot block of chol_rows is the ill-conditioned part."""
    lam = np.logspace(0, np.log10(cond), NV)
    if not pivot:
        Q, _ = np.linalg.qr(rng.normal(size=(NV, NV)))
    else:
        Q = np.zeros((NV, NV))
        for k in range(13):
            Q[2 * k, k], Q[2 * k + 1, k] = 2 ** -0.5, -2 ** -0.5
        R = np.zeros((NV, 14))
        for k in range(13):
            R[2 * k, k] = R[2 * k + 1, k] = 2 ** -0.5
        R[26, 13] = 1
        W, _ = np.linalg.qr(rng.normal(size=(14, 14)))
        Q[:, 13:] = R @ W
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


CONDS = (1e2, 1e4, 1e6, 2e7)      # 2e7: 100 x the largest cond(H) of the oracle's states


@functools.lru_cache(maxsize=None)
def dense_classes():
    """{class: float64 [B][27][27]}: a_* harvested, b_* synthetic (6 matrices per cond and kind), c semi-definite."""
    Ms, Hs, _ = harvest()
    out = {"a_H": Hs, "a_M": Ms}
    rng = np.random.default_rng(5)
    for cond in CONDS:
        for pivot in (False, True):
            out[f"b_{cond:.0e}{'_pivot' if pivot else ''}"] = np.array([_spd(rng, cond, pivot) for _ in range(6)])
    c = []
    for zero in C_ZERO_ROWS:          # exact zero rows and columns: first, second and both of a pivot pair, the last column
        A = _spd(rng, 1e2, False)
        A[zero, :] = 0
        A[:, zero] = 0
        c.append(A)
    out["c_semidefinite"] = np.array(c)
    return out


C_ZERO_ROWS = ([20, 21, 22, 23, 24, 25, 26], [5, 12, 13, 26], [0], [1], [26])


def dense_rhs(B, g=1, seed=9):
    return np.random.default_rng(seed).normal(size=(B, g, NV)) if g > 1 else np.random.default_rng(seed).normal(size=(B, NV))


def chol_mp(A):
    """Cholesky factor of one float64 matrix at 50 digits, as longdouble [27][27]."""
    n = len(A)
    Am = [[mpmath.mpf(float(A[i, j])) for j in range(n)] for i in range(n)]
    L = [[mpmath.mpf(0)] * n for _ in range(n)]
    for j in range(n):
        L[j][j] = mpmath.sqrt(Am[j][j] - mpmath.fdot(L[j][:j], L[j][:j]))
        for i in range(j + 1, n):
            L[i][j] = (Am[i][j] - mpmath.fdot(L[i][:j], L[j][:j])) / L[j][j]
    return np.array([[mp_to_ld(L[i][j]) for j in range(n)] for i in range(n)], dtype=LD)


@functools.lru_cache(maxsize=None)
def chol_truth(prec):
    """{class: truth factor [B][27][27] longdouble} of the classes' matrices as the working precision holds them
    (the rounded matrix is the exact input).  fp32: numpy float64 Cholesky (NaN where the rounded matrix is not
    positive definite any more)."""
    out = {}
    for name, As in dense_classes().items():
        if name.startswith("c_"):
            continue
        Aw = As.astype(DT[prec]).astype(np.float64)
        if prec == "fp64":
            out[name] = np.array([chol_mp(A) for A in Aw])
        else:
            Ls = []
            for A in Aw:
                try:
                    Ls.append(np.linalg.cholesky(A))
                except np.linalg.LinAlgError:
                    Ls.append(np.full((NV, NV), np.nan))
            out[name] = np.array(Ls).astype(LD)
    return out


def chol_textbook(A, prec):
    """Column Cholesky as oracle/hsim_oracle.c chol(), in the working precision, batched over [B]."""
    dt = DT[prec]
    A = A.astype(dt)
    L = np.zeros_like(A)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(NV):
            s = A[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            L[:, j, j] = np.sqrt(s)
            t = A[:, j + 1:, j].copy()
            for k in range(j):
                t = t - L[:, j + 1:, k] * L[:, j, k, None]
            L[:, j + 1:, j] = t / L[:, j, j, None]
    return L


def solve_textbook(L, b, prec):
    """chol_solve of hsim_oracle.c: forward and back substitution with divisions, working precision, batched."""
    dt = DT[prec]
    L, b = L.astype(dt), b.astype(dt)
    y = np.zeros_like(b)
    x = np.zeros_like(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(NV):
            t = b[:, i].copy()
            for k in range(i):
                t = t - L[:, i, k] * y[:, k]
            y[:, i] = t / L[:, i, i]
        for i in range(NV - 1, -1, -1):
            t = y[:, i].copy()
            for k in range(i + 1, NV):
                t = t - L[:, k, i] * x[:, k]
            x[:, i] = t / L[:, i, i]
    return x


def ldl_textbook(A, prec):
    """Naive L D L' (unit lower L, d) in the working precision, batched."""
    dt = DT[prec]
    A = A.astype(dt)
    B = len(A)
    L = np.tile(np.eye(NV, dtype=dt), (B, 1, 1))
    d = np.zeros((B, NV), dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(NV):
            s = A[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k] * d[:, k]
            d[:, j] = s
            t = A[:, j + 1:, j].copy()
            for k in range(j):
                t = t - L[:, j + 1:, k] * (L[:, j, k] * d[:, k])[:, None]
            L[:, j + 1:, j] = t / s[:, None]
    return L, d


def ldl_solve_textbook(L, d, b, prec):
    dt = DT[prec]
    L, d, b = L.astype(dt), d.astype(dt), b.astype(dt)
    y = np.zeros_like(b)
    x = np.zeros_like(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(NV):
            t = b[:, i].copy()
            for k in range(i):
                t = t - L[:, i, k] * y[:, k]
            y[:, i] = t
        y = y / d
        for i in range(NV - 1, -1, -1):
            t = y[:, i].copy()
            for k in range(i + 1, NV):
                t = t - L[:, k, i] * x[:, k]
            x[:, i] = t
    return x


def factor_err(L, Lt):
    """max |L - L_true| / max |L_true| over the lower triangle, per matrix (NaN truth: NaN)."""
    L = np.tril(np.asarray(L).astype(LD))
    return np.array([float(np.abs(a - b).max() / np.abs(b).max()) if np.isfinite(b).all() else np.nan for a, b in zip(L, Lt)])


def backward_err(A, x, b, prec):
    """Normwise backward error |b - A x| / (|A| |x| + |b|) (Frobenius / 2-norms), per item; A, x, b as the working
    precision holds them.  The residual at 50 digits for fp64, in float64 for fp32."""
    A, x, b = (np.asarray(a).astype(np.float64) for a in (A, x, b))
    out = np.empty(len(A))
    for i in range(len(A)):
        if not np.isfinite(x[i]).all():
            out[i] = np.inf
            continue
        if prec == "fp64":
            xm = [mpmath.mpf(float(t)) for t in x[i]]
            r = np.array([float(mpmath.mpf(float(b[i, k])) - mpmath.fdot([mpmath.mpf(float(t)) for t in A[i, k]], xm)) for k in range(NV)])
        else:
            r = b[i] - A[i] @ x[i]
        out[i] = np.linalg.norm(r) / (np.linalg.norm(A[i]) * np.linalg.norm(x[i]) + np.linalg.norm(b[i]))
    return out


def ldl_err(A, L, d):
    """|A - L D L'|_F / |A|_F per matrix, accumulated in longdouble (module docstring)."""
    A, L, d = np.asarray(A).astype(LD), np.asarray(L).astype(LD), np.asarray(d).astype(LD)
    R = np.einsum("bik,bk,bjk->bij", L, d, L) - A
    with np.errstate(invalid="ignore"):
        return np.array([float(np.sqrt((r * r).sum()) / np.sqrt((a * a).sum())) for r, a in zip(R, A)])


def fwd_truth(Ls, dinv, b, prec):
    """y_i = (b_i - sum_k<i L_ik y_k) dinv_i, the operation chol_fwd is given (strictly lower L and the rounded
    reciprocals dinv are the exact inputs): 50 digits for fp64, float64 for fp32.  b [B][G][27] -> [B][G][27]."""
    Ls, dinv, b = (np.asarray(a).astype(np.float64) for a in (Ls, dinv, b))
    out = np.zeros(b.shape, dtype=LD)
    for i in range(len(Ls)):
        if prec == "fp64":
            Lm = [[mpmath.mpf(float(t)) for t in row] for row in Ls[i]]
            for g in range(b.shape[1]):
                y = []
                for r in range(NV):
                    y.append((mpmath.mpf(float(b[i, g, r])) - mpmath.fdot(Lm[r][:r], y)) * mpmath.mpf(float(dinv[i, r])))
                out[i, g] = [mp_to_ld(t) for t in y]
        else:
            for g in range(b.shape[1]):
                y = np.zeros(NV)
                for r in range(NV):
                    y[r] = (b[i, g, r] - Ls[i, r, :r] @ y[:r]) * dinv[i, r]
                out[i, g] = y
    return out


def fwd_textbook(Ls, dinv, b, prec):
    dt = DT[prec]
    Ls, dinv, b = Ls.astype(dt), dinv.astype(dt), b.astype(dt)
    y = np.zeros_like(b)
    for r in range(NV):
        t = b[:, :, r].copy()
        for k in range(r):
            t = t - Ls[:, None, r, k] * y[:, :, k]
        y[:, :, r] = t * dinv[:, None, r]
    return y


def matvec_truth(A, v, prec):
    A, v = np.asarray(A).astype(np.float64), np.asarray(v).astype(np.float64)
    if prec == "fp32":
        return np.einsum("bij,bj->bi", A, v).astype(LD)
    out = np.zeros(v.shape, dtype=LD)
    for i in range(len(A)):
        vm = [mpmath.mpf(float(t)) for t in v[i]]
        out[i] = [mp_to_ld(mpmath.fdot([mpmath.mpf(float(t)) for t in A[i, r]], vm)) for r in range(NV)]
    return out


def matvec_textbook(A, v, prec):
    dt = DT[prec]
    A, v = A.astype(dt), v.astype(dt)
    acc = np.zeros(v.shape, dt)
    for j in range(NV):
        acc = acc + A[:, :, j] * v[:, None, j]
    return acc


def rel_err(got, truth):
    """max |got - truth| / max |truth| per item (leading axis)."""
    got, truth = np.asarray(got).astype(LD), np.asarray(truth).astype(LD)
    ax = tuple(range(1, got.ndim))
    with np.errstate(invalid="ignore"):
        return (np.abs(got - truth).max(axis=ax) / np.abs(truth).max(axis=ax)).astype(np.float64)


def _cmax(e):
    """Class maximum; any NaN (a broken-down reference or result) makes it NaN."""
    e = np.asarray(e, dtype=np.float64)
    return float("nan") if np.isnan(e).any() else float(e.max())


def dense_textbook_run(prec):
    """The textbook references in the shape of the device calls (a stand-in 'kernel' for the CPU suite)."""
    def chol(A, b, ldl):
        if not ldl:
            L = chol_textbook(A, prec)
            x = solve_textbook(L, b, prec)
            with np.errstate(divide="ignore"):
                dinv = 1 / np.einsum("bii->bi", L)
            return np.tril(L, -1), dinv, np.zeros_like(dinv), x
        L, d = ldl_textbook(A, prec)
        with np.errstate(divide="ignore"):
            return np.tril(L, -1), 1 / d, d, ldl_solve_textbook(L, d, b, prec)

    def fwd(Ls, dinv, b):
        y = fwd_textbook(Ls, dinv, b, prec)
        return y[:, 0], y[:, :2], y

    return dict(chol=chol, fwd=fwd, matvec=lambda A, v: matvec_textbook(A, v, prec))


def dense_device_run(prec):
    dt = DT[prec]

    def chol(A, b, ldl):
        B = len(A)
        L, dinv, diag, xs = dev(prec, "chol", [A.astype(dt), b.astype(dt)],
                                [((B, NV, NV), dt), ((B, 32), dt), ((B, 32), dt), ((B, 32), dt)], B, ints=(int(ldl),))
        return L, dinv[:, :NV], diag[:, :NV], xs[:, :NV]

    def fwd(Ls, dinv, b):
        B, G = len(Ls), b.shape[1]
        assert G == entry("fwd_group", prec)()
        di = np.zeros((B, 32), dt)
        di[:, :NV] = dinv
        y1, y2, yg = dev(prec, "fwd", [Ls.astype(dt), di, b.astype(dt)], [((B, 32), dt), ((B, 2, 32), dt), ((B, G, 32), dt)], B)
        return y1[:, :NV], y2[:, :, :NV], yg[:, :, :NV]

    def matvec(A, v):
        B = len(A)
        return dev(prec, "matvec", [A.astype(dt), v.astype(dt)], [((B, 32), dt)], B)[0][:, :NV]

    return dict(chol=chol, fwd=fwd, matvec=matvec)


def fwd_group(prec):
    return 4 if prec == "fp64" else 8      # the PGS instance's own G (hs_stepper.h)


def dense_check(prec, run, rows=None):
    """Run every dense operation through ``run`` (device or stand-in) on all classes in one call each and check the
    bar class by class.  Returns the list of failed labels."""
    dt, eps = DT[prec], EPS[prec]
    cls = dense_classes()
    truth = chol_truth(prec)
    names = [n for n in cls if not n.startswith("c_")]
    A = np.concatenate([cls[n] for n in names]).astype(dt)
    idx = np.cumsum([0] + [len(cls[n]) for n in names])
    if len(A) % 2 == 0:                       # an odd item count leaves a ghost half in the last wave
        A = A[:-1]
    B = len(A)
    b = dense_rhs(B).astype(dt)
    sl = {n: slice(idx[i], min(idx[i + 1], B)) for i, n in enumerate(names)}
    Lt = np.concatenate([truth[n] for n in names])[:B]
    fails = []

    def bar(label, ke, re):
        if not bar_ok(f"{prec} {label}", ke, re, BAR * eps, rows):
            fails.append(label)

    # --- L L'
    L, dinv, _, xs = run["chol"](A, b, False)
    assert (np.triu(L) == 0).all(), "chol_rows leaves the diagonal and the upper part zeroed"
    with np.errstate(divide="ignore"):
        Lk = np.tril(L, -1).astype(LD) + np.array([np.diag(1 / d.astype(LD)) for d in dinv])
    Lr = chol_textbook(A, prec)
    xr = solve_textbook(Lr, b, prec)
    ek, er = factor_err(Lk, Lt), factor_err(Lr, Lt)
    bk, br = backward_err(A, xs, b, prec), backward_err(A, xr, b, prec)
    for n in names:
        bar(f"chol_rows LL' factor {n}", _cmax(ek[sl[n]]), _cmax(er[sl[n]]))
        bar(f"chol_solve LL' backward {n}", _cmax(bk[sl[n]]), _cmax(br[sl[n]]))
    # --- L D L'
    L, dinv, diag, xs = run["chol"](A, b, True)
    assert (np.triu(L) == 0).all()
    Lu = np.tril(L, -1) + np.eye(NV, dtype=dt)
    Lr, dr = ldl_textbook(A, prec)
    xr = ldl_solve_textbook(Lr, dr, b, prec)
    ek, er = ldl_err(A, Lu, diag), ldl_err(A, Lr, dr)
    bk, br = backward_err(A, xs, b, prec), backward_err(A, xr, b, prec)
    with np.errstate(invalid="ignore", divide="ignore"):
        dd = np.abs(dinv.astype(LD) * diag.astype(LD) - 1).max(axis=1).astype(np.float64)
    for n in names:
        bar(f"chol_rows LDL' reconstruction {n}", _cmax(ek[sl[n]]), _cmax(er[sl[n]]))
        bar(f"chol_solve LDL' backward {n}", _cmax(bk[sl[n]]), _cmax(br[sl[n]]))
        bar(f"chol_rows LDL' dinv * diag - 1 {n}", _cmax(dd[sl[n]]), eps)
    # --- forward substitutions and matvec: the truth factor, rounded, is the input
    ok = np.isfinite(Lt.astype(np.float64)).all(axis=(1, 2))
    Lw = np.where(ok[:, None, None], Lt, np.eye(NV)).astype(dt)
    Ls = np.tril(Lw, -1)
    with np.errstate(divide="ignore"):
        di = (1 / np.einsum("bii->bi", Lw).astype(LD)).astype(dt)
    G = fwd_group(prec)
    bg = dense_rhs(B, G, seed=10).astype(dt)
    y1, y2, yg = run["fwd"](Ls, di, bg)
    yt = fwd_truth(Ls, di, bg, prec)
    yr = fwd_textbook(Ls, di, bg, prec)
    for lab, got, tr, rf in (("chol_fwd", y1, yt[:, 0], yr[:, 0]), ("chol_fwd_multi<2>", y2, yt[:, :2], yr[:, :2]),
                             (f"chol_fwd_multi<{G}>", yg, yt, yr)):
        e, e_ref = rel_err(got, tr), rel_err(rf, tr)
        for n in names:
            bar(f"{lab} {n}", _cmax(e[sl[n]]), _cmax(e_ref[sl[n]]))
    v = dense_rhs(B, seed=11).astype(dt)
    e, e_ref = rel_err(run["matvec"](A, v), matvec_truth(A, v, prec)), rel_err(matvec_textbook(A, v, prec), matvec_truth(A, v, prec))
    for n in names:
        bar(f"matvec_lds {n}", _cmax(e[sl[n]]), _cmax(e_ref[sl[n]]))
    return fails


# ------------------------------------------------------------------ narrow phase: geometry in longdouble
def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def _clamp(x):
    return np.clip(x, -1, 1)


def seg_seg(p1, e1, p2, e2):
    """True closest points of the segments p1 + s e1 and p2 + t e2, s, t in [-1, 1]: the least distance among the
    interior critical point (where it lies in the square) and the clamped minima on the square's four edges.
    Returns s, t, the unconstrained (s0, t0) and sin^2 of the angle between the axes."""
    w = p1 - p2
    A, B, Cc, D, E = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(e1, w), _dot(e2, w)
    det = A * Cc - B * B
    with np.errstate(divide="ignore", invalid="ignore"):
        s0, t0 = (B * E - Cc * D) / det, (A * E - B * D) / det
    cand = []
    inside = (np.abs(s0) <= 1) & (np.abs(t0) <= 1) & (det > 0)
    cand.append((np.where(inside, s0, 0), np.where(inside, t0, 0), inside))
    for s in (-1, 1):
        ss = np.full(A.shape, s, dtype=LD)
        cand.append((ss, _clamp((E + B * ss) / Cc), np.ones(A.shape, bool)))
    for t in (-1, 1):
        tt = np.full(A.shape, t, dtype=LD)
        cand.append((_clamp((B * tt - D) / A), tt, np.ones(A.shape, bool)))
    best, bs, bt = np.full(A.shape, np.inf, dtype=LD), np.zeros(A.shape, LD), np.zeros(A.shape, LD)
    for s, t, ok in cand:
        d = w + s[..., None] * e1 - t[..., None] * e2
        d2 = np.where(ok, _dot(d, d), np.inf)
        take = d2 < best
        best, bs, bt = np.where(take, d2, best), np.where(take, s, bs), np.where(take, t, bt)
    return bs, bt, s0, t0, det / (A * Cc)


def point_seg(q, p, e):
    t = _clamp(_dot(q - p, e) / _dot(e, e))
    return t, _dot(q - p, e) / _dot(e, e)


def frame_truth(n, hint):
    """mju_makeFrame in longdouble: unit normal, then t1 = the hint (the default tangent where the hint is shorter
    than 0.5: y for |n_y| < 0.5, else z) less its part along n, normalized.  Returns n, t1, |n_y| and the sine of
    the angle between hint and normal (the tangent's conditioning)."""
    n = _unit(n)
    short = np.sqrt(_dot(hint, hint)) < 0.5
    ydef = np.abs(n[..., 1]) < 0.5
    dflt = np.where(ydef[..., None], np.array([0, 1, 0], LD), np.array([0, 0, 1], LD))
    h = np.where(short[..., None], dflt, hint)
    t = h - n * _dot(n, h)[..., None]
    sine = np.sqrt(_dot(t, t)) / np.sqrt(_dot(h, h))
    with np.errstate(invalid="ignore", divide="ignore"):
        return n, _unit(t), np.abs(n[..., 1]), sine, short


def _sphere_pair(c1, r1, c2, r2):
    d = c2 - c1
    ln = np.sqrt(_dot(d, d))
    dist = ln - r1 - r2
    with np.errstate(invalid="ignore", divide="ignore"):
        n = d / ln[..., None]
    pos = c1 + n * (r1 + dist / 2)[..., None]
    return dist, n, pos, ln


def geo_reference(fn, g, sz, prec, parallel=False):
    """Geometric reference of collide_pair on cases (fn [n], g [n][2][6], sz [n][4], float64 values the working
    precision holds): contact count, contacts [n][2][10] = (pos, n, t1, dist) and ``valid`` [n], false where the
    closest pair is not unique or a decision is a tie (sin^2 < 1e-6 between capsule axes, |dist| < 1e-12,
    coincident closest points, | |n_y| - 0.5 | within a tie's width of the default tangent's switch; fp32: 1e-3,
    1e-5, 1e-4).  parallel: the convention for parallel capsule axes instead (mjc_CapsuleCapsule: the two ends of
    capsule 1, +axis first, each against capsule 2 -- a point and a segment, so unique again).
    Also returns the census quantities: the unconstrained (x1, x2) of capsule pairs, whether x1 clamps a second
    time after the x2 clamp, and the sphere's axial coordinate over h for sphere-capsule."""
    fn = np.asarray(fn)
    g, sz = np.asarray(g).astype(LD), np.asarray(sz).astype(LD)
    n = len(fn)
    tie_sin, tie_dist, tie_ny = (1e-6, 1e-12, 1e-9) if prec == "fp64" else (1e-3, 1e-5, 1e-4)
    p1, a1, p2, a2 = g[:, 0, :3], g[:, 0, 3:], g[:, 1, :3], g[:, 1, 3:]
    r1, h1, r2, h2 = sz.T
    cnt = np.zeros(n, int)
    con = np.zeros((n, 2, 10), LD)
    valid = np.ones(n, bool)
    x0 = np.full((n, 2), np.nan)
    reclamp = np.zeros(n, bool)
    axial = np.full(n, np.nan)
    cand = []                 # per slot candidates: (mask, dist, normal, pos, hint, len)
    zero3 = np.zeros((n, 3), LD)
    m = fn == PAIR_PLANE_SPHERE
    cd = _dot(p2 - p1, a1)
    cand.append((m, cd - r2, a1, p2 - a1 * ((cd - r2) / 2 + r2)[:, None], zero3, np.ones(n, LD)))
    m = fn == PAIR_PLANE_CAPSULE
    for sgn in (1, -1):
        e = p2 + sgn * h2[:, None] * a2
        cd = _dot(e - p1, a1)
        cand.append((m, cd - r2, a1, e - a1 * ((cd - r2) / 2 + r2)[:, None], a2, np.ones(n, LD)))
    m = fn == PAIR_SPHERE_SPHERE
    cand.append((m,) + _sphere_pair(p1, r1, p2, r2)[:3] + (zero3, _sphere_pair(p1, r1, p2, r2)[3]))
    m = fn == PAIR_SPHERE_CAPSULE
    e2 = a2 * h2[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        t, traw = point_seg(p1, p2, e2)
    axial = np.where(m, traw.astype(np.float64), axial)
    sp = _sphere_pair(p1, r1, p2 + t[:, None] * e2, r2)
    cand.append((m,) + sp[:3] + (zero3, sp[3]))
    m = fn == PAIR_CAPSULE_CAPSULE
    e1 = a1 * h1[:, None]
    if not parallel:
        with np.errstate(invalid="ignore", divide="ignore"):
            s, t, s0, t0, sin2 = seg_seg(p1, e1, p2, e2)
            # the clamp sequence's second x1 clamp, from the reference's quantities (mjc_CapsuleCapsule)
            A, B, Cc, D, E = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(e1, p1 - p2), _dot(e2, p1 - p2)
            s1 = _clamp(s0)
            t1 = np.where(np.abs(s0) > 1, (E + B * s1) / Cc, t0)
            s2 = (B * _clamp(t1) - D) / A
            reclamp = m & (np.abs(t1) > 1) & (np.abs(s2) > 1)
        x0[m] = np.stack([s0, t0], 1)[m].astype(np.float64)
        valid &= ~m | (sin2 >= tie_sin)
        sp = _sphere_pair(p1 + s[:, None] * e1, r1, p2 + t[:, None] * e2, r2)
        cand.append((m,) + sp[:3] + (zero3, sp[3]))
    else:
        for sgn in (1, -1):
            end = p1 + sgn * e1
            with np.errstate(invalid="ignore", divide="ignore"):
                t, _ = point_seg(end, p2, e2)
            sp = _sphere_pair(end, r1, p2 + t[:, None] * e2, r2)
            cand.append((m,) + sp[:3] + (zero3, sp[3]))
    for m, dist, nrm, pos, hint, ln in cand:
        hit = m & (dist <= 0)
        valid &= ~m | (np.abs(dist) >= tie_dist)
        coincident = hit & (ln < 1e-9)
        nrm = np.where(coincident[:, None], np.array([1, 0, 0], LD), nrm)
        valid &= ~coincident
        with np.errstate(invalid="ignore", divide="ignore"):
            nn, t1, ny, _, short = frame_truth(np.where(hit[:, None], nrm, np.array([1, 0, 0], LD)), hint)
        valid &= ~(hit & short & (np.abs(ny - 0.5) < tie_ny))
        for i in np.nonzero(hit)[0]:
            k = cnt[i]
            con[i, k] = np.r_[pos[i], nn[i], t1[i], dist[i]]
            cnt[i] += 1
    return dict(cnt=cnt, con=con, valid=valid, x0=x0, reclamp=reclamp, axial=axial)


# ------------------------------------------------------------------ narrow phase: textbook in the working precision
def narrow_textbook(fn, g, sz, prec):
    """mjc_PlaneSphere / PlaneCapsule / SphereSphere / SphereCapsule / CapsuleCapsule and mju_makeFrame written
    plainly in the working precision (numpy, case by case: a few thousand cases)."""
    dt = DT[prec]
    fn = np.asarray(fn)
    g, sz = np.asarray(g).astype(dt), np.asarray(sz).astype(dt)
    n = len(fn)
    cnt = np.zeros(n, int)
    con = np.zeros((n, 2, 10), dt)
    one, half, tiny = dt(1), dt(0.5), dt(1e-15)

    def d3(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    def plane_sphere(pp, pn, c, r):
        cd = d3(c - pp, pn)
        if cd > r:
            return None
        dist = cd - r
        return c - pn * (dist * half + r), pn.copy(), dist

    def sphere_sphere(c1, ra, c2, rb):
        d = c2 - c1
        ln = np.sqrt(d3(d, d))
        dist = ln - ra - rb
        if dist > 0:
            return None
        nrm = np.array([1, 0, 0], dt) if ln < tiny else d / ln
        return c1 + nrm * (ra + dist * half), nrm, dist

    def norm3(v):
        n2 = d3(v, v)
        return np.array([1, 0, 0], dt) if n2 < dt(1e-30) else v / np.sqrt(n2)

    def frame(nrm, hint):
        nrm = norm3(nrm)
        if np.sqrt(d3(hint, hint)) < half:
            hint = np.array([0, 1, 0], dt) if abs(nrm[1]) < half else np.array([0, 0, 1], dt)
        return nrm, norm3(hint - nrm * d3(nrm, hint))

    def cl(x):
        return min(max(x, -one), one)

    with np.errstate(all="ignore"):
        for i in range(n):
            p1, a1, p2, a2 = g[i, 0, :3], g[i, 0, 3:], g[i, 1, :3], g[i, 1, 3:]
            r1, h1, r2, h2 = sz[i]
            f, res, hint = fn[i], [], np.zeros(3, dt)
            if f >= PAIR_SPHERE_SPHERE:
                d = p1 - p2
                if np.sqrt(d3(d, d)) > r1 + h1 + r2 + h2:
                    continue
            if f == PAIR_PLANE_SPHERE:
                res = [plane_sphere(p1, a1, p2, r2)]
            elif f == PAIR_PLANE_CAPSULE:
                res = [plane_sphere(p1, a1, p2 + h2 * a2, r2), plane_sphere(p1, a1, p2 - h2 * a2, r2)]
                hint = a2
            elif f == PAIR_SPHERE_SPHERE:
                res = [sphere_sphere(p1, r1, p2, r2)]
            elif f == PAIR_SPHERE_CAPSULE:
                x = d3(a2, p1 - p2)
                x = min(max(x, -h2), h2)
                res = [sphere_sphere(p1, r1, p2 + x * a2, r2)]
            else:
                e1, e2, dif = a1 * h1, a2 * h2, p1 - p2
                ma, mb, mc, u, v = d3(e1, e1), -d3(e1, e2), d3(e2, e2), -d3(e1, dif), d3(e2, dif)
                det = ma * mc - mb * mb
                if abs(det) >= tiny:
                    x1, x2 = (mc * u - mb * v) / det, (ma * v - mb * u) / det
                    if x1 > 1:
                        x1, x2 = one, (v - mb) / mc
                    elif x1 < -1:
                        x1, x2 = -one, (v + mb) / mc
                    if x2 > 1:
                        x2, x1 = one, cl((u - mb) / ma)
                    elif x2 < -1:
                        x2, x1 = -one, cl((u + mb) / ma)
                    res = [sphere_sphere(p1 + x1 * e1, r1, p2 + x2 * e2, r2)]
                else:
                    for side in (one, -one):
                        x2 = cl((v - side * mb) / mc)
                        res.append(sphere_sphere(p1 + side * e1, r1, p2 + x2 * e2, r2))
            for r in res:
                if r is None:
                    continue
                nrm, t1 = frame(r[1], hint)
                con[i, cnt[i]] = np.r_[r[0], nrm, t1, r[2]]
                cnt[i] += 1
    return cnt, con


# ------------------------------------------------------------------ narrow phase: input classes
def _rand_unit(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _perp(rng, a):
    v = np.cross(a, rng.normal(size=a.shape))
    return _unit(v)


def _radii(rng, d, lo=0.6, hi=1.5):
    """Radii whose sum is the true distance times U(lo, hi): about half the cases touch, all lie near the decision."""
    rs = np.maximum(d * rng.uniform(lo, hi, len(d)), 0.02)
    f = rng.uniform(0.3, 0.7, len(d))
    return rs * f, rs * (1 - f)


def _case(fn, p1, a1, p2, a2, r1, h1, r2, h2):
    n = len(p1)
    g = np.stack([np.concatenate([p1, a1], 1), np.concatenate([p2, a2], 1)], 1).astype(np.float64)
    sz = np.stack([np.broadcast_to(np.asarray(x, np.float64), (n,)) for x in (r1, h1, r2, h2)], 1)
    return np.full(n, fn, np.int32), g, sz


def _cc_random(rng, n):
    p1, a1, a2 = rng.uniform(-1, 1, (n, 3)), _rand_unit(rng, n), _rand_unit(rng, n)
    h1, h2 = rng.uniform(0.05, 0.4, n), rng.uniform(0.05, 0.4, n)
    p2 = p1 + rng.uniform(-0.5, 0.5, (n, 3))
    s, t, *_ = seg_seg(p1.astype(LD), (a1 * h1[:, None]).astype(LD), p2.astype(LD), (a2 * h2[:, None]).astype(LD))
    d = np.linalg.norm(p1 + s[:, None].astype(float) * a1 * h1[:, None] - p2 - t[:, None].astype(float) * a2 * h2[:, None], axis=1)
    r1, r2 = _radii(rng, d)
    return _case(4, p1, a1, p2, a2, r1, h1, r2, h2)


def _dyadic(rng, lo, hi, n, q=64):
    return rng.integers(int(lo * q), int(hi * q) + 1, n) / q


def _cc_parallel(rng, n, kind):
    """a2 = +-a1 bitwise.  First half: coordinate axes and dyadic numbers (every product exact in both precisions,
    so det == 0 exactly); second half: oblique axes (fp64 only takes the parallel branch there: |det| is rounding
    noise of 1e-17 h^4, far below 1e-15, where the fp32 noise is far above it)."""
    ex = np.arange(n) < n // 2
    a1 = np.where(ex[:, None], np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1, 1], (n, 1)), _rand_unit(rng, n))
    if kind == "collinear":
        ex[:] = True
        a1 = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1))
    a2 = a1 * rng.choice([-1.0, 1.0], (n, 1))
    h1 = rng.choice([0.125, 0.25], n)
    h2 = rng.choice([0.25, 0.5], n)
    p1 = np.stack([_dyadic(rng, -1, 1, n) for _ in range(3)], 1)
    pv = _perp(rng, a1)
    pv = np.where(ex[:, None], np.roll(np.abs(a1), 1, axis=1), pv)     # exact half: another coordinate axis
    r1, r2 = rng.choice([0.0625, 0.125], n), rng.choice([0.0625, 0.125], n)
    gap = {"overlap": rng.choice([0.5, 0.75], n), "partial": rng.choice([0.5, 0.75], n), "apart": rng.choice([1.25, 1.5], n),
           "collinear": np.zeros(n)}[kind] * (r1 + r2)
    if kind in ("overlap", "collinear", "apart"):      # capsule 1's span inside capsule 2's
        shift = rng.choice([-1, 0, 1], n) * (h2 - h1) * np.where(kind == "collinear", 0.5, 1.0)
    else:                                               # one end of capsule 1 past capsule 2's end
        shift = rng.choice([-1, 1], n) * (h2 + rng.choice([0.0, 0.0625], n))
    p2 = p1 + a1 * shift[:, None] + pv * gap[:, None]
    fn, g, sz = _case(4, p1, a1, p2, a2, r1, h1, r2, h2)
    return fn, g, sz, ex


def _cc_near_parallel(rng, n):
    a1 = _rand_unit(rng, n)
    th = 10.0 ** rng.uniform(-9, -5, n)
    a2 = _unit(a1 + th[:, None] * _perp(rng, a1)) * rng.choice([-1.0, 1.0], (n, 1))
    h1, h2 = rng.uniform(0.2, 0.3, n), rng.uniform(0.2, 0.3, n)
    p1 = rng.uniform(-1, 1, (n, 3))
    r1, r2 = rng.uniform(0.05, 0.1, n), rng.uniform(0.05, 0.1, n)
    p2 = p1 + a1 * rng.uniform(-0.2, 0.2, (n, 1)) + _perp(rng, a1) * ((r1 + r2) * rng.choice([0.6, 0.8, 1.2], n))[:, None]
    return _case(4, p1, a1, p2, a2, r1, h1, r2, h2)


def _ss(rng, n, coincident=False):
    p1 = rng.uniform(-1, 1, (n, 3))
    d = rng.uniform(0.05, 0.5, n)
    p2 = p1.copy() if coincident else p1 + _rand_unit(rng, n) * d[:, None]
    r1, r2 = (rng.uniform(0.02, 0.2, n), rng.uniform(0.02, 0.2, n)) if coincident else _radii(rng, d)
    return _case(2, p1, np.tile([0, 0, 1.0], (n, 1)), p2, np.tile([0, 0, 1.0], (n, 1)), r1, 0.0, r2, 0.0)


def _sc(rng, n):
    p2, a2, h2 = rng.uniform(-1, 1, (n, 3)), _rand_unit(rng, n), rng.uniform(0.05, 0.4, n)
    ax = rng.uniform(-2, 2, n) * h2
    d = rng.uniform(0.05, 0.4, n)
    p1 = p2 + a2 * ax[:, None] + _perp(rng, a2) * d[:, None]
    t = np.clip(ax, -h2, h2)
    dt_ = np.linalg.norm(p1 - p2 - a2 * t[:, None], axis=1)
    r1, r2 = _radii(rng, dt_)
    return _case(3, p1, np.tile([0, 0, 1.0], (n, 1)), p2, a2, r1, 0.0, r2, h2)


def _plane(rng, n, exact_z=False):
    pn = np.tile([0, 0, 1.0], (n, 1)) if exact_z else np.where((np.arange(n) % 2 == 0)[:, None], [0, 0, 1.0], _rand_unit(rng, n))
    return rng.uniform(-0.5, 0.5, (n, 3)) * (0 if exact_z else 1), pn


def _pc(rng, n, kind):
    pp, pn = _plane(rng, n, exact_z=kind == "flat")
    h2, r2 = rng.uniform(0.05, 0.4, n), rng.uniform(0.03, 0.1, n)
    if kind == "random":
        a2 = _rand_unit(rng, n)
        lift = rng.uniform(-1.3, 1.3, n) * (np.abs((a2 * pn).sum(1)) * h2 + r2)      # 0, 1 or 2 ends within r2
    elif kind == "flat":                                # axis in the plane exactly: both ends at the same height
        ang = rng.uniform(0, 2 * np.pi, n)
        a2 = np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1)
        lift = r2 * rng.choice([0.5, 0.75, 1.25], n)
    else:                                               # upright: the axis within 1e-6 rad of the normal
        a2 = _unit(pn + _perp(rng, pn) * (10.0 ** rng.uniform(-12, -6.3, n))[:, None]) * rng.choice([-1.0, 1.0], (n, 1))
        lift = h2 + r2 * rng.choice([0.5, 0.75, 1.25], n)
    p2 = pp + _perp(rng, pn) * rng.uniform(0, 1, (n, 1)) + pn * lift[:, None]
    return _case(1, pp, pn, p2, a2, 0.0, 0.0, r2, h2)


def _ps(rng, n):
    pp, pn = _plane(rng, n)
    r2 = rng.uniform(0.03, 0.2, n)
    p2 = pp + _perp(rng, pn) * rng.uniform(0, 1, (n, 1)) + pn * (r2 * rng.uniform(-0.5, 2.0, n))[:, None]
    return _case(0, pp, pn, p2, np.tile([0, 0, 1.0], (n, 1)), 0.0, 0.0, r2, 0.0)


def _bound(rng, n, rel):
    """Pairs whose centres lie at the bounding-sphere distance R (1 -+ rel): sphere-sphere, a sphere past a capsule's
    end on its axis, and two capsules end to end on one coordinate axis: inside R they touch, outside they do not."""
    k = np.arange(n) % 3
    a = np.eye(3)[rng.integers(0, 3, n)]
    r1, r2 = rng.uniform(0.05, 0.1, n), rng.uniform(0.05, 0.1, n)
    h1 = np.where(k == 2, rng.choice([0.125, 0.25], n), 0.0)
    h2 = np.where(k >= 1, rng.choice([0.125, 0.25], n), 0.0)
    R = r1 + h1 + r2 + h2
    inside = rng.random(n) < 0.5
    p1 = rng.uniform(-1, 1, (n, 3))
    p2 = p1 + a * (R * np.where(inside, 1 - rel, 1 + rel))[:, None]
    fn, g, sz = _case(2, p1, a, p2, a, r1, h1, r2, h2)
    return (k + 2).astype(np.int32), g, sz, inside


@functools.lru_cache(maxsize=None)
def narrow_classes(prec):
    """{class: dict(fn, g, sz, ...)} with the values the working precision holds (float64 arrays of them)."""
    rng = np.random.default_rng(21)
    out = {}

    def add(name, c, **kw):
        fn, g, sz = c[:3]
        g, sz = g.astype(DT[prec]).astype(np.float64), sz.astype(DT[prec]).astype(np.float64)
        out[name] = dict(fn=fn, g=g, sz=sz, **kw)

    add("cc_random", _cc_random(rng, 2400))
    for kind in ("overlap", "partial", "apart", "collinear"):
        c = _cc_parallel(rng, 200, kind)
        add(f"cc_parallel_{kind}", c, exact=c[3], parallel=True, **({"coincident": True} if kind == "collinear" else {}))
    add("cc_near_parallel", _cc_near_parallel(rng, 400), near=True)
    add("ss_random", _ss(rng, 300))
    add("ss_coincident", _ss(rng, 100, coincident=True), coincident=True)
    add("sc_random", _sc(rng, 600))
    add("pc_random", _pc(rng, 600, "random"))
    add("pc_flat", _pc(rng, 200, "flat"))
    add("pc_upright", _pc(rng, 200, "upright"), upright=True)
    add("ps_random", _ps(rng, 300))
    c = _bound(rng, 300, 1e-6 if prec == "fp64" else 1e-3)
    add("bound_sphere", c, inside=c[3], parallel=True)
    return out


# census floors (cases per class that the reference alone puts in each branch), as model_variants.check_coverage
FLOORS = {"cc_region": 20, "cc_reclamp": 20, "cc_contact": 300, "cc_free": 300, "sc_region": 60, "pc_count": 60,
          "parallel_two": 150, "near_each_side": 60, "frame_branch": 100, "bound_side": 100}
SKIP_CAP = 0.02


def narrow_census(prec):
    """Census of every class from the references alone; asserts the floors and the skipped shares.  Returns the
    counts (for the table) and {class: reference}."""
    cls = narrow_classes(prec)
    ref, census = {}, {}
    for name, c in cls.items():
        r = geo_reference(c["fn"], c["g"], c["sz"], prec, parallel=c.get("parallel", False))
        ref[name] = r
        n = len(c["fn"])
        if not (c.get("near") or c.get("coincident") or c.get("upright")):
            skipped = 1 - r["valid"].mean()
            census[f"{name} skipped share"] = round(float(skipped), 4)
            assert skipped <= SKIP_CAP, (name, skipped)
        census[f"{name} contacts 0/1/2"] = tuple(int((r["cnt"] == k).sum()) for k in range(3))
        assert n >= 100
    r = ref["cc_random"]
    reg = (np.sign(r["x0"][:, 0]) * (np.abs(r["x0"][:, 0]) > 1)).astype(int) * 3 + (np.sign(r["x0"][:, 1]) * (np.abs(r["x0"][:, 1]) > 1)).astype(int)
    for code in range(-4, 5):
        k = int((reg == code).sum())
        census[f"cc_random region x1 {(code + 4) // 3 - 1:+d} x2 {(code + 4) % 3 - 1:+d}"] = k
        assert k >= FLOORS["cc_region"], (code, k)
    census["cc_random x1 clamped again after the x2 clamp"] = int(r["reclamp"].sum())
    assert r["reclamp"].sum() >= FLOORS["cc_reclamp"]
    assert (r["cnt"] == 1).sum() >= FLOORS["cc_contact"] and (r["cnt"] == 0).sum() >= FLOORS["cc_free"]
    assert (ref["cc_parallel_overlap"]["cnt"] == 2).sum() >= FLOORS["parallel_two"]
    assert (ref["cc_parallel_partial"]["cnt"] == 1).sum() >= 50 and (ref["cc_parallel_apart"]["cnt"] == 0).all()
    assert (ref["cc_parallel_collinear"]["cnt"] == 2).all()
    c = cls["cc_near_parallel"]
    e1, e2 = c["g"][:, 0, 3:] * c["sz"][:, 1, None], c["g"][:, 1, 3:] * c["sz"][:, 3, None]
    e1, e2 = e1.astype(LD), e2.astype(LD)
    det = (_dot(e1, e1) * _dot(e2, e2) - _dot(e1, e2) ** 2).astype(np.float64)
    c["det"] = det
    census["cc_near_parallel det below / above 1e-15 (ties within [0.5, 2] left out)"] = (int((det < 0.5e-15).sum()), int((det > 2e-15).sum()))
    assert (det < 0.5e-15).sum() >= FLOORS["near_each_side"] and (det > 2e-15).sum() >= FLOORS["near_each_side"]
    ax = ref["sc_random"]["axial"]
    for lab, m in (("end -", ax < -1), ("middle", np.abs(ax) <= 1), ("end +", ax > 1)):
        census[f"sc_random {lab}"] = int(m.sum())
        assert m.sum() >= FLOORS["sc_region"]
    for k in range(3):
        assert (ref["pc_random"]["cnt"] == k).sum() >= FLOORS["pc_count"], k
    assert (ref["pc_flat"]["cnt"] == 2).sum() >= 60 and (ref["pc_flat"]["cnt"] == 0).sum() >= 30
    assert (ref["pc_upright"]["cnt"] == 1).sum() >= 60
    ins = cls["bound_sphere"]["inside"]
    assert ins.sum() >= FLOORS["bound_side"] and (~ins).sum() >= FLOORS["bound_side"]
    assert ((ref["bound_sphere"]["cnt"] >= 1) == ins).all()
    # default tangents: both branches among the contacts whose hint is zero
    ny = np.concatenate([np.abs(ref[n]["con"][:, 0, 4][(ref[n]["cnt"] > 0)]).astype(float) for n in ("cc_random", "ss_random", "sc_random")])
    census["default tangent |n_y| < 0.5 / >= 0.5"] = (int((ny < 0.5).sum()), int((ny >= 0.5).sum()))
    assert (ny < 0.5).sum() >= FLOORS["frame_branch"] and (ny >= 0.5).sum() >= FLOORS["frame_branch"]
    return census, ref


def narrow_all(prec):
    cls = narrow_classes(prec)
    names = list(cls)
    fn = np.concatenate([cls[n]["fn"] for n in names])
    g = np.concatenate([cls[n]["g"] for n in names])
    sz = np.concatenate([cls[n]["sz"] for n in names])
    idx = np.cumsum([0] + [len(cls[n]["fn"]) for n in names])
    return names, fn, g, sz, {n: slice(idx[i], idx[i + 1]) for i, n in enumerate(names)}


def narrow_device_run(prec):
    def run(fn, g, sz):
        dt = DT[prec]
        n = len(fn)
        cnt, con = dev(prec, "collide", [g.astype(dt), sz.astype(dt), fn.astype(np.int32)], [((n,), np.int32), ((n, 2, 10), dt)], n)
        return cnt, con
    return run


def _con_err(got, truth, cnt, fields=slice(0, 10)):
    """max abs difference over the contacts both hold (positions, normals, tangents and distances are all O(1))."""
    got, truth = np.asarray(got).astype(LD), np.asarray(truth).astype(LD)
    e = np.abs(got - truth)[:, :, fields]
    k = np.arange(2)[None, :] < np.asarray(cnt)[:, None]
    return np.where(k[:, :, None], e, 0).max(axis=(1, 2)).astype(np.float64)


def orthonormal_err(con, cnt):
    con = np.asarray(con).astype(np.float64)
    nrm, t1 = con[:, :, 3:6], con[:, :, 6:9]
    unit = np.maximum(np.abs((nrm * nrm).sum(-1) - 1), np.abs((t1 * t1).sum(-1) - 1))
    k = np.arange(2)[None, :] < np.asarray(cnt)[:, None]
    return np.where(k, unit, 0).max(axis=1), np.where(k, np.abs((nrm * t1).sum(-1)), 0).max(axis=1)


def narrow_check(prec, run, rows=None):
    """collide_pair through ``run`` on every class in one call; the bar against the geometric reference with the
    textbook as the yardstick, counts and slot order against the oracle's conventions.  Returns failed labels."""
    from oracle.oracle import collide_pairs
    eps = EPS[prec]
    census, ref = narrow_census(prec)
    names, fn, g, sz, sl = narrow_all(prec)
    cls = narrow_classes(prec)
    cnt, con = run(fn, g, sz)
    tcnt, tcon = narrow_textbook(fn, g, sz, prec)
    ocnt, ocon = collide_pairs(fn, g, sz)
    fails = []
    assert np.isfinite(con).all(), "collide_pair: non-finite output"
    assert ((cnt >= 0) & (cnt <= 2)).all()
    # frames: unit vectors always; orthogonal to eps / sin(axis, normal) for a plane-capsule tangent (the capsule's
    # axis less its part along the normal).  Where the capsule stands upright to within rounding (sin <= 16 eps)
    # the tangent is what is left of the axis, a unit vector of rounding noise that may lie along the normal --
    # in the kernel, in the oracle and in mju_makeFrame alike -- and nothing is asserted of its direction.
    cr = np.cross(g[:, 0, 3:].astype(LD), g[:, 1, 3:].astype(LD))
    sine = np.where(fn == PAIR_PLANE_CAPSULE, np.sqrt(_dot(cr, cr)).astype(np.float64), 1.0)
    unit_e, dot_e = orthonormal_err(con, cnt)
    assert (unit_e <= 16 * eps).all(), "contact frames: unit normal and tangent"
    assert (dot_e <= 16 * eps / np.maximum(sine, 1e-300))[sine > 16 * eps].all(), "contact frames: tangent orthogonal to normal"
    for n in names:
        c, r, s = cls[n], ref[n], sl[n]
        k, kc, tk, tc, ok_, oc = cnt[s], con[s], tcnt[s], tcon[s], ocnt[s], ocon[s]
        v = r["valid"].copy()
        if prec == "fp32" and "exact" in c:
            v &= c["exact"]           # oblique parallel axes: the fp32 determinant is noise, frames and finiteness only
        if c.get("near"):
            # no unique closest pair: count and distance against the oracle, away from the det tie (fp64 only)
            if prec == "fp64":
                m = (c["det"] < 0.5e-15) | (c["det"] > 2e-15)
                if not (k[m] == ok_[m]).all():
                    fails.append(f"{n} count vs oracle")
                both = m & (k == ok_)
                e = _con_err(kc[both], oc[both], k[both], slice(9, 10))
                print(f"UNIT {prec} collide_pair {n}: max |dist - oracle| {e.max():.3e} over {both.sum()} cases")
                if e.max() > 1e-9:
                    fails.append(f"{n} dist vs oracle")
            continue
        if c.get("upright"):
            # t1 is rounding noise where the axis is the normal: positions, normals and distances only
            fields = np.r_[0:6, 9]
        else:
            fields = np.r_[0:10]
        if not (k[v] == r["cnt"][v]).all():
            fails.append(f"{n} count vs geometry")
            print(f"UNIT {prec} collide_pair {n}: {int((k[v] != r['cnt'][v]).sum())} counts differ from the geometric reference")
        if c.get("coincident"):
            # coincident centres: n = (1, 0, 0), dist = -(r1 + r2), the textbook's own formula in the working precision
            same = (k == tk).all() and np.array_equal(kc[:, 0, 3:6], tc[:, 0, 3:6]) and _con_err(kc, tc, k).max() <= BAR * eps
            if not same:
                fails.append(f"{n} vs textbook")
            continue
        agree = v & (k == r["cnt"]) & (tk == r["cnt"])
        ek = _con_err(kc[agree][:, :, fields], r["con"][agree][:, :, fields], k[agree])
        et = _con_err(tc[agree][:, :, fields], r["con"][agree][:, :, fields], k[agree])
        scale = max(1.0, float(np.abs(c["g"][:, :, :3]).max()))
        if not bar_ok(f"{prec} collide_pair {n}", ek.max(), et.max(), BAR * eps * scale, rows):
            fails.append(n)
        # the oracle's conventions: count, slot order (contacts compared slot by slot), away from its ties
        # (the oracle on the values the working precision holds; both lie within their own error of the truth, so
        # within the sum of the two of each other -- a contact in the other slot is off by O(1))
        if not (k[v] == ok_[v]).all():
            fails.append(f"{n} count vs oracle")
        both = v & (k == ok_)
        e = _con_err(kc[both][:, :, fields], oc[both][:, :, fields], k[both])
        et2 = _con_err(oc[both][:, :, fields], r["con"][both][:, :, fields], k[both])
        if e.size and e.max() > 2 * max(ek.max(), et2.max()) + BAR * eps * scale:
            fails.append(f"{n} slots vs oracle")
            print(f"UNIT {prec} collide_pair {n}: max difference from the oracle's slots {e.max():.3e}")
    return fails, census


# ------------------------------------------------------------------ make_frame on its own
def frame_inputs(prec, seed=31):
    """(normal, hint) records: unnormalized normals of several scales; zero hints (both default-tangent branches),
    short hints (< 0.5: default too) and real hints."""
    rng = np.random.default_rng(seed)
    n = 1500
    nrm = _rand_unit(rng, n) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    hint = np.zeros((n, 3))
    hint[500:1000] = _rand_unit(rng, 500) * rng.uniform(0.6, 2.0, (500, 1))
    hint[1000:] = _rand_unit(rng, 500) * rng.uniform(0.01, 0.4, (500, 1))
    f = np.concatenate([nrm, hint], 1).astype(DT[prec]).astype(np.float64)
    return f


def frame_check(prec, got, rows=None):
    """got [n][6] = make_frame of frame_inputs(prec); returns failed labels and the census."""
    from oracle.oracle import make_frames
    f = frame_inputs(prec)
    eps = EPS[prec]
    tie = 1e-9 if prec == "fp64" else 1e-4
    n_t, t_t, ny, sine, short = frame_truth(f[:, :3].astype(LD), f[:, 3:].astype(LD))
    valid = ~(short & (np.abs(ny - 0.5) < tie)) & (np.abs(np.sqrt(_dot(f[:, 3:], f[:, 3:])) - 0.5) > tie)
    census = {"make_frame default tangent y / z / own hint": (int((short & (ny < 0.5)).sum()), int((short & (ny >= 0.5)).sum()), int((~short).sum())),
              "make_frame skipped share": round(float(1 - valid.mean()), 4)}
    assert (short & (ny < 0.5)).sum() >= 100 and (short & (ny >= 0.5)).sum() >= 100 and 1 - valid.mean() <= SKIP_CAP
    truth = np.concatenate([n_t, t_t], 1)
    if prec == "fp64":
        tb = make_frames(f)                      # the oracle's make_frame is the fp64 textbook
    else:
        dt = DT[prec]
        tb = np.zeros((len(f), 6), dt)
        ff = f.astype(dt)
        with np.errstate(all="ignore"):
            for i in range(len(f)):
                nn = ff[i, :3] / np.sqrt((ff[i, :3] * ff[i, :3]).sum(dtype=dt))
                h = ff[i, 3:]
                if np.sqrt((h * h).sum(dtype=dt)) < dt(0.5):
                    h = np.array([0, 1, 0], dt) if abs(nn[1]) < dt(0.5) else np.array([0, 0, 1], dt)
                t = h - nn * (nn * h).sum(dtype=dt)
                tb[i] = np.r_[nn, t / np.sqrt((t * t).sum(dtype=dt))]
    # the tangent's error grows with 1 / sin(hint, normal): classes by that conditioning
    fails = []
    got = np.asarray(got)
    assert np.isfinite(got).all()
    for lab, m in (("default tangents", short), ("own hint, sin >= 0.5", ~short & (sine >= 0.5)), ("own hint, sin < 0.5", ~short & (sine < 0.5))):
        m = m & valid
        ek = np.abs(got[m].astype(LD) - truth[m]).max()
        et = np.abs(tb[m].astype(LD) - truth[m]).max()
        if not bar_ok(f"{prec} make_frame {lab}", ek, et, BAR * eps, rows):
            fails.append(lab)
    return fails, census


# ------------------------------------------------------------------ impedance
def impedance_cases(prec):
    """solimp records and positions: x = 0, tiny, mid +- 1 ulp, 1 - tiny, >= 1 and negative; powers 1, 2, 3, 13/7;
    midpoints 0.3, 0.5, 0.7; d0 == dmax; width <= 1e-15; d0, dmax outside [1e-4, 0.9999].  Widths are powers of two
    and the margin 0 on the grid, so x = pos / width is exact and lands where it is meant to; a second set has
    arbitrary widths and margins.  Returns the model's five solimp values (as the working precision holds them),
    the device records (fill_solimp), pos, margin."""
    dt = DT[prec]
    rng = np.random.default_rng(41)
    rec, pos, mar = [], [], []
    for power in (1.0, 2.0, 3.0, 13.0 / 7.0):
        for mid in (0.3, 0.5, 0.7):
            for d0, dmax in ((0.9, 0.95), (0.95, 0.9), (0.5, 0.5), (1e-5, 0.99999), (0.2, 1.5), (-0.1, 0.6)):
                for width in (2.0 ** -9, 0.5, 5e-16, 1e-17, 0.0):      # (not 1e-15 itself: its float32 rounding lies above it)
                    m = float(dt(mid))
                    xs = [0.0, 1e-12, 1e-30, m, float(np.nextafter(dt(m), dt(0))), float(np.nextafter(dt(m), dt(1))),
                          1 - EPS[prec], 1 - 2.0 ** -20, 1.0, 1.5, 1e6, -0.25, -m, -1.0, -3.0] + list(rng.uniform(0, 1, 6))
                    for x in xs:
                        rec.append([d0, dmax, width, mid, power])
                        pos.append(x * width)
                        mar.append(0.0)
    for _ in range(1500):
        rec.append([rng.uniform(0.5, 0.95), rng.uniform(0.9, 0.999), 10.0 ** rng.uniform(-4, -1), rng.choice([0.3, 0.5, 0.7]),
                    rng.choice([1.0, 2.0, 3.0, 13.0 / 7.0, rng.uniform(1, 6)])])
        mar.append(rng.uniform(0, 0.01))
        pos.append(mar[-1] + rng.uniform(-1.3, 1.3) * rec[-1][2])
    si = np.array(rec).astype(dt).astype(np.float64)
    pos, mar = np.array(pos).astype(dt).astype(np.float64), np.array(mar).astype(dt).astype(np.float64)
    dev_rec = np.zeros((len(si), 8))
    dev_rec[:, :5] = si
    with np.errstate(divide="ignore"):
        dev_rec[:, 5] = np.where(si[:, 2] > 0, 1.0 / si[:, 2], 0.0)
    dev_rec[:, 6] = 1.0 / np.power(si[:, 3], si[:, 4] - 1)
    dev_rec[:, 7] = 1.0 / np.power(1 - si[:, 3], si[:, 4] - 1)
    return si, dev_rec.astype(dt), pos, mar


def impedance_truth(si, pos, mar):
    """getimpedance (mj_makeImpedance) at 50 digits, from the model's five values."""
    out = np.zeros(len(si), LD)
    for i, (s, p, m) in enumerate(zip(si, pos, mar)):
        d0, d1 = (min(0.9999, max(0.0001, float(t))) for t in s[:2])
        if d0 == d1 or s[2] <= 1e-15:
            out[i] = (LD(d0) + LD(d1)) / 2
            continue
        x = abs((mpmath.mpf(float(p)) - mpmath.mpf(float(m))) / mpmath.mpf(float(s[2])))
        if x >= 1 or x <= 0:
            out[i] = d1 if x >= 1 else d0
            continue
        mid, pw = mpmath.mpf(float(s[3])), mpmath.mpf(float(s[4]))
        if s[4] == 1:
            y = x
        elif x <= mid:
            y = x ** pw / mid ** (pw - 1)
        else:
            y = 1 - (1 - x) ** pw / (1 - mid) ** (pw - 1)
        out[i] = mp_to_ld(mpmath.mpf(d0) + y * (mpmath.mpf(d1) - mpmath.mpf(d0)))
    return out


def impedance_textbook(si, pos, mar, prec):
    """The formula of getimpedance (oracle/hsim_oracle.c) in the working precision."""
    dt = DT[prec]
    out = np.zeros(len(si), dt)
    with np.errstate(all="ignore"):
        for i, (s, p, m) in enumerate(zip(si.astype(dt), pos.astype(dt), mar.astype(dt))):
            d0, d1 = (min(dt(0.9999), max(dt(0.0001), t)) for t in s[:2])
            if d0 == d1 or s[2] <= dt(1e-15):
                out[i] = dt(0.5) * (d0 + d1)
                continue
            x = abs((p - m) / s[2])
            if x >= 1 or x <= 0:
                out[i] = d1 if x >= 1 else d0
                continue
            if s[4] == 1:
                y = x
            elif x <= s[3]:
                y = (dt(1) / np.power(s[3], s[4] - dt(1))) * np.power(x, s[4])
            else:
                y = dt(1) - (dt(1) / np.power(dt(1) - s[3], s[4] - dt(1))) * np.power(dt(1) - x, s[4])
            out[i] = d0 + y * (d1 - d0)
    return out


def impedance_check(prec, got, rows=None):
    si, _, pos, mar = impedance_cases(prec)
    truth = impedance_truth(si, pos, mar)
    tb = impedance_textbook(si, pos, mar, prec)
    got = np.asarray(got)
    assert np.isfinite(got).all()
    fails = []
    x = np.abs(pos - mar) / np.where(si[:, 2] > 0, si[:, 2], 1)
    flat = (np.clip(si[:, 0], 1e-4, 0.9999) == np.clip(si[:, 1], 1e-4, 0.9999)) | (si[:, 2] <= 1e-15)
    groups = {"flat (d0 == dmax or width <= 1e-15)": flat, "outside (x <= 0 or x >= 1)": ~flat & ((x <= 0) | (x >= 1))}
    inside = ~flat & (x > 0) & (x < 1)
    for p, lab in ((1.0, "1"), (2.0, "2"), (3.0, "3"), (float(DT[prec](13.0 / 7.0)), "13/7")):
        groups[f"sigmoid power {lab}"] = inside & (si[:, 4] == p)
    groups["sigmoid other powers"] = inside & ~np.isin(si[:, 4], [1.0, 2.0, 3.0, float(DT[prec](13.0 / 7.0))])
    for lab, m in groups.items():
        assert m.sum() >= 50, lab
        ek = np.abs(got[m].astype(LD) - truth[m]).max()
        et = np.abs(tb[m].astype(LD) - truth[m]).max()
        if lab.startswith(("flat", "outside")):
            if not np.array_equal(got[m], tb[m]):      # no arithmetic beyond the clamp and one mean: exact
                fails.append(lab)
                print(f"UNIT {prec} impedance {lab}: differs from the textbook value")
            continue
        if not bar_ok(f"{prec} impedance {lab}", ek, et, BAR * EPS[prec], rows):
            fails.append(lab)
    return fails
