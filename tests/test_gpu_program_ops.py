"""reward_program_kernel op by op and field by field on the device (csrc/hs_reward_prog.hip, hs_api_reward.cpp
rp_batch_fields): the grids, references and special cases of tests/program_op_cases.py, which
tests/test_program_ops.py proves sound on the CPU first.

(a) every op against a one-op reference in both dtypes, (b) the (T) narrowing of constants and parameters,
(c) the slot and instruction limits, (d) batch sizes around the wave edge, (e) field addressing on live
batches, (f) the truth semantics of a termination predicate.  Each test's docstring states its bar and where
the bar comes from.  fp32 subnormals are out of scope (program_op_cases.py).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import XML
import program_op_cases as pc
from test_lane_table import write_variant

pytestmark = pytest.mark.gpu

REG = pc.registry()
PRECS = ["fp64", "fp32"]
# the mpmath references, once at import: off the GPU's clock
for _prec in PRECS:
    for _op in pc.OPS:
        pc.reference(_op, _prec)
SPECIAL = {p: pc.special_cases(p) for p in PRECS}

# (a) the asserted bound of every measured op, in ulps of the dtype at the exact value: the maximum measured on
# an MI355X over the op's grid (profiles/reward_programs.md, "op conformance"), rounded up to a whole ulp,
# plus 1.  None exceeds 8.  fp32 div and sqrt: the build's stated bound for KFLAGS (<= 2.5 ulp), in whole ulps.
ULP_BOUND = {
    ("exp", "fp64"): 2, ("log", "fp64"): 2, ("sin", "fp64"): 2, ("cos", "fp64"): 2, ("tanh", "fp64"): 2,
    ("arcsin", "fp64"): 2, ("arccos", "fp64"): 2, ("arctan2", "fp64"): 3,
    ("exp", "fp32"): 2, ("log", "fp32"): 4, ("sin", "fp32"): 2, ("cos", "fp32"): 2, ("tanh", "fp32"): 2,
    ("arcsin", "fp32"): 4, ("arccos", "fp32"): 3, ("arctan2", "fp32"): 3,
    ("div", "fp32"): 3, ("sqrt", "fp32"): 3,
}


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


def _dt(prec):
    import torch
    return torch.float64 if prec == "fp64" else torch.float32


def _dev(a, prec):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0").to(_dt(prec)).contiguous()


def _eval(model, name, prec, qpos=None, qvel=None, params=None, n=None):
    """reward_eval of the registry's program `name`: [n] float64 on the host (widening is exact)."""
    from mujocoposelearning_amd.batch import reward_eval
    if qpos is None:
        qpos = np.zeros((len(qvel) if qvel is not None else n, model.nq))
    q = _dev(qpos, prec)
    v = None if qvel is None else _dev(qvel, prec)
    out = reward_eval(model, name, q, v, None, None, None, None, None, None, params=params, registry=REG)
    assert out.dtype == _dt(prec) and tuple(out.shape) == (len(qpos),)
    return out.double().cpu().numpy()


def _run_op(model, op, prec, cols):
    return _eval(model, "op_" + op, prec, qpos=pc.qpos_rows(cols, model.nq))


# ------------------------------------------------------------------ (a) per-op conformance
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("op", pc.OPS)
def test_op_conformance(model, op, prec):
    """One op per program over its whole grid; no row is dropped (the count compared is asserted).
    * fp64 add sub mul div sqrt neg abs, fp32 add sub mul neg abs, and in both dtypes every comparison, logical
      op, where, minimum, maximum and ** 2 / 3 / 4: BITWISE numpy's one op in the dtype -- they are IEEE
      operations and selects, NaN, inf and signed zero are values to match.
    * fp32 div and sqrt: within 3 ulp of the exact value (mpmath) -- the build's stated bound for this
      translation unit's flags (-fno-hip-fp32-correctly-rounded-divide-sqrt, "<= 2.5 ulp"), in whole ulps.
      Measured 1.454 and 0.804 ulp: inside the bound and not correctly rounded, so the bar is not bitwise.
    * libm ops in both dtypes: within ULP_BOUND of the exact value (mpmath), the measured maximum rounded up
      plus 1, never more than 8 -- a wrong op or operand shows at 2^20 ulp and beyond.  Rows whose exact result
      is 0, +-inf or NaN must match exactly."""
    cols = pc.grid(op, prec)
    ref = pc.reference(op, prec)
    got = _run_op(model, op, prec, cols)
    assert got.size == len(cols[0]) == len(ref.expected)
    if ref.kind == "bits":
        same = pc.same_bits(got, ref.expected)
        assert same.size == len(cols[0])
        assert same.all(), [(tuple(c[i] for c in cols), got[i], ref.expected[i]) for i in np.flatnonzero(~same)[:5]]
        return
    err = pc.ulp_errors(got, ref, prec)
    w, at = pc.worst(err, cols)
    print(f"CONFORMANCE {op} {prec}: max {w:.3f} ulp at {at} over {err.size} rows ({int(ref.special.sum())} exact)")
    assert err.size == len(cols[0])
    assert ULP_BOUND[(op, prec)] <= 8
    assert w <= ULP_BOUND[(op, prec)], (w, at)


@pytest.mark.parametrize("prec", PRECS)
def test_special_cases_are_exact_on_the_device(model, prec):
    """The C99 Annex F table of program_op_cases.special_cases (x/0, 0/0, inf-inf, 0*inf, sqrt(-0.0) = -0.0,
    log(0), exp(+-inf), asin / acos one ulp outside [-1, 1], atan2 of +-0 and +-inf, where with a NaN or inf in
    the unselected arm, where with a NaN condition -- NaN != 0, so the FIRST arm --, not / and / or of NaN,
    minimum / maximum with a NaN operand): exact in both dtypes, the sign of zero included; the fp32 rows are
    the dtype's own edge values."""
    rows = 0
    bad = []
    for op, (cols, want) in SPECIAL[prec].items():
        got = _run_op(model, op, prec, cols)
        same = pc.same_bits(got, want)
        bad += [(op, tuple(c[i] for c in cols), got[i], want[i]) for i in np.flatnonzero(~same)]
        rows += same.size
    assert rows == sum(len(w) for _, w in SPECIAL[prec].values()) and rows > 150
    assert not bad, bad


# ------------------------------------------------------------------ (b) narrowing
@pytest.mark.parametrize("prec", PRECS)
def test_constants_and_parameters_are_narrowed_once(model, prec):
    """A program that returns a constant and one that returns a parameter: in fp32 bitwise np.float32(value)
    -- (float)double, round to nearest even: 0.1, 1/3, 1e-3, pi are not float-representable, 1e39 becomes inf,
    16777217.0 rounds to 16777216 --, in fp64 bitwise the double."""
    n = 5
    for k, v in enumerate(pc.NARROW_VALUES):
        with np.errstate(over="ignore"):
            want = np.full(n, float(pc.DTYPE[prec](v)))
        assert pc.same_bits(_eval(model, f"const_{k}", prec, n=n), want).all(), ("const", v)
        assert pc.same_bits(_eval(model, "param", prec, n=n, params={"v": v}), want).all(), ("param", v)
    with np.errstate(over="ignore"):
        assert float(np.float32(pc.NARROW_VALUES[4])) == np.inf and float(np.float32(pc.NARROW_VALUES[5])) == 16777216.0


# ------------------------------------------------------------------ (c) limits
@pytest.mark.parametrize("prec", PRECS)
def test_slot_and_instruction_limits(model, prec):
    """The 64-slot program (64 live values: all 32 KB of dynamic LDS in fp64, the top of the (s * 64 + lane)
    addressing) and the 4096-instruction program, 131 envs (three waves, the last partial).  They use sub, mul
    and add only, exact ops: fp64 bitwise eval_host, fp32 bitwise the float32 numpy restatement.  The 64-slot
    program is also run directly after a 1-slot program on the same stream: the dynamic LDS size must follow
    the program, not the previous launch."""
    from mujocoposelearning_amd import reward_program as rw
    rng = np.random.default_rng(17)
    n = 131
    qpos, qvel = pc.cast(rng.normal(size=(n, model.nq)), prec), pc.cast(rng.normal(size=(n, model.nv)), prec)
    s = rw.device_reward_program("slots64", REG).compile(model)
    lp = rw.device_reward_program("long", REG).compile(model)
    assert (s.traced.n_slots, s.traced.n_instr) == (64, 279) and lp.traced.n_instr == 4096
    if prec == "fp64":
        want_s, want_l = s.eval_host({"qvel": qvel}), lp.eval_host({"qpos": qpos, "qvel": qvel})
    else:
        want_s, want_l = pc.slots64_numpy(qvel, np.float32), pc.long_numpy(qpos, qvel, np.float32)
    assert np.isfinite(want_s).all() and np.ptp(want_s) > 1 and np.isfinite(want_l).all() and np.ptp(want_l) > 1
    got = _eval(model, "slots64", prec, qpos=qpos, qvel=qvel)
    assert got.size == n and pc.same_bits(got, want_s).all()
    got = _eval(model, "long", prec, qpos=qpos, qvel=qvel)
    assert got.size == n and pc.same_bits(got, want_l).all()
    one = _eval(model, "one_slot", prec, qpos=qpos, qvel=qvel)
    got = _eval(model, "slots64", prec, qpos=qpos, qvel=qvel)
    assert pc.same_bits(one, qvel[:, 0]).all() and pc.same_bits(got, want_s).all()


# ------------------------------------------------------------------ (d) batch sizes
@pytest.mark.parametrize("prec", PRECS)
def test_batch_sizes_around_the_wave_edge(model, prec):
    """n in {1, 63, 64, 65, 1000}: a lane past n mirrors env n - 1 and writes nothing, so each result is
    bitwise the first n rows of the n = 1000 result (one arithmetic program; its value per env does not depend
    on the batch), and the row behind the last one keeps what it held."""
    import torch
    from mujocoposelearning_amd import _lib
    from mujocoposelearning_amd import reward_program as rw
    rng = np.random.default_rng(23)
    qpos = pc.cast(rng.normal(size=(1000, model.nq)), prec)
    full = _eval(model, "batch_size", prec, qpos=qpos)
    q = qpos.astype(pc.DTYPE[prec])
    want = ((q[:, 0] * q[:, 1] + q[:, 2]) / (np.abs(q[:, 1]) + pc.DTYPE[prec](1.5))).astype(np.float64)
    if prec == "fp64":
        assert pc.same_bits(full, want).all()
    else:                                            # the fp32 divide is within 3 ulp, not exact
        assert (np.abs(full - want) <= 3 * pc.ulp_of(want, prec)).all()
    assert len(np.unique(full)) > 990
    for n in (1, 63, 64, 65, 1000):
        got = _eval(model, "batch_size", prec, qpos=qpos[:n])
        assert got.size == n and pc.same_bits(got, full[:n]).all(), n
    # the kernel's own output buffer, one row longer than n: the extra row is not written
    prog = rw.device_reward_program("batch_size", REG).compile(model)
    for n in (1, 63, 65):
        out = torch.full((n + 1,), -7.0, dtype=_dt(prec), device="cuda:0")
        qd = _dev(qpos[:n], prec)
        f = _lib.hs_reward_fields(qpos=qd.data_ptr())
        _lib.check(_lib.lib().hs_reward_program_eval(prog.handle, 1 if prec == "fp64" else 0, prog.params(None), n,
                                                     C.byref(f), out.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream))
        o = out.double().cpu().numpy()
        assert pc.same_bits(o[:n], full[:n]).all() and o[n] == -7.0, n


# ------------------------------------------------------------------ (e) field addressing on live batches
def _field_lens(nq, nv, nu, nbody):
    return dict(qpos=nq, qvel=nv, ctrl=nu, time=1, qfrc_actuator=nv, cinert=10 * nbody, cvel=6 * nbody,
                subtree_com=3, cfrc_ext=6 * nbody, subtree_linvel=3 * nbody)


def _identity_programs(dims):
    """(registry, {(field, which): (name, flat index)}) for a model of `dims`: programs that return one loaded
    value -- the first, the last and two interior flat indices of every field (time has one value,
    subtree_com[0] three), built in one loop."""
    from mujocoposelearning_amd import reward_program as rw
    reg, picks = {}, {}
    for f, L in _field_lens(*dims).items():
        seen = set()
        for which, i in (("first", 0), ("interior1", L // 3), ("interior2", (2 * L) // 3 + 1), ("last", L - 1)):
            if i >= L or i in seen:
                continue
            seen.add(i)

            def fn(d, p, f=f, i=i):
                if f == "time":
                    return d.time
                if f == "subtree_com":
                    return d.subtree_com[0][i]
                return getattr(d, f).reshape(-1)[i]
            name = f"{f}_{i}"
            rw.register_device_reward(name, fn, registry=reg)
            picks[(f, which)] = (name, i)
    return reg, picks


def _one_of_each(d, p):
    return (d.qpos[5] + d.qvel[7] + d.ctrl[3] + d.time + d.qfrc_actuator[10] + d.cinert[4][2] + d.cvel[6][1]
            + d.subtree_com[0][1] + d.cfrc_ext[8][3] + d.subtree_linvel[2][1])


def _humanoid_programs():
    from mujocoposelearning_amd import reward_program as rw
    reg, picks = _identity_programs((28, 27, 21, 17))
    rw.register_device_reward("one_of_each", _one_of_each, registry=reg)
    return reg, picks


FREG, PICKS = _humanoid_programs()


def _batch_fields(b):
    """The batch's own tensors as the ten fields [n, len]: the obs row is qpos[2:], qvel, cinert [nbody][10],
    cvel [nbody][6], qfrc_actuator (custom_env.py:242-256; full_state appends cfrc_ext[1:]), subtree_com[0] is
    aux[32:35]; cfrc_ext / subtree_linvel are the batch's buffers with full_state and zeros without."""
    import torch
    m = b.model
    o2 = (m.nq - 2) + m.nv
    o3 = o2 + 10 * m.nbody
    o4 = o3 + 6 * m.nbody
    obs = b.t["obs"]
    z = lambda k: torch.zeros(b.n, k, dtype=b.dtype, device=b.device)  # noqa: E731
    return dict(qpos=b.t["qpos"], qvel=b.t["qvel"], ctrl=b.t["ctrl"], time=b.t["time"].reshape(b.n, 1),
                qfrc_actuator=obs[:, o4:o4 + m.nv], cinert=obs[:, o2:o3], cvel=obs[:, o3:o4],
                subtree_com=b.t["aux"][:, 32:35],
                cfrc_ext=b.t["cfrc_ext"].reshape(b.n, -1) if b.full_state else z(6 * m.nbody),
                subtree_linvel=b.t["subtree_linvel"].reshape(b.n, -1) if b.full_state else z(3 * m.nbody))


def _stepped_batch(model, prec, full_state, seed):
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    n = 70
    b = HsBatch(model, n, precision=prec, seed=seed, full_state=full_state)
    b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1)
    b.reset()
    rng = np.random.default_rng(seed)
    for _ in range(3):
        b.step(torch.tensor(rng.uniform(-1, 1, (n, model.nu)), dtype=torch.float32, device=b.device))
    return b, rng


def _check_identity_programs(b, rng, which, step_too):
    """Every picked identity program through compute_reward (hs_reward_program_batch) and, step_too, as the
    reward of one step_program (the outcome launch on the post-step state): bitwise the batch's own entry."""
    import torch
    m = b.model
    checked = 0
    for (f, w), (name, i) in PICKS.items():
        if w not in which:
            continue
        assert i < _field_lens(m.nq, m.nv, m.nu, m.nbody)[f]
        want = _batch_fields(b)[f][:, i].clone()
        got = b.compute_reward(name, registry=FREG)
        assert got.shape == (b.n,) and torch.equal(got, want), (f, i, "compute_reward")
        if f in ("cfrc_ext", "subtree_linvel") and not b.full_state:
            assert (got == 0).all() and not torch.signbit(got).any(), (f, i)
        elif w != "first" and f not in ("cfrc_ext", "subtree_linvel") and (f, w) != ("cinert", "last"):
            assert len(torch.unique(got)) > b.n // 2, (f, i)        # a live column: the envs differ (cinert's last
                                                                    # entry is a body mass, the same in every env)
        if step_too:
            prog = b.compile_reward(name, FREG)
            a = torch.tensor(rng.uniform(-1, 1, (b.n, m.nu)), dtype=torch.float32, device=b.device)
            b.step_program(a, prog)
            assert not b.truncated.any() and not b.terminated.any()
            assert torch.equal(b.reward, _batch_fields(b)[f][:, i]), (f, i, "step_program")
        checked += 1
    return checked


@pytest.mark.parametrize("full_state", [False, True], ids=["obs_state", "full_state"])
@pytest.mark.parametrize("prec", PRECS)
def test_every_field_reads_the_batch_s_own_entry(model, prec, full_state):
    """Identity programs -- the first, the last and two interior flat indices of each of the ten fields -- on a
    70-env batch stepped three times with random actions: bitwise the corresponding entry of the batch's own
    tensors (qpos, qvel, time, the ctrl copy, the obs row's cinert / cvel / qfrc_actuator segments, the aux row's
    subtree_com; an identity, so no tolerance).  With full_state, cfrc_ext and subtree_linvel equal the batch's
    buffers (also with distinct values written into every entry of the two); without, exactly +0.0."""
    import torch
    b, rng = _stepped_batch(model, prec, full_state, seed=31)
    n_prog = _check_identity_programs(b, rng, ("first", "interior1", "interior2", "last"), step_too=True)
    assert n_prog == len(PICKS) == 8 * 4 + 1 + 3
    if full_state:
        # distinct values in every entry of the two side buffers, so that no wrong index can read a right value
        for f in ("cfrc_ext", "subtree_linvel"):
            t = b.t[f]
            t.copy_(torch.arange(1, t.numel() + 1, dtype=torch.float64, device=b.device).reshape(t.shape) * 0.25)
        for (f, w), (name, i) in PICKS.items():
            if f in ("cfrc_ext", "subtree_linvel"):
                want = b.t[f].reshape(b.n, -1)[:, i]
                assert len(torch.unique(want)) == b.n
                assert torch.equal(b.compute_reward(name, registry=FREG), want), (f, i)
    b.close()


def test_field_programs_on_a_second_model(model, tmp_path_factory):
    """The interior and last-index programs on the variant model of tests/test_lane_table.py (other damping,
    armature, gear, ranges; the step kernels take nv = 27 only, so its nq / nv / nbody are the humanoid's), alive
    beside a humanoid batch: each program is compiled per model and reads that model's batch, bitwise."""
    import torch
    from mujocoposelearning_amd.model import HsModel
    var = HsModel(write_variant(tmp_path_factory.mktemp("gpu_program_ops")))
    assert (var.nq, var.nv, var.nu, var.nbody) == (model.nq, model.nv, model.nu, model.nbody)
    b0, _ = _stepped_batch(model, "fp64", False, seed=37)
    b1, rng = _stepped_batch(var, "fp64", False, seed=37)
    assert not torch.equal(b0.qpos, b1.qpos)                    # the two models do step differently
    assert _check_identity_programs(b1, rng, ("interior1", "interior2", "last"), step_too=False) == 8 * 3 + 2
    assert _check_identity_programs(b0, rng, ("interior1",), step_too=False) == 9
    b0.close()
    b1.close()


@pytest.mark.parametrize("prec", PRECS)
def test_field_offsets_move_with_the_model_s_dimensions(prec, tmp_path_factory):
    """A model of other nq, nv, nu and nbody: humanoid.xml without its left arm (25, 24, 18, 14).  The step
    kernels have an instance for nv = 27 only, so this batch is never stepped; every tensor a field lives in
    (qpos, qvel, ctrl, time, obs, aux, cfrc_ext, subtree_linvel; full_state) is filled with values that are
    distinct over ALL of them, so no wrong offset or stride can read a right value.  The first, interior and
    last identity programs of every field, traced for these dimensions, must return bitwise the entry at the
    offsets restated in _batch_fields: an offset or stride that kept the humanoid's 28 / 27 / 17 fails."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.model import HsModel
    m = HsModel(pc.write_one_armed(tmp_path_factory.mktemp("gpu_program_ops_dims"), XML))
    dims = (m.nq, m.nv, m.nu, m.nbody)
    assert dims == pc.ONE_ARMED_DIMS
    reg, picks = _identity_programs(dims)
    b = HsBatch(m, 70, precision=prec, seed=1, full_state=True)
    assert b.obs_dim == (m.nq - 2) + m.nv + 16 * m.nbody + m.nv + 6 * (m.nbody - 1)
    k = 1
    for key in ("qpos", "qvel", "ctrl", "time", "obs", "aux", "cfrc_ext", "subtree_linvel"):
        t = b.t[key]
        t.copy_(((torch.arange(t.numel(), dtype=torch.float64, device=b.device) + k) * 0.5).reshape(t.shape))
        k += t.numel()
    assert k * 0.5 < 2 ** 23                                    # every value is exact and distinct in fp32 too
    fields = _batch_fields(b)
    for (f, w), (name, i) in picks.items():
        want = fields[f][:, i]
        assert len(torch.unique(want)) == b.n
        got = b.compute_reward(name, registry=reg)
        assert torch.equal(got, want), (f, w, i, got[:3].tolist(), want[:3].tolist())
    assert len(picks) == 8 * 4 + 1 + 3
    b.close()


@pytest.mark.parametrize("full_state", [False, True], ids=["obs_state", "full_state"])
@pytest.mark.parametrize("prec", PRECS)
def test_one_value_of_each_field_summed(model, prec, full_state):
    """One program that adds one value of each of the ten fields, on the batch's own buffers: fp64 bitwise
    eval_host fed from the same tensors; fp32 bitwise the same left-to-right float32 additions in numpy
    (additions are exact ops)."""
    b, _ = _stepped_batch(model, prec, full_state, seed=41)
    got = b.compute_reward("one_of_each", registry=FREG).double().cpu().numpy()
    F = {k: v.double().cpu().numpy() for k, v in _batch_fields(b).items()}
    if prec == "fp64":
        prog = b.compile_reward("one_of_each", FREG)
        want = prog.eval_host(dict(F, time=F["time"][:, 0]))
    else:
        cols = [("qpos", 5), ("qvel", 7), ("ctrl", 3), ("time", 0), ("qfrc_actuator", 10), ("cinert", 42), ("cvel", 37),
                ("subtree_com", 1), ("cfrc_ext", 51), ("subtree_linvel", 7)]
        acc = F["qpos"][:, 5].astype(np.float32)
        for f, i in cols[1:]:
            acc = acc + F[f][:, i].astype(np.float32)
        want = acc.astype(np.float64)
    assert got.size == b.n and np.isfinite(want).all() and len(np.unique(want)) > b.n // 2
    assert pc.same_bits(got, want).all()
    b.close()


# ------------------------------------------------------------------ (f) truth semantics
class _DeviceInts:
    """A [n] int32 buffer of the native library as torch sees it."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<i4", "data": (int(ptr), False),
                                         "strides": None, "version": 2}


def _grace_state(b):
    import torch
    from mujocoposelearning_amd import _lib
    cnt, tag = C.c_void_p(), C.c_void_p()
    assert _lib.lib().hs_termination_state(b._h, None, None, C.byref(cnt), C.byref(tag)) == 1
    torch.cuda.synchronize()
    return tuple(torch.as_tensor(_DeviceInts(p.value, b.n), device=b.device).cpu().numpy() for p in (cnt, tag))


@pytest.mark.parametrize("prec", PRECS)
def test_truth_semantics_of_a_predicate_on_the_device(model, prec):
    """rp_truth on the device: the predicate `lambda d, p: d.qvel[0]` reads crafted values written straight into
    the batch's qvel -- 0.0, -0.0 and NaN are false; +-inf, 1.0, the negative tiny value (-1e-300 in fp64, minus
    the smallest normal in fp32) and, fp64 only, the subnormal 5e-324 are true.  early_terminated and the grace
    counters equal termination_eval_host on the same values (exactly: booleans and integers), with grace_steps 1
    in one call, and with grace_steps 2 over two calls with one true env's value set to 0.0 in between (its
    counter must clear).  No step runs on the crafted state."""
    import torch
    from mujocoposelearning_amd import reward_program as rw
    from mujocoposelearning_amd.batch import HsBatch
    reg = {}
    rw.register_device_termination("raw", lambda d, p: d.qvel[0], registry=reg)
    tiny = -1e-300 if prec == "fp64" else -float(np.finfo(np.float32).tiny)
    vals = [0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, tiny] + ([5e-324] if prec == "fp64" else [])
    truth = [False, False, False, True, True, True, True] + ([True] if prec == "fp64" else [])
    n = 70
    v = np.array([vals[i % len(vals)] for i in range(n)])
    want_truth = np.array([truth[i % len(vals)] for i in range(n)])
    b = HsBatch(model, n, precision=prec, seed=3)
    b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1)
    b.reset()
    b.step(torch.zeros(n, model.nu, device=b.device))
    assert not b.terminated.any()
    pred = b.set_termination("raw", grace_steps=1, registry=reg)
    episode = b.episode.cpu().numpy().astype(np.int32)

    def write(values):
        b.t["qvel"][:, 0] = torch.tensor(values, dtype=torch.float64, device=b.device).to(b.dtype)
        back = b.t["qvel"][:, 0].double().cpu().numpy()
        assert pc.same_bits(back, values).all()                    # nothing was lost on the way in
        q = b.t["qvel"].double().cpu().numpy()
        return {"qvel": np.ascontiguousarray(q)}

    fields = write(v)
    cnt, tag = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    want = pred.termination_eval_host(fields, episode, cnt, tag, grace_steps=1)
    assert np.array_equal(want, want_truth)                        # the host says what the docstring says
    term, early = b.apply_termination()
    torch.cuda.synchronize()
    dcnt, dtag = _grace_state(b)
    assert np.array_equal(early.cpu().numpy() != 0, want) and np.array_equal(term.cpu().numpy() != 0, want)
    assert np.array_equal(dcnt, cnt) and np.array_equal(dtag, tag) and np.array_equal(cnt, want.astype(np.int32))
    # grace_steps = 2 over two calls; env `flip` (true) is set to 0.0 in between
    b.t["terminated"].zero_()
    pred = b.set_termination("raw", grace_steps=2, registry=reg)
    cnt, tag = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    flip = 3
    assert want_truth[flip]
    want1 = pred.termination_eval_host(fields, episode, cnt, tag, grace_steps=2)
    _, early = b.apply_termination()
    dcnt, dtag = _grace_state(b)
    assert not want1.any() and not early.any() and not b.terminated.any()
    assert np.array_equal(dcnt, cnt) and np.array_equal(dcnt, want_truth.astype(np.int32)) and np.array_equal(dtag, tag)
    v2 = v.copy()
    v2[flip] = 0.0
    fields = write(v2)
    want2 = pred.termination_eval_host(fields, episode, cnt, tag, grace_steps=2)
    _, early = b.apply_termination()
    dcnt, dtag = _grace_state(b)
    expect = want_truth.copy()
    expect[flip] = False
    assert np.array_equal(want2, expect) and np.array_equal(early.cpu().numpy() != 0, want2)
    assert np.array_equal(dcnt, cnt) and dcnt[flip] == 0 and np.array_equal(dcnt, 2 * expect.astype(np.int32))
    assert np.array_equal(b.terminated.cpu().numpy() != 0, want2)
    b.close()
