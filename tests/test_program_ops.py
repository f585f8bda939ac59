"""The reward-program op table on the CPU, op by op (csrc/hs_reward_prog.h rp_op through
``CompiledProgram.eval_host``): the fp64 grids, references and special cases of tests/program_op_cases.py.

It proves the grids and references sound before anything reaches a GPU (tests/test_gpu_program_ops.py runs the
same cases through reward_program_kernel) and keeps the CPU suite guarding the op table.  The bars:
arithmetic, sqrt, comparisons, logic, where and the select-based compositions are IEEE operations, so bitwise
the numpy reference; the libm ops within 1 ulp of mpmath (numpy's double libm was measured at <= 0.93 ulp on
such grids and the C library's at <= 0.502, except its tanh: 1.234 ulp at 0.000839967675886535, which is why
rp_op's host tanh goes through long double, 0.500 ulp); the C99 Annex F special cases exact.
"""
import numpy as np
import pytest

from conftest import XML
import program_op_cases as pc

REG = pc.registry()


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


def _host(model, name, cols, params=None):
    from mujocoposelearning_amd import reward_program as rw
    c = rw.device_reward_program(name, REG).compile(model)
    return c.eval_host({"qpos": pc.qpos_rows(cols, model.nq)}, params)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("op", pc.OPS)
def test_grids_are_in_scope(op, prec):
    """Every operand is exactly representable in the dtype, and zero or normal in fp32 (fp32 subnormals are out
    of scope); a bitwise reference is zero, normal, inf or NaN in fp32; the row count is a few hundred to a few
    thousand and no multiple of 64.  (mp_reference itself refuses an fp32 row with a subnormal exact result.)"""
    cols = pc.grid(op, prec)
    n = len(cols[0])
    assert len(cols) == pc.NARGS[op] and all(len(c) == n for c in cols)
    assert 200 <= n <= 6000 and n % 64 != 0
    dt = pc.DTYPE[prec]
    tiny = float(np.finfo(dt).tiny)
    for c in cols:
        assert pc.same_bits(c.astype(dt).astype(np.float64), c).all()
        if prec == "fp32":
            assert not ((c != 0) & (np.abs(c) < tiny)).any()
    ref = pc.reference(op, prec)
    assert ref.kind == pc.ref_kind(op, prec) and len(ref.expected) == n
    if prec == "fp32":
        v = ref.expected if ref.kind == "bits" else ref.hi[~ref.special]
        assert not ((v != 0) & (np.abs(v) < tiny)).any()
    if ref.kind == "ulp":
        assert 0 < (~ref.special).sum() and ref.special.sum() < 16     # the grid measures; specials are the edges


@pytest.mark.parametrize("op", [o for o in pc.OPS if pc.ref_kind(o, "fp64") == "bits"])
def test_exact_ops_equal_numpy_bitwise(model, op):
    """IEEE operations, comparisons and selects in double: bitwise numpy's, NaN positions included."""
    cols = pc.grid(op, "fp64")
    got = _host(model, "op_" + op, cols)
    ref = pc.reference(op, "fp64")
    same = pc.same_bits(got, ref.expected)
    assert same.size == len(cols[0])
    assert same.all(), [(tuple(c[i] for c in cols), got[i], ref.expected[i]) for i in np.flatnonzero(~same)[:5]]


@pytest.mark.parametrize("op", pc.LIBM)
def test_libm_ops_within_one_ulp_of_mpmath(model, op):
    """The host interpreter calls the C library's double libm: <= 1 ulp of the exact value on every row (the
    rows whose exact result is 0, +-inf or NaN must match exactly)."""
    cols = pc.grid(op, "fp64")
    err = pc.ulp_errors(_host(model, "op_" + op, cols), pc.reference(op, "fp64"), "fp64")
    w, at = pc.worst(err, cols)
    print(f"{op} fp64 host: max {w:.3f} ulp at {at}")
    assert err.size == len(cols[0])
    assert w <= 1.0, (w, at)


def test_special_cases_are_exact(model):
    """C99 Annex F, written out by hand in program_op_cases.special_cases: exact, the sign of zero included."""
    rows = 0
    for op, (cols, want) in pc.special_cases("fp64").items():
        got = _host(model, "op_" + op, cols)
        same = pc.same_bits(got, want)
        assert same.all(), (op, [(tuple(c[i] for c in cols), got[i], want[i]) for i in np.flatnonzero(~same)])
        rows += same.size
    assert rows == sum(len(w) for _, w in pc.special_cases("fp64").values()) and rows > 150


def test_fp32_special_cases_hold_in_numpy_float32():
    """The fp32 rows of the table are the same statements about float32: the IEEE ones checked against numpy's
    float32 operations, so the table itself is sound in that dtype before the device sees it."""
    sc = pc.special_cases("fp32")
    rows = 0
    for op in ("add", "sub", "mul", "div", "neg", "abs", "sqrt", "where", "not", "and", "or", "lt", "eq", "ne",
               "minimum", "maximum", "pow2", "pow3"):
        cols, want = sc[op]
        assert pc.same_bits(pc.numpy_reference(op, "fp32", *cols), want).all(), op
        rows += len(want)
    assert rows > 80


def test_narrowing_on_the_host_is_the_double(model):
    """The host interpreter is always double: a constant and a parameter come back as the double itself."""
    cols = (np.zeros(3),)
    for k, v in enumerate(pc.NARROW_VALUES):
        assert pc.same_bits(_host(model, f"const_{k}", cols), np.full(3, v)).all(), v
        assert pc.same_bits(_host(model, "param", cols, {"v": v}), np.full(3, v)).all(), v


def test_limit_programs_equal_their_numeric_twins(model):
    """The 64-slot program (the tracer's slot limit: 64 slots, 279 instructions) and the 4096-instruction program
    (the validator's limit, 29 slots): bitwise their numeric twins -- sub, mul and add only -- and their float64
    numpy restatements, which the GPU test's fp32 reference restates in float32."""
    from mujocoposelearning_amd import reward_program as rw
    rng = np.random.default_rng(3)
    n = 67
    qpos, qvel = rng.normal(size=(n, model.nq)), rng.normal(size=(n, model.nv))
    s = rw.device_reward_program("slots64", REG).compile(model)
    assert (s.traced.n_slots, s.traced.n_instr) == (64, 279)
    got = s.eval_host({"qvel": qvel})
    assert pc.same_bits(got, pc.twin_values(REG, "slots64", n, qvel=qvel)).all()
    assert pc.same_bits(got, pc.slots64_numpy(qvel, np.float64)).all()
    lp = rw.device_reward_program("long", REG).compile(model)
    assert lp.traced.n_instr == 4096 and lp.traced.n_slots == 29
    got = lp.eval_host({"qpos": qpos, "qvel": qvel})
    assert pc.same_bits(got, pc.twin_values(REG, "long", n, qpos=qpos, qvel=qvel)).all()
    assert pc.same_bits(got, pc.long_numpy(qpos, qvel, np.float64)).all()
    assert np.isfinite(got).all() and np.ptp(got) > 1.0
    # one more live value is refused
    def too_many(d, p):
        ys = [d.qvel[i % 27] * (1.0 + 0.125 * i) for i in range(pc.SLOTS64_N + 1)]
        acc = ys[-1]
        for y in reversed(ys[:-1]):
            acc = acc - 0.5 * y
        return acc
    with pytest.raises(ValueError, match="64 live values"):
        rw.trace(too_many, (model.nq, model.nv, model.nu, model.nbody))


def test_the_one_armed_model_has_other_dimensions(model, tmp_path):
    """The second model of the GPU test's field-addressing section: every dimension differs from the humanoid's."""
    from mujocoposelearning_amd.model import HsModel
    m = HsModel(pc.write_one_armed(tmp_path, XML))
    assert (m.nq, m.nv, m.nu, m.nbody) == pc.ONE_ARMED_DIMS
    assert all(a != b for a, b in zip(pc.ONE_ARMED_DIMS, (model.nq, model.nv, model.nu, model.nbody)))
