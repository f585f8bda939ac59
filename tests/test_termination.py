"""Termination conditions on the CPU (reward_program.py register_device_termination, csrc/hs_reward_prog.h
rp_grace_update / rp_termination_eval_host): the registry, the two built-ins' numeric twins against the host
interpreter, the grace counter's semantics, the refusals, and the same host code under sanitizers.

The predicates are comparisons, so the twin and the interpreter must agree EXACTLY: `fallen` compares a loaded
value with a parameter (no arithmetic at all), and `lost_balance` adds |roll|, |pitch| > max with numpy's against
glibc's atan2 / asin, which differ by an ulp or two -- no golden state's angle lies that close to a threshold
(checked below: the margin is printed and must exceed 1e-9).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, XML
from reward_program_cases import FIELDS, N, env_data

from mujocoposelearning_amd import reward_program as rw
from mujocoposelearning_amd.utils import quaternion_to_euler

DIMS = (28, 27, 21, 17)
CASES = [("fallen", None), ("fallen", {"min_height": 1.0}), ("lost_balance", None),
         ("lost_balance", {"min_height": 0.6, "max_roll_pitch": 0.2})]
IDS = ["fallen", "fallen_overrides", "lost_balance", "lost_balance_overrides"]


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


def _states():
    """The 203 golden reward states (unit quaternions) and hand-made ones: the height exactly at the 0.8 and 1.0
    thresholds and 1 ulp to either side, and an upright non-unit quaternion whose pitch is arcsin(1.2) = NaN."""
    q = FIELDS["qpos"].copy()
    extra = []
    for thr in (0.8, 1.0, 0.6):
        for h in (thr, np.nextafter(thr, 0.0), np.nextafter(thr, 2.0)):
            row = q[0].copy()
            row[2] = h
            row[3:7] = [1.0, 0.0, 0.0, 0.0]
            extra.append(row)
    nan_pitch = q[0].copy()
    nan_pitch[2] = 1.2
    nan_pitch[3:7] = [1.0, 0.0, 0.6, 0.0]          # 2 (w y - z x) = 1.2: beyond arcsin's domain; roll = 0
    extra.append(nan_pitch)
    return np.ascontiguousarray(np.vstack([q, np.array(extra)]))


QPOS = _states()
NS = len(QPOS)


def _twin(name, params):
    from types import SimpleNamespace
    fn = rw.TERMINATION_FUNCTIONS[name]
    out = [fn(SimpleNamespace(qpos=QPOS[i]), dict(params) if params else None) for i in range(NS)]
    assert all(type(v) is bool for v in out)
    return np.array(out)


def _fresh(n):
    return np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32)   # episode, count, tag


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_builtin_twins_equal_the_host_interpreter(model, case):
    name, params = CASES[case]
    twin = _twin(name, params)
    c = rw.device_termination(name).compile(model)
    ep, cnt, tag = _fresh(NS)
    early = c.termination_eval_host({"qpos": QPOS}, ep, cnt, tag, params, grace_steps=1)
    print(f"{name} {params}: {int(twin.sum())}/{NS} states terminate; {c.traced.n_instr} instructions, "
          f"{c.traced.n_slots} slots")
    assert 0 < twin.sum() < NS
    assert np.array_equal(early, twin), np.flatnonzero(early != twin)
    assert np.array_equal(cnt, twin.astype(np.int32)) and (tag == 0).all()
    assert c.fields == ["qpos"]


def test_threshold_and_nan_states():
    """h < 0.8 exactly: false at 0.8 and 1 ulp above, true 1 ulp below; a NaN pitch does not terminate."""
    fallen, lost = _twin("fallen", None), _twin("lost_balance", None)
    at, below, above, nanp = N, N + 1, N + 2, NS - 1
    assert QPOS[at, 2] == 0.8 and QPOS[below, 2] < 0.8 < QPOS[above, 2]
    assert (fallen[at], fallen[below], fallen[above]) == (False, True, False)
    assert (lost[at], lost[below], lost[above]) == (False, True, False)
    with np.errstate(all="ignore"):
        roll, pitch, _ = quaternion_to_euler(QPOS[nanp, 3:7])
    assert np.isnan(pitch) and abs(roll) < np.pi / 4
    assert not lost[nanp] and not fallen[nanp]
    # the 1.0 override moves the threshold: the states at 1.0 -+ 1 ulp
    f1 = _twin("fallen", {"min_height": 1.0})
    assert (f1[N + 3], f1[N + 4], f1[N + 5]) == (False, True, False)
    # the golden states keep away from the angle thresholds by far more than atan2 / asin differ between libms
    margin = np.inf
    with np.errstate(all="ignore"):
        for i in range(NS):
            r, p, _ = quaternion_to_euler(QPOS[i, 3:7])
            for m in (np.pi / 4, 0.2):
                for a in (r, p):
                    if np.isfinite(a):
                        margin = min(margin, abs(abs(a) - m))
    print(f"min | |angle| - max | over the states: {margin:.3e}")
    assert margin > 1e-9


def _trace_fields(holds):
    q = np.tile(QPOS[0], (len(holds), 1))
    q[:, 2] = np.where(holds, 0.7, 0.9)
    return {"qpos": np.ascontiguousarray(q)}


def test_grace_counter_semantics(model):
    """T T F T T T with grace_steps = 3: the episode ends at the sixth step, not the third; one env stepped
    six times (counter and tag carried from call to call)."""
    c = rw.device_termination("fallen").compile(model)
    holds = np.array([1, 1, 0, 1, 1, 1], bool)
    f = _trace_fields(holds)
    cnt, tag, ep = np.zeros(1, np.int32), np.full(1, -1, np.int32), np.zeros(1, np.int32)
    early, counts = [], []
    for k in range(6):
        e = c.termination_eval_host({"qpos": f["qpos"][k:k + 1]}, ep, cnt, tag, grace_steps=3)
        early.append(bool(e[0]))
        counts.append(int(cnt[0]))
    assert counts == [1, 2, 0, 1, 2, 3] and early == [False] * 5 + [True]
    # grace_steps = 1: every step at which the predicate holds ends the episode
    cnt[:], tag[:] = 0, -1
    e1 = [bool(c.termination_eval_host({"qpos": f["qpos"][k:k + 1]}, ep, cnt, tag)[0]) for k in range(6)]
    assert e1 == list(holds)
    # a change of the episode number clears the count: T T | T with grace 3 does not end
    cnt[:], tag[:] = 0, -1
    for k, epi in enumerate((4, 4, 5, 5, 5)):
        e = c.termination_eval_host({"qpos": f["qpos"][0:1]}, np.array([epi], np.int32), cnt, tag, grace_steps=3)
        assert int(cnt[0]) == (1, 2, 1, 2, 3)[k] and int(tag[0]) == epi and bool(e[0]) == (k == 4)


def test_registry_and_validation(model):
    assert {"fallen", "lost_balance"} <= set(rw.TERMINATION_FUNCTIONS)
    assert rw.device_termination("fallen").defaults == {"min_height": 0.8}
    assert rw.device_termination("lost_balance").defaults == {"min_height": 0.8, "max_roll_pitch": np.pi / 4}
    with pytest.raises(ValueError, match="Unknown termination type: nope"):
        rw.device_termination("nope")
    with pytest.raises(ValueError, match="Unknown termination type"):
        rw.termination_from_config({"type": "stand"})            # a reward is not a termination
    with pytest.raises(ValueError, match="unknown parameter 'height' for termination 'fallen'"):
        rw.termination_from_config({"type": "fallen", "params": {"height": 1.0}})
    with pytest.raises(ValueError, match="unknown parameter"):
        rw.TERMINATION_FUNCTIONS["fallen"](env_data(0), {"height": 1.0})
    for g in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="grace_steps"):
            rw.termination_from_config({"type": "fallen", "grace_steps": g})
    with pytest.raises(ValueError, match="unknown key"):
        rw.termination_from_config({"type": "fallen", "grace": 2})
    assert rw.termination_from_config(None) is None
    rec, params, grace = rw.termination_from_config({"type": "fallen", "params": {"min_height": 0.9}, "grace_steps": 4})
    assert rec is rw.device_termination("fallen") and params == {"min_height": 0.9} and grace == 4

    reg = {}

    @rw.register_device_termination("mine", defaults={"v": 2.0}, registry=reg)
    def mine(d, p):
        return (d.qvel[2] < -p["v"]) & (d.qpos[2] < 1.0)
    assert "mine" not in rw.TERMINATION_FUNCTIONS and rw.device_termination("mine", reg).fn is mine
    assert type(reg["mine"](env_data(0))) is bool
    # the tracer's refusals are the rewards': an unknown parameter key, bool() of a traced value, the limits
    tr = lambda fn, keys=(): rw.trace(fn, DIMS, keys)  # noqa: E731
    with pytest.raises(ValueError, match="unknown reward parameter 'nope'"):
        tr(lambda d, p: d.qpos[2] < p["nope"], ["min_height"])

    def with_if(d, p):
        if d.qpos[2] < 0.8:
            return True
        return abs(d.qpos[3]) < 0.5
    with pytest.raises(TypeError, match="rw.where"):
        tr(with_if)
    with pytest.raises(TypeError, match="rw.where"):
        tr(lambda d, p: d.qpos[2] < 0.8 or d.qpos[2] > 2.0)

    def all_alive(d, p):
        xs = [d.qpos[i % 28] * float(i + 2) for i in range(70)]
        acc = xs[0]
        for x in xs[1:]:
            acc = acc * x
        return acc > 0.0
    with pytest.raises(ValueError, match="64 live values"):
        rw.DeviceTermination("alive", all_alive, None).trace(DIMS)


def test_validator_refuses_an_over_limit_predicate_and_null_arguments_fail(model):
    """A predicate is validated by hs_reward_program_create like any program: 4098 instructions are refused."""
    import ctypes as C

    from mujocoposelearning_amd import _lib
    L = _lib.lib()
    O = rw.OP
    rows = [[O["const"], 0, 0, 0, 0]] * 4097 + [[O["result"], 0, 0, 0, 0]]
    code = np.ascontiguousarray(rows, dtype=np.int32)
    consts = np.zeros(1)
    h = C.c_void_p(1)
    assert L.hs_reward_program_create(model.handle, code.ctypes.data, len(rows), consts.ctypes.data, 1, 0, C.byref(h)) < 0
    assert not h.value and b"4098 instructions, the limit is 4096" in L.hs_last_error()
    c = rw.device_termination("fallen").compile(model)
    ep, cnt, tag = _fresh(4)
    early = np.zeros(4, np.uint8)
    f = _lib.hs_reward_fields(qpos=QPOS.ctypes.data)
    par = c.params(None)
    args = (f, ep, cnt, tag, early)
    call = lambda pred, p, g, n, fl, e, k, t, o: L.hs_termination_eval_host(  # noqa: E731
        pred, p, g, n, C.byref(fl), e.ctypes.data, k.ctypes.data, t.ctypes.data, o.ctypes.data)
    assert call(c.handle, par, 1, 4, *args) == 0
    assert call(c.handle, par, 0, 4, *args) < 0 and b"grace_steps must be >= 1" in L.hs_last_error()
    assert call(c.handle, None, 1, 4, *args) < 0
    assert call(None, par, 1, 4, *args) < 0
    assert call(c.handle, par, 1, 4, _lib.hs_reward_fields(), ep, cnt, tag, early) < 0
    assert b"reads qpos, which is NULL" in L.hs_last_error()
    assert L.hs_set_termination(None, None, None, 1) < 0 and L.hs_apply_termination(None, None) < 0
    assert L.hs_termination_state(None, None, None, None, None) < 0


# -- the same host code under AddressSanitizer / UBSan, as a stand-alone program ------------------
def _file(path, code, consts, params, qpos, episodes, grace, n_instr=None):
    rows = np.asarray(code, dtype=np.int64).reshape(-1, 5)
    n = len(qpos)
    head = list(DIMS) + [len(rows) if n_instr is None else n_instr, len(consts), len(params), n, grace]
    parts = [" ".join(map(str, head)), " ".join(map(str, rows.reshape(-1))),
             " ".join(repr(float(v)) for v in consts), " ".join(repr(float(v)) for v in params)]
    lens = dict(qpos=28, qvel=27, ctrl=21, time=1, qfrc_actuator=27, cinert=170, cvel=102, subtree_com=3,
                cfrc_ext=102, subtree_linvel=51)
    for name in rw.FIELDS:
        a = qpos if name == "qpos" else np.zeros((n, lens[name]))
        parts.append(" ".join(repr(float(v)) for v in np.asarray(a).reshape(-1)))
    parts.append(" ".join(str(int(e)) for e in episodes))
    path.write_text("\n".join(parts) + "\n")
    return str(path)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_validator_interpreter_and_grace_update_under_sanitizers(model, tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mujocoposelearning_amd", "csrc"), "asan-termination"])
    exe = os.path.join(ROOT, "build", "asan", "termination_check")
    files, expect = [], []
    # the built-ins on every state with grace 1 (one env's sequence: the count runs on while the predicate holds)
    for k, (name, params) in enumerate(CASES):
        rec = rw.device_termination(name)
        c = rec.compile(model)
        files.append(_file(tmp_path / f"case{k}.txt", c.traced.code, c.traced.consts, rec.params(params), QPOS,
                           np.zeros(NS, int), 1))
        twin = _twin(name, params)
        counts, run = [], 0
        for t in twin:
            run = run + 1 if t else 0
            counts.append(run)
        expect.append(("OK", [f"{int(t)}:{n}" for t, n in zip(twin, counts)]))
    # the grace trace T T F T T T, grace 3, and the episode change
    rec = rw.device_termination("fallen")
    c = rec.compile(model)
    q = _trace_fields(np.array([1, 1, 0, 1, 1, 1], bool))["qpos"]
    files.append(_file(tmp_path / "grace.txt", c.traced.code, c.traced.consts, rec.params(), q, [0] * 6, 3))
    expect.append(("OK", ["0:1", "0:2", "0:0", "0:1", "0:2", "1:3"]))
    q = _trace_fields(np.ones(5, bool))["qpos"]
    files.append(_file(tmp_path / "episode.txt", c.traced.code, c.traced.consts, rec.params(), q, [4, 4, 5, 5, 5], 3))
    expect.append(("OK", ["0:1", "0:2", "0:1", "0:2", "1:3"]))
    # refused by the validator: over the instruction limit, a field index outside the model, and a bad grace period
    O = rw.OP
    files.append(_file(tmp_path / "long.txt", [[O["const"], 0, 0, 0, 0]] * 4097 + [[O["result"], 0, 0, 0, 0]], [0.0],
                       [], q, [0] * 5, 1))
    expect.append(("ERR", "4098 instructions, the limit is 4096"))
    files.append(_file(tmp_path / "index.txt", [[O["load"], 0, 0, 28, 0], [O["result"], 0, 0, 0, 0]], [], [], q,
                       [0] * 5, 1))
    expect.append(("ERR", "field index 28 outside the model's dimensions"))
    files.append(_file(tmp_path / "grace0.txt", c.traced.code, c.traced.consts, rec.params(), q, [0] * 5, 0))
    expect.append(("ERR", "grace_steps must be >= 1"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(files)
    for line, (kind, want), f in zip(lines, expect, files):
        assert line.startswith(kind), (f, line)
        if kind == "OK":
            assert line.split()[1:] == want, f
        else:
            assert want in line, (f, line)
