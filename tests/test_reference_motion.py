"""Reference-motion targets on the CPU (mujocoposelearning_amd/reference_motion.py, reward_program.py,
csrc/hs_reward_prog.h): the two reference fields, the phase function and the host interpreter against the numpy
restatement, the registered "track" / "off_track", the refusals, and the same host code under sanitizers.

Bars.  The host interpreter against ``reference_motion.sample``: BITWISE, float64 and float32 -- the sample is five
correctly rounded operations (a divide and an add in float64, a subtraction, a product and an add in T), which C
and numpy round alike, so there is no error to allow for.  "track" / "off_track", numeric twin against host
interpreter: the 1e-14 relative of tests/test_reward_program.py (glibc's exp against numpy's).
"""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, XML
from reference_motion_cases import (DIMS, KEY_DT, NQ, NV, PROBE_NAMES, SEED, edge_times, probe_expected, probe_registry,
                                    reference, rows, times_of)
from reward_program_cases import FIELDS, N, bits_equal

from mujocoposelearning_amd import _lib
from mujocoposelearning_amd import reference_motion as rm
from mujocoposelearning_amd import reward_functions as rf
from mujocoposelearning_amd import reward_program as rw

REG = probe_registry()

# (instructions, slots, sha256 of the int32 code bytes followed by the float64 constant bytes) of the built-in
# programs traced for humanoid.xml's dimensions, recorded from the commit before the reference fields existed
PARENT_TRACES = {
    "stand_program": (167, 28, "812a99e458d2c7918c594d71b90813353d3a6500feb317377e96770ab7639c7e"),
    "kneeling_program": (241, 27, "a55d5fdef129d4d2b4539946d4637ff00d4df308b1fccb0495c37fda25ca5864"),
    "walk_program": (119, 24, "29913fffdfccbb73badd506a287698737fd58a6939fb59e6e8ecad0f610c6a9b"),
    "stand_components_program": (172, 28, "6766758743b4fd13ade8c82097505b444afca367a19be4804117ceeecc4788a9"),
    "kneeling_components_program": (247, 27, "cd5ac427782ced58a81362ec28a3ef00902eef78bcc6bff4b1bc962406e7ddde"),
    "walk_components_program": (123, 24, "aebffafa9178bdd04813a3aca6740f60318dcf86849439c3255d201029ab77bc"),
}


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


@pytest.fixture(scope="module")
def probe_prog(model):
    return rw.device_reward_program("ref_probe", REG).compile(model)


# ------------------------------------------------------------------ field ids
def test_old_fields_keep_their_ids_and_old_programs_their_bytes():
    old = ("qpos", "qvel", "ctrl", "time", "qfrc_actuator", "cinert", "cvel", "subtree_com", "cfrc_ext", "subtree_linvel")
    assert rw.FIELDS == old and [rw.FIELD_ID[k] for k in old] == list(range(10))
    assert (rw.FIELD_ID["ref_qpos"], rw.FIELD_ID["ref_qvel"]) == (16, 17) and rw.REFERENCE_FIELDS == ("ref_qpos", "ref_qvel")
    for name, (n_instr, n_slots, digest) in PARENT_TRACES.items():
        keys = list(rw.KNEEL_DEFAULTS) if name.startswith("kneeling") else ()
        t = rw.trace(getattr(rw, name), DIMS, keys)
        got = hashlib.sha256(np.ascontiguousarray(t.code, dtype=np.int32).tobytes() +
                             np.ascontiguousarray(t.consts, dtype=np.float64).tobytes()).hexdigest()
        assert (t.n_instr, t.n_slots, got) == (n_instr, n_slots, digest), name
        assert not set(t.fields) & set(rw.REFERENCE_FIELDS)


def test_reference_fields_are_loads_reported_in_the_mask_and_bounded(model, probe_prog):
    t = probe_prog.traced
    assert t.fields == ["ref_qpos", "ref_qvel"] and t.outputs == PROBE_NAMES
    loads = t.code[t.code[:, 0] == rw.OP["load"]]
    assert set(loads[:, 2]) == {16, 17} and len(t.code[t.code[:, 0] >= len(rw._OPS)]) == 0      # no new opcode
    L = _lib.lib()
    fl = C.c_uint()
    assert L.hs_reward_program_info(probe_prog.handle, None, None, C.byref(fl)) == 0 and fl.value == (1 << 16) | (1 << 17)
    h = C.c_void_p()
    for field, bad, msg in ((16, NQ, b"field 16 has 28 values"), (17, NV, b"field 17 has 27 values"),
                            (18, 0, b"unknown field 18"), (12, 0, b"unknown field 12")):
        code = np.array([[rw.OP["load"], 0, field, bad, 0], [rw.OP["result"], 0, 0, 0, 0]], dtype=np.int32)
        assert L.hs_reward_program_create(model.handle, code.ctypes.data, 2, None, 0, 0, C.byref(h)) < 0 and not h.value
        assert msg in L.hs_last_error(), L.hs_last_error()
    code = np.array([[rw.OP["load"], 0, 17, NV - 1, 0], [rw.OP["result"], 0, 0, 0, 0]], dtype=np.int32)
    assert L.hs_reward_program_create(model.handle, code.ctypes.data, 2, None, 0, 0, C.byref(h)) == 0
    L.hs_reward_program_destroy(h)
    assert C.sizeof(_lib.hs_reward_fields) == 10 * C.sizeof(C.c_void_p)                         # the layout stays


# ------------------------------------------------------------------ host interpreter against sample
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("K", [1, 2, 7])
def test_host_interpreter_equals_sample_bitwise(probe_prog, K, dtype):
    t = times_of(K, dtype)
    n = len(t)
    episode = np.arange(n) % 4                                  # episode 0 (never reset) among them
    for end in rm.END_MODES:
        for start in rm.START_MODES:
            ref = reference(K, end, start)
            x, i, i1, frac = rm.phase(ref, t, episode, SEED)
            assert i.min() >= 0 and i.max() <= K - 1 and i1.min() >= 0 and i1.max() <= K - 1
            assert (frac >= 0).all() and (frac < 1).all() and np.isfinite(x).all()
            q, v = rm.sample(ref, t, episode, SEED, dtype=dtype)
            assert q.dtype == dtype and q.shape == (n, NQ) and v.shape == (n, NV)
            out, comp = probe_prog.eval_host({"time": t}, components=True,
                                             reference={"motion": ref, "episode": episode, "seed": SEED, "dtype": dtype})
            want = probe_expected(q.astype(np.float64), v.astype(np.float64))
            for c, name in enumerate(PROBE_NAMES):
                assert bits_equal(comp[c], want[c]), (K, end, start, name, np.flatnonzero(comp[c] != want[c])[:5])
            assert bits_equal(out, want[-1])
            if K == 1:                                          # the row itself, whatever the time
                assert np.array_equal(q, np.broadcast_to(ref.qpos.astype(dtype), (n, NQ)))
                assert np.array_equal(v, np.broadcast_to(ref.qvel.astype(dtype), (n, NV)))


def test_phase_semantics():
    """The definition on hand-worked cases: boundaries give the row exactly, hold clamps, loop wraps, a drawn
    start is initial_state.draw_index (0 for episode 0), NaN / negative / huge times index inside the table."""
    from mujocoposelearning_amd.initial_state import draw_index
    K = 7
    hold, loop = reference(K, "hold"), reference(K, "loop")
    t = np.array([0.0, KEY_DT, 0.5 * KEY_DT, 6 * KEY_DT, 6.5 * KEY_DT, 7 * KEY_DT, 15.25 * KEY_DT, np.nan, -3.0, np.inf,
                  1e300])
    x, i, i1, w = rm.phase(hold, t)
    assert i.tolist() == [0, 1, 0, 6, 6, 6, 6, 0, 0, 6, 6] and i1.tolist() == [1, 2, 1, 6, 6, 6, 6, 1, 1, 6, 6]
    assert w.tolist() == [0, 0, 0.5, 0, 0, 0, 0, 0, 0, 0, 0]
    x, i, i1, w = rm.phase(loop, t)
    assert i.tolist()[:8] == [0, 1, 0, 6, 6, 0, 1, 0] and i1.tolist()[:8] == [1, 2, 1, 0, 0, 1, 2, 1]
    assert w.tolist()[:7] == [0, 0, 0.5, 0, 0.5, 0, 0.25] and i[9] == i[10] == 2 ** 52 % K and w[9] == w[10] == 0
    q, _ = rm.sample(hold, t[:2])
    assert np.array_equal(q, hold.qpos[:2])                     # w == 0 gives the row exactly
    drawn = reference(K, "hold", "drawn")
    ep = np.array([0, 1, 2, 3, 4, 5])
    j0 = rm.start_rows(drawn, 6, ep, SEED)
    assert j0[0] == 0 and np.array_equal(j0[1:], draw_index(SEED, np.arange(1, 6), ep[1:], K))
    assert len(set(rm.start_rows(drawn, 64, np.full(64, 3), SEED).tolist())) > 3
    x, i, _, _ = rm.phase(drawn, np.full(6, 1.5 * KEY_DT), ep, SEED)
    assert np.array_equal(i, np.minimum(j0 + 1, K - 1))
    # quaternions are interpolated like any coordinate and not renormalised
    q, _ = rm.sample(hold, np.array([0.5 * KEY_DT]))
    assert np.linalg.norm(q[0, 3:7]) < 1.0 and np.allclose(np.linalg.norm(hold.qpos[:, 3:7], axis=1), 1.0)


# ------------------------------------------------------------------ "track" and "off_track"
def _states_with_reference(ref, dtype=np.float64):
    """The golden states with a reference sampled at their own times: (fields, env_data(i), reference dict)."""
    from types import SimpleNamespace
    episode = np.arange(N) % 3
    q, v = rm.sample(ref, FIELDS["time"], episode, SEED, dtype=dtype)

    def env_data(i):
        d = {k: (float(a[i]) if k == "time" else a[i]) for k, a in FIELDS.items()}
        return SimpleNamespace(ref_qpos=q[i].astype(np.float64), ref_qvel=v[i].astype(np.float64), **d)
    return env_data, {"motion": ref, "episode": episode, "seed": SEED, "dtype": dtype}


def golden_reference(K=7, end="loop", start="drawn"):
    """A reference near the golden states: rows taken from them (so that the errors are moderate and the
    exponentials of "track" neither vanish nor saturate everywhere)."""
    idx = np.linspace(0, N - 1, K).astype(int)
    return rm.Reference(FIELDS["qpos"][idx], FIELDS["qvel"][idx] * 0.1, key_dt=0.5, end=end, start=start)


@pytest.mark.parametrize("params", [None, {"k_pose": 0.3, "w_root": 1.5, "k_root": 0.7}], ids=["defaults", "overrides"])
def test_track_twin_equals_host_interpreter(model, params):
    ref = golden_reference()
    env_data, refd = _states_with_reference(ref)
    rec = rw.device_reward_program("track")
    assert rec is not None and rec.component_names == ("pose", "velocity", "root", "total")
    assert set(rf.REWARD_FUNCTIONS) == {"default", "kneeling", "stand", "walk"} and rf.device_reward_id("track") is None
    twin = np.array([rec.twin(env_data(i), params) for i in range(N)])
    comps = [rec.twin_components(env_data(i), params) for i in range(N)]
    assert bits_equal(twin, [c["total"] for c in comps])                       # bit for bit the twin's value
    c = rec.compile(model)
    assert {"ref_qpos", "ref_qvel", "qpos", "qvel"} == set(c.fields)
    h, hc = c.eval_host(FIELDS, params, components=True, reference=refd)
    ok = np.isfinite(twin)
    assert ok.sum() > 190 and np.array_equal(np.isnan(h), np.isnan(twin))
    rel = np.abs(h[ok] - twin[ok]) / np.abs(twin[ok]).clip(1e-300)
    print(f"track: host interpreter vs twin max rel {rel.max():.2e}; total in [{twin[ok].min():.3g}, {twin[ok].max():.3g}]; "
          f"{c.traced.n_instr} instructions, {c.traced.n_slots} slots")
    assert rel.max() <= 1e-14
    assert twin[ok].max() > 0.05 and twin[ok].min() < twin[ok].max() * 0.5      # the states spread over the reward
    for k, name in enumerate(c.outputs):
        t = np.array([cc[name] for cc in comps])
        assert (np.abs(hc[k][ok] - t[ok]) <= 1e-14 * np.abs(t[ok])).all(), name
    assert bits_equal(h, hc[c.outputs.index("total")])


def test_off_track_twin_equals_host_interpreter(model):
    ref = golden_reference(end="hold", start="zero")
    env_data, refd = _states_with_reference(ref)
    rec = rw.device_termination("off_track")
    c = rec.compile(model)
    assert set(c.fields) == {"qpos", "ref_qpos"}
    for dist in (0.5, 1.2):
        twin = np.array([rec.twin(env_data(i), {"max_root_dist": dist}) for i in range(N)])
        assert twin.dtype == bool and 0 < twin.sum() < N
        value = c.eval_host(FIELDS, {"max_root_dist": dist}, reference=refd)
        assert np.array_equal(value != 0, twin)
        count, tag = np.zeros(N, np.int32), np.full(N, -1, np.int32)
        early = c.termination_eval_host(FIELDS, refd["episode"], count, tag, {"max_root_dist": dist}, grace_steps=1,
                                        reference=refd)
        assert np.array_equal(early, twin) and np.array_equal(count, twin.astype(np.int32))
        early = c.termination_eval_host(FIELDS, refd["episode"], count, tag, {"max_root_dist": dist}, grace_steps=3,
                                        reference=refd)
        assert not early.any() and np.array_equal(count, 2 * twin.astype(np.int32))       # the grace period counts on


# ------------------------------------------------------------------ refusals
def test_refusals_python(model):
    with pytest.raises(ValueError, match="unknown key.*'speed'.*valid: keyframe, keyframes, trajectory, stride, states, "
                                         "key_dt, end, start, from_initial_state"):
        rm.build_reference(model, {"keyframe": "squat", "speed": 2})
    with pytest.raises(ValueError, match="key_dt .* is required with more than one row"):
        rm.build_reference(model, {"keyframes": ["squat", "prone"]})
    with pytest.raises(ValueError, match="key_dt must be finite and > 0"):
        rm.build_reference(model, {"keyframes": ["squat", "prone"], "key_dt": 0.0})
    with pytest.raises(ValueError, match="end must be one of 'hold', 'loop'"):
        rm.build_reference(model, {"keyframe": "squat", "end": "bounce"})
    with pytest.raises(ValueError, match="start must be one of 'zero', 'drawn'"):
        rm.build_reference(model, {"keyframe": "squat", "start": "random"})
    with pytest.raises(ValueError, match="unknown keyframe 'sit'"):
        rm.build_reference(model, {"keyframe": "sit"})
    with pytest.raises(ValueError, match="'from_initial_state' needs an initial_state spec"):
        rm.build_reference(model, {"from_initial_state": True, "key_dt": 0.1})
    with pytest.raises(ValueError, match="the limit is 4096"):
        rm.Reference(np.ones((4097, NQ)), key_dt=0.1)
    one = rm.build_reference(model, {"keyframe": "squat"})                      # K == 1: key_dt not needed
    assert one.K == 1 and one.key_dt is None and one.qvel.shape == (1, NV)
    ref = rm.build_reference(model, {"from_initial_state": True, "key_dt": 0.1, "end": "loop"},
                             {"keyframes": ["squat", "prone", "default"], "noise_scale": 0.02})
    assert (ref.K, ref.start, ref.end, ref.flags) == (3, "drawn", "loop", 3)
    with pytest.raises(ValueError, match="start='drawn' needs 'episode'"):
        rw.device_reward_program("ref_probe", REG).compile(model).eval_host(
            {"time": np.zeros(2)}, reference={"motion": reference(2, start="drawn")})


def test_env_configs_are_refused_before_a_batch_exists(model):
    """The checks run on the CPU ahead of HsBatch: on a machine without a GPU the batch itself would raise
    RuntimeError, so a ValueError here is raised before one is made."""
    from mujocoposelearning_amd.env import HumanoidEnv
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    base = {"model_path": XML}
    for make in (lambda cfg: HumanoidVecEnv(cfg, n_envs=2, model=model), HumanoidEnv):
        with pytest.raises(ValueError, match="reward 'track' reads ref_qpos, ref_qvel, but the env config has no "
                                             "'reference_motion'"):
            make(dict(base, reward_config={"type": "track"}))
        with pytest.raises(ValueError, match="termination 'off_track' reads ref_qpos"):
            make(dict(base, termination={"type": "off_track"}))
        with pytest.raises(ValueError, match="unknown key.*'dt'"):
            make(dict(base, reference_motion={"keyframe": "squat", "dt": 0.1}))
        with pytest.raises(ValueError, match="start='drawn' needs an 'initial_state' bank of the same 2 rows.*has 3"):
            make(dict(base, initial_state={"keyframes": ["squat", "prone", "default"]},
                      reference_motion={"keyframes": ["squat", "prone"], "key_dt": 0.1, "start": "drawn"}))
        with pytest.raises(ValueError, match="start='drawn' needs an 'initial_state' bank.*the config has none"):
            make(dict(base, reference_motion={"keyframes": ["squat", "prone"], "key_dt": 0.1, "start": "drawn"}))


def test_refusals_c_abi(model, probe_prog):
    """The fields-struct entry points refuse a program that reads a reference field and name the batch entry
    point; the new entries check their reference.  Nothing is launched: every call fails on the host."""
    L = _lib.lib()
    t = np.zeros(4)
    out = np.zeros(4)
    f = _lib.hs_reward_fields(time=t.ctypes.data)
    par = probe_prog.params(None)
    assert L.hs_reward_program_eval_host(probe_prog.handle, par, 4, C.byref(f), out.ctypes.data) < 0
    msg = L.hs_last_error()
    assert b"reads ref_qpos" in msg and b"hs_reward_program_batch" in msg and b"hs_set_reference_motion" in msg
    with pytest.raises(_lib.HsimError, match="reads ref_qpos.*hs_reward_program_batch"):
        probe_prog.eval_host({"time": t})
    assert L.hs_reward_program_eval(probe_prog.handle, _lib.HS_FP64, par, 4, C.byref(f), out.ctypes.data, None) < 0
    assert b"hs_reward_program_eval: the program reads ref_qpos" in L.hs_last_error()
    pred = rw.device_termination("off_track").compile(model)
    cnt, tag, early, ep = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint8), np.zeros(4, np.int32)
    fq = _lib.hs_reward_fields(qpos=FIELDS["qpos"].ctypes.data, time=t.ctypes.data)
    assert L.hs_termination_eval_host(pred.handle, pred.params(None), 1, 4, C.byref(fq), ep.ctypes.data, cnt.ctypes.data,
                                      tag.ctypes.data, early.ctypes.data) < 0
    assert b"the predicate reads ref_qpos" in L.hs_last_error() and b"hs_step_program" in L.hs_last_error()
    # the reference entry: its own checks
    q, v = rows(3)
    q, v = np.ascontiguousarray(q), np.ascontiguousarray(v)

    def call(**kw):
        ref = _lib.hs_reference_host(**{**dict(n_rows=3, qpos=q.ctypes.data, qvel=v.ctypes.data, key_dt=0.25, flags=0,
                                               precision=_lib.HS_FP64), **kw})
        rc = L.hs_reward_program_eval_host_reference(probe_prog.handle, par, 4, C.byref(kw.pop("fields", f)),
                                                     C.byref(ref), out.ctypes.data, None)
        return rc, L.hs_last_error()
    assert call()[0] == 0
    assert call(qvel=None)[0] == 0                                             # NULL qvel: zeros
    for kw, msg in ((dict(n_rows=0), b"n_rows in [1, 4096]"), (dict(n_rows=5000), b"n_rows in [1, 4096]"),
                    (dict(qpos=None), b"qpos must not be NULL"), (dict(key_dt=0.0), b"key_dt must be finite and > 0"),
                    (dict(key_dt=float("nan")), b"key_dt must be finite and > 0"), (dict(flags=4), b"neither HS_REF_LOOP"),
                    (dict(precision=7), b"precision must be HS_FP32 or HS_FP64"),
                    (dict(flags=2), b"HS_REF_START_DRAWN needs the per-state episode and seed")):
        rc, err = call(**kw)
        assert rc < 0 and msg in err, (kw, err)
    rc = L.hs_reward_program_eval_host_reference(
        probe_prog.handle, par, 4, C.byref(_lib.hs_reward_fields()),
        C.byref(_lib.hs_reference_host(n_rows=3, qpos=q.ctypes.data, key_dt=0.25, precision=_lib.HS_FP64)),
        out.ctypes.data, None)
    assert rc < 0 and b"sampled at the state's time, which is NULL" in L.hs_last_error()
    # the batch entry points: null batch
    assert L.hs_set_reference_motion(None, 3, q.ctypes.data, None, 0.25, 0) < 0 and b"null batch" in L.hs_last_error()
    assert L.hs_get_reference_motion(None, None, None, None) < 0
    assert {"hs_set_reference_motion", "hs_get_reference_motion", "hs_reward_program_eval_host_reference",
            "hs_termination_eval_host_reference"} <= set(_lib.EXPORTED)


# ------------------------------------------------------------------ the same host code under sanitizers
def _case_file(path, traced, params, ref, times, episode, fp32):
    code = np.asarray(traced.code, dtype=np.int64).reshape(-1)
    head = list(DIMS) + [traced.n_instr, len(traced.consts), len(params), len(times), ref.K,
                         repr(float(ref.key_dt or 1.0)), ref.flags, int(fp32), SEED]
    T = np.float32 if fp32 else np.float64
    nums = lambda a: " ".join(repr(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1))  # noqa: E731
    parts = [" ".join(map(str, head)), " ".join(map(str, code)), nums(traced.consts), nums(params), nums(times),
             " ".join(str(int(e)) for e in episode), nums(ref.qpos.astype(T)), nums(ref.qvel.astype(T))]
    path.write_text("\n".join(parts) + "\n")
    return str(path)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_validator_phase_and_host_interpreter_under_sanitizers(model, tmp_path):
    """tools/reference_motion_check.cpp, a stand-alone program built with -fsanitize=address,undefined: the
    validator, the phase function and the host interpreter over the edge times, K = 1 and K = 7, every mode, both
    dtypes; its values are the library's own bit for bit, and a bad program is refused there too."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mujocoposelearning_amd", "csrc"),
                           "asan-reference-motion"])
    exe = os.path.join(ROOT, "build", "asan", "reference_motion_check")
    prog = rw.device_reward_program("ref_scalar", REG).compile(model)
    t = prog.traced
    assert not t.outputs and {"ref_qpos", "ref_qvel", "time"} == set(t.fields)
    files, expect = [], []
    for K in (1, 7):
        for end in rm.END_MODES:
            for start in rm.START_MODES:
                for fp32 in (False, True):
                    dt = np.float32 if fp32 else np.float64
                    times = times_of(K, dt)
                    episode = np.arange(len(times)) % 4
                    ref = reference(K, end, start)
                    files.append(_case_file(tmp_path / f"k{K}_{end}_{start}_{int(fp32)}.txt", t, [], ref, times,
                                            episode, fp32))
                    expect.append(("OK", prog.eval_host({"time": times}, reference={
                        "motion": ref, "episode": episode, "seed": SEED, "dtype": dt})))
    bad = rw.TracedProgram(np.array([[rw.OP["load"], 0, 16, NQ, 0], [rw.OP["result"], 0, 0, 0, 0]]), np.zeros(0), [],
                           1, [])
    files.append(_case_file(tmp_path / "bad_index.txt", bad, [], reference(7), edge_times(7), np.zeros(24, int), False))
    expect.append(("ERR", "field index 28 outside the model's dimensions"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(files)
    for line, (kind, want), f in zip(lines, expect, files):
        assert line.startswith(kind), (f, line)
        if kind == "OK":
            assert bits_equal(np.array([float(x) for x in line.split()[1:]]), want), f
        else:
            assert want in line, (f, line)
