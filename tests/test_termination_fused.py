"""The built-in termination conditions of the fused launches, on the CPU (csrc/hs_term_builtin.h,
hs_termination_builtin_eval_host; reward_program.py termination_fused_from_config): the predicate the step kernel's
TERM instances run against the registry's numeric twins, the ``"fused"`` flag's parsing, and the predicate and the
probe-table check of hs_set_termination_builtin under sanitizers as a stand-alone program.

The twins go through numpy's arctan2 / arcsin, the built-in through the C library's atan2 / asin: an ulp or two
apart, so a row whose |roll|, |pitch| or height lies within 1e-9 of its threshold is left out of the comparison.
At most 1 % of the rows may be left out (asserted; with this seed none is).
"""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT, XML

from mujocoposelearning_amd import reward_program as rw
from mujocoposelearning_amd.utils import quaternion_to_euler

DIMS = (28, 27, 21, 17)
KIND = {"fallen": rw.TERM_FALLEN, "lost_balance": rw.TERM_LOST_BALANCE}
CASES = [("fallen", None), ("fallen", {"min_height": 1.0}), ("lost_balance", None),
         ("lost_balance", {"min_height": 0.6, "max_roll_pitch": 0.2})]
IDS = ["fallen", "fallen_override", "lost_balance", "lost_balance_override"]
NROWS = 512


def _rows():
    """512 seeded qpos rows: heights U(0.2, 1.4), random unit quaternions, every fourth scaled by 1.05 so that
    |2 (w y - z x)| > 1 (a NaN pitch) occurs."""
    rng = np.random.default_rng(20260)
    q = np.zeros((NROWS, 28))
    q[:, 2] = rng.uniform(0.2, 1.4, NROWS)
    quat = rng.normal(size=(NROWS, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    quat[::4] *= 1.05
    q[:, 3:7] = quat
    return q


QPOS = _rows()


def _resolved(name, params):
    rec = rw.device_termination(name)
    return dict(zip(rec.param_keys, rec.params(params)))


def _twin(name, params):
    fn = rw.TERMINATION_FUNCTIONS[name]
    with np.errstate(invalid="ignore"):
        return np.array([fn(SimpleNamespace(qpos=QPOS[i]), dict(params) if params else None) for i in range(NROWS)])


def _near_threshold(name, vals):
    """Rows whose height, |roll| or |pitch| lies within 1e-9 of the threshold it is compared with."""
    near = np.abs(QPOS[:, 2] - vals["min_height"]) <= 1e-9
    if name == "lost_balance":
        with np.errstate(invalid="ignore"):
            rp = np.array([quaternion_to_euler(QPOS[i, 3:7])[:2] for i in range(NROWS)])
        near |= (np.abs(np.abs(rp) - vals["max_roll_pitch"]) <= 1e-9).any(axis=1)   # (a NaN pitch is not near)
    return near


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_builtin_equals_the_registered_twin(case):
    name, params = CASES[case]
    vals = _resolved(name, params)
    got = rw.builtin_termination_eval_host(KIND[name], QPOS, vals["min_height"], vals.get("max_roll_pitch", 0.0))
    twin = _twin(name, params)
    left_out = _near_threshold(name, vals)
    print(f"{name} {params}: {int(left_out.sum())} of {NROWS} rows within 1e-9 of a threshold; "
          f"{int(twin.sum())} hold, {int((~twin).sum())} do not")
    assert left_out.mean() <= 0.01
    keep = ~left_out
    assert np.array_equal(got[keep], twin[keep])
    assert twin.any() and not twin.all() and got.any() and not got.all()
    with np.errstate(invalid="ignore"):
        pitch = np.array([quaternion_to_euler(QPOS[i, 3:7])[1] for i in range(NROWS)])
    assert np.isnan(pitch).any()
    # a NaN pitch alone does not terminate: no roll, well above min_height, 2 (w y - z x) = 1.08
    row = np.zeros((1, 28))
    row[0, 2:7] = [vals["min_height"] + 0.5, 0.9, 0.0, 0.6, 0.0]
    assert np.isnan(quaternion_to_euler(row[0, 3:7])[1])
    assert not rw.builtin_termination_eval_host(KIND[name], row, vals["min_height"], vals.get("max_roll_pitch", 0.0))[0]


def test_builtin_eval_host_refusals():
    from mujocoposelearning_amd import _lib
    L = _lib.lib()
    out = np.zeros(4, np.uint8)
    q = np.ascontiguousarray(QPOS[:4])
    assert L.hs_termination_builtin_eval_host(3, 0.8, 0.7, 4, q.ctypes.data, 28, out.ctypes.data) < 0
    assert b"kind" in L.hs_last_error()
    assert L.hs_termination_builtin_eval_host(1, 0.8, 0.7, 4, q.ctypes.data, 6, out.ctypes.data) < 0
    assert L.hs_termination_builtin_eval_host(1, 0.8, 0.7, 4, None, 28, out.ctypes.data) < 0
    assert L.hs_termination_builtin_eval_host(1, 0.8, 0.7, 0, None, 28, None) == 0
    assert L.hs_set_termination_builtin(None, None, None, 1, 1, 0.8, 0.7) < 0


def test_fused_flag_parsing():
    base = {"type": "fallen", "params": {"min_height": 0.9}, "grace_steps": 2}
    assert rw.termination_fused_from_config(None) is False
    assert rw.termination_fused_from_config(base) is False
    assert rw.termination_fused_from_config(dict(base, fused=False)) is False
    assert rw.termination_fused_from_config(dict(base, fused=True)) is True
    assert rw.termination_fused_from_config({"type": "lost_balance", "fused": True}) is True
    # termination_from_config keeps its 3-tuple and accepts the key
    rec, params, grace = rw.termination_from_config(dict(base, fused=True))
    assert (rec.name, params, grace) == ("fallen", {"min_height": 0.9}, 2)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="fused must be a bool"):
            rw.termination_fused_from_config(dict(base, fused=bad))
        with pytest.raises(ValueError, match="fused must be a bool"):
            rw.termination_from_config(dict(base, fused=bad))
    with pytest.raises(ValueError, match="unknown key"):
        rw.termination_from_config(dict(base, fuse=True))
    # a user-registered predicate is not one of the built-ins, whatever it computes
    reg = {}
    rw.register_device_termination("low", lambda d, p: d.qpos[2] < p["min_height"], defaults={"min_height": 0.8},
                                   registry=reg)
    assert rw.termination_fused_from_config({"type": "low"}, reg) is False
    with pytest.raises(ValueError, match="user-registered predicate"):
        rw.termination_fused_from_config({"type": "low", "fused": True}, reg)
    # the built-in functions are recognised under another name too
    rw.register_device_termination("fallen_again", rw.fallen, defaults={"min_height": 0.7}, registry=reg)
    assert rw.termination_fused_from_config({"type": "fallen_again", "fused": True}, reg) is True
    assert rw.builtin_termination_kind(rw.device_termination("lost_balance")) == rw.TERM_LOST_BALANCE


# -- the predicate and the probe-table check under AddressSanitizer / UBSan, as a stand-alone program ----------
def _file(path, code, consts, params, kind, min_height, max_roll_pitch, rows):
    code = np.asarray(code, dtype=np.int64).reshape(-1, 5)
    head = list(DIMS) + [len(code), len(consts), len(params), kind, repr(float(min_height)),
                         repr(float(max_roll_pitch)), len(rows)]
    parts = [" ".join(map(str, head)), " ".join(map(str, code.reshape(-1))),
             " ".join(repr(float(v)) for v in consts), " ".join(repr(float(v)) for v in params),
             " ".join(repr(float(v)) for v in np.asarray(rows).reshape(-1))]
    path.write_text("\n".join(parts) + "\n")
    return str(path)


def test_builtin_and_probe_check_under_sanitizers(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mujocoposelearning_amd", "csrc"),
                           "asan-term-builtin"])
    exe = os.path.join(ROOT, "build", "asan", "term_builtin_check")
    rows = QPOS[:, 2:7]
    files, expect = [], []

    def add(tag, prog_name, prog_params, kind_name, kind_params, probe):
        rec = rw.device_termination(prog_name)
        t = rec.trace(DIMS)
        vals = _resolved(kind_name, kind_params)
        mh, mrp = vals["min_height"], vals.get("max_roll_pitch", 0.0)
        files.append(_file(tmp_path / f"{tag}.txt", t.code, t.consts, rec.params(prog_params), KIND[kind_name], mh, mrp,
                           rows))
        bits = rw.builtin_termination_eval_host(KIND[kind_name], QPOS, mh, mrp)
        expect.append((probe, "".join("1" if b else "0" for b in bits)))

    # program and built-in the same predicate: the probe table finds no difference
    for k, (name, params) in enumerate(CASES):
        add(f"same{k}", name, params, name, params, lambda p: p == -1)
    # mismatches the table must find: the other kind, another min_height, another max_roll_pitch
    add("kind", "fallen", None, "lost_balance", None, lambda p: p >= 4)          # (the height rows agree)
    add("kind2", "lost_balance", None, "fallen", None, lambda p: p >= 4)
    add("height", "fallen", {"min_height": 0.9}, "fallen", None, lambda p: 0 <= p < 4)
    add("angle", "lost_balance", {"max_roll_pitch": 0.5}, "lost_balance", None, lambda p: p >= 4)
    # a predicate that reads ctrl is not a function of qpos alone
    reg = {}
    rw.register_device_termination("ctrl", lambda d, p: (d.qpos[2] < 0.8) | (d.ctrl[0] > 2.0), registry=reg)
    t = rw.device_termination("ctrl", reg).trace(DIMS)
    files.append(_file(tmp_path / "ctrl.txt", t.code, t.consts, [], rw.TERM_FALLEN, 0.8, 0.0, rows))
    expect.append((lambda p: p == -2, "".join("1" if b else "0" for b in
                                               rw.builtin_termination_eval_host(rw.TERM_FALLEN, QPOS, 0.8, 0.0))))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(files)
    for line, (probe_ok, bits), f in zip(lines, expect, files):
        tok = line.split()
        assert tok[0] == "OK" and len(tok) == 3, (f, line)
        assert probe_ok(int(tok[1])), (f, tok[1])
        assert tok[2] == bits, f
