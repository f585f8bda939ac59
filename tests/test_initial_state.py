"""Banks of initial states and the numpy restatement of the device's draw (mujocoposelearning_amd/initial_state.py).
CPU only: build_bank on every spec form and every ValueError case, draw_index / uniform_pm as functions of their
counters, the ABI's argument checks that need no device, and the env-config pass-through of train.py."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from conftest import GOLDEN, XML

TRAJ = os.path.join(GOLDEN, "humanoid_trajectory.xml")


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


def unit(q):
    return q / np.sqrt(((q[3] * q[3] + q[4] * q[4]) + q[5] * q[5]) + q[6] * q[6])


# ------------------------------------------------------------------ build_bank
@pytest.mark.parametrize("name", ["squat", "stand_on_left_leg", "prone", "supine"])
def test_model_keyframes(model, name):
    from mujocoposelearning_amd.initial_state import build_bank
    q, v = build_bank(model, {"keyframe": name})
    assert q.shape == (1, model.nq) and v.shape == (1, model.nv) and q.dtype == v.dtype == np.float64
    key = model.keyframe(name)
    np.testing.assert_array_equal(np.delete(q[0], range(3, 7)), np.delete(key, range(3, 7)))
    np.testing.assert_array_equal(q[0, 3:7], unit(key)[3:7])       # the XML's 6-digit quaternion, normalised
    assert abs(np.linalg.norm(q[0, 3:7]) - 1.0) < 1e-15 and not v.any()


def test_default_row_is_the_reference_start(model):
    from mujocoposelearning_amd.initial_state import build_bank
    q, v = build_bank(model, {"keyframes": ["default"]})
    ref = model.qpos0.copy()
    ref[2] = 1.282
    ref[3:7] = [1, 0, 0, 0]
    np.testing.assert_array_equal(q[0], ref)
    assert not v.any()


def test_trajectory_golden(model):
    """The reference's recorded file: the four model keyframes (no qvel, not part of the recording) and 151
    recorded keys with qpos and qvel."""
    from mujocoposelearning_amd.initial_state import build_bank
    keys = [k for k in ET.parse(TRAJ).getroot().iter("key") if k.get("qvel") is not None]
    assert len(keys) == 151
    q, v = build_bank(model, {"trajectory": TRAJ})
    assert q.shape == (151, model.nq) and v.shape == (151, model.nv)
    for i in (0, 2, 150):
        raw = np.array(keys[i].get("qpos").split(), float)
        np.testing.assert_array_equal(np.delete(q[i], range(3, 7)), np.delete(raw, range(3, 7)))
        np.testing.assert_array_equal(v[i], np.array(keys[i].get("qvel").split(), float))
    assert np.abs(v[2]).max() > 1.0                                  # qvel is read, not zeroed
    # (four components rounded to half an ulp each and the norm's own roundings: within 2 ulp of 1)
    np.testing.assert_allclose(np.linalg.norm(q[:, 3:7], axis=1), 1.0, atol=4.5e-16, rtol=0)
    q2, v2 = build_bank(model, {"trajectory": TRAJ, "stride": 2})
    assert len(q2) == 76
    np.testing.assert_array_equal(q2, q[::2])
    np.testing.assert_array_equal(v2, v[::2])


def test_trajectory_five_keys_stride(model, tmp_path):
    """A keyframe file of 5 recorded keys, as trajectories.write_trajectory_xml lays them out: 5 rows, qvel read,
    stride=2 keeps keys 0, 2, 4."""
    from mujocoposelearning_amd.initial_state import build_bank
    rng = np.random.default_rng(5)
    qs = rng.normal(size=(5, model.nq))
    vs = rng.normal(size=(5, model.nv))
    root = ET.parse(XML).getroot()
    kf = root.find("keyframe")
    for i in range(5):
        key = ET.SubElement(kf, "key")
        key.set("time", f"{0.015 * i:.3f}")
        key.set("qpos", " ".join(repr(float(x)) for x in qs[i]))
        key.set("qvel", " ".join(repr(float(x)) for x in vs[i]))
    path = tmp_path / "five.xml"
    ET.ElementTree(root).write(path)
    q, v = build_bank(model, {"trajectory": str(path)})
    assert q.shape == (5, model.nq)
    np.testing.assert_array_equal(v, vs)
    np.testing.assert_array_equal(q[:, :3], qs[:, :3])
    q2, v2 = build_bank(model, {"trajectory": str(path), "stride": 2})
    assert len(q2) == 3
    np.testing.assert_array_equal(v2, vs[[0, 2, 4]])


def test_states_arrays_and_concatenation_order(model):
    from mujocoposelearning_amd.initial_state import build_bank, default_pose
    sq = default_pose(model)
    sq[7:] = 0.25
    sv = np.full(model.nv, 0.5)
    q, v = build_bank(model, {"states": (sq, sv)})                   # one row given as a vector
    assert q.shape == (1, model.nq)
    np.testing.assert_array_equal(q[0], sq)
    np.testing.assert_array_equal(v[0], sv)
    q0, _ = build_bank(model, {"states": (np.stack([sq, sq]), None)})
    assert q0.shape == (2, model.nq)
    spec = {"states": (sq, sv), "trajectory": TRAJ, "stride": 75, "keyframes": ["prone", "default"],
            "keyframe": "squat", "noise_scale": 0.002}
    q, v = build_bank(model, spec)
    assert len(q) == 1 + 2 + 3 + 1       # keyframe, keyframes, trajectory, states -- whatever the dict's order
    np.testing.assert_array_equal(q[0], build_bank(model, {"keyframe": "squat"})[0][0])
    np.testing.assert_array_equal(q[1], build_bank(model, {"keyframe": "prone"})[0][0])
    np.testing.assert_array_equal(q[2], default_pose(model))
    np.testing.assert_array_equal(q[3:6], build_bank(model, {"trajectory": TRAJ})[0][[0, 75, 150]])
    np.testing.assert_array_equal(q[6], sq)
    assert not v[:3].any() and v[3:6].any() and (v[6] == 0.5).all()


def test_scaled_quaternion_comes_back_normalised(model):
    from mujocoposelearning_amd.initial_state import build_bank, default_pose
    row = default_pose(model)
    row[3:7] = 3.0 * np.array([0.5, -0.5, 0.5, 0.5])
    q, _ = build_bank(model, {"states": (row[None], None)})
    np.testing.assert_allclose(q[0, 3:7], [0.5, -0.5, 0.5, 0.5], atol=1e-16, rtol=0)
    np.testing.assert_array_equal(q[0, :3], row[:3])
    np.testing.assert_array_equal(q[0, 7:], row[7:])


def test_value_errors(model, tmp_path):
    from mujocoposelearning_amd.initial_state import build_bank, default_pose, noise_scale_of
    with pytest.raises(ValueError, match=r"unknown keyframe 'sit'.*squat, stand_on_left_leg, prone, supine, default"):
        build_bank(model, {"keyframe": "sit"})
    with pytest.raises(ValueError, match="unknown keyframe 'kneel'"):
        build_bank(model, {"keyframes": ["squat", "kneel"]})
    with pytest.raises(ValueError, match="unknown key"):
        build_bank(model, {"keyframez": ["squat"]})
    with pytest.raises(ValueError, match="names no states"):
        build_bank(model, {"noise_scale": 0.01})
    with pytest.raises(ValueError, match="non-empty list"):
        build_bank(model, {"keyframes": []})
    with pytest.raises(ValueError, match="'stride' goes with 'trajectory'"):
        build_bank(model, {"keyframe": "squat", "stride": 2})
    with pytest.raises(ValueError, match="stride must be >= 1"):
        build_bank(model, {"trajectory": TRAJ, "stride": 0})
    good = default_pose(model)
    with pytest.raises(ValueError, match="qpos rows must have length 28"):
        build_bank(model, {"states": (good[:-1][None], None)})
    with pytest.raises(ValueError, match="qvel rows must have length 27"):
        build_bank(model, {"states": (good[None], np.zeros((1, model.nv + 1)))})
    with pytest.raises(ValueError, match="1 qpos rows but 2 qvel rows"):
        build_bank(model, {"states": (good[None], np.zeros((2, model.nv)))})
    bad = good.copy()
    bad[9] = np.nan
    with pytest.raises(ValueError, match="qpos holds a value that is not finite"):
        build_bank(model, {"states": (bad[None], None)})
    vbad = np.zeros((1, model.nv))
    vbad[0, 3] = np.inf
    with pytest.raises(ValueError, match="qvel holds a value that is not finite"):
        build_bank(model, {"states": (good[None], vbad)})
    zq = good.copy()
    zq[3:7] = 0
    with pytest.raises(ValueError, match="zero quaternion"):
        build_bank(model, {"states": (zq[None], None)})
    with pytest.raises(ValueError, match="a pair"):
        build_bank(model, {"states": good[None]})
    # a keyframe file whose keys do not fit the model
    root = ET.Element("mujoco")
    key = ET.SubElement(ET.SubElement(root, "keyframe"), "key")
    key.set("qpos", "0 0 1 1 0 0 0")
    key.set("qvel", "0 0 0 0 0 0")
    short = tmp_path / "short.xml"
    ET.ElementTree(root).write(short)
    with pytest.raises(ValueError, match="qpos rows must have length 28"):
        build_bank(model, {"trajectory": str(short)})
    with pytest.raises(ValueError, match="no <key> with qpos and qvel"):
        build_bank(model, {"trajectory": XML})                       # the model's own keyframes carry no qvel
    with pytest.raises(ValueError, match="noise_scale"):
        noise_scale_of({"noise_scale": -1.0})
    assert noise_scale_of({"noise_scale": 0.003}) == 0.003 and noise_scale_of({}, 0.01) == 0.01


# ------------------------------------------------------------------ the draw
def test_draw_index_range_and_k1():
    from mujocoposelearning_amd.initial_state import draw_index
    env = np.arange(64)[:, None]
    ep = np.arange(1, 65)[None, :]
    assert not draw_index(7, env, ep, 1).any()
    for K in (2, 3, 7, 4096):
        j = draw_index(7, env, ep, K)
        assert j.shape == (64, 64) and j.dtype == np.int64 and j.min() >= 0 and j.max() <= K - 1
    with pytest.raises(ValueError):
        draw_index(7, 0, 1, 0)


@pytest.mark.parametrize("K", [2, 3, 7])
def test_draw_index_hits_every_row(K):
    """Over 4096 (env, episode) pairs every row is drawn, about equally often (a uniform draw: each count within 5
    standard deviations of 4096 / K)."""
    from mujocoposelearning_amd.initial_state import draw_index
    j = draw_index(0, np.arange(64)[:, None], np.arange(1, 65)[None, :], K)
    counts = np.bincount(j.ravel(), minlength=K)
    assert (counts > 0).all()
    assert np.abs(counts - 4096 / K).max() < 5 * np.sqrt(4096 * (1 / K) * (1 - 1 / K))


def test_hash_depends_on_every_counter():
    from mujocoposelearning_amd.initial_state import INIT_SLOT, draw_index, hash_bits, uniform01, uniform_pm
    base = uniform01(3, 5, 9, INIT_SLOT)
    assert 0.0 <= base < 1.0
    for other in (uniform01(3, 5, 9, 2), uniform01(3, 6, 9, INIT_SLOT), uniform01(3, 5, 10, INIT_SLOT),
                  uniform01(4, 5, 9, INIT_SLOT)):
        assert other != base
    # the draw's slot is none of the noise slots: its value differs from every noise draw's of the same reset
    noise_slots = np.r_[np.arange(28), 64 + np.arange(27)]
    assert INIT_SLOT not in noise_slots
    assert (uniform01(3, 5, 9, noise_slots) != base).all()
    # the slot occupies the counter's low 8 bits, the episode the bits above them
    assert hash_bits(3, 0, 1, 0) == hash_bits(3, 0, 0, 256) and hash_bits(3, 0, 1, 0) != hash_bits(3, 0, 0, 128)
    # splitmix64's published first output for state 0, through the seed-free inner hash
    from mujocoposelearning_amd.initial_state import _splitmix
    assert int(_splitmix(np.uint64(0))) == 0xE220A8397B1DCDAF
    # uniform_pm: in range, zero-mean-ish, and its two roundings agree to an ulp of the scale
    slots = np.arange(55)
    a = uniform_pm(1, 2, 3, slots, 0.01)
    b = uniform_pm(1, 2, 3, slots, 0.01, fused=False)
    assert (np.abs(a) <= 0.01).all() and np.abs(a - b).max() <= 2e-18 and len(np.unique(a)) == 55
    np.testing.assert_array_equal(draw_index(3, 5, 9, 7), np.minimum(6, np.floor(base * 7).astype(np.int64)))


def test_uniform_pm_is_the_single_rounding_of_the_exact_value():
    """fused=True states fma(2 scale, u, -scale) exactly: compared with rational arithmetic."""
    from fractions import Fraction

    from mujocoposelearning_amd.initial_state import hash_bits, uniform_pm
    for scale in (0.01, float(np.float32(0.01))):
        for slot in (0, 2, 27, 64, 90):
            m = int(hash_bits(11, 4, 2, slot))
            exact = Fraction(scale) * (Fraction(2 * m, 1 << 53) - 1)
            assert float(uniform_pm(11, 4, 2, slot, scale)) == float(exact)


# ------------------------------------------------------------------ the ABI without a device, the config surface
def test_abi_null_arguments():
    import ctypes as C

    from mujocoposelearning_amd import _lib
    L = _lib.lib()
    assert {"hs_set_initial_states", "hs_get_initial_states"} <= set(_lib.EXPORTED)
    assert L.hs_set_initial_states(None, 1, None, None) < 0 and b"null batch" in L.hs_last_error()
    n = C.c_int(0)
    assert L.hs_get_initial_states(None, C.byref(n)) < 0 and b"null" in L.hs_last_error()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hsim.h")).read()
    assert f"#define HS_MAX_INITIAL_STATES {_lib.HS_MAX_INITIAL_STATES}" in hdr


def test_train_config_passes_initial_state_through():
    from mujocoposelearning_amd.train import env_config_from_kwargs
    spec = {"keyframe": "squat"}
    assert env_config_from_kwargs({"initial_state": spec})["initial_state"] is spec
    assert "initial_state" not in env_config_from_kwargs({})
