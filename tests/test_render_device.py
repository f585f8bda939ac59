"""CPU side of the device render path: the tile layout of VecEnv.render, the packing of the MJCF
cameras and the free camera into the device renderer's (mode, body, pos, rot, fovy), and the video
callback's bookkeeping.  The poses come from the fp64 oracle (the stand-in of tests/test_render.py);
tests/test_gpu_render_device.py compares the device frames themselves with the host renderer's."""
import numpy as np
import pytest

from conftest import XML
from test_render import _OracleBatch


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


@pytest.mark.parametrize("n,rows,cols", [(1, 1, 1), (2, 2, 1), (5, 3, 2), (9, 3, 3)])
def test_tile_images_layout(n, rows, cols):
    """SB3 tile_images: rows = ceil(sqrt(n)), cols = ceil(n / rows), row-major, black padding."""
    from mujocoposelearning_amd.render import tile_images
    h, w = 3, 4
    imgs = [np.full((h, w, 3), k + 1, np.uint8) for k in range(n)]
    imgs[0][0, 1] = (7, 8, 9)                     # orientation inside a tile is kept
    out = tile_images(imgs)
    assert out.shape == (rows * h, cols * w, 3) and out.dtype == np.uint8
    for k in range(rows * cols):
        r, c = divmod(k, cols)
        tile = out[r * h:(r + 1) * h, c * w:(c + 1) * w]
        if k < n:
            np.testing.assert_array_equal(tile, imgs[k])
        else:
            assert not tile.any()


def _camera_from_pack(pack, pose):
    """What the kernel computes from a packed camera and a pose (include/hsim.h hs_camera)."""
    from mujocoposelearning_amd.render import CAM_BODY, CAM_COM
    mode, body, pos, rot, fovy = pack
    pos, rot = np.asarray(pos, float), np.asarray(rot, float).reshape(3, 3)
    if mode == CAM_BODY:
        bR = pose["xmat"][body].reshape(3, 3)
        return pose["xpos"][body] + bR @ pos, bR @ rot, fovy
    assert mode == CAM_COM
    return pose["com"] + pos, rot, fovy


def test_camera_packing_matches_camera_pose(model):
    from mujocoposelearning_amd.render import CAM_BODY, CAM_COM, DeviceRenderer, Renderer, parse_cameras
    b = _OracleBatch()
    rng = np.random.default_rng(5)
    for _ in range(3):
        b.o.step(rng.uniform(-1, 1, 21), 7)       # a stepped state: the body frames are not the identity
    pose = b.kinematics()
    host = Renderer(model, height=8, width=8)
    dev = DeviceRenderer(model, b, height=8, width=8)
    cams = parse_cameras(XML)
    assert [c.name for c in cams] == ["back", "side", "egocentric"]
    modes = {}
    for camera in ["back", "side", "egocentric", 0, 1, 2, None, -1]:
        pack = dev.camera_pack(camera, b)
        modes[camera] = pack[0]
        cpos, R, fovy = host._camera_pose(host._resolve(camera), b, 0, pose)
        got = _camera_from_pack(pack, pose)
        np.testing.assert_allclose(got[0], cpos, rtol=0, atol=1e-15)
        np.testing.assert_allclose(got[1], R, rtol=0, atol=1e-15)
        assert got[2] == fovy
    # MuJoCo's modes: trackcom cameras and the free camera ride the COM, a fixed camera its body
    for c in cams:
        assert modes[c.name] == modes[c.id] == (CAM_COM if c.mode == "trackcom" else CAM_BODY)
    assert modes["side"] == CAM_COM and modes["egocentric"] == CAM_BODY and modes[None] == CAM_COM
    ego = dev.camera_pack("egocentric", b)
    assert ego[1] == cams[2].body and ego[4] == 80.0
    np.testing.assert_array_equal(ego[2], cams[2].pos)
    np.testing.assert_array_equal(ego[3], cams[2].rot)
    free = dev.camera_pack(None, b)
    assert free[4] == 45.0 and np.linalg.norm(free[2]) == pytest.approx(3.0)
    np.testing.assert_allclose(free[2], 3.0 * np.asarray(free[3])[:, 2], atol=1e-15)   # it looks along -z at the COM
    with pytest.raises(ValueError):
        dev.camera_pack("nope", b)


class _StubModel:
    def __init__(self, rank=0):
        self.ep_returns, self.rank = [], rank


def _recorder(tmp_path, interval, monkeypatch, **kw):
    from mujocoposelearning_amd import evaluation
    calls = []

    def fake(model, env, out_path, **k):
        calls.append((out_path, k))
        return out_path
    monkeypatch.setattr(evaluation, "record_episode", fake)
    cb = evaluation.VideoRecorderCallback(interval, {"framerate": 30}, run_name="r", out_dir=str(tmp_path), **kw)
    monkeypatch.setattr(cb, "_eval_env", lambda: None)        # no GPU here: record_episode is stubbed
    return cb, calls


def test_video_recorder_crossing_logic(tmp_path, monkeypatch):
    cb, calls = _recorder(tmp_path, 10, monkeypatch, height=48, width=64)
    m = _StubModel()
    grow = lambda k: m.ep_returns.extend([0.0] * k)   # noqa: E731
    assert cb(m) is True and calls == []              # nothing finished
    grow(9)
    assert cb(m) is True and calls == []              # 9: no multiple of 10 crossed
    grow(1)
    assert cb(m) is True                              # 10: exactly on the multiple
    assert [c[0] for c in calls] == [str(tmp_path / "r" / "episode_10.gif")]
    assert calls[0][1]["deterministic"] is False and calls[0][1]["framerate"] == 30
    assert (calls[0][1]["height"], calls[0][1]["width"], calls[0][1]["renderer"]) == (48, 64, "device")
    grow(5)
    assert cb(m) is True and len(calls) == 1          # 15: none crossed since 10
    grow(30)
    assert cb(m) is True                              # 45: 20, 30 and 40 crossed -> one video, the largest
    assert [c[0] for c in calls][1:] == [str(tmp_path / "r" / "episode_40.gif")]
    grow(4)
    assert cb(m) is True and len(calls) == 2          # 49
    grow(1)
    assert cb(m) is True and len(calls) == 3          # 50
    assert cb.videos == [c[0] for c in calls]
    assert (tmp_path / "r").is_dir()


def test_video_recorder_other_ranks_write_nothing(tmp_path, monkeypatch):
    cb, calls = _recorder(tmp_path, 2, monkeypatch)
    m = _StubModel(rank=1)
    m.ep_returns.extend([0.0] * 7)
    assert cb(m) is True and calls == [] and cb.videos == []
    assert not (tmp_path / "r").exists()
    with pytest.raises(ValueError):
        from mujocoposelearning_amd.evaluation import VideoRecorderCallback
        VideoRecorderCallback(0, {})


def test_callback_list():
    from mujocoposelearning_amd.evaluation import CallbackList
    seen = []

    def make(tag, ret):
        def cb(model):
            seen.append((tag, model))
            return ret
        return cb
    assert CallbackList([make("a", True), make("b", None)])("m") is True
    assert seen == [("a", "m"), ("b", "m")]
    del seen[:]
    # a False stops training, and the callbacks after it still run
    assert CallbackList([make("a", True), make("b", False), make("c", True)])("m") is False
    assert [t for t, _ in seen] == ["a", "b", "c"]
    assert CallbackList([])("m") is True


def test_new_names_are_exported_lazily():
    import mujocoposelearning_amd as pkg
    from mujocoposelearning_amd import _lib
    for name in ("VideoRecorderCallback", "CallbackList", "record_episode", "DeviceRenderer", "tile_images"):
        assert getattr(pkg, name).__name__ == name
    assert {"hs_kinematics_batch", "hs_render_frames"} <= set(_lib.EXPORTED)
    L = _lib.lib()
    # refusals that need no device: nothing is launched without a batch
    assert L.hs_kinematics_batch(None, 1, None, None, None, None) < 0 and b"null" in L.hs_last_error()
    assert L.hs_render_frames(None, 1, None, None, 8, 8, None, None) < 0 and b"null" in L.hs_last_error()
