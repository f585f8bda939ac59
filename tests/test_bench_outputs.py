"""bench.py's plain run and ``--dump-outputs``: the writer (dtypes, the 64 MB budget and its fixed
seeded row sample) on the CPU, and one small plain run on the GPU -- the line keeps its headline
keys, runs none of the ``--full`` legs, and the dumped arrays are the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FULL_ONLY = ("cpu_baseline", "sim_stats", "sim_only_fp32", "sim_only_episode", "rollout", "train", "gae",
             "sim_only_tape", "dropin", "other_configs")


def test_dump_outputs_dtypes_and_names(tmp_path):
    import bench
    rng = np.random.default_rng(0)
    arrays = {"obs": rng.normal(size=(5, 7)), "reward": rng.normal(size=5).astype(np.float32),
              "terminated": np.array([0, 1, 0, 0, 1], dtype=np.uint8)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["obs.npy", "reward.npy", "terminated.npy"]
    obs = np.load(tmp_path / "d" / "obs.npy")
    assert obs.dtype == np.float64 and np.array_equal(obs, arrays["obs"])
    assert np.load(tmp_path / "d" / "reward.npy").dtype == np.float32
    term = np.load(tmp_path / "d" / "terminated.npy")
    assert term.dtype == np.float32 and np.array_equal(term, arrays["terminated"])


def test_dump_outputs_samples_rows_above_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    n = 100
    arrays = {"obs": np.arange(n * 10, dtype=np.float64).reshape(n, 10), "reward": np.arange(n, dtype=np.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(a) == ["env_index.npy", "obs.npy", "reward.npy"]
    assert sum(x.nbytes for x in a.values()) <= 4000
    idx = a["env_index.npy"].astype(int)
    assert 0 < idx.size < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["obs.npy"], arrays["obs"][idx]) and np.array_equal(a["reward.npy"], arrays["reward"][idx])
    for f, x in a.items():          # the same sample on every call
        assert np.array_equal(x, np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_prints_headline_only_and_dumps_last_step(tmp_path):
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--envs", "64", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 2 and out["unit"] == "env_steps/s" and out["dtype"] == "f64"
    assert out["higher_is_better"] is True and out["ms_per_step"] > 0
    assert abs(out["value"] - 64 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    for k in FULL_ONLY:
        assert out[k] is None, k
    got = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert sorted(got) == ["obs", "reward", "terminated", "truncated"]
    assert got["obs"].shape == (64, 352) and got["obs"].dtype == np.float64
    assert got["reward"].shape == (64,) and got["reward"].dtype == np.float64
    assert all(np.isfinite(x).all() for x in got.values())
    assert np.abs(got["obs"]).max() > 0
    for k in ("terminated", "truncated"):
        assert got[k].shape == (64,) and got[k].dtype == np.float32 and set(np.unique(got[k])) <= {0.0, 1.0}
