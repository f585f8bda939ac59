"""VecNormalize on the CPU path: the wrapper's moments and normalised rewards against a numpy restatement of
SB3 2.3.2's ``RunningMeanStd`` (common/running_mean_std.py) and ``VecNormalize``
(common/vec_env/vec_normalize.py) fed the same batches one step at a time.  SB3 is not imported.

Bounds: the device semantics merge a rollout's batches in blocks where SB3 merges them one by one; Chan's
merge is exact in exact arithmetic, float64 sums of <= 2^17 fp32 values round at ~1.5e-11 and the two orders
were measured <= 3.1e-11 std apart in the mean, so 1e-9 std (mean) and 1e-9 relative (var) leave more than an
order.  A normalised reward is the float64 quotient rounded to fp32: it may differ from the restatement's by
one fp32 rounding (1.2e-7 relative) where the two float64 quotients straddle a rounding boundary.
"""
import ctypes as C
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from mujocoposelearning_amd import VecNormalize
from mujocoposelearning_amd.ppo import PPO

GAMMA = 0.97


class RefRunningMeanStd:
    """running_mean_std.py: float64, mean 0, var 1, count 1e-4; update -> update_from_moments."""

    def __init__(self, shape=()):
        self.mean, self.var, self.count = np.zeros(shape, np.float64), np.ones(shape, np.float64), 1e-4

    def update(self, arr):
        arr = np.asarray(arr, dtype=np.float64)
        self.update_from_moments(np.mean(arr, axis=0), np.var(arr, axis=0), arr.shape[0])

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        tot_count = self.count + batch_count
        new_mean = self.mean + delta * batch_count / tot_count
        m_a = self.var * self.count
        m_b = batch_var * batch_count
        m_2 = m_a + m_b + np.square(delta) * self.count * batch_count / (self.count + batch_count)
        self.mean, self.var, self.count = new_mean, m_2 / (self.count + batch_count), batch_count + self.count


class RefVecNormalize:
    """vec_normalize.py's reset / step_wait on given raw batches (training=True)."""

    def __init__(self, n, d, clip_obs=10.0, clip_reward=10.0, gamma=GAMMA, epsilon=1e-8):
        self.obs_rms, self.ret_rms = RefRunningMeanStd((d,)), RefRunningMeanStd(())
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.returns = np.zeros(n)

    def normalize_obs(self, obs):
        return np.clip((obs - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon), -self.clip_obs,
                       self.clip_obs).astype(np.float32)

    def reset(self, obs):
        self.returns = np.zeros_like(self.returns)
        self.obs_rms.update(obs)
        return self.normalize_obs(obs)

    def step(self, obs, rewards, dones):
        self.obs_rms.update(obs)
        obs = self.normalize_obs(obs)
        self.returns = self.returns * self.gamma + rewards
        self.ret_rms.update(self.returns)
        rewards = np.clip(rewards / np.sqrt(self.ret_rms.var + self.epsilon), -self.clip_reward, self.clip_reward)
        self.returns[dones] = 0
        return obs, rewards


class ToyEnv:
    """Device vec-env protocol stand-in on the CPU (the idea of tests/test_ppo.py's ToyEnv) with obs
    columns of very different offset (up to 1e3) and scale (down to 1e-2), episodes that end by termination
    (odd envs) or truncation (even envs) at per-env horizons, a record of every raw batch it returned, and
    a numpy VecEnv surface (reset / step_async / step_wait with SB3's info keys)."""

    def __init__(self, n=7, obs_dim=6, act_dim=3, seed=0):
        self.g = torch.Generator().manual_seed(seed)
        self.num_envs, self.obs_dim, self.act_dim, self.device = n, obs_dim, act_dim, torch.device("cpu")
        self.offset = torch.tensor([0.0, 1e3, -30.0, 5.0, 200.0, -1e3][:obs_dim]).float()
        self.scale = torch.tensor([1.0, 1e-2, 10.0, 0.1, 300.0, 1e-2][:obs_dim]).float()
        self.horizon = 3 + torch.arange(n) % 4
        self.t = torch.zeros(n, dtype=torch.long)
        self.terminal_obs = torch.zeros(n, obs_dim)
        self.record = []          # ("reset", obs) / ("step", obs, rew, term, trunc)

    def _draw(self):
        return self.offset + self.scale * torch.randn(self.num_envs, self.obs_dim, generator=self.g)

    def reset_tensors(self):
        self.t.zero_()
        self.obs = self._draw()
        self.record.append(("reset", self.obs.clone()))
        return self.obs

    def step_tensors(self, a):
        rew = 5.0 - 3.0 * (a ** 2).sum(-1) + self.obs[:, 0]
        self.t += 1
        end = self.t >= self.horizon
        odd = torch.arange(self.num_envs) % 2 == 1
        term, trunc = end & odd, end & ~odd
        nxt = self._draw()
        self.terminal_obs = nxt.clone()
        self.obs = torch.where(end[:, None], self._draw(), nxt)
        self.t[end] = 0
        self.record.append(("step", self.obs.clone(), rew.clone(), term.clone(), trunc.clone()))
        return self.obs, rew, term, trunc

    # numpy VecEnv surface
    def reset(self):
        return self.reset_tensors().double().numpy()

    def step_async(self, actions):
        self._a = torch.as_tensor(np.asarray(actions), dtype=torch.float32)

    def step_wait(self):
        obs, rew, term, trunc = self.step_tensors(self._a)
        done = (term | trunc).numpy()
        infos = [{"TimeLimit.truncated": bool(trunc[i])} for i in range(self.num_envs)]
        for i in np.flatnonzero(done):
            infos[i]["terminal_observation"] = self.terminal_obs[i].double().numpy()
        return obs.double().numpy(), rew.double().numpy(), done, infos


def _close(rms, ref):
    std = np.sqrt(ref.var)
    assert np.all(np.abs(rms.mean - ref.mean) <= 1e-9 * std), np.max(np.abs(rms.mean - ref.mean) / std)
    assert np.all(np.abs(rms.var - ref.var) <= 1e-9 * ref.var), np.max(np.abs(rms.var / ref.var - 1))
    assert abs(rms.count - ref.count) <= 1e-9 * ref.count


def _replay(ref, record):
    """Feed the recorded raw batches to the restatement; returns the normalised rewards [steps][N]."""
    out = []
    for rec in record:
        if rec[0] == "reset":
            ref.reset(rec[1].double().numpy())
        else:
            _, obs, rew, term, trunc = rec
            out.append(ref.step(obs.double().numpy(), rew.double().numpy(), (term | trunc).numpy())[1])
    return np.array(out)


def _f32_norm(x, mean, var, clip=10.0, eps=1e-8):
    m = torch.as_tensor(mean.astype(np.float32))
    s = torch.as_tensor((1.0 / np.sqrt(var + eps)).astype(np.float32))
    return ((x - m) * s).clamp(-clip, clip)


def test_exported_and_delegating():
    import mujocoposelearning_amd as pkg
    assert pkg.VecNormalize is VecNormalize
    raw = ToyEnv()
    env = VecNormalize(raw)
    assert (env.training, env.norm_obs, env.norm_reward, env.clip_obs, env.clip_reward, env.gamma, env.epsilon) == \
        (True, True, True, 10.0, 10.0, 0.99, 1e-8)
    assert env.num_envs == 7 and env.obs_dim == 6 and env.act_dim == 3 and env.device == raw.device
    assert env.obs_rms.count == 1e-4 and np.all(env.obs_rms.mean == 0) and np.all(env.obs_rms.var == 1)
    assert env.obs_rms.mean.dtype == np.float64 and env.ret_rms.var.dtype == np.float64
    with pytest.raises(ValueError, match="already wrapped"):
        VecNormalize(env)


def test_rollout_moments_and_rewards_equal_sb3_step_by_step():
    """Two rollouts of PPO(VecNormalize(env)): after each, obs_rms equals the restatement fed the reset obs
    and the rollout's T obs batches one at a time; ret_rms and every normalised reward equal it step by step,
    across episode ends and across the two rollouts (the return carry); the buffered obs are the fp32
    normalisation of the raw obs with the moments of the rollout's start."""
    raw = ToyEnv()
    env = VecNormalize(raw, gamma=GAMMA)
    T, N = 6, raw.num_envs
    model = PPO(env, n_steps=T, batch_size=14, n_epochs=1, gamma=GAMMA, policy_kwargs={"net_arch": [8, 8]})
    ref = RefVecNormalize(N, raw.obs_dim)
    assert env.obs_rms.count == 1e-4, "the moments must not move before the first rollout"
    for k in range(2):
        start_mean, start_var = env.obs_rms.mean.copy(), env.obs_rms.var.copy()
        first_obs = model.obs.clone()
        n0 = len(raw.record)
        model.collect_rollouts()
        recs = raw.record[(0 if k == 0 else n0):]
        want_rew = _replay(ref, recs)
        _close(env.obs_rms, ref.obs_rms)
        _close(env.ret_rms, ref.ret_rms)
        steps = [r for r in recs if r[0] == "step"]
        boot = torch.stack([r[4] & ~r[3] for r in steps])
        got = model.buf["rew"].numpy()
        assert boot.any() and (~boot).any()
        np.testing.assert_allclose(got[~boot.numpy()], want_rew[~boot.numpy()].astype(np.float32), rtol=1.2e-7, atol=0)
        # the TimeLimit bootstrap is added to the already normalised reward
        assert np.all(np.abs(got[boot.numpy()] - want_rew[boot.numpy()]) > 0)
        raw_obs = torch.stack([first_obs] + [r[1] for r in steps[:-1]])
        assert torch.equal(model.buf["obs"], _f32_norm(raw_obs, start_mean, start_var))
        assert torch.equal(model.obs, steps[-1][1]), "self.obs stays raw"
    assert env.obs_rms.count == pytest.approx(1e-4 + N * (1 + 2 * T))
    assert np.array_equal(env.returns, ref.returns)


def test_numpy_surface_follows_sb3_step_by_step():
    raw = ToyEnv(seed=3)
    env = VecNormalize(raw, gamma=GAMMA)
    ref = RefVecNormalize(raw.num_envs, raw.obs_dim)
    obs = env.reset()
    want = ref.reset(raw.record[-1][1].double().numpy())
    assert obs.dtype == np.float32 and np.array_equal(obs, want)
    rng = np.random.default_rng(0)
    seen_terminal = 0
    for _ in range(9):
        env.step_async(rng.uniform(-1, 1, (raw.num_envs, raw.act_dim)))
        obs, rew, dones, infos = env.step_wait()
        _, robs, rrew, term, trunc = raw.record[-1]
        tobs = raw.terminal_obs.double().numpy()
        wobs, wrew = ref.step(robs.double().numpy(), rrew.double().numpy(), (term | trunc).numpy())
        assert np.array_equal(obs, wobs) and np.array_equal(rew, wrew)
        assert np.array_equal(env.get_original_obs(), robs.double().numpy())
        assert np.array_equal(env.get_original_reward(), rrew.double().numpy())
        for i in np.flatnonzero(dones):
            assert np.array_equal(infos[i]["terminal_observation"], ref.normalize_obs(tobs[i]))
            seen_terminal += 1
        assert np.array_equal(env.returns, ref.returns)
        assert np.array_equal(env.obs_rms.mean, ref.obs_rms.mean) and np.array_equal(env.obs_rms.var, ref.obs_rms.var)
        assert env.ret_rms.var == ref.ret_rms.var and env.ret_rms.count == ref.ret_rms.count
    assert seen_terminal > 3
    assert np.array_equal(env.normalize_obs(tobs), ref.normalize_obs(tobs))
    assert np.array_equal(env.normalize_reward(rrew.numpy()),
                          np.clip(rrew.numpy() / np.sqrt(ref.ret_rms.var + 1e-8), -10, 10))


def test_training_false_freezes_the_moments():
    raw = ToyEnv()
    env = VecNormalize(raw, gamma=GAMMA)
    model = PPO(env, n_steps=4, batch_size=14, n_epochs=1, gamma=GAMMA, policy_kwargs={"net_arch": [8, 8]})
    model.collect_rollouts()
    env.training = False
    state = (env.obs_rms.mean.copy(), env.obs_rms.var.copy(), env.obs_rms.count, float(env.ret_rms.var),
             env.ret_rms.count)
    first_obs = model.obs.clone()
    model.collect_rollouts()
    model.predict(raw.obs.numpy())
    env.step_async(np.zeros((raw.num_envs, raw.act_dim)))
    env.step_wait()
    after = (env.obs_rms.mean, env.obs_rms.var, env.obs_rms.count, float(env.ret_rms.var), env.ret_rms.count)
    for a, b in zip(state, after):
        assert np.array_equal(a, b)
    # still normalising, with the frozen moments
    assert torch.equal(model.buf["obs"][0], _f32_norm(first_obs, state[0], state[1]))
    steps = [r for r in raw.record if r[0] == "step"][4:8]
    notboot = ~torch.stack([r[4] & ~r[3] for r in steps]).numpy()
    want = np.clip(torch.stack([r[2] for r in steps]).double().numpy() / np.sqrt(state[3] + 1e-8), -10, 10)
    np.testing.assert_allclose(model.buf["rew"].numpy()[notboot], want.astype(np.float32)[notboot], rtol=1.2e-7)


def test_predict_normalises_with_the_models_moments():
    raw = ToyEnv()
    env = VecNormalize(raw, gamma=GAMMA)
    model = PPO(env, n_steps=4, batch_size=14, n_epochs=1, gamma=GAMMA, policy_kwargs={"net_arch": [8, 8]})
    model.collect_rollouts()
    x = raw.obs.clone()
    a, _ = model.predict(x.numpy(), deterministic=True)
    mean, _ = model.policy(_f32_norm(x, env.obs_rms.mean, env.obs_rms.var))
    assert np.array_equal(a, mean.detach().clamp(-1, 1).numpy())
    assert np.array_equal(model.predict(x[0].numpy(), deterministic=True)[0], a[0])


def test_save_load_roundtrip_and_bare_env_raises(tmp_path):
    import zipfile
    kw = dict(n_steps=4, batch_size=14, n_epochs=1, gamma=GAMMA, policy_kwargs={"net_arch": [8, 8]})
    env = VecNormalize(ToyEnv(), gamma=GAMMA, clip_obs=7.0)
    a = PPO(env, **kw)
    a.learn(2 * 4 * 7)
    path = a.save(tmp_path / "m")
    names = zipfile.ZipFile(path).namelist()
    assert "vec_normalize.npz" in names and "policy.pth" in names and "data" in names
    env2 = VecNormalize(ToyEnv(seed=9))
    b = PPO(env2, seed=5, **kw).load(path)
    for k in ("mean", "var", "count"):
        assert np.array_equal(getattr(env2.obs_rms, k), getattr(env.obs_rms, k))
        assert np.array_equal(getattr(env2.ret_rms, k), getattr(env.ret_rms, k))
    assert np.array_equal(env2.returns, env.returns)
    assert env2.gamma == GAMMA and env2.clip_obs == 7.0 and env2.training is True
    x = env.venv.obs.numpy()
    assert np.array_equal(a.predict(x, deterministic=True)[0], b.predict(x, deterministic=True)[0])
    with pytest.raises(ValueError, match="saved with VecNormalize"):
        PPO(ToyEnv(), **kw).load(path)
    # a checkpoint without normalisation still loads onto a wrapped env (its moments stay)
    plain = PPO(ToyEnv(), **kw)
    p2 = plain.save(tmp_path / "plain")
    assert "vec_normalize.npz" not in zipfile.ZipFile(p2).namelist()
    PPO(VecNormalize(ToyEnv()), **kw).load(p2)


def test_load_running_stats_from_sb3_arrays():
    env = VecNormalize(ToyEnv())
    ref = RefVecNormalize(7, 6)
    rng = np.random.default_rng(1)
    ref.obs_rms.update(rng.normal(3.0, 2.0, (50, 6)))
    ref.ret_rms.update(rng.normal(0.0, 5.0, 50))
    env.load_running_stats({"obs_rms": {"mean": ref.obs_rms.mean, "var": ref.obs_rms.var, "count": ref.obs_rms.count},
                            "ret_rms": ref.ret_rms})
    assert np.array_equal(env.obs_rms.mean, ref.obs_rms.mean) and np.array_equal(env.obs_rms.var, ref.obs_rms.var)
    assert env.ret_rms.var == ref.ret_rms.var and env.ret_rms.count == ref.ret_rms.count
    x = rng.normal(3.0, 2.0, (4, 6))
    assert np.array_equal(env.normalize_obs(x), ref.normalize_obs(x))
    with pytest.raises(ValueError, match="do not fit"):
        env.load_running_stats({"obs_rms": {"mean": np.zeros(5), "var": np.ones(5), "count": 1.0}})


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_worker(rank, world, port, out_dir, shards):
    import torch.distributed as dist
    from mujocoposelearning_amd.train import init_distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world))
    init_distributed("gloo")
    try:
        raw = ToyEnv(n=shards[rank], seed=50 + rank)
        env = VecNormalize(raw, gamma=GAMMA)
        model = PPO(env, n_steps=5, batch_size=9, n_epochs=1, gamma=GAMMA, policy_kwargs={"net_arch": [8, 8]})
        for _ in range(2):
            model.collect_rollouts()
        torch.save({"obs": env.obs_rms.state.clone(), "ret": env.ret_rms.state.clone(), "record": raw.record,
                    "rew": model.buf["rew"].clone()}, os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_uneven_shards_share_the_moments(tmp_path):
    """Two ranks with 4 and 3 envs: both end with bitwise the same obs_rms / ret_rms, equal (1e-9) to the
    restatement fed the union of the two ranks' batches step by step -- what a world-1 run over the union
    of the envs computes."""
    shards = (4, 3)
    mp.start_processes(_rank_worker, args=(2, _free_port(), str(tmp_path), shards), nprocs=2, join=True,
                       start_method="spawn")
    r = [torch.load(tmp_path / f"r{i}.pt", weights_only=False) for i in range(2)]
    assert torch.equal(r[0]["obs"], r[1]["obs"]) and torch.equal(r[0]["ret"], r[1]["ret"])
    ref = RefVecNormalize(sum(shards), 6)
    union = []
    for a, b in zip(r[0]["record"], r[1]["record"]):
        assert a[0] == b[0]
        union.append((a[0],) + tuple(torch.cat([x, y]) for x, y in zip(a[1:], b[1:])))
    want_rew = _replay(ref, union)

    class View:
        def __init__(self, s, d):
            self.count, self.mean, self.var = float(s[0]), s[1:1 + d].numpy(), s[1 + d:].numpy()
    _close(View(r[0]["obs"], 6), ref.obs_rms)
    _close(View(r[0]["ret"], 1), ref.ret_rms)
    # the last rollout's rewards of rank 0 were scaled with the shared ret_rms
    steps = [x for x in union if x[0] == "step"][-5:]
    notboot = ~torch.stack([x[4] & ~x[3] for x in steps]).numpy()[:, :shards[0]]
    np.testing.assert_allclose(r[0]["rew"].numpy()[notboot], want_rew[-5:, :shards[0]].astype(np.float32)[notboot],
                               rtol=1.2e-7)


def test_obs_norm_args_layout_matches_the_c_compiler(tmp_path):
    from mujocoposelearning_amd import _lib
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    cls = _lib.hs_obs_norm_args
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hsim.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(hs_obs_norm_args));']
    for f, _ in cls._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(hs_obs_norm_args, {f}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if l)
    assert int(got["size"]) == C.sizeof(cls) == 24
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    # existing layouts are untouched
    assert C.sizeof(_lib.hs_policy) == 72


def test_norm_entry_points_validate_arguments():
    """hs_obs_norm & co. reject bad sizes and null buffers with a message before touching the device."""
    from mujocoposelearning_amd import _lib
    L = _lib.lib()

    def err(rc):
        assert rc < 0
        return L.hs_last_error().decode()
    assert "obs_dim <= 512" in err(L.hs_obs_norm(None, 600, 4, 600, None, None, 10.0, None, 600, None, None, None))
    assert "ldx >= obs_dim" in err(L.hs_obs_norm(None, 300, 4, 352, None, None, 10.0, None, 352, None, None, None))
    assert "clip > 0" in err(L.hs_obs_norm(None, 352, 4, 352, None, None, 0.0, None, 352, None, None, None))
    assert "null" in err(L.hs_obs_norm(None, 352, 4, 352, None, None, 10.0, None, 352, None, None, None))
    assert "workspace" in err(L.hs_obs_norm(16, 352, 4, 352, 16, 16, 10.0, 16, 352, 16, None, None))
    assert L.hs_obs_norm(None, 352, 0, 352, None, None, 10.0, None, 352, None, None, None) == 0
    assert L.hs_obs_norm_workspace(1000, 352) >= (352 * 4 + 2 * 352 * 8)
    assert "set_stride" in err(L.hs_rms_merge(16, 352, 16, 2, 700, 1e-8, None, None, None))
    assert "null" in err(L.hs_rms_merge(None, 352, None, 0, 0, 1e-8, None, None, None))
    assert "null" in err(L.hs_return_moments(None, None, 4, 4, 0.99, None, None, None, None))
    assert "negative" in err(L.hs_return_moments(None, None, -1, 4, 0.99, None, None, None, None))
    assert "set_stride" in err(L.hs_reward_scale(None, 4, 4, None, None, 1, 3, 1e-8, 10.0, None, None))
    assert "null" in err(L.hs_reward_scale(None, 4, 4, None, None, 1, 12, 1e-8, 10.0, None, None))
    assert "null argument" in err(L.hs_rollout_norm(None, None, 1, None, None, 0, 1, 1, None))
    assert "null argument" in err(L.hs_evaluate_norm(None, None, 1, None, None, 0, 1, 1, None))
    assert {"hs_rollout_norm", "hs_evaluate_norm", "hs_obs_norm", "hs_rms_merge", "hs_return_moments",
            "hs_reward_scale"} <= set(_lib.EXPORTED)
