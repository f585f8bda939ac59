"""Policy evaluation (mujocoposelearning_amd/evaluation.py) without a GPU: SB3's evaluate_policy
semantics (common/evaluation.py, 2.3.2) and EvalCallback's bookkeeping on a toy env with known rewards and
episode lengths, the RNG isolation of a stochastic evaluation, and the hs_evaluate binding."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mujocoposelearning_amd.evaluation import EvalCallback, evaluate_policy, evaluate_policy_device
from mujocoposelearning_amd.ppo import PPO


class CountEnv:
    """PPO env protocol on the CPU.  Env i's episodes last 3 + i % 3 steps and every step of its episode
    number k pays (i + 1) + k / 4, whatever the action: returns and lengths are known in closed form."""

    def __init__(self, n):
        self.num_envs, self.obs_dim, self.act_dim, self.device = n, 4, 2, torch.device("cpu")
        self.horizon = torch.tensor([3 + i % 3 for i in range(n)])
        self.terminal_obs = torch.zeros(n, 4)
        self.reset_tensors()

    def episode_length(self):
        return int(self.horizon.max())

    def reset_tensors(self):
        self.t = torch.zeros(self.num_envs, dtype=torch.long)
        self.k = torch.zeros(self.num_envs, dtype=torch.long)
        return self._obs()

    def _obs(self):
        return torch.stack([self.t, self.k, self.t * 0 + 1, self.t - self.k], dim=1).float()

    def step_tensors(self, a):
        assert a.shape == (self.num_envs, self.act_dim) and float(a.abs().max()) <= 1.0
        rew = torch.arange(1, self.num_envs + 1).double() + self.k.double() / 4
        self.t += 1
        trunc = self.t >= self.horizon
        self.terminal_obs = self._obs()
        self.t[trunc] = 0
        self.k[trunc] += 1
        return self._obs(), rew, torch.zeros_like(trunc), trunc


def _sb3_evaluate(n_envs, n_eval_episodes):
    """SB3's evaluate_policy loop restated on CountEnv's closed form: step every env, append an env's
    finished episode while its count is below its target, until all targets are met."""
    targets = np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)])
    counts = np.zeros(n_envs, int)
    t, k = np.zeros(n_envs, int), np.zeros(n_envs, int)
    cur_r, cur_l = np.zeros(n_envs), np.zeros(n_envs, int)
    rewards, lengths = [], []
    while (counts < targets).any():
        for i in range(n_envs):
            cur_r[i] += (i + 1) + k[i] / 4
            cur_l[i] += 1
            t[i] += 1
            if t[i] >= 3 + i % 3:
                if counts[i] < targets[i]:
                    rewards.append(cur_r[i])
                    lengths.append(int(cur_l[i]))
                    counts[i] += 1
                cur_r[i], cur_l[i], t[i] = 0.0, 0, 0
                k[i] += 1
    return rewards, lengths


def _model(env, **kw):
    return PPO(env, n_steps=4, batch_size=4, n_epochs=1, seed=0, **kw)


@pytest.mark.parametrize("n_eval", [3, 5, 12, 1])          # below, equal to, not divisible by n_envs = 5; one
def test_evaluate_policy_allotment_order_and_statistics(n_eval):
    env = CountEnv(5)
    model = _model(env)
    want_r, want_l = _sb3_evaluate(5, n_eval)
    assert len(want_r) == n_eval
    rewards, lengths = evaluate_policy(model, env, n_eval_episodes=n_eval, return_episode_rewards=True)
    assert rewards == want_r and lengths == want_l
    mean, std = evaluate_policy(model, env, n_eval_episodes=n_eval)
    assert mean == float(np.mean(want_r)) and std == float(np.std(want_r))


def test_evaluate_policy_device_slots_on_the_step_by_step_path():
    env = CountEnv(4)
    res = evaluate_policy_device(_model(env), env, 2, deterministic=False)
    assert res.fused_launches == 0 and res.fallbacks == 0 and res.trace is None
    for i in range(4):
        h = 3 + i % 3
        assert res.lengths[:, i].tolist() == [h, h]
        assert res.end_step[:, i].tolist() == [h - 1, 2 * h - 1]
        assert res.returns[:, i].tolist() == [h * (i + 1), h * (i + 1 + 0.25)]
    with pytest.raises(ValueError):
        evaluate_policy_device(_model(env), env, 1, n_trace=1)        # a trace needs an HsBatch env


def test_stochastic_evaluation_leaves_the_global_rng_and_the_trainer_alone():
    env, eval_env = CountEnv(4), CountEnv(3)
    model = _model(env)
    before = torch.get_rng_state()
    ctr, steps = model._noise_ctr.clone(), model.num_timesteps
    a = evaluate_policy(model, eval_env, n_eval_episodes=4, deterministic=False, return_episode_rewards=True)
    assert torch.equal(torch.get_rng_state(), before)
    assert torch.equal(model._noise_ctr, ctr) and model.num_timesteps == steps and model.env is env
    assert evaluate_policy(model, eval_env, n_eval_episodes=4, deterministic=False, return_episode_rewards=True) == a


def test_eval_callback_bookkeeping(tmp_path):
    env, eval_env = CountEnv(4), CountEnv(5)
    model = _model(env)
    saves = []
    model.save = lambda path: saves.append(path)
    cb = EvalCallback(eval_env, eval_freq=100, n_eval_episodes=5, best_model_save_path=str(tmp_path / "best"))
    want_r, want_l = _sb3_evaluate(5, 5)
    for steps, n_evals in [(50, 0), (100, 1), (150, 1), (199, 1), (200, 2), (450, 3)]:
        model.num_timesteps = steps
        assert cb(model) is True
        assert len(cb.evaluations) == n_evals
    assert [e[0] for e in cb.evaluations] == [100, 200, 450]
    assert all(e[1] == float(np.mean(want_r)) and e[2] == float(np.std(want_r)) for e in cb.evaluations)
    assert model.logger["eval/mean_reward"] == float(np.mean(want_r))
    assert model.logger["eval/mean_ep_length"] == float(np.mean(want_l))
    assert cb.best_mean_reward == float(np.mean(want_r))
    # the mean never improved after the first evaluation: one save, by rank 0
    assert saves == [os.path.join(str(tmp_path / "best"), "best_model")]
    model.rank = 1
    cb2 = EvalCallback(eval_env, eval_freq=1, n_eval_episodes=5, best_model_save_path=str(tmp_path / "r1"))
    cb2(model)
    assert len(saves) == 1 and len(cb2.evaluations) == 1


def test_eval_callback_runs_inside_learn():
    env, eval_env = CountEnv(4), CountEnv(2)
    model = _model(env)
    cb = EvalCallback(eval_env, eval_freq=16, n_eval_episodes=2)
    model.learn(48, callback=cb)
    assert [e[0] for e in cb.evaluations] == [16, 32, 48] and "eval/mean_reward" in model.logger


def test_hs_evaluate_is_bound_and_exported():
    import mujocoposelearning_amd as pkg
    from mujocoposelearning_amd import _lib
    assert "hs_evaluate" in _lib.EXPORTED
    fn = _lib.lib().hs_evaluate
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    names = [f[0] for f in _lib.hs_eval_bufs._fields_]
    assert names == ["actions_clipped", "episode0", "max_episodes", "n_trace", "ep_return", "ep_length", "ep_end_step",
                     "trace_qpos", "trace_qvel", "trace_actions", "trace_rewards", "trace_dones", "counter_base",
                     "seed", "deterministic"]
    assert C.sizeof(_lib.hs_eval_bufs) == 2 * 8 + 2 * 4 + 9 * 8 + 8 + 8      # as the C struct (tail padded)
    for name in ("evaluate_policy", "evaluate_policy_device", "EvalCallback", "render_policy"):
        assert callable(getattr(pkg, name))
