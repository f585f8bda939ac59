"""Fused policy evaluation (hs_evaluate, evaluation.evaluate_policy_device): whole episodes in launches
of the fp64 chunk-queue kernel's evaluation instance (hs_env_step.h step_pair, EVAL: eval_rows, next_action; hs_policy.h) -- env step, pi net on
the env's wave from the env's one staging row, clipped action to the pair's next step -- with per-episode
results and an optional trace instead of the RolloutBuffer.

Checked against the pieces the step-by-step path is built from, as tests/test_gpu_rollout.py does:
* the env: a twin batch stepped with the traced actions, one hs_step at a time, reproduces every traced
  reward and done flag BITWISE, the traced state of every non-done step, and at every done the result
  slot (return, length, end step) is the twin's terminal info, bitwise;
* the policy: every traced action is clamp(net_forward(obs)) on the twin's obs (or hs_ppo_act's sample of
  it with the evaluation's seed and counter) to fp32 rounding of the mean (rtol 1e-5, atol 2e-5: the
  in-kernel forward sums in another order -- _check_rollout's bound for the same comparison).  A stale
  staging row would show here: the action would be that of an earlier step's obs.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import XML

pytestmark = pytest.mark.gpu

NETS = {"tanh64": ("Tanh", [64, 64]), "relu256": ("ReLU", [256, 256])}


def _env(n, duration, seed=0, precision="fp64"):
    from mujocoposelearning_amd.model import HsModel
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    cfg = {"model_path": XML, "duration": duration, "frame_skip": 3, "reward_config": {"type": "stand"}}
    return HumanoidVecEnv(cfg, n_envs=n, model=HsModel(XML), seed=seed, precision=precision)


def _model(env, net="tanh64", seed=0):
    import warnings

    from mujocoposelearning_amd.ppo import PPO
    act, arch = NETS[net]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # (short rollouts: not what is tested here)
        return PPO(env, n_steps=2, batch_size=64, n_epochs=1, seed=seed,
                   policy_kwargs={"activation_fn": act, "net_arch": {"pi": arch, "vf": arch}})


def _copy_env(src, dst):
    for k, v in src.batch.t.items():
        dst.batch.t[k].copy_(v)


def _check_replay(model, res, twin, E, deterministic):
    """The twin holds the state (and obs) the evaluation started from; the trace covers every env."""
    from mujocoposelearning_amd.ppo_ops import ppo_act
    tr = res.trace
    T, N = tr["actions"].shape[:2]
    assert N == twin.num_envs
    cols = torch.arange(N, device="cuda")
    ep = torch.zeros(N, dtype=torch.int64, device="cuda")
    ls = model.policy.log_std.detach()
    zero, ctr = torch.zeros(N, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    finished = 0
    for t in range(T):
        with torch.no_grad():
            mean = model.policy.net_forward(twin.batch.obs.float(), 0)
        if deterministic:
            want = mean.clamp(-1, 1)
        else:
            out = [torch.empty(N, 21, device="cuda"), torch.empty(N, 21, device="cuda")] + \
                  [torch.empty(N, device="cuda") for _ in range(3)]
            ppo_act(mean, zero, ls, zero, res.noise_seed, t, False, *out, counter_base=ctr)
            want = out[1]
        a = tr["actions"][t]
        assert torch.allclose(a, want, rtol=1e-5, atol=2e-5), (t, float((a - want).abs().max()))
        _, rew, term, trunc = twin.step_tensors(a.contiguous())
        done = (term != 0) | (trunc != 0)
        assert torch.equal(rew, tr["rewards"][t]), t
        assert torch.equal(done, tr["dones"][t]), t
        assert torch.equal(twin.batch.qpos[~done], tr["qpos"][t][~done]), t
        assert torch.equal(twin.batch.qvel[~done], tr["qvel"][t][~done]), t
        sel = done & (ep < E)
        e = ep.clamp(max=E - 1)
        assert torch.equal(res.returns[e, cols][sel], twin.batch.terminal_total_reward[sel]), t
        assert torch.equal(res.lengths[e, cols][sel], twin.batch.terminal_step_count[sel]), t
        assert bool((res.end_step[e, cols][sel] == t).all()), t
        finished += int(sel.sum())
        ep += done.long()
    # every filled slot was met at its done (and nothing else is filled)
    assert finished == int((res.end_step >= 0).sum())
    return finished


@pytest.mark.parametrize("net", ["tanh64", "relu256"])
@pytest.mark.parametrize("duration,E", [(0.1, 3), (0.5, 2)])
@pytest.mark.parametrize("n", [64, 1101])
def test_fused_evaluation_matches_env_replay_and_policy(n, duration, E, net):
    """n = 64 is queued as single envs; 1101 has more pairs than resident waves, an odd count and a ghost
    half.  duration 0.1: 7-step episodes in launches of at most 6 steps (E = 3: four launches, every
    episode end inside a launch and across launch boundaries); 0.5: 33-step episodes, launches of 32."""
    from mujocoposelearning_amd import _lib
    from mujocoposelearning_amd.evaluation import evaluate_policy_device
    env, twin = _env(n, duration), _env(n, duration)
    model = _model(env, net)
    env.reset_tensors()
    _copy_env(env, twin)
    L = _lib.check(_lib.lib().hs_rollout_max_steps(env.rollout_handle()))
    length = env.episode_length()
    assert (length, L) == ((7, 6) if duration == 0.1 else (33, 32))
    res = evaluate_policy_device(model, env, E, deterministic=True, n_trace=n, reset=False)
    torch.cuda.synchronize()
    assert res.fused_launches == math.ceil(E * length / L) and res.fallbacks == 0
    assert _check_replay(model, res, twin, E, True) == E * n
    assert bool((res.lengths == length).all())
    # the launch's last step committed the batch state: the env is where the twin is
    for k in ("qpos", "qvel", "time", "step_count", "episode", "total_reward"):
        assert torch.equal(env.batch.t[k], twin.batch.t[k]), k
    env.close()
    twin.close()


def test_fused_stochastic_evaluation_draws_the_evaluations_own_noise():
    from mujocoposelearning_amd.evaluation import evaluate_policy_device
    env, twin = _env(64, 0.1), _env(64, 0.1)
    model = _model(env, "tanh64")
    ctr = model._noise_ctr.clone()
    env.reset_tensors()
    _copy_env(env, twin)
    res = evaluate_policy_device(model, env, 3, deterministic=False, n_trace=64, reset=False, seed=5)
    torch.cuda.synchronize()
    assert res.fused_launches == 4 and res.fallbacks == 0
    assert _check_replay(model, res, twin, 3, False) == 3 * 64
    assert torch.equal(model._noise_ctr, ctr)
    env.close()
    twin.close()


def test_whole_episode_at_the_workload_shape_equals_the_step_by_step_path(monkeypatch):
    """4096 envs, 10 s episodes, no trace.  The action head's weights are zero and its bias random, so the
    action is clip(b3) whatever the summation order: the closed loop has no fp32 fork and the two paths
    must agree bitwise."""
    from mujocoposelearning_amd import ppo as ppo_mod
    from mujocoposelearning_amd.evaluation import evaluate_policy_device
    env, twin = _env(4096, 10.0), _env(4096, 10.0)
    model = _model(env, "relu256")
    twin.reset_tensors()      # PPO's constructor reset env once: the twin's episode counters (reset noise) follow
    with torch.no_grad():
        model.policy.action_net.weight.zero_()
        model.policy.action_net.bias.uniform_(-1.0, 1.0)
    res = evaluate_policy_device(model, env, 1)
    assert res.fused_launches > 0 and res.fallbacks == 0 and res.trace is None
    monkeypatch.setattr(ppo_mod, "FUSED_ROLLOUT", False)
    ref = evaluate_policy_device(model, twin, 1)
    assert ref.fused_launches == 0 and ref.fallbacks == 0
    torch.cuda.synchronize()
    assert torch.equal(res.returns, ref.returns)
    assert torch.equal(res.lengths, ref.lengths) and torch.equal(res.end_step, ref.end_step)
    assert bool((res.lengths == 667).all())
    env.close()
    twin.close()


def test_overflow_undoes_the_launch_and_the_rest_runs_step_by_step():
    from oracle.oracle import Oracle
    from test_gpu_contacts import lying_states
    from mujocoposelearning_amd.evaluation import evaluate_policy_device
    n = 4096
    q = np.stack(lying_states(Oracle(XML), 16, seed=11))
    idx = np.arange(16) * 255 + 7
    env, twin = _env(n, 0.1), _env(n, 0.1)
    model = _model(env, "relu256")
    env.reset_tensors()
    st = env.batch.get_state()
    st["qpos"][idx] = q
    st["qvel"][idx] = 0.0
    st["qacc_warmstart"][idx] = 0.0
    env.batch.set_state(**st)
    _copy_env(env, twin)
    res = evaluate_policy_device(model, env, 1, deterministic=True, n_trace=n, reset=False)   # a 6-step launch first
    torch.cuda.synchronize()
    assert res.fallbacks == 1 and env.batch.tape_aborts() == 1 and res.fused_launches == 0
    assert env.batch.wide_reruns() >= len(idx)
    assert _check_replay(model, res, twin, 1, True) == n
    env.close()
    twin.close()


def test_hs_evaluate_refuses_what_it_cannot_run():
    from mujocoposelearning_amd import _lib
    from mujocoposelearning_amd._lib import HsimError
    from mujocoposelearning_amd.evaluation import _fused_args
    n = 64
    env32, env = _env(n, 10.0, precision="fp32"), _env(n, 10.0)
    model = _model(env, "relu256")
    assert _fused_args(model, env32) is None
    h, pol, keep = _fused_args(model, env)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")      # noqa: E731
    bufs = dict(act=z(n, 21), ep0=z(n, dt=torch.int32), ret=z(2, n, dt=torch.float64), ln=z(2, n, dt=torch.int32),
                end=z(2, n, dt=torch.int32), ctr=z(1, dt=torch.int64))

    def eb(**kw):
        e = _lib.hs_eval_bufs()
        e.actions_clipped, e.episode0, e.max_episodes = bufs["act"].data_ptr(), bufs["ep0"].data_ptr(), 2
        e.ep_return, e.ep_length, e.ep_end_step = bufs["ret"].data_ptr(), bufs["ln"].data_ptr(), bufs["end"].data_ptr()
        e.counter_base, e.deterministic = bufs["ctr"].data_ptr(), 1
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    def call(handle, e, n_steps=4, t_total=8):
        return _lib.check(_lib.lib().hs_evaluate(handle, C.byref(pol), 0, C.byref(e), 0, n_steps, t_total, None))

    cap = _lib.check(_lib.lib().hs_rollout_max_steps(h))
    with pytest.raises(HsimError, match="fp64"):
        call(env32.batch._groups[0][0], eb())
    with pytest.raises(HsimError, match="must be given"):
        call(h, eb(ep_return=None))
    with pytest.raises(HsimError, match="n_steps"):
        call(h, eb(), n_steps=cap + 1, t_total=cap + 1)
    with pytest.raises(HsimError, match="max_episodes"):
        call(h, eb(max_episodes=0))
    with pytest.raises(HsimError, match="n_trace"):
        call(h, eb(n_trace=n + 1))
    with pytest.raises(HsimError, match="trace arrays"):
        call(h, eb(n_trace=1))
    assert call(h, eb()) == 0                                   # and the same buffers, asked properly, run
    del keep
    env.close()
    env32.close()


def test_eval_callback_leaves_training_bitwise_untouched():
    from mujocoposelearning_amd.evaluation import EvalCallback

    def run(with_eval):
        import warnings

        from mujocoposelearning_amd.ppo import PPO
        env = _env(64, 10.0, seed=3)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ppo = PPO(env, n_steps=8, batch_size=128, n_epochs=2, seed=1,
                      policy_kwargs={"activation_fn": "Tanh", "net_arch": {"pi": [64, 64], "vf": [64, 64]}})
        cb = None
        if with_eval:
            eval_env = _env(8, 0.1, seed=9)
            inner = EvalCallback(eval_env, eval_freq=1, n_eval_episodes=8)

            def cb(m):
                inner.deterministic = len(inner.evaluations) == 0       # once deterministic, once stochastic
                return inner(m)
        ppo.learn(2 * 8 * 64, callback=cb)
        torch.cuda.synchronize()
        if with_eval:
            assert len(inner.evaluations) == 2 and "eval/mean_reward" in ppo.logger
            eval_env.close()
        out = ([p.detach().clone() for p in ppo.policy.parameters()], ppo._noise_ctr.clone())
        env.close()
        return out

    (pa, ca), (pb, cb_) = run(False), run(True)
    assert torch.equal(ca, cb_)
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))


def test_render_policy_writes_the_traced_episode(tmp_path, monkeypatch):
    from PIL import Image

    from mujocoposelearning_amd import render
    from mujocoposelearning_amd.evaluation import render_policy
    env = _env(4, 0.1)
    model = _model(env, "tanh64")
    ckpt = model.save(str(tmp_path / "ckpt"))
    env.close()
    seen = []
    real = render.write_video
    monkeypatch.setattr(render, "write_video", lambda p, frames, fps: (seen.append(frames), real(p, frames, fps))[1])
    out = render_policy(ckpt if isinstance(ckpt, str) else str(tmp_path / "ckpt"), str(tmp_path / "demo.gif"),
                        height=48, width=64, framerate=30, env_config={"duration": 0.1})
    # a frame after step t while len(frames) < time x framerate, time = 0.005 (1 + 3 (t + 1)), 7 steps
    want = 0
    for t in range(7):
        if want < 0.005 * (1 + 3 * (t + 1)) * 30:
            want += 1
    assert want == 4 and len(seen) == 1 and len(seen[0]) == want
    assert seen[0][0].shape == (48, 64, 3)
    with Image.open(out) as im:       # (the GIF writer merges frames that do not differ: no frame count here)
        assert 1 <= im.n_frames <= want and im.size == (64, 48)
    # num_steps cuts the episode short
    out2 = render_policy(str(tmp_path / "ckpt"), str(tmp_path / "demo2.gif"), num_steps=2, height=48, width=64,
                         framerate=30, env_config={"duration": 0.1})
    assert len(seen[1]) == 2 and out2 is not None
