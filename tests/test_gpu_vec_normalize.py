"""VecNormalize on the device: the hs_obs_norm / hs_rms_merge / hs_return_moments / hs_reward_scale kernels
against numpy float64, the fused rollout and evaluation with normalisation inside the kernel
(hs_rollout_norm, hs_evaluate_norm) against the env replayed step by step and the per-step path, and a
short training run.  The numpy restatement of SB3 2.3.2's RunningMeanStd / VecNormalize and its bounds are
tests/test_vec_normalize.py's (1e-9 std in the mean, 1e-9 relative in the variance; one fp32 rounding,
1.2e-7, for a normalised reward)."""
import math

import numpy as np
import pytest
import torch

from conftest import XML
from test_vec_normalize import RefRunningMeanStd, RefVecNormalize, _close

pytestmark = pytest.mark.gpu

GAMMA = 0.99
NETS = {"tanh64": ("Tanh", [64, 64]), "relu256": ("ReLU", [256, 256])}


def _env(n, seed=0, full_state=False, duration=10.0):
    from mujocoposelearning_amd.model import HsModel
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    cfg = {"model_path": XML, "duration": duration, "frame_skip": 3,
           "reward_config": {"type": "kneeling" if full_state else "stand"}}
    if full_state:
        cfg["full_state_obs"] = True
    return HumanoidVecEnv(cfg, n_envs=n, model=HsModel(XML), seed=seed, precision="fp64")


def _ppo(env, T, net, **kw):
    import warnings

    from mujocoposelearning_amd.ppo import PPO
    act, arch = NETS[net]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return PPO(env, n_steps=T, batch_size=kw.pop("batch_size", 1024), n_epochs=1, seed=0, gamma=GAMMA,
                   policy_kwargs={"activation_fn": act, "net_arch": {"pi": arch, "vf": arch}}, **kw)


def _copy_env(src, dst):
    for k, v in src.batch.t.items():
        dst.batch.t[k].copy_(v)


def _obs_norm(x, mean, inv_std, clip, out=None, moments=False):
    """hs_obs_norm through the C ABI on 2-D fp32 views (row strides taken from the tensors)."""
    from mujocoposelearning_amd import _lib
    L = _lib.lib()
    R, D = x.shape
    out = x if out is None else out
    mom = ws = None
    if moments:
        mom = torch.full((1 + 2 * D,), float("nan"), dtype=torch.float64, device="cuda")
        ws = torch.zeros(int(L.hs_obs_norm_workspace(R, D)) // 8, dtype=torch.float64, device="cuda")
    _lib.check(L.hs_obs_norm(x.data_ptr(), x.stride(0), R, D, mean.data_ptr(), inv_std.data_ptr(), clip,
                             out.data_ptr(), out.stride(0), mom.data_ptr() if moments else None,
                             ws.data_ptr() if moments else None, torch.cuda.current_stream().cuda_stream))
    return out, mom


@pytest.mark.parametrize("D", [352, 448])
@pytest.mark.parametrize("R", [1, 63, 1000, 4161])
def test_obs_norm_against_numpy_two_pass(R, D):
    """Columns cycle through offsets up to 1e3 and standard deviations down to 1e-2 (offset 1e3 with std
    1e-2 among them, where a plain float64 sum of squares is off by 1e-4 in the variance).  Packed rows in
    place, rows padded to a multiple of 4 out of place (16-byte accesses), rows padded by 1 (scalar path)."""
    g = torch.Generator().manual_seed(R * 1000 + D)
    off = torch.tensor([0.0, 1e3, -30.0, 5.0, 200.0, -1e3, 1e3])[torch.arange(D) % 7]
    std = torch.tensor([1.0, 1e-2, 10.0, 0.1, 300.0])[torch.arange(D) % 5]
    x = (off + std * torch.randn(R, D, generator=g)).float()
    x64 = x.double().numpy()
    rmean = x64.mean(0)
    rvar = np.square(x64 - rmean).sum(0) / R
    mean = (off + 0.3 * std).float().cuda()
    inv = (1.0 / (1.1 * std)).float().cuda()
    clip = 2.5
    xd = x.cuda()
    want = ((xd - mean) * inv).clamp(-clip, clip)
    assert float((want.abs() == clip).float().mean()) > 0.001 or R == 1      # the clip is exercised
    for ld, inplace in ((D, True), (D + 4, False), (D + 1, False), (D + 4, True)):
        src = torch.zeros(R, ld, device="cuda")
        src[:, :D] = xd
        dst = src if inplace else torch.full((R, ld), 7.0, device="cuda")
        runs = []
        for _ in range(2):
            src[:, :D] = xd
            _, mom = _obs_norm(src[:, :D], mean, inv, clip, out=dst[:, :D], moments=True)
            runs.append(mom.clone())
            assert torch.equal(dst[:, :D], want), (ld, inplace)
            if ld > D and not inplace:
                assert bool((dst[:, D:] == 7.0).all()), "padding columns are not written"
        assert torch.equal(runs[0], runs[1]), "two runs must be bitwise equal"
        m = runs[0].cpu().numpy()
        assert m[0] == R
        sd = np.sqrt(rvar)
        assert np.all(np.abs(m[1:1 + D] - rmean) <= 1e-9 * sd), np.max(np.abs(m[1:1 + D] - rmean) / np.maximum(sd, 1e-300))
        assert np.all(np.abs(m[1 + D:] / R - rvar) <= 1e-9 * rvar), (ld, inplace)
        # without moments: the same rows
        src[:, :D] = xd
        _obs_norm(src[:, :D], mean, inv, clip, out=dst[:, :D])
        assert torch.equal(dst[:, :D], want)


def test_rms_merge_follows_update_from_moments():
    from mujocoposelearning_amd import _lib
    D = 352
    rng = np.random.default_rng(0)
    ref = RefRunningMeanStd((D,))
    state = torch.zeros(1 + 2 * D, dtype=torch.float64, device="cuda")
    state[0], state[1 + D:] = 1e-4, 1.0
    m32, s32 = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    batches = [rng.normal(1e3, 1e-2, (n, D)) for n in (130, 1, 777)]
    sets = np.zeros((4, 1 + 2 * D))
    for k, b in zip((0, 2, 3), batches):        # set 1 stays empty (count 0): skipped
        sets[k] = np.concatenate([[len(b)], b.mean(0), b.var(0) * len(b)])
        ref.update(b)
    sd = torch.as_tensor(sets, device="cuda")
    _lib.check(_lib.lib().hs_rms_merge(state.data_ptr(), D, sd.data_ptr(), 4, 1 + 2 * D, 1e-8, m32.data_ptr(),
                                       s32.data_ptr(), torch.cuda.current_stream().cuda_stream))
    h = state.cpu().numpy()
    assert h[0] == ref.count
    np.testing.assert_allclose(h[1:1 + D], ref.mean, rtol=1e-15, atol=0)
    np.testing.assert_allclose(h[1 + D:], ref.var, rtol=1e-12, atol=0)
    assert np.array_equal(m32.cpu().numpy(), h[1:1 + D].astype(np.float32))
    assert np.array_equal(s32.cpu().numpy(), (1.0 / np.sqrt(h[1 + D:] + 1e-8)).astype(np.float32))


@pytest.mark.parametrize("N", [1, 130])
def test_return_moments_and_reward_scale_against_numpy(N):
    from mujocoposelearning_amd import _lib
    L = _lib.lib()
    T = 5
    rng = np.random.default_rng(N)
    rew = rng.normal(4.0, 3.0, (T, N)).astype(np.float32)
    done = rng.random((T, N)) < 0.2
    done[0, 0] = done[T - 1, N - 1] = done[T - 1, 0] = True
    carry0 = rng.normal(20.0, 5.0, N)
    ref = RefVecNormalize(N, 1, gamma=GAMMA)
    ref.ret_rms.update(rng.normal(10.0, 4.0, 50))         # a running state from earlier rollouts
    ref.returns = carry0.copy()
    state = torch.tensor([ref.ret_rms.count, float(ref.ret_rms.mean), float(ref.ret_rms.var)], dtype=torch.float64,
                         device="cuda")
    want = np.array([ref.step(np.zeros((N, 1)), rew[t].astype(np.float64), done[t])[1] for t in range(T)])
    r, d = torch.as_tensor(rew).cuda(), torch.as_tensor(done).cuda().view(torch.uint8)
    carry = torch.as_tensor(carry0).cuda()
    ws, sets, scale = (torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((T, N), (T, 3), (T,)))
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.hs_return_moments(r.data_ptr(), d.data_ptr(), T, N, GAMMA, carry.data_ptr(), ws.data_ptr(),
                                   sets.data_ptr(), st))
    _lib.check(L.hs_reward_scale(r.data_ptr(), T, N, state.data_ptr(), sets.data_ptr(), 1, 3 * T, 1e-8, 10.0,
                                 scale.data_ptr(), st))
    np.testing.assert_allclose(carry.cpu().numpy(), ref.returns, rtol=1e-14, atol=1e-14)
    assert bool((carry[torch.as_tensor(done[T - 1]).cuda()] == 0).all())

    class View:
        count, mean, var = (float(v) for v in state.cpu())
    _close(View, ref.ret_rms)
    np.testing.assert_allclose(r.cpu().numpy(), want.astype(np.float32), rtol=1.2e-7, atol=0)


def _replay_ref(ref, reset_obs, obs_batches, raw_rew, done):
    if reset_obs is not None:
        ref.reset(reset_obs)
    return np.array([ref.step(o, r, d)[1] for o, r, d in zip(obs_batches, raw_rew, done)])


@pytest.mark.parametrize("n,T,net,full,duration", [(130, 6, "tanh64", False, 10.0), (777, 6, "relu256", False, 10.0),
                                                   (130, 40, "tanh64", False, 0.5), (130, 6, "tanh64", True, 10.0)])
def test_fused_rollout_with_normalisation(n, T, net, full, duration, monkeypatch):
    """Two consecutive fused rollouts of PPO(VecNormalize(env)) (the second on updated moments).  The
    duration 0.5 case: 33-step episodes, so the 40-step rollout is two launches, every env auto-resets and
    episodes end by termination.  The first case puts four envs a few steps before the 750-step TimeLimit, so
    their terminal obs are normalised for the deferred bootstrap r += gamma V(terminal obs)."""
    from mujocoposelearning_amd import VecNormalize, _lib
    from mujocoposelearning_amd import ppo as ppo_mod
    from mujocoposelearning_amd.ppo_ops import ppo_act
    env, replay, env2 = (_env(n, full_state=full, duration=duration) for _ in range(3))
    vn, vn2 = VecNormalize(env, gamma=GAMMA), VecNormalize(env2, gamma=GAMMA)
    ppo, ppo2 = _ppo(vn, T, net), _ppo(vn2, T, net)
    ppo2.graphs = False
    D = env.obs_dim
    assert D == (448 if full else 352)
    ppo.policy.pack_heads()
    assert ppo._fused_rollout_args() is not None
    if duration < 1.0:
        assert _lib.check(_lib.lib().hs_rollout_max_steps(env.rollout_handle())) < T
    ref = RefVecNormalize(n, D, gamma=GAMMA)
    raw = {}
    real_norm = ppo._normalize_rollout

    def keep_raw():
        raw["obs"], raw["rew"] = ppo.buf["obs"].clone(), ppo.buf["rew"].clone()
        real_norm()
    monkeypatch.setattr(ppo, "_normalize_rollout", keep_raw)
    assert vn.obs_rms.count == 1e-4
    truncating = n == 130 and T == 6 and not full
    if truncating:
        env.batch.t["step_count"][5:9] = 746
    for it in range(2):
        _copy_env(env, replay)
        _copy_env(env, env2)
        mean0, inv0 = vn._mean32.clone(), vn._inv32.clone()
        state0 = vn.obs_rms.state.clone()
        first_obs = ppo.obs.clone()
        start0, ctr0 = ppo.episode_start.clone(), int(ppo._noise_ctr.item())
        ppo.collect_rollouts()
        torch.cuda.synchronize()
        assert getattr(ppo, "fused_fallbacks", 0) == 0
        b = ppo.buf
        # (a) the env stepped with the rollout's clipped actions reproduces the RAW obs, rewards, dones bitwise
        for t in range(T):
            obs, rew, term, trunc = replay.step_tensors(b["act"][t].clamp(-1, 1))
            nxt = raw["obs"][t + 1] if t + 1 < T else ppo.obs
            assert torch.equal(obs.float(), nxt), t
            assert torch.equal(rew.float(), raw["rew"][t]), t
            assert torch.equal((term != 0) | (trunc != 0), b["done"][t]), t
        assert torch.equal(raw["obs"][0], first_obs)
        if duration < 1.0:
            assert int(b["done"].sum()) >= n
        # (b) the buffer is hs_obs_norm of the raw rows with the moments of the rollout's start
        want, _ = _obs_norm(raw["obs"].view(T * n, D).clone(), mean0, inv0, 10.0)
        assert torch.equal(b["obs"].view(T * n, D), want)
        assert torch.equal(want, ((raw["obs"].view(T * n, D) - mean0) * inv0).clamp(-10.0, 10.0))
        assert not torch.equal(b["obs"], raw["obs"])
        # (c) the GEMM chain on the normalised rows + hs_ppo_act reproduce actions and log-probs
        ls = ppo.policy.log_std.detach()
        base = torch.tensor([ctr0], dtype=torch.int64, device="cuda")
        zero = torch.zeros(n, device="cuda")
        for t in range(T):
            with torch.no_grad():
                mean = ppo.policy.net_forward(b["obs"][t], 0)
            out = [torch.empty(n, 21, device="cuda"), torch.empty(n, 21, device="cuda")] + \
                  [torch.empty(n, device="cuda") for _ in range(3)]
            st_in = start0 if t == 0 else b["done"][t - 1].float()
            ppo_act(mean, zero, ls, st_in, ppo._noise_seed, t, False, *out, counter_base=base)
            assert torch.allclose(b["act"][t], out[0], rtol=1e-5, atol=2e-5), (t, float((b["act"][t] - out[0]).abs().max()))
            assert torch.allclose(b["logp"][t], out[2], rtol=1e-5, atol=2e-4), t
        # (d) the per-step path from the same start, given the same actions: bitwise the same buffers, moments
        fused_act = b["act"].clone()
        real_act = ppo_mod.ppo_act

        def forced(mean, value, log_std, start, seed, t, det, act, act_clip, *rest, **kw):
            real_act(mean, value, log_std, start, seed, t, det, act, act_clip, *rest, **kw)
            act.copy_(fused_act[t])
            act_clip.copy_(fused_act[t].clamp(-1, 1))
        with monkeypatch.context() as mp:
            mp.setattr(ppo_mod, "FUSED_ROLLOUT", False)
            mp.setattr(ppo_mod, "ppo_act", forced)
            ppo2.collect_rollouts()
        torch.cuda.synchronize()
        assert getattr(ppo2, "rollout_launches", None) is None
        for k in ("obs", "rew", "done", "val", "epret"):
            assert torch.equal(ppo2.buf[k], b[k]), k
        assert torch.equal(vn2.obs_rms.state, vn.obs_rms.state) and torch.equal(vn2.ret_rms.state, vn.ret_rms.state)
        assert torch.equal(vn2._mean32, vn._mean32) and torch.equal(vn2._inv32, vn._inv32)
        assert torch.equal(ppo2.obs, ppo.obs)
        # (e) the moments after the rollout equal the restatement fed the same batches one at a time
        batches = [raw["obs"][t].double().cpu().numpy() for t in range(1, T)] + [ppo.obs.double().cpu().numpy()]
        want_rew = _replay_ref(ref, first_obs.double().cpu().numpy() if it == 0 else None, batches,
                               raw["rew"].double().cpu().numpy(), b["done"].cpu().numpy())
        _close(vn.obs_rms, ref.obs_rms)
        _close(vn.ret_rms, ref.ret_rms)
        assert not torch.equal(vn.obs_rms.state, state0)
        notboot = ~b["boot"].cpu().numpy()
        np.testing.assert_allclose(b["rew"].cpu().numpy()[notboot], want_rew.astype(np.float32)[notboot], rtol=1.2e-7)
        if truncating and it == 0:      # the bootstrap is added to the normalised reward, from normalised terminal obs
            boot = b["boot"]
            assert int(boot.sum()) == 4
            x, _ = _obs_norm(b["tobs"][boot].clone(), mean0, inv0, 10.0)
            with torch.no_grad():
                want_b = torch.as_tensor(want_rew.astype(np.float32)).cuda()[boot] + GAMMA * ppo.policy.value(x)
            assert torch.allclose(b["rew"][boot], want_b, rtol=1e-6, atol=1e-6)
        # ep_returns stay raw
        acc_raw = raw["rew"].double().sum(0)
        if duration >= 1.0 and it == 0:
            alive = ~b["done"].any(0)
            assert torch.allclose(ppo.ep_acc[alive], acc_raw[alive], rtol=1e-12, atol=0)
    for e in (env, replay, env2):
        e.close()


def test_fused_rollout_overflow_falls_back_with_normalisation(monkeypatch):
    """tests/test_gpu_rollout.py's overflow case (lying bodies overflow the resident contact tier, the
    library undoes the launch, the rollout runs step by step) with the wrapper on."""
    from oracle.oracle import Oracle
    from test_gpu_contacts import lying_states
    from mujocoposelearning_amd import VecNormalize
    n, T = 4096, 6
    q = np.stack(lying_states(Oracle(XML), 16, seed=11))
    idx = np.arange(16) * 255 + 7
    env, replay = _env(n), _env(n)
    vn = VecNormalize(env, gamma=GAMMA)
    ppo = _ppo(vn, T, "relu256")
    st = env.batch.get_state()
    st["qpos"][idx] = q
    st["qvel"][idx] = 0.0
    st["qacc_warmstart"][idx] = 0.0
    env.batch.set_state(**st)
    _copy_env(env, replay)
    raw = {}
    real_norm = ppo._normalize_rollout

    def keep_raw():
        raw["obs"], raw["rew"] = ppo.buf["obs"].clone(), ppo.buf["rew"].clone()
        real_norm()
    monkeypatch.setattr(ppo, "_normalize_rollout", keep_raw)
    mean0, inv0 = vn._mean32.clone(), vn._inv32.clone()
    ppo.collect_rollouts()
    torch.cuda.synchronize()
    assert getattr(ppo, "fused_fallbacks", 0) == 1 and env.batch.tape_aborts() == 1
    b = ppo.buf
    for t in range(T):
        obs, rew, term, trunc = replay.step_tensors(b["act"][t].clamp(-1, 1))
        assert torch.equal(obs.float(), raw["obs"][t + 1] if t + 1 < T else ppo.obs), t
        assert torch.equal(rew.float(), raw["rew"][t]), t
    assert torch.equal(b["obs"], ((raw["obs"] - mean0) * inv0).clamp(-10.0, 10.0))
    assert vn.obs_rms.count == pytest.approx(1e-4 + n * (T + 1))
    env.close()
    replay.close()


def test_hs_rollout_norm_validates_the_moments():
    from mujocoposelearning_amd import VecNormalize, _lib
    import ctypes as C
    env = _env(8)
    vn = VecNormalize(env)
    ppo = _ppo(vn, 2, "tanh64", batch_size=16)
    ppo.policy.pack_heads()
    handle, cpol, keep = ppo._fused_rollout_args()
    b = ppo.buf
    rb = _lib.hs_rollout_bufs(b["obs"].data_ptr(), ppo.obs.data_ptr(), b["act"].data_ptr(), b["logp"].data_ptr(),
                              b["start"].data_ptr(), b["rew"].data_ptr(), b["done"].data_ptr(), b["epret"].data_ptr(),
                              b["boot"].data_ptr(), b["tobs"].data_ptr(), ppo.ep_acc.data_ptr(),
                              ppo.episode_start.data_ptr(), ppo._act_clip.data_ptr(), ppo._noise_ctr.data_ptr(), 1, 0)
    L = _lib.lib()

    def err(norm):
        rc = L.hs_rollout_norm(handle, C.byref(cpol), 1, C.byref(rb), norm, 0, 1, 2, None)
        assert rc < 0
        return L.hs_last_error().decode()
    good = vn.norm_args()
    assert "null hs_obs_norm_args" in err(None)
    assert "null mean" in err(C.byref(_lib.hs_obs_norm_args(0, good.inv_std, 10.0, 352)))
    assert "obs_dim 448 is not the batch's obs_dim 352" in err(C.byref(_lib.hs_obs_norm_args(good.mean, good.inv_std, 10.0, 448)))
    assert "clip > 0" in err(C.byref(_lib.hs_obs_norm_args(good.mean, good.inv_std, 0.0, 352)))
    env.close()


def _trained_moments(vn, model):
    """Moments as after some training: the obs the reset returned, spread a little."""
    obs = model.obs.double().cpu().numpy()
    vn.obs_rms.update(obs)
    vn.obs_rms.update(obs * 1.5 + 0.2)
    vn._obs_changed()


@pytest.mark.parametrize("net,n", [("tanh64", 64), ("relu256", 1101)])
def test_fused_evaluation_with_normalisation_matches_replay(net, n):
    """tests/test_gpu_evaluate.py's replay check with a model trained over VecNormalize: every traced action
    is the policy's on the twin's obs normalised by hs_obs_norm with the model's moments (the fp32 summation
    order tolerances of the rollout), the twin stepped with the traced actions reproduces rewards, dones and
    episode returns bitwise; the returns are raw, differ from the same policy's on raw obs, and the
    moments do not move."""
    from mujocoposelearning_amd import VecNormalize
    from mujocoposelearning_amd.evaluation import evaluate_policy_device
    E, duration = 2, 0.1
    env, twin = _env(n, duration=duration), _env(n, duration=duration)
    vn = VecNormalize(env, gamma=GAMMA)
    model = _ppo(vn, 2, net, batch_size=64)
    _trained_moments(vn, model)
    with torch.no_grad():
        model.policy.action_net.weight.mul_(30.0)       # actions that depend visibly on the obs
    state0, ret0 = vn.obs_rms.state.clone(), vn.ret_rms.state.clone()
    env.reset_tensors()
    _copy_env(env, twin)
    res = evaluate_policy_device(model, vn, E, deterministic=True, n_trace=n, reset=False)
    torch.cuda.synchronize()
    assert res.fused_launches == math.ceil(E * 7 / 6) and res.fallbacks == 0
    tr = res.trace
    cols = torch.arange(n, device="cuda")
    ep = torch.zeros(n, dtype=torch.int64, device="cuda")
    for t in range(tr["actions"].shape[0]):
        x, _ = _obs_norm(twin.batch.obs.float().contiguous(), vn._mean32, vn._inv32, 10.0)
        with torch.no_grad():
            want = model.policy.net_forward(x, 0).clamp(-1, 1)
        a = tr["actions"][t]
        assert torch.allclose(a, want, rtol=1e-5, atol=2e-5), (t, float((a - want).abs().max()))
        _, rew, term, trunc = twin.step_tensors(a.contiguous())
        done = (term != 0) | (trunc != 0)
        assert torch.equal(rew, tr["rewards"][t]) and torch.equal(done, tr["dones"][t]), t
        sel = done & (ep < E)
        assert torch.equal(res.returns[ep.clamp(max=E - 1), cols][sel], twin.batch.terminal_total_reward[sel]), t
        ep += done.long()
    assert bool((res.end_step >= 0).all())
    assert torch.equal(vn.obs_rms.state, state0) and torch.equal(vn.ret_rms.state, ret0)
    # the same policy on raw obs plays other episodes
    model.vec_normalize = None
    plain = evaluate_policy_device(model, env, E, deterministic=True)
    assert plain.fused_launches > 0
    assert not torch.equal(plain.returns, res.returns)
    env.close()
    twin.close()


def test_evaluate_policy_fused_equals_step_by_step_on_a_normalised_model(monkeypatch):
    """As tests/test_gpu_evaluate.py compares the two paths: the action head's weights are zero, so the
    action is clip(b3) whatever the summation order and the closed loop has no fp32 fork; the fused
    (hs_evaluate_norm) and the step-by-step (hs_obs_norm + net_forward) evaluations agree bitwise."""
    from mujocoposelearning_amd import VecNormalize
    from mujocoposelearning_amd import ppo as ppo_mod
    from mujocoposelearning_amd.evaluation import evaluate_policy, evaluate_policy_device
    env, twin = _env(1101, duration=0.5), _env(1101, duration=0.5)
    vn = VecNormalize(env, gamma=GAMMA)
    model = _ppo(vn, 2, "tanh64", batch_size=64)
    _trained_moments(vn, model)
    twin.reset_tensors()
    with torch.no_grad():
        model.policy.action_net.weight.zero_()
        model.policy.action_net.bias.uniform_(-1.0, 1.0)
    state0 = vn.obs_rms.state.clone()
    res = evaluate_policy_device(model, vn, 1)
    assert res.fused_launches == 2 and res.fallbacks == 0
    monkeypatch.setattr(ppo_mod, "FUSED_ROLLOUT", False)
    ref = evaluate_policy_device(model, twin, 1)
    assert ref.fused_launches == 0
    torch.cuda.synchronize()
    assert torch.equal(res.returns, ref.returns) and torch.equal(res.lengths, ref.lengths)
    assert bool((res.lengths == 33).all())
    mean, std = evaluate_policy(model, twin, n_eval_episodes=1101)
    assert math.isfinite(mean) and torch.equal(vn.obs_rms.state, state0)
    env.close()
    twin.close()


def test_short_training_run_and_checkpoint(tmp_path):
    """PPO(VecNormalize(env)), 256 envs, n_steps 8, two iterations: finite losses, the graphed update, moving
    moments; save / load into a fresh model reproduces predict bitwise."""
    from mujocoposelearning_amd import VecNormalize
    env, env2 = _env(256), _env(256, seed=3)
    vn = VecNormalize(env, gamma=GAMMA)
    model = _ppo(vn, 8, "tanh64", batch_size=512)
    states = []
    model.learn(2 * 8 * 256, callback=lambda m: states.append(vn.obs_rms.state.clone()) or True)
    assert model.logger["iteration"] == 2 and model._graphs is not None and model.graphs
    assert len(getattr(model, "rollout_launches", [])) == 2, "the rollouts ran fused"
    for k in ("policy_loss", "value_loss", "loss", "approx_kl"):
        assert math.isfinite(model.logger[k]), k
    assert not torch.equal(states[0], states[1])
    assert vn.obs_rms.count == pytest.approx(1e-4 + 256 * 17) and vn.ret_rms.count == pytest.approx(1e-4 + 256 * 16)
    assert bool((model.buf["obs"].abs() <= 10.0).all()) and bool((model.buf["rew"].abs() <= 10.0 + GAMMA * 1e3).all())
    path = model.save(tmp_path / "m")
    vn2 = VecNormalize(env2)
    fresh = _ppo(vn2, 8, "tanh64", batch_size=512).load(path)
    assert torch.equal(vn2.obs_rms.state, vn.obs_rms.state) and torch.equal(vn2.ret_rms.state, vn.ret_rms.state)
    assert torch.equal(vn2._mean32, vn._mean32) and torch.equal(vn2._inv32, vn._inv32)
    x = model.obs.cpu().numpy()
    for det in (True, False):
        torch.manual_seed(1)
        a = model.predict(x, deterministic=det)[0]
        torch.manual_seed(1)
        assert np.array_equal(a, fresh.predict(x, deterministic=det)[0])
    with pytest.raises(ValueError, match="saved with VecNormalize"):
        _ppo(env2, 8, "tanh64", batch_size=512).load(path)
    env.close()
    env2.close()
