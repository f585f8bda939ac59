"""The fused rollout-time kernels at hidden widths 64 and 128 (the reference's config.py trains
[64, 64]): hs_mlp2_forward_h (ppo_mlp.hip mlp2_fwd_kernel<.., H>) against the packed GEMM chain, and
hs_rollout's in-kernel policy forward (hs_policy.h policy_mean_body<H / 64, ACT>) with the checks of
tests/test_gpu_rollout.py -- env replay bitwise, the per-step sampler on the chain's mean, episode
returns bitwise.  Every case asserts that it runs the fused path, not the fallback."""
import ctypes as C

import pytest
import torch

from test_gpu_rollout import _check_rollout, _copy_env, _env, _stagger

pytestmark = pytest.mark.gpu


def _kw(pi, vf=None):
    return dict(batch_size=1024, n_epochs=1, seed=0,
                policy_kwargs={"activation_fn": "ReLU", "net_arch": {"pi": list(pi), "vf": list(vf or pi)}})


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("N,D", [(33, 7), (1000, 350), (4096, 352), (9001, 350)])
def test_fused_mlp_forward_matches_gemm_chain_at_narrow_widths(N, D, H):
    """hs_mlp2_forward_h == the packed GEMM chain of ActorCritic.net_forward (torch fp32) for the pi
    mean and the vf value at the bar of test_fused_mlp_forward_matches_gemm_chain: no full k-group
    (7), a partial last group with element loads (350), the aligned case (352) and the
    two-row-block instance (9001 rows)."""
    from mujocoposelearning_amd import ppo as P
    torch.manual_seed(0)
    pol = P.ActorCritic(D, 21, [H, H], [H, H], torch.nn.ReLU).cuda()
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.05 * torch.randn_like(p))
    pol.pack_heads()
    obs = torch.randn(N, D, device="cuda") * 2
    assert pol._fused_mlp_ok(obs)
    outs = {}
    for fused in (True, False):
        P.FUSED_MLP = fused
        try:
            assert pol._fused_mlp_ok(obs) == fused
            outs[fused] = [pol.net_forward(obs, 0).clone(), pol.net_forward(obs, 1).clone()]
        finally:
            P.FUSED_MLP = True
    for a, b in zip(outs[True], outs[False]):
        assert a.shape == b.shape
        err = float((a - b).abs().max())
        print(f"H {H} N {N} D {D}: max |fused - chain| {err:.3e}, max |chain| {float(b.abs().max()):.3e}")
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4 * (1 + float(b.abs().max()))), err


def test_fused_mlp_abi_with_padded_strides_at_64():
    """hs_mlp2_forward_h (H = 64) through the C ABI on strided operands: input rows of 400 floats
    holding 352 features, weight rows padded (ld1 = 360, ld2 = ld3 = 72), an output of stride 32
    holding 21 columns (the padding untouched) -- against the fp32 torch chain on the same values."""
    from mujocoposelearning_amd import _lib
    torch.manual_seed(1)
    N, D, H, A = 1000, 352, 64, 21
    xs = torch.randn(N, 400, device="cuda")
    w1s, w2s, w3s = (torch.randn(H, 360, device="cuda") * 0.05, torch.randn(H, 72, device="cuda") * 0.05,
                     torch.randn(A, 72, device="cuda") * 0.05)
    b1, b2, b3 = (torch.randn(H, device="cuda") * 0.1, torch.randn(H, device="cuda") * 0.1,
                  torch.randn(A, device="cuda") * 0.1)
    out = torch.full((N, 32), 7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert _lib.lib().hs_mlp2_forward_h(xs.data_ptr(), 400, D, N, H, w1s.data_ptr(), 360, b1.data_ptr(),
                                        w2s.data_ptr(), 72, b2.data_ptr(), w3s.data_ptr(), 72, b3.data_ptr(), A,
                                        out.data_ptr(), 32, st) == 0
    x, w1, w2, w3 = xs[:, :D], w1s[:, :D], w2s[:, :H], w3s[:, :H]
    ref = torch.relu(torch.relu(x @ w1.t() + b1) @ w2.t() + b2) @ w3.t() + b3
    torch.cuda.synchronize()
    assert torch.allclose(out[:, :A], ref, rtol=1e-4, atol=1e-4 * (1 + float(ref.abs().max())))
    assert torch.all(out[:, A:] == 7.0)


def _pair_path_envs():
    """The smallest odd batch r + 257 (r = the resident waves, from a 2-env probe batch): more envs
    than resident waves, so the rollout queues env pairs, and the last pair has a ghost half."""
    probe = _env(2)
    r = probe.batch.resident_waves
    probe.close()
    assert r > 0
    return (r + 257) | 1


@pytest.mark.parametrize("case", ["h64_pairs", "h128_single", "h64_three_launches", "h64_full_state"])
def test_fused_rollout_at_narrow_widths(case):
    """Two consecutive fused rollouts per case, checked as test_fused_rollout_matches_env_replay_and_policy
    checks the [256, 256] net.  h64_pairs: the pair-per-wave queue with a ghost half; h128_single:
    the env-per-wave queue; h64_three_launches: 0.5 s episodes, hs_rollout_max_steps < T // 2, every
    env auto-resets; h64_full_state: the 448-wide obs with the kneeling reward."""
    from mujocoposelearning_amd import _lib
    from mujocoposelearning_amd.ppo import PPO
    H, n, T, full, duration = {"h64_pairs": (64, None, 12, False, 10.0),
                               "h128_single": (128, 777, 12, False, 10.0),
                               "h64_three_launches": (64, 512, 80, False, 0.5),
                               "h64_full_state": (64, 1024, 8, True, 10.0)}[case]
    if n is None:
        n = _pair_path_envs()
    env, replay = _env(n, full_state=full, duration=duration), _env(n, full_state=full, duration=duration)
    if case == "h64_pairs":
        assert n % 2 == 1 and n > env.batch.resident_waves
    if case == "h128_single":
        assert n <= env.batch.resident_waves
    ppo = PPO(env, n_steps=T, **_kw([H, H]))
    ppo.policy.pack_heads()
    args = ppo._fused_rollout_args()
    assert args is not None and args[1].hidden == H
    if duration < 1.0:
        assert _lib.check(_lib.lib().hs_rollout_max_steps(env.rollout_handle())) < T // 2
    _stagger(env, round(duration / 0.015))
    for it in range(2):            # the second rollout continues from the first (obs, ep_acc, starts, noise)
        _copy_env(env, replay)
        ep_acc0, start0, ctr0 = ppo.ep_acc.clone(), ppo.episode_start.clone(), int(ppo._noise_ctr.item())
        ppo.collect_rollouts()
        torch.cuda.synchronize()
        assert ppo._fused_rollout_args() is not None
        assert getattr(ppo, "fused_fallbacks", 0) == 0
        assert len(getattr(ppo, "rollout_launches", [])) > 0
        assert int(ppo.buf["done"].sum()) > 0                     # episodes ended inside the rollout
        _check_rollout(ppo, replay, ep_acc0, start0, ctr0)
    env.close()
    replay.close()


def test_hs_rollout_refuses_other_widths():
    """hs_rollout raises for a hidden width it has no instance for (96) and for ld1 < hidden; a PPO
    whose hidden layers differ in width ([64, 128]) keeps the per-step path and still collects."""
    from mujocoposelearning_amd import _lib
    from mujocoposelearning_amd._lib import HsimError
    from mujocoposelearning_amd.ppo import PPO
    env = _env(64)
    p = PPO(env, n_steps=4, **_kw([64, 64]))
    p.policy.pack_heads()
    h, pol, keep = p._fused_rollout_args()
    b = p.buf
    rb = _lib.hs_rollout_bufs(b["obs"].data_ptr(), p.obs.data_ptr(), b["act"].data_ptr(), b["logp"].data_ptr(),
                              b["start"].data_ptr(), b["rew"].data_ptr(), b["done"].data_ptr(), b["epret"].data_ptr(),
                              b["boot"].data_ptr(), b["tobs"].data_ptr(), p.ep_acc.data_ptr(),
                              p.episode_start.data_ptr(), p._act_clip.data_ptr(), p._noise_ctr.data_ptr(), 1, 0)
    ptrs = [t.data_ptr() for t in keep]
    for bad in (_lib.hs_policy(*ptrs, 128, 352, 21, 96),       # no instance for 96
                _lib.hs_policy(*ptrs, 32, 352, 21, 64)):       # ld1 < hidden
        with pytest.raises(HsimError, match="policy shape"):
            _lib.check(_lib.lib().hs_rollout(h, C.byref(bad), C.byref(rb), 0, 4, 4, None))
    env.close()
    env2 = _env(64)
    q = PPO(env2, n_steps=4, **_kw([64, 128]))
    q.policy.pack_heads()
    assert q._fused_rollout_args() is None
    assert not q.policy._fused_mlp_ok(q.obs)
    q.collect_rollouts()
    torch.cuda.synchronize()
    assert not getattr(q, "rollout_launches", [])
    assert torch.isfinite(q.buf["rew"]).all() and torch.isfinite(q.buf["act"]).all()
    env2.close()


def test_train_humanoid_with_the_reference_config_shape():
    """train_humanoid with the network of the reference's config.py ([64, 64] ReLU for pi and vf) runs
    its rollouts fused, and the update changes every parameter."""
    from mujocoposelearning_amd import ppo as P
    from mujocoposelearning_amd.train import train_humanoid
    ppo_kwargs = {"n_steps": 16, "batch_size": 256, "n_epochs": 2, "learning_rate": 3e-4,
                  "policy_kwargs": {"net_arch": {"pi": [64, 64], "vf": [64, 64]}, "activation_fn": "ReLU"}}
    env_kwargs = {"n_envs": 64, "total_timesteps": 2 * 16 * 64, "reward_function": "stand"}
    torch.manual_seed(0)             # PPO seeds its initial weights the same way (seed 0)
    init = dict(P.ActorCritic(352, 21, [64, 64], [64, 64], torch.nn.ReLU).named_parameters())
    model = train_humanoid(env_kwargs, ppo_kwargs, seed=0)
    assert model.num_timesteps == 2 * 16 * 64
    assert len(getattr(model, "rollout_launches", [])) > 0
    assert getattr(model, "fused_fallbacks", 0) == 0
    params = dict(model.policy.named_parameters())
    assert params.keys() == init.keys()
    for name, q in params.items():
        assert q.shape == init[name].shape
        assert torch.isfinite(q).all(), name
        assert not torch.equal(q.detach().cpu(), init[name].detach()), name
