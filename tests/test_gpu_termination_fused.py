"""Fused launches under the built-in termination conditions (hs_set_termination_builtin; the TERM instances of
step_kernel_queue, csrc/hs_env_step.h env_outcome, csrc/hs_term_builtin.h).

The yardstick is always the existing per-step path -- ``step`` / ``step_tensors`` (step, outcome launch with the
interpreter, masked reset) on a twin with the same seed and the same condition set WITHOUT ``fused`` -- and every
comparison is ``torch.equal``.  n = 64 is queued as single envs; n = 1027 as env pairs, an odd count with a ghost
half.  Auto-resets draw the on-device noise (the fused launches ask for it), the first reset explicit noise.

The tape cases run two fused launches back to back: K steps (the case's K), then TAIL more.  TAIL is fixed so
that, in every case's reference, some env ends on the second launch's last step and some env ends earlier in that
launch without ending on its last step (both asserted): the terminal rows are compared under the mask "done on the
launch's last step", which is their contract after a fused launch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import XML

pytestmark = pytest.mark.gpu

FS = 3
STATE = ("qpos", "qvel", "time", "step_count", "episode", "total_reward", "obs")
TAPE_CASES = {
    # name: (condition, params, grace_steps, duration, K)
    "fallen_g1": ("fallen", {"min_height": 0.8}, 1, 10.0, 90),
    "fallen_g3": ("fallen", {"min_height": 0.8}, 3, 10.0, 90),
    "lost_balance": ("lost_balance", None, 1, 10.0, 90),
    "several_episodes": ("fallen", {"min_height": 1.28}, 1, 10.0, 40),
    # 13-step episodes by the clock: the zero-action envs are still above 1.275 m then, the others mostly not
    "clock_and_early": ("fallen", {"min_height": 1.275}, 1, 0.2, 40),
}
# the second launch's length (module docstring), read off the reference's done flags: in every case and shape
# step K + 12 ends at least 2 episodes, and at least 10 envs end one in steps K + 1 .. K + 11 only
TAIL = 12


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


def _inputs(n, steps):
    """Explicit first-reset noise and the action tape: the first half of the envs zero actions (they fall below
    0.8 m at env steps 70-75), the second half U(-1, 1) (27-40)."""
    rng = np.random.default_rng(42)
    noise = [rng.uniform(-0.01, 0.01, s) for s in ((n, 28), (n, 27))]
    act = np.zeros((steps, n, 21), np.float32)
    act[:, n // 2:] = rng.uniform(-1, 1, (steps, n - n // 2, 21))
    return noise, act


def _batch(model, n, noise, fused, condition, params, grace, duration):
    from mujocoposelearning_amd.batch import HsBatch
    b = HsBatch(model, n, precision="fp64", seed=5)
    b.configure(frame_skip=FS, duration=duration, reward_id=0, autoreset=1)
    b.set_termination(condition, params, grace, fused=fused)
    assert b.termination_fused == fused
    b.reset(qpos_noise=noise[0], qvel_noise=noise[1])
    return b


def _per_step(ref, act):
    """`ref` stepped once per tape row: the four outputs and the early bytes of every step, stacked."""
    rows = [[], [], [], [], []]
    for a in act:
        out = ref.step(a)
        for dst, src in zip(rows, tuple(out) + (ref.early_terminated,)):
            dst.append(src.clone())
    return [torch.stack(r) for r in rows]


def _one_launch(fus, act):
    """step_tape as ONE fused launch, by the library's own evidence: a queued launch advances the queue's epoch
    by one (its last wave out), the per-step path of these batch sizes never queues, nothing was replayed."""
    e0 = fus.queue_counters()["epoch"]
    out = fus.step_tape(act)
    assert fus.queue_counters()["epoch"] == e0 + 1 and fus.tape_aborts() == 0
    return out


def _compare_after_launch(fus, ref, got, want, tag):
    for name, g, w in zip(("obs", "reward", "terminated", "truncated"), got, want[:4]):
        assert torch.equal(g, w), (tag, name)
    for key in STATE:
        assert torch.equal(fus.t[key], ref.t[key]), (tag, key)
    assert torch.equal(fus.early_terminated, ref.early_terminated), tag
    assert torch.equal(fus.grace_counts(), ref.grace_counts()), tag
    last = (want[2][-1] != 0) | (want[3][-1] != 0)                  # done on the launch's last step
    assert torch.equal(fus.terminal_obs[last], ref.terminal_obs[last]), tag
    assert torch.equal(fus.terminal_step_count[last], ref.terminal_step_count[last]), tag
    assert torch.equal(fus.terminal_total_reward[last], ref.terminal_total_reward[last]), tag
    return last


@pytest.mark.parametrize("n", [64, 1027])
@pytest.mark.parametrize("case", list(TAPE_CASES))
def test_tape_launch_equals_the_per_step_path(model, case, n):
    from mujocoposelearning_amd import _lib
    condition, params, grace, duration, K = TAPE_CASES[case]
    tail = TAIL
    noise, act = _inputs(n, K + tail)
    ref = _batch(model, n, noise, False, condition, params, grace, duration)
    fus = _batch(model, n, noise, True, condition, params, grace, duration)
    assert _lib.check(_lib.lib().hs_rollout_max_steps(fus._h)) == 511 >= K
    act = torch.tensor(act, device=ref.device)
    # the first launch: the case's K steps
    want = _per_step(ref, act[:K])
    got = _one_launch(fus, act[:K])
    _compare_after_launch(fus, ref, got, want, "first")
    done = (want[2] != 0) | (want[3] != 0)
    early, clock = want[4] != 0, (want[2] != 0) & (want[4] == 0)
    per_env = done.sum(0)
    print(f"{case} n={n}: {int(done.sum())} episode ends in {K} steps ({int(early.sum())} early, {int(clock.sum())} "
          f"by the clock), at most {int(per_env.max())} per env, {int(done[-1].sum())} on step {K}")
    assert early.any() and not want[3].any()
    if case == "several_episodes":
        assert int(per_env.max()) >= 3
    if case == "clock_and_early":
        assert int(early.sum()) > 0 and int(clock.sum()) > 0
    # the second launch: its last step ends episodes, and others ended earlier in it
    want2 = _per_step(ref, act[K:])
    got2 = _one_launch(fus, act[K:])
    last = _compare_after_launch(fus, ref, got2, want2, "second")
    done2 = (want2[2] != 0) | (want2[3] != 0)
    earlier = done2[:-1].any(0) & ~last
    print(f"  second launch of {tail}: {int(last.sum())} envs done on its last step, {int(earlier.sum())} earlier only")
    assert last.any() and earlier.any()
    ref.close()
    fus.close()


# -- rollouts ------------------------------------------------------------------------------------
NETS = {"tanh64": ("Tanh", [64, 64]), "relu256": ("ReLU", [256, 256])}
GAMMA = 0.99


def _vec_env(n, term, fused, seed=0, duration=10.0):
    from mujocoposelearning_amd.model import HsModel
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    cfg = {"model_path": XML, "duration": duration, "frame_skip": FS, "reward_config": {"type": "stand"},
           "termination": dict(term, fused=True) if fused else dict(term)}
    return HumanoidVecEnv(cfg, n_envs=n, model=HsModel(XML), seed=seed, precision="fp64")


def _ppo(env, T, net, **kw):
    import warnings

    from mujocoposelearning_amd.ppo import PPO
    act, arch = NETS[net]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return PPO(env, n_steps=T, batch_size=kw.pop("batch_size", 1024), n_epochs=1, seed=0, gamma=GAMMA,
                   policy_kwargs={"activation_fn": act, "net_arch": {"pi": arch, "vf": arch}}, **kw)


class _Replay:
    """The twin env behind step_tensors, keeping every step's early bytes."""

    def __init__(self, env):
        self.env, self.early = env, []

    def step_tensors(self, a):
        out = self.env.step_tensors(a)
        self.early.append(self.env.batch.early_terminated.clone() != 0)
        return out


ROLLOUTS = [(64, "tanh64", {"min_height": 1.28}, 1), (1027, "relu256", {"min_height": 1.28}, 1),
            (64, "relu256", {"min_height": 0.8}, 2), (1027, "tanh64", {"min_height": 0.8}, 2)]


@pytest.mark.parametrize("n,net,params,grace", ROLLOUTS)
def test_fused_rollout_matches_env_replay_and_policy(n, net, params, grace):
    """tests/test_gpu_rollout.py's three checks (env replay bitwise, sampler to fp32 rounding, returns exact) on
    two consecutive 40-step rollouts, one launch each."""
    from test_gpu_rollout import _check_rollout, _copy_env
    from mujocoposelearning_amd import _lib
    T = 40
    term = {"type": "fallen", "params": params, "grace_steps": grace}
    env, twin = _vec_env(n, term, True), _vec_env(n, term, False)
    assert env.rollout_handle() is not None and twin.rollout_handle() is None
    ppo = _ppo(env, T, net)
    ppo.policy.pack_heads()
    assert ppo._fused_rollout_args() is not None
    assert _lib.check(_lib.lib().hs_rollout_max_steps(env.rollout_handle())) == 511 >= T
    early_total = 0
    for it in range(2):
        _copy_env(env, twin)
        assert torch.equal(env.batch.grace_counts(), twin.batch.grace_counts())
        ep_acc0, start0, ctr0 = ppo.ep_acc.clone(), ppo.episode_start.clone(), int(ppo._noise_ctr.item())
        ppo.collect_rollouts()
        torch.cuda.synchronize()
        assert getattr(ppo, "fused_fallbacks", 0) == 0 and env.batch.tape_aborts() == 0
        assert len(ppo.rollout_launches) == it + 1 and ppo.rollout_launches[-1][0] == T * n     # one launch
        replay = _Replay(twin)
        _check_rollout(ppo, replay, ep_acc0, start0, ctr0)
        early = torch.stack(replay.early)
        assert ppo.buf["done"][early].all() and not ppo.buf["boot"][early].any()
        early_total += int(early.sum())
        for k in STATE:
            assert torch.equal(env.batch.t[k], twin.batch.t[k]), k
        assert torch.equal(env.batch.grace_counts(), twin.batch.grace_counts())
    print(f"n={n} {net} {params} grace {grace}: {early_total} early ends in 2 x {T} steps")
    assert early_total > 0
    env.close()
    twin.close()


def test_fused_rollout_with_normalisation(monkeypatch):
    """The NORM instance: PPO(VecNormalize(env)), `fallen` at 1.28, two 40-step rollouts of one launch each.  The
    raw rows are bitwise the twin's replay, the sampler reproduces the actions on the normalised rows."""
    from test_gpu_rollout import _copy_env
    from mujocoposelearning_amd import VecNormalize
    from mujocoposelearning_amd.ppo_ops import ppo_act
    n, T = 130, 40
    term = {"type": "fallen", "params": {"min_height": 1.28}, "grace_steps": 1}
    env, twin = _vec_env(n, term, True), _vec_env(n, term, False)
    vn = VecNormalize(env, gamma=GAMMA)
    ppo = _ppo(vn, T, "tanh64")
    ppo.policy.pack_heads()
    assert ppo._fused_rollout_args() is not None and ppo._norm_obs()
    raw = {}
    real_norm = ppo._normalize_rollout

    def keep_raw():
        raw["obs"], raw["rew"] = ppo.buf["obs"].clone(), ppo.buf["rew"].clone()
        real_norm()
    monkeypatch.setattr(ppo, "_normalize_rollout", keep_raw)
    for it in range(2):
        _copy_env(env, twin)
        start0, ctr0, acc = ppo.episode_start.clone(), int(ppo._noise_ctr.item()), ppo.ep_acc.clone()
        ppo.collect_rollouts()
        torch.cuda.synchronize()
        assert getattr(ppo, "fused_fallbacks", 0) == 0 and len(ppo.rollout_launches) == it + 1
        b = ppo.buf
        early_total = 0
        for t in range(T):
            obs, rew, term_f, trunc = twin.step_tensors(b["act"][t].clamp(-1, 1))
            nxt = raw["obs"][t + 1] if t + 1 < T else ppo.obs
            assert torch.equal(obs.float(), nxt), t
            assert torch.equal(rew.float(), raw["rew"][t]), t
            assert torch.equal((term_f != 0) | (trunc != 0), b["done"][t]), t
            early = twin.batch.early_terminated != 0
            assert b["done"][t][early].all() and not b["boot"][t][early].any()
            early_total += int(early.sum())
            acc = acc + raw["rew"][t].double()
            assert torch.equal(b["epret"][t], acc), t
            acc = torch.where(b["done"][t], torch.zeros_like(acc), acc)
        assert early_total > 0 and torch.equal(ppo.ep_acc, acc)
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
            assert torch.allclose(b["act"][t], out[0], rtol=1e-5, atol=2e-5), t
            assert torch.allclose(b["logp"][t], out[2], rtol=1e-5, atol=2e-4), t
        assert torch.equal(env.batch.grace_counts(), twin.batch.grace_counts())
    env.close()
    twin.close()


# -- evaluation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1027])
def test_fused_evaluation_equals_the_step_by_step_path(n, monkeypatch):
    """E = 2 episodes per env, 1 s episodes (67 steps by the clock), `fallen` at 1.28.  The action head's weights
    are zero and its bias random, so the action is clip(b3) whatever the summation order: the closed loop has no
    fp32 fork and the two paths must agree bitwise (tests/test_gpu_evaluate.py).  The trace is compared as far as
    the step-by-step path records it: on a done step that path rebuilds the terminal row from the terminal obs,
    which carries no root x, y, and fills those two from the step before (evaluation.py _Stepwise), so they are
    compared on the other steps only."""
    from mujocoposelearning_amd import ppo as ppo_mod
    from mujocoposelearning_amd.evaluation import evaluate_policy_device
    term = {"type": "fallen", "params": {"min_height": 1.28}, "grace_steps": 1}
    env, twin = _vec_env(n, term, True, duration=1.0), _vec_env(n, term, False, duration=1.0)
    model = _ppo(env, 2, "relu256", batch_size=64)
    twin.reset_tensors()      # PPO's constructor reset env once: the twin's episode counters (reset noise) follow
    with torch.no_grad():
        model.policy.action_net.weight.zero_()
        model.policy.action_net.bias.uniform_(-1.0, 1.0)
    length = env.episode_length()
    assert length == 67
    res = evaluate_policy_device(model, env, 2, n_trace=4)
    assert res.fused_launches >= 1 and res.fallbacks == 0 and env.batch.tape_aborts() == 0
    monkeypatch.setattr(ppo_mod, "FUSED_ROLLOUT", False)
    ref = evaluate_policy_device(model, twin, 2, n_trace=4)
    assert ref.fused_launches == 0 and ref.fallbacks == 0
    torch.cuda.synchronize()
    assert bool((ref.end_step >= 0).all())
    assert torch.equal(res.returns, ref.returns)
    assert torch.equal(res.lengths, ref.lengths) and torch.equal(res.end_step, ref.end_step)
    for k in ("qvel", "actions", "rewards", "dones"):
        assert torch.equal(res.trace[k], ref.trace[k]), k
    done = ref.trace["dones"]
    assert bool(done.any()) and torch.equal(res.trace["qpos"][..., 2:], ref.trace["qpos"][..., 2:])
    assert torch.equal(res.trace["qpos"][~done], ref.trace["qpos"][~done])
    print(f"n={n}: episode lengths {int(res.lengths.min())}-{int(res.lengths.max())} of {length}")
    assert int(res.lengths.max()) < length
    for k in STATE:
        assert torch.equal(env.batch.t[k], twin.batch.t[k]), k
    assert torch.equal(env.batch.grace_counts(), twin.batch.grace_counts())
    env.close()
    twin.close()


# -- the overflow fallback -------------------------------------------------------------------------
def test_fused_rollout_overflow_falls_back_step_by_step():
    """tests/test_gpu_rollout.py's lying states (they overflow the resident contact tier; 4096 envs, T = 6) under
    `fallen` with grace_steps 8, so the lying envs -- below 0.8 m from the start -- do not end before the overflow.
    The library undoes the launch, the grace counters included, and the rollout runs step by step."""
    from oracle.oracle import Oracle
    from test_gpu_contacts import lying_states
    from test_gpu_rollout import _check_rollout, _copy_env
    n, T = 4096, 6
    term = {"type": "fallen", "params": {"min_height": 0.8}, "grace_steps": 8}
    q = np.stack(lying_states(Oracle(XML), 16, seed=11))
    idx = np.arange(16) * 255 + 7
    env, twin = _vec_env(n, term, True), _vec_env(n, term, False)
    ppo = _ppo(env, T, "relu256")
    st = env.batch.get_state()
    st["qpos"][idx] = q
    st["qvel"][idx] = 0.0
    st["qacc_warmstart"][idx] = 0.0
    env.batch.set_state(**st)
    _copy_env(env, twin)
    ep_acc0, start0, ctr0 = ppo.ep_acc.clone(), ppo.episode_start.clone(), int(ppo._noise_ctr.item())
    ppo.collect_rollouts()
    torch.cuda.synchronize()
    assert getattr(ppo, "fused_fallbacks", 0) == 1 and env.batch.tape_aborts() == 1
    assert env.batch.wide_reruns() >= len(idx)
    _check_rollout(ppo, twin, ep_acc0, start0, ctr0)
    counts = env.batch.grace_counts()
    assert torch.equal(counts, twin.batch.grace_counts())
    assert int(counts.max()) == T and not ppo.buf["done"].any()      # the lying envs held all T steps: none ended
    assert torch.equal(env.batch.early_terminated, twin.batch.early_terminated)
    env.close()
    twin.close()


# -- refusals --------------------------------------------------------------------------------------
def test_refusals(model):
    from mujocoposelearning_amd import _lib
    from mujocoposelearning_amd import reward_program as rw
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.ppo import PPO
    L = _lib.lib()
    n = 64
    noise, act = _inputs(n, 4)
    b = HsBatch(model, n, precision="fp64", seed=5)
    b.configure(frame_skip=FS, duration=10.0, reward_id=0, autoreset=1)
    b.reset(qpos_noise=noise[0], qvel_noise=noise[1])
    act = torch.tensor(act, device=b.device)
    before = b.step_count.clone()
    # program / kind mismatch: the `fallen` program with kind = LOST_BALANCE, refused by the probe table
    fallen = rw.device_termination("fallen").compile(model)
    rc = L.hs_set_termination_builtin(b._h, fallen.handle, fallen.params(None), 1, rw.TERM_LOST_BALANCE, 0.8, np.pi / 4)
    assert rc < 0 and "differ on probe row" in L.hs_last_error().decode()
    # ... and with another min_height, or the other way round
    assert L.hs_set_termination_builtin(b._h, fallen.handle, fallen.params(None), 1, rw.TERM_FALLEN, 0.9, 0.0) < 0
    lost = rw.device_termination("lost_balance").compile(model)
    assert L.hs_set_termination_builtin(b._h, lost.handle, lost.params(None), 1, rw.TERM_FALLEN, 0.8, np.pi / 4) < 0
    assert L.hs_set_termination_builtin(b._h, fallen.handle, fallen.params(None), 1, 3, 0.8, 0.0) < 0
    # a predicate that reads ctrl is no function of qpos alone
    reg = {}
    rw.register_device_termination("effort", lambda d, p: (d.qpos[2] < 0.8) | (rw.sum(rw.square(d.ctrl)) > 10.0),
                                   registry=reg)
    effort = rw.device_termination("effort", reg).compile(model)
    rc = L.hs_set_termination_builtin(b._h, effort.handle, None, 1, rw.TERM_FALLEN, 0.8, 0.0)
    assert rc < 0 and "reads ctrl" in L.hs_last_error().decode()
    # nothing was set or launched by any of them
    assert L.hs_termination_state(b._h, None, None, None, None) == 0 and torch.equal(b.step_count, before)
    with pytest.raises(ValueError, match="user-registered predicate"):
        b.set_termination("effort", registry=reg, fused=True)
    assert b.termination is None
    # fused-capable, but with host reset-noise arrays bound: the fused entry points still refuse
    b.set_termination("fallen", fused=True)
    nz = [torch.zeros(n, 28, dtype=b.dtype, device=b.device), torch.zeros(n, 27, dtype=b.dtype, device=b.device)]
    b.set_autoreset_noise(*nz)
    rc = L.hs_step_tape(b._h, act.data_ptr(), 4, None, b.stream)
    assert rc < 0 and "on-device reset noise" in L.hs_last_error().decode()
    assert torch.equal(b.step_count, before)
    b.set_autoreset_noise(None, None)
    b.step_tape(act[:2], outputs=False)                      # without them it launches
    assert (b.step_count == 2).all() or bool(b.early_terminated.any())
    # hs_set_termination after the builtin call drops the mark
    b.set_termination("fallen")
    assert not b.termination_fused
    rc = L.hs_step_tape(b._h, act.data_ptr(), 4, None, b.stream)
    assert rc < 0 and "termination condition" in L.hs_last_error().decode()
    b.close()
    # hs_rollout on a fused-capable batch with bound host noise
    term = {"type": "fallen", "params": {"min_height": 0.8}, "grace_steps": 1}
    env = _vec_env(n, term, True)
    p = _ppo(env, 4, "relu256")
    p.policy.pack_heads()
    h, pol, keep = p._fused_rollout_args()
    buf = p.buf
    rb = _lib.hs_rollout_bufs(buf["obs"].data_ptr(), p.obs.data_ptr(), buf["act"].data_ptr(), buf["logp"].data_ptr(),
                              buf["start"].data_ptr(), buf["rew"].data_ptr(), buf["done"].data_ptr(),
                              buf["epret"].data_ptr(), buf["boot"].data_ptr(), buf["tobs"].data_ptr(),
                              p.ep_acc.data_ptr(), p.episode_start.data_ptr(), p._act_clip.data_ptr(),
                              p._noise_ctr.data_ptr(), 1, 0)
    env.batch.set_autoreset_noise(torch.zeros(n, 28, dtype=env.batch.dtype, device=env.device),
                                  torch.zeros(n, 27, dtype=env.batch.dtype, device=env.device))
    with pytest.raises(_lib.HsimError, match="on-device reset noise"):
        _lib.check(L.hs_rollout_act(h, C.byref(pol), 0, C.byref(rb), 0, 4, 4, None))
    env.close()
