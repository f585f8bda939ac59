"""Episodes that start from a bank of initial states (hs_set_initial_states; csrc/hs_env_step.h reset_draw).

fp64 unless stated, 5 envs (an odd count: one wave has a ghost half), frame_skip 3.  The yardsticks:
* a bank of the one row "default" is bitwise the unbound reset;
* a reset from row j is ``set_state(row j + noise)`` + one ``physics_step`` on a second batch, with j and the noise
  restated on the host (``initial_state.draw_index`` / ``uniform_pm``);
* every launch shape (tape, schedules, chunk queue, fused rollout and evaluation, the TERM instances) is bitwise the
  per-step path with the same bank bound.
"""
import numpy as np
import pytest
import torch

from conftest import GOLDEN, XML

pytestmark = pytest.mark.gpu

N, FS = 5, 3
TRAJ = GOLDEN + "/humanoid_trajectory.xml"
STATE = ("qpos", "qvel", "time", "step_count", "episode", "total_reward", "obs")
OUT = ("obs", "reward", "terminated", "truncated")


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


@pytest.fixture(scope="module")
def bank4(model):
    """default, squat, stand_on_left_leg and one recorded key (the second recorded step: standing, qvel up to 26)."""
    from mujocoposelearning_amd.initial_state import build_bank
    tq, tv = build_bank(model, {"trajectory": TRAJ})
    assert np.abs(tv[2]).max() > 1.0
    q, v = build_bank(model, {"keyframes": ["default", "squat", "stand_on_left_leg"], "states": (tq[2], tv[2])})
    assert q.shape == (4, 28)
    return q, v


def _batch(model, n=N, precision="fp64", seed=3, max_steps=750, schedule=None, groups=1, bank=None, duration=10.0):
    from mujocoposelearning_amd.batch import HsBatch
    b = HsBatch(model, n, precision=precision, seed=seed, groups=groups)
    b.configure(frame_skip=FS, duration=duration, reward_id=0, autoreset=1, max_steps=max_steps, schedule=schedule)
    if bank is not None:
        b.set_initial_states(*bank)
    return b


def _actions(steps, n, seed=1):
    return torch.tensor(np.random.default_rng(seed).uniform(-1, 1, (steps, n, 21)).astype(np.float32), device="cuda")


def _snap(b, keys=STATE):
    torch.cuda.synchronize()
    return {k: b.t[k].clone() for k in keys}


def _expected_start(b, noise=None):
    """(j, qpos, qvel) every env's current episode starts from, restated on the host in the batch precision: row j
    of the bank as the library holds it + the reset noise (the counter RNG's, or the rows ``noise`` = (qn, vn)),
    the free joint's z noise x 0.1 and no quaternion noise."""
    from mujocoposelearning_amd.initial_state import QVEL_SLOT0, draw_index, uniform_pm
    T = np.float64 if b.precision == "fp64" else np.float32
    bq, bv = b.initial_states
    n, nq, nv = b.n, bq.shape[1], bv.shape[1]
    ep = b.t["episode"].cpu().numpy().astype(np.int64)
    j = np.zeros(n, np.int64)
    qn, vn = np.zeros((n, nq), T), np.zeros((n, nv), T)
    scale = float(T(b.cfg.noise_scale))
    for g, (_, lo, hi) in enumerate(b._groups):
        seed = b._group_seed(g)
        env = np.arange(hi - lo)
        j[lo:hi] = draw_index(seed, env, ep[lo:hi], len(bq))
        qn[lo:hi] = uniform_pm(seed, env[:, None], ep[lo:hi, None], np.arange(nq)[None], scale).astype(T)
        vn[lo:hi] = uniform_pm(seed, env[:, None], ep[lo:hi, None], QVEL_SLOT0 + np.arange(nv)[None], scale).astype(T)
    if noise is not None:
        qn, vn = noise[0].astype(T), noise[1].astype(T)
    qn = qn.copy()
    qn[:, 2] = qn[:, 2] * T(0.1)
    qn[:, 3:7] = 0
    return j, (bq.astype(T)[j] + qn).astype(np.float64), (bv.astype(T)[j] + vn).astype(np.float64)


def _construct(ref, qpos, qvel):
    """The reset restated on a second batch: the state, zero warm start, clock and ctrl, then one mj_step."""
    ref.set_state(qpos=qpos, qvel=qvel, qacc_warmstart=0.0, time=0.0, ctrl=0.0)
    ref.physics_step(None, 1)
    torch.cuda.synchronize()


def _check_starts(b, ref, done=None, noise=None, tag=""):
    """The envs in ``done`` (all: None) hold the state of a reset from their row, bitwise."""
    j, q, v = _expected_start(b, noise=noise)
    assert np.array_equal(b.initial_state_index(), j), tag
    _construct(ref, q, v)
    sel = slice(None) if done is None else done
    for k in ("qpos", "qvel", "time"):
        assert torch.equal(b.t[k][sel], ref.t[k][sel]), (tag, k)
    assert torch.equal(b.t["obs"][sel], ref.t["obs"][sel]), (tag, "obs")
    return j


# 1 ------------------------------------------------------------------------------------------------
def test_default_row_is_the_default_reset(model):
    from mujocoposelearning_amd.initial_state import build_bank
    a = _batch(model, max_steps=2)
    b = _batch(model, max_steps=2, bank=build_bank(model, {"keyframes": ["default"]}))
    assert b.initial_states[0].shape == (1, 28) and a.initial_states is None
    act = _actions(5, N)
    a.reset()
    b.reset()
    dones = 0
    for t in range(5):
        oa = [x.clone() for x in a.step(act[t])]
        ob = [x.clone() for x in b.step(act[t])]
        for name, x, y in zip(OUT, oa, ob):
            assert torch.equal(x, y), (t, name)
        for k in STATE:
            assert torch.equal(a.t[k], b.t[k]), (t, k)
        dones += int(((oa[2] != 0) | (oa[3] != 0)).sum())
    assert dones == 2 * N                       # auto-resets happened: steps 2 and 4
    a.close()
    b.close()


# 2, 7 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_row_and_noise(model, bank4, precision):
    """After reset() and after the auto-resets that begin episodes 2 and 3: row index, state and obs."""
    b = _batch(model, precision=precision, max_steps=2, bank=bank4)
    ref = _batch(model, precision=precision)
    b.reset()
    seen = set(_check_starts(b, ref, tag="reset").tolist())
    act = _actions(4, N)
    for t in range(4):
        _, _, term, trunc = b.step(act[t])
        if t % 2 == 1:
            assert bool(trunc.all()) and int(b.t["episode"][0]) == 2 + t // 2
            seen |= set(_check_starts(b, ref, tag=f"episode {2 + t // 2}").tolist())
    assert len(seen) >= 3, seen                 # 15 draws over 4 rows
    assert int(b.t["warning"].sum()) == 0
    b.close()
    ref.close()


# 3 ------------------------------------------------------------------------------------------------
def test_host_supplied_noise(model, bank4):
    """Bound noise rows: the row index still follows the device draw, the noise is the rows'."""
    rng = np.random.default_rng(7)
    qn, vn = rng.uniform(-0.01, 0.01, (N, 28)), rng.uniform(-0.01, 0.01, (N, 27))
    b = _batch(model, max_steps=2, bank=bank4)
    ref = _batch(model)
    b.reset(qpos_noise=qn, qvel_noise=vn)
    j1 = _check_starts(b, ref, noise=(qn, vn), tag="reset")
    qn2, vn2 = rng.uniform(-0.01, 0.01, (N, 28)), rng.uniform(-0.01, 0.01, (N, 27))
    b.set_autoreset_noise(qn2, vn2)
    act = _actions(2, N)
    b.step(act[0])
    _, _, _, trunc = b.step(act[1])
    assert bool(trunc.all())
    j2 = _check_starts(b, ref, noise=(qn2, vn2), tag="auto-reset")
    # (the same counters without bound rows would give the same indices: the draw does not see the noise source)
    c = _batch(model, max_steps=2, bank=bank4)
    c.reset()
    assert np.array_equal(c.initial_state_index(), j1)
    c.step(act[0])
    c.step(act[1])
    assert np.array_equal(c.initial_state_index(), j2)
    for x in (b, ref, c):
        x.close()


# 4 ------------------------------------------------------------------------------------------------
def _eight_steps(b, act):
    rows = [[], [], [], []]
    for t in range(len(act)):
        for dst, src in zip(rows, b.step(act[t])):
            dst.append(src.clone())
    return [torch.stack(r) for r in rows], _snap(b)


@pytest.fixture(scope="module")
def eight_step_reference(model, bank4):
    b = _batch(model, max_steps=3, bank=bank4)
    b.reset()
    act = _actions(8, N)
    want, state = _eight_steps(b, act)
    done = (want[2] != 0) | (want[3] != 0)
    assert int(done.sum()) == 2 * N            # every env auto-reset twice, from drawn rows
    b.close()
    return act, want, state


def test_tape_equals_eight_steps(model, bank4, eight_step_reference):
    act, want, state = eight_step_reference
    b = _batch(model, max_steps=3, bank=bank4)
    b.reset()
    got = b.step_tape(act)
    for name, g, w in zip(OUT, got, want):
        assert torch.equal(g, w), name
    for k, v in _snap(b).items():
        assert torch.equal(v, state[k]), k
    print(f"tape_aborts {b.tape_aborts()} wide_reruns {b.wide_reruns()}")
    b.close()


@pytest.mark.parametrize("schedule", ["direct", "single", "auto", "fixed_order"])
def test_schedules_equal_eight_steps(model, bank4, eight_step_reference, schedule):
    act, want, state = eight_step_reference
    b = _batch(model, max_steps=3, bank=bank4, schedule=schedule)
    b.reset()
    got, snap = _eight_steps(b, act)
    for name, g, w in zip(OUT, got, want):
        assert torch.equal(g, w), name
    for k in STATE:
        assert torch.equal(snap[k], state[k]), k
    b.close()


def test_chunk_queue_equals_direct(model, bank4):
    """2 * resident_waves + 3 envs: the smallest odd batch HS_SCHED_AUTO queues (tests/test_gpu_queue_boundaries.py)."""
    probe = _batch(model, 2)
    n = 2 * probe.resident_waves + 3
    probe.close()
    act = _actions(8, n)
    res = []
    for sched in ("direct", "auto"):
        b = _batch(model, n, max_steps=3, bank=bank4, schedule=sched)
        assert b.queued() == (sched == "auto")
        b.reset()
        res.append(_eight_steps(b, act))
        if sched == "auto":
            j = b.initial_state_index()
            assert set(j.tolist()) == {0, 1, 2, 3}
            print(f"n={n} wide_reruns {b.wide_reruns()}")
        b.close()
    (wo, ws), (go, gs) = res
    for name, g, w in zip(OUT, go, wo):
        assert torch.equal(g, w), name
    for k in STATE:
        assert torch.equal(gs[k], ws[k]), k


# 5 ------------------------------------------------------------------------------------------------
def _vec_env(n, spec, duration, termination=None, seed=0):
    from mujocoposelearning_amd.model import HsModel
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    cfg = {"model_path": XML, "duration": duration, "frame_skip": FS, "reward_config": {"type": "stand"}}
    if spec is not None:
        cfg["initial_state"] = spec
    if termination is not None:
        cfg["termination"] = termination
    return HumanoidVecEnv(cfg, n_envs=n, model=HsModel(XML), seed=seed, precision="fp64")


def _ppo(env, T, **kw):
    import warnings

    from mujocoposelearning_amd.ppo import PPO
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return PPO(env, n_steps=T, batch_size=kw.pop("batch_size", 64), n_epochs=1, seed=0,
                   policy_kwargs={"activation_fn": "Tanh", "net_arch": {"pi": [64, 64], "vf": [64, 64]}}, **kw)


SPEC4 = {"keyframes": ["default", "squat", "stand_on_left_leg"], "trajectory": TRAJ, "stride": 1000}
FALLEN = {"type": "fallen", "params": {"min_height": 1.0}, "grace_steps": 1}


@pytest.mark.parametrize("term", [None, FALLEN], ids=["plain", "fallen"])
def test_fused_rollout_equals_per_step(term, n=64, T=8):
    """0.06 s episodes (4 env steps: launches of 3), so every env draws two or three rows in two rollouts.  With
    `fallen` below 1.0 m fused, the squat rows (0.6 m) end at once: the TERM instances draw too, several episodes
    of one env in one launch."""
    from test_gpu_rollout import _check_rollout, _copy_env
    fterm = dict(term, fused=True) if term else None
    env, twin = _vec_env(n, SPEC4, 0.06, fterm), _vec_env(n, SPEC4, 0.06, term)
    assert env.batch.initial_states[0].shape == (4, 28)
    ppo = _ppo(env, T)
    ppo.policy.pack_heads()
    assert ppo._fused_rollout_args() is not None
    rows = set()
    for it in range(2):
        _copy_env(env, twin)
        ep_acc0, start0, ctr0 = ppo.ep_acc.clone(), ppo.episode_start.clone(), int(ppo._noise_ctr.item())
        ppo.collect_rollouts()
        torch.cuda.synchronize()
        assert getattr(ppo, "fused_fallbacks", 0) == 0 and env.batch.tape_aborts() == 0
        _check_rollout(ppo, twin, ep_acc0, start0, ctr0)
        assert int(ppo.buf["done"].sum()) >= n
        for k in STATE:
            assert torch.equal(env.batch.t[k], twin.batch.t[k]), k
        rows |= set(env.batch.initial_state_index().tolist())
    assert rows == {0, 1, 2, 3}
    env.close()
    twin.close()


@pytest.mark.parametrize("term", [None, FALLEN], ids=["plain", "fallen"])
def test_fused_evaluation_equals_step_by_step(term, monkeypatch, n=64):
    from mujocoposelearning_amd import ppo as ppo_mod
    from mujocoposelearning_amd.evaluation import evaluate_policy_device
    fterm = dict(term, fused=True) if term else None
    env, twin = _vec_env(n, SPEC4, 0.06, fterm), _vec_env(n, SPEC4, 0.06, term)
    model = _ppo(env, 2)
    twin.reset_tensors()          # PPO's constructor reset env once: the twin's episode counters follow
    with torch.no_grad():         # the action is clip(b3) whatever the summation order: no fp32 fork
        model.policy.action_net.weight.zero_()
        model.policy.action_net.bias.uniform_(-1.0, 1.0)
    res = evaluate_policy_device(model, env, 3)
    assert res.fused_launches > 0 and res.fallbacks == 0
    monkeypatch.setattr(ppo_mod, "FUSED_ROLLOUT", False)
    ref = evaluate_policy_device(model, twin, 3)
    assert ref.fused_launches == 0
    torch.cuda.synchronize()
    assert torch.equal(res.returns, ref.returns)
    assert torch.equal(res.lengths, ref.lengths) and torch.equal(res.end_step, ref.end_step)
    if term:
        assert int((res.lengths == 1).sum()) > 0           # a squat start ends at its first step
    env.close()
    twin.close()


# 6 ------------------------------------------------------------------------------------------------
def test_floor_lying_rows(model):
    from mujocoposelearning_amd.initial_state import build_bank
    bank = build_bank(model, {"keyframes": ["prone", "supine"]})
    b = _batch(model, max_steps=2, bank=bank)
    ref = _batch(model)
    b.reset()
    j = _check_starts(b, ref, tag="reset")
    act = _actions(4, N)
    for t in range(3):
        b.step(act[t])
    torch.cuda.synchronize()
    for k in ("qpos", "qvel", "obs"):
        assert bool(torch.isfinite(b.t[k]).all()), k
    assert int(b.t["warning"][:, 3].sum()) == 0                  # HS_WARN_OVERFLOW: nothing past the wide tier
    print(f"rows {j.tolist()} after reset + 3 steps: wide_reruns {b.wide_reruns()} tape_aborts {b.tape_aborts()}")
    # a 4-step tape is the step loop, whether or not it aborted
    c, d = _batch(model, max_steps=2, bank=bank), _batch(model, max_steps=2, bank=bank)
    c.reset()
    d.reset()
    want, state = _eight_steps(c, act)
    got = d.step_tape(act)
    for name, g, w in zip(OUT, got, want):
        assert torch.equal(g, w), name
    for k, v in _snap(d).items():
        assert torch.equal(v, state[k]), k
    assert int(d.t["warning"][:, 3].sum()) == 0
    print(f"4-step tape: tape_aborts {d.tape_aborts()} wide_reruns {d.wide_reruns()} (step loop: {c.wide_reruns()})")
    for x in (b, ref, c, d):
        x.close()


# 8 ------------------------------------------------------------------------------------------------
def test_groups_draw_with_their_own_seeds(model, bank4):
    b = _batch(model, 6, groups=2, bank=bank4, seed=11)
    ref = _batch(model, 6)
    assert len(b._groups) == 2
    b.reset()
    j = _check_starts(b, ref, tag="groups")
    from mujocoposelearning_amd.initial_state import draw_index
    for g, (_, lo, hi) in enumerate(b._groups):
        seed = (11 + 0x9E3779B97F4A7C15 * g) & (2 ** 64 - 1)
        assert np.array_equal(j[lo:hi], draw_index(seed, np.arange(hi - lo), 1, 4))
    # another seed, other draws (24 envs: the chance that 24 draws of 4 rows repeat is 4^-24)
    big = _batch(model, 24, groups=2, bank=bank4, seed=11)
    big.reset()
    j11 = big.initial_state_index()
    q11 = big.t["qpos"].clone()
    big.set_seed(12)
    big.t["episode"].zero_()
    big.reset()
    assert not np.array_equal(big.initial_state_index(), j11) and not torch.equal(big.t["qpos"], q11)
    assert np.array_equal(big.initial_state_index()[:12], draw_index(12, np.arange(12), 1, 4))
    for x in (b, ref, big):
        x.close()


# 9 ------------------------------------------------------------------------------------------------
def test_unbind_is_the_unbound_reset(model, bank4):
    a, b = _batch(model, max_steps=2), _batch(model, max_steps=2, bank=bank4)
    act = _actions(4, N)
    a.reset()
    b.reset()
    assert not torch.equal(a.t["qpos"], b.t["qpos"])
    b.set_initial_states(None)
    assert b.initial_states is None and (b.initial_state_index() == -1).all()
    b.t["episode"].zero_()
    b.reset()
    for t in range(4):
        a.step(act[t])
        b.step(act[t])
    for k in STATE:
        assert torch.equal(a.t[k], b.t[k]), k
    a.close()
    b.close()


def test_rebinding_is_seen_by_the_next_launch(model, monkeypatch):
    """Between per-step rollouts PPO replays a recorded graph of its env launches; a rebind makes it record anew."""
    import warnings

    from mujocoposelearning_amd import ppo as ppo_mod
    from mujocoposelearning_amd.initial_state import build_bank
    from test_gpu_rollout import _check_rollout, _copy_env
    n, T = 64, 4
    squat = build_bank(model, {"keyframe": "squat"})
    left = build_bank(model, {"keyframe": "stand_on_left_leg"})
    env, twin = _vec_env(n, None, 0.06), _vec_env(n, None, 0.06)
    monkeypatch.setattr(ppo_mod, "FUSED_ROLLOUT", False)          # the per-step path, as a graph
    ppo = _ppo(env, T)
    ppo.policy.pack_heads()
    assert ppo._fused_rollout_args() is None
    for it, bank in enumerate((squat, squat, left, None)):
        for e in (env, twin):
            e.batch.set_initial_states(*bank) if bank is not None else e.batch.set_initial_states(None)
        _copy_env(env, twin)
        ep_acc0, start0, ctr0 = ppo.ep_acc.clone(), ppo.episode_start.clone(), int(ppo._noise_ctr.item())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ppo.collect_rollouts()
        torch.cuda.synchronize()
        assert ppo._rollout_graph is not None, "the per-step rollout was not recorded as a graph"
        _check_rollout(ppo, twin, ep_acc0, start0, ctr0)
        # every env began an episode at the rollout's last step (4-step episodes): its height says which bank
        z = env.batch.t["qpos"][:, 2]
        lo, hi = ((0.3, 0.9) if bank is squat else (1.0, 1.25) if bank is left else (1.25, 1.3))
        fresh = env.batch.t["step_count"] == 0
        assert bool(fresh.all()) and bool(((z > lo) & (z < hi)).all()), (it, z)
    env.close()
    twin.close()


def test_abi_errors(model, bank4):
    from mujocoposelearning_amd import _lib
    from mujocoposelearning_amd._lib import HsimError
    b = _batch(model)
    q, v = bank4
    with pytest.raises(HsimError, match=r"qpos must be \[K, 28\]"):
        b.set_initial_states(q[:, :-1], None)
    with pytest.raises(HsimError, match=r"qvel must be \[4, 27\]"):
        b.set_initial_states(q, v[:3])
    bad = q.copy()
    bad[1, 9] = np.nan
    with pytest.raises(HsimError, match=r"qpos\[1\]\[9\] is not finite"):
        b.set_initial_states(bad, v)
    vbad = v.copy()
    vbad[2, 0] = np.inf
    with pytest.raises(HsimError, match=r"qvel\[2\]\[0\] is not finite"):
        b.set_initial_states(q, vbad)
    zq = q.copy()
    zq[3, 3:7] = 0
    with pytest.raises(HsimError, match="row 3 has a zero free-joint quaternion"):
        b.set_initial_states(zq, v)
    with pytest.raises(HsimError, match="HS_MAX_INITIAL_STATES"):
        b.set_initial_states(np.repeat(q, 1025, axis=0), None)
    L = _lib.lib()
    assert L.hs_set_initial_states(b._h, -1, q.ctypes.data, None) < 0
    assert L.hs_set_initial_states(b._h, 2, None, None) < 0 and b"qpos must not be NULL" in L.hs_last_error()
    import ctypes as C
    k = C.c_int(-1)
    _lib.check(L.hs_get_initial_states(b._h, C.byref(k)))
    assert k.value == 0 and b.initial_states is None          # a refused bind binds nothing
    b.set_initial_states(np.repeat(q, 1024, axis=0), None)    # the cap itself is fine
    _lib.check(L.hs_get_initial_states(b._h, C.byref(k)))
    assert k.value == 4096
    b.set_initial_states(q, v)                                 # and a smaller bank after it
    _lib.check(L.hs_get_initial_states(b._h, C.byref(k)))
    assert k.value == 4
    b.reset()
    assert set(b.initial_state_index().tolist()) <= {0, 1, 2, 3}
    b.close()


# 10 -----------------------------------------------------------------------------------------------
def test_env_surfaces(model):
    """The reset obs's height entry is within 0.02 of the keyframe's z: noise 0.001 plus one 5 ms substep of free
    fall and settling."""
    from mujocoposelearning_amd.env import HumanoidEnv
    z = float(model.keyframe("squat")[2])
    venv = _vec_env(N, {"keyframe": "squat"}, 10.0)
    obs = venv.reset()
    assert obs.shape == (N, 352) and np.abs(obs[:, 0] - z).max() < 0.02
    obs2, rew, dones, infos = venv.step(np.zeros((N, 21), np.float32))
    assert np.isfinite(obs2).all() and np.isfinite(rew).all() and len(infos) == N
    venv.close()
    env = HumanoidEnv({"model_path": XML, "duration": 10.0, "frame_skip": FS, "reward_config": {"type": "stand"},
                       "initial_state": {"keyframe": "squat"}})
    o, info = env.reset(seed=1)
    assert abs(o[0] - z) < 0.02 and abs(info["height"] - z) < 0.02
    o, r, term, trunc, info = env.step(np.zeros(21, np.float32))
    assert np.isfinite(o).all() and np.isfinite(r)
    with pytest.raises(ValueError, match="unknown keyframe"):
        _vec_env(N, {"keyframe": "sit"}, 10.0)


def test_without_the_key_nothing_changes(model):
    """HumanoidVecEnv without ``initial_state`` against a batch configured as the env configures it today."""
    venv = _vec_env(N, None, 10.0, seed=4)
    b = _batch(model, precision="fp64", seed=4)
    b.configure(frame_skip=FS, duration=10.0, max_steps=750, reward_id=0, autoreset=1, init_height=1.282,
                noise_scale=0.01)
    o1 = venv.reset_tensors().clone()
    o2 = b.reset().clone()
    assert torch.equal(o1, o2)
    act = _actions(3, N)
    for t in range(3):
        x = venv.step_tensors(act[t])
        y = b.step(act[t])
        for name, p, q in zip(OUT, x, y):
            assert torch.equal(p, q), (t, name)
    assert venv.batch.initial_states is None
    venv.close()
    b.close()
