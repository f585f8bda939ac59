"""Reference-motion targets on the device (csrc/hs_reward_prog.hip: the lane's phase prologue and the two-row
gather of a reference load; hs_set_reference_motion; env_config["reference_motion"]; "track").

Bars.  Sampling and the step path: BITWISE against ``reference_motion.sample`` -- the sample is a float64 divide
and add, then a subtraction, a product and an add in the batch dtype, all correctly rounded on the device as in
numpy (the fp32 build's approximate divide is not involved: the phase is float64).  "track" against the host
interpreter on the same states: the bar tests/test_gpu_reward_program.py holds user programs to, 1e-12 relative
in fp64 and 2e-6 (1 + |r|) in fp32.
"""
import numpy as np
import pytest

from conftest import XML
from reference_motion_cases import KEY_DT, NQ, NV, PROBE_NAMES, probe_expected, probe_registry, reference

pytestmark = pytest.mark.gpu

REG = probe_registry()


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


def _near_default(model, K, seed=5, spread=0.15):
    """K states near the reference's own start pose: joint angles and velocities perturbed, heights spread a little."""
    from mujocoposelearning_amd.initial_state import default_pose
    rng = np.random.default_rng(seed)
    q = np.tile(default_pose(model), (K, 1))
    q[:, 7:] += rng.uniform(-spread, spread, size=(K, NQ - 7))
    q[:, 2] += rng.uniform(-0.02, 0.02, size=K)
    q[:, :2] += rng.uniform(-0.05, 0.05, size=(K, 2))
    v = rng.uniform(-0.2, 0.2, size=(K, NV))
    return q, v


# ------------------------------------------------------------------ 1. sampling
@pytest.mark.parametrize("end", ["hold", "loop"])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_sampling_equals_the_numpy_restatement_bitwise(model, precision, end):
    """130 envs: two full waves and a 2-lane tail.  Finite times over boundaries, interiors and beyond the end."""
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd import reference_motion as rm
    n, K = 130, 7
    b = HsBatch(model, n, precision=precision, seed=3)
    ref = b.set_reference_motion(reference(K, end))
    assert b.reference_motion is ref and ref.K == K and np.allclose(ref.qpos, reference(K, end).qpos, rtol=1e-15)
    last = (K - 1) * KEY_DT
    rng = np.random.default_rng(0)
    t = np.concatenate([np.arange(K + 3) * KEY_DT, [0.5 * KEY_DT, last - 1e-7, last + 1e-7, 2.5 * last, 123.456],
                        rng.uniform(0, 1.3 * last, n)])[:n]
    b.set_state(time=t)
    held = b.time.cpu().numpy()                                  # the times as the batch holds them
    T = held.dtype.type
    r, comp = b.compute_reward("ref_probe", registry=REG, components=True)
    q, v = rm.sample(ref, held, dtype=T)
    want = probe_expected(q, v)
    comp = comp.cpu().numpy()
    assert comp.dtype == T and comp.shape == (16, n)
    for c, name in enumerate(PROBE_NAMES):
        assert np.array_equal(comp[c].view(np.uint8), want[c].view(np.uint8)), (name, np.flatnonzero(comp[c] != want[c])[:8])
    assert np.array_equal(r.cpu().numpy(), want[-1])
    x = b.reference_phase()
    assert x.shape == (n,) and (x[:K] == np.arange(K)).all()
    assert (x.max() <= K - 1) if end == "hold" else (x.max() > K)
    b.close()


# ------------------------------------------------------------------ 2. the step path across resets
@pytest.fixture()
def step_probe():
    from mujocoposelearning_amd import reward_functions as rf
    from mujocoposelearning_amd import reward_program as rw
    rw.register_device_reward("ref_step_probe", lambda d, p: d.ref_qpos[2] + d.ref_qvel[0])
    yield "ref_step_probe"
    del rf.REWARD_FUNCTIONS["ref_step_probe"]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_step_rewards_follow_the_reference_across_auto_resets(model, step_probe, precision):
    """67 envs, a bank of 5 initial states that is also the reference (start 'drawn'), 6-step episodes, 20 steps:
    every step's reward is the sample at the env's pre-reset (episode, time), bitwise."""
    import torch
    from mujocoposelearning_amd import reference_motion as rm
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    n, K, fs = 67, 5, 5
    h = float(model.opt.timestep)
    cfg = {"model_path": XML, "frame_skip": fs, "duration": h * (1 + 5.5 * fs), "reward_config": {"type": step_probe},
           "initial_state": {"states": _near_default(model, K)},
           "reference_motion": {"from_initial_state": True, "key_dt": 0.05}}
    env = HumanoidVecEnv(cfg, n_envs=n, model=model, seed=21, precision=precision)
    b = env.batch
    ref = b.reference_motion
    assert env.episode_length() == 6 and (ref.K, ref.start) == (K, "drawn") and env.rollout_handle() is None
    assert np.array_equal(ref.qpos, b.initial_states[0]) and np.array_equal(ref.qvel, b.initial_states[1])
    env.reset_tensors()
    T = np.float64 if precision == "fp64" else np.float32
    seed = b._group_seed(0)
    rng = np.random.default_rng(2)
    rows_seen = set()
    for k in range(20):
        t0, ep0 = b.time.cpu().numpy(), b.episode.cpu().numpy()
        j0 = b.initial_state_index()                              # the row each current episode started from
        assert (j0 >= 0).all() and np.array_equal(rm.start_rows(ref, n, ep0, seed), j0)
        a = torch.tensor(rng.uniform(-1, 1, (n, 21)), dtype=torch.float32, device=env.device)
        _, rew, term, trunc = env.step_tensors(a)
        done = ((term != 0) | (trunc != 0)).cpu().numpy()
        # the pre-reset time: the kernel adds the timestep once per substep, in the batch dtype
        t1 = t0.copy()
        for _ in range(fs):
            t1 = t1 + T(h)
        now = b.time.cpu().numpy()
        assert np.array_equal(now[~done], t1[~done]) and (now[done] == T(h)).all()
        q, v = rm.sample(ref, t1, ep0, seed, dtype=T)
        want = q[:, 2] + v[:, 0]
        got = rew.cpu().numpy()
        assert got.dtype == T and np.array_equal(got, want), (k, np.flatnonzero(got != want)[:8])
        rows_seen |= set(j0.tolist())
    assert int(b.episode.min()) >= 3                              # the reset() and at least two auto-resets each
    assert len(rows_seen) == K
    env.close()


# ------------------------------------------------------------------ 3. "track" on the device
def _track_env(model, n, precision, K=4, duration=15, seed=4):
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    cfg = {"model_path": XML, "duration": duration, "reward_config": {"type": "track"},
           "initial_state": {"states": _near_default(model, K)},
           "reference_motion": {"from_initial_state": True, "key_dt": 0.04, "end": "loop"}}
    return HumanoidVecEnv(cfg, n_envs=n, model=model, seed=seed, precision=precision)


def _track_host(env, state=None, motion=None, params=None):
    """"track" on the host interpreter for the env batch's current states: (reward [n], components [4, n])."""
    from mujocoposelearning_amd import reward_program as rw
    b = env.batch
    st = b.get_state() if state is None else state
    refd = {"motion": motion or b.reference_motion, "episode": b.episode.cpu().numpy(), "seed": b._group_seed(0),
            "dtype": np.float64 if b.precision == "fp64" else np.float32}
    c = rw.device_reward_program("track").compile(env.model)
    return c.eval_host({k: st[k] for k in ("qpos", "qvel", "time")}, params, components=True, reference=refd)


def _assert_at_the_bar(got, want, precision, what):
    assert np.isfinite(want).all() and np.isfinite(got).all()
    if precision == "fp64":
        err = np.abs(got - want) / np.abs(want).clip(1e-300)
        print(f"{what} fp64: max rel {err.max():.2e}")
        assert err.max() <= 1e-12, what
    else:
        err = np.abs(got - want) / (1 + np.abs(want))
        print(f"{what} fp32: max {err.max():.2e} of (1 + |r|)")
        assert err.max() <= 2e-6, what


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_track_on_the_device_agrees_with_the_host_interpreter(model, precision):
    import torch
    n = 70
    env = _track_env(model, n, precision)
    assert env.reward_component_names == ("pose", "velocity", "root", "total") and env.rollout_handle() is None
    env.reset()
    rng = np.random.default_rng(8)
    for k in range(4):
        env.step_async(rng.uniform(-1, 1, (n, 21)).astype(np.float32))
        obs, rew, dones, infos = env.step_wait()
    assert not dones.any()
    assert list(infos[0]["reward_components"]) == ["pose", "velocity", "root", "total"]
    assert infos[3]["reward_components"]["total"] == rew[3]
    want, wcomp = _track_host(env)
    _assert_at_the_bar(rew, want, precision, "track step reward")
    assert want.min() > 1e-3 and want.max() - want.min() > 1e-3          # neither vanished nor saturated
    for params in (None, {"k_pose": 0.5, "w_vel": 0.3}):
        r, comp = env.batch.compute_reward("track", params, components=True)
        want, wcomp = _track_host(env, params=params)
        _assert_at_the_bar(r.double().cpu().numpy(), want, precision, "track")
        for c, name in enumerate(("pose", "velocity", "root", "total")):
            _assert_at_the_bar(comp[c].double().cpu().numpy(), wcomp[c], precision, name)
    assert torch.equal(r, comp[3])
    env.close()


def test_off_track_ends_episodes_on_the_device(model):
    """The termination twin: an env pushed off the reference's root ends its episode, the others do not."""
    import torch
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    n = 8
    cfg = {"model_path": XML, "reward_config": {"type": "stand"},
           "reference_motion": {"states": _near_default(model, 3), "key_dt": 0.05},
           "termination": {"type": "off_track", "params": {"max_root_dist": 0.4}, "grace_steps": 2}}
    env = HumanoidVecEnv(cfg, n_envs=n, model=model, seed=1, precision="fp64")
    env.reset_tensors()
    q = env.batch.get_state()["qpos"]
    q[5, 0] += 1.0                                                # env 5: a metre off the track
    env.batch.set_state(qpos=q)
    zero = torch.zeros(n, 21, device=env.device)
    _, _, term, _ = env.step_tensors(zero)
    assert not term.any() and env.batch.grace_counts().tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    _, _, term, _ = env.step_tensors(zero)
    assert term.cpu().numpy().tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    assert env.batch.early_terminated.cpu().numpy().tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    env.close()


def test_single_env_runs_the_numeric_twins_on_its_data_view(model):
    """HumanoidEnv: the data view carries ref_qpos / ref_qvel (reference_motion.sample), so "track" runs as its
    numeric twin and agrees with the device program on the same state; "off_track" is evaluated on the device."""
    from mujocoposelearning_amd import reference_motion as rm
    from mujocoposelearning_amd.env import HumanoidEnv
    cfg = {"model_path": XML, "reward_config": {"type": "track"}, "initial_state": {"states": _near_default(model, 3)},
           "reference_motion": {"from_initial_state": True, "key_dt": 0.04},
           "termination": {"type": "off_track", "params": {"max_root_dist": 5.0}}}
    env = HumanoidEnv(cfg)
    env.reset(seed=3)
    rng = np.random.default_rng(1)
    for _ in range(3):
        _, reward, terminated, truncated, info = env.step(rng.uniform(-1, 1, 21).astype(np.float32))
    assert not terminated and not truncated and info["early_termination"] is False
    assert list(info["reward_components"]) == ["pose", "velocity", "root", "total"]
    assert info["reward_components"]["total"] == reward and 0.0 < reward < 1.0
    b = env._batch
    q, v = rm.sample(b.reference_motion, b.time.cpu().numpy(), b.episode.cpu().numpy(), b._group_seed(0))
    assert np.array_equal(env.data.ref_qpos, q[0]) and np.array_equal(env.data.ref_qvel, v[0])
    dev = b.compute_reward("track")
    _assert_at_the_bar(dev.cpu().numpy(), np.array([reward]), "fp64", "single env track")
    env.close()


# ------------------------------------------------------------------ 4. graph recapture
def test_ppo_records_its_rollout_again_after_a_rebind(model):
    """PPO with "track" collects on its captured per-step path; a rebind to a larger bank (new device blocks) moves
    launch_generation, the graph is recorded again, and the next rollout's rewards follow the new bank."""
    import warnings

    import torch
    from mujocoposelearning_amd import reference_motion as rm
    from mujocoposelearning_amd.ppo import PPO
    from test_gpu_rollout import _copy_env
    n, T = 64, 8
    env, twin = _track_env(model, n, "fp32"), _track_env(model, n, "fp32")
    ppo = PPO(env, n_steps=T, batch_size=n, n_epochs=1, seed=0, stagger_episodes=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ppo.learn(n * T)
    assert ppo._fused_rollout_args() is None and ppo._rollout_graph is not None
    gen0 = env.batch.launch_generation
    assert ppo._rollout_graph_gen == gen0
    old = env.batch.reference_motion
    q, v = _near_default(model, 9, seed=77, spread=0.3)
    new = rm.Reference(q, v, key_dt=0.03, end="hold", start="zero")
    for e in (env, twin):
        e.batch.set_reference_motion(new)
    assert env.batch.launch_generation == gen0 + 1
    _copy_env(env, twin)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ppo.learn(2 * n * T)
    torch.cuda.synchronize()
    assert ppo._rollout_graph is not None and ppo._rollout_graph_gen == gen0 + 1      # the recapture happened
    b = ppo.buf
    moved = 0.0
    for t in range(T):
        twin.step_tensors(b["act"][t].clamp(-1, 1))
        assert not bool(b["done"][t].any())
        st = twin.batch.get_state()
        want, _ = _track_host(twin, st)
        got = b["rew"][t].double().cpu().numpy()
        _assert_at_the_bar(got, want, "fp32", f"rollout step {t}")
        stale, _ = _track_host(twin, st, motion=old)
        moved = max(moved, float(np.abs(want - stale).max()))
    assert moved > 1e-2                                           # the old bank would have given other rewards
    env.close()
    twin.close()


# ------------------------------------------------------------------ 5. a reference bound but unread
def test_a_reference_nobody_reads_changes_nothing(model):
    import torch
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    n = 16
    cfg = {"model_path": XML, "reward_config": {"type": "stand"}}
    a = HumanoidVecEnv(cfg, n_envs=n, model=model, seed=9, precision="fp64")
    b = HumanoidVecEnv(dict(cfg, reference_motion={"states": _near_default(model, 6), "key_dt": 0.1, "end": "loop"}),
                       n_envs=n, model=model, seed=9, precision="fp64")
    assert b.batch.reference_motion.K == 6 and a.batch.reference_motion is None
    assert a.rollout_handle() is not None and b.rollout_handle() is not None and b._program is None
    assert torch.equal(a.reset_tensors(), b.reset_tensors())
    rng = np.random.default_rng(3)
    for k in range(5):
        act = torch.tensor(rng.uniform(-1, 1, (n, 21)), dtype=torch.float32, device=a.device)
        ra, rb = a.step_tensors(act), b.step_tensors(act)
        for x, y in zip(ra, rb):
            assert torch.equal(x, y), k
    a.close()
    b.close()


# ------------------------------------------------------------------ refusals that need a batch
def test_launch_refusals_and_rebinding(model):
    from mujocoposelearning_amd._lib import HsimError
    from mujocoposelearning_amd.batch import HsBatch
    b = HsBatch(model, 8, precision="fp64")
    with pytest.raises(HsimError, match="hs_reward_program_batch: the program reads ref_qpos, but the batch has no "
                                        "reference motion bound"):
        b.compute_reward("ref_probe", registry=REG)
    prog = b.compile_reward("ref_probe", REG)
    import torch
    zero = torch.zeros(8, 21, device=b.device)
    ep = b.episode.clone()
    with pytest.raises(HsimError, match="hs_step_program: the program reads ref_qpos, but the batch has no reference"):
        b.step_program(zero, prog)
    assert torch.equal(b.episode, ep) and float(b.time.abs().max()) == 0.0      # refused before any launch
    with pytest.raises(HsimError, match="hs_set_termination: the program reads ref_qpos"):
        b.set_termination("off_track")
    b.set_reference_motion(reference(5, start="drawn"))
    with pytest.raises(HsimError, match="HS_REF_START_DRAWN.*same 5 rows.*none is bound"):
        b.compute_reward("ref_probe", registry=REG)
    b.set_initial_states(*_near_default(model, 4))
    with pytest.raises(HsimError, match="HS_REF_START_DRAWN.*same 5 rows.*the bank bound has 4"):
        b.compute_reward("ref_probe", registry=REG)
    b.set_initial_states(*_near_default(model, 5))
    b.compute_reward("ref_probe", registry=REG)
    gen = b.launch_generation
    b.set_reference_motion(None)
    assert b.reference_motion is None and b.launch_generation == gen + 1
    with pytest.raises(HsimError, match="no reference motion bound"):
        b.compute_reward("ref_probe", registry=REG)
    with pytest.raises(HsimError, match=r"rows must be \[K, 28\]"):
        b.set_reference_motion(np.ones((2, 27)), None, key_dt=0.1)
    with pytest.raises(ValueError, match="key_dt .* is required"):
        b.set_reference_motion(np.ones((2, 28)))
    with pytest.raises(HsimError, match="reference_phase: the batch has no reference motion bound"):
        b.reference_phase()
    b.close()
