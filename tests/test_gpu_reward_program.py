"""Reward programs on the device (csrc/hs_reward_prog.hip reward_program_kernel, hs_step_program).

One formula, two paths: the three built-in rewards restated in the language (reward_program.py) and traced to
programs must equal the built-in ids -- the step kernel's reward_formula, which holds the <= 2 ulp bar against
the reference -- BITWISE, in fp64 and fp32: on the 203 golden states through reward_eval, and as whole env
steps (obs, reward, flags, terminal rows, counters) across auto-resets and the truncation branch.  A program
that is not a built-in is checked against its numeric twin: fp64 to 1e-12 relative (a wrong operand, op or
summation order shows at 1e-6 and above; the device libm was measured at <= 2 ulp per built-in), fp32 to the
project's 2e-6 (1 + |r|).
"""
import numpy as np
import pytest

from conftest import XML
from reward_program_cases import FIELDS, KNEEL_OVERRIDES, N, bits_equal, example_reward, registry, twin_values

pytestmark = pytest.mark.gpu

REG = registry()
CFG = {"model_path": XML, "duration": 0.1, "frame_skip": 3}


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


@pytest.fixture()
def registered():
    """The restated stand reward and the example in the global registry (what HumanoidVecEnv reads): the
    example twice, as a program and -- the same twin behind a plain function -- as a host callable."""
    from mujocoposelearning_amd import reward_functions as rf
    from mujocoposelearning_amd import reward_program as rw
    from reward_program_cases import EXAMPLE_DEFAULTS
    rw.register_device_reward("stand_program", rw.stand_program)
    rw.register_device_reward("example", example_reward, defaults=EXAMPLE_DEFAULTS)
    twin = rf.REWARD_FUNCTIONS["example"]
    rf.REWARD_FUNCTIONS["example_host"] = lambda data, params=None: twin(data, params)
    yield
    for k in ("stand_program", "example", "example_host"):
        del rf.REWARD_FUNCTIONS[k]


def _tensors(dtype):
    import torch
    d = torch.device("cuda", 0)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=d)  # noqa: E731
    G = FIELDS
    args = [t(G["qpos"]), t(G["qvel"]), t(G["ctrl"]), t(G["time"]), t(G["subtree_com"][:, 0]),
            t(G["subtree_linvel"][:, 0]), t(G["cfrc_ext"]), t(G["qfrc_actuator"])]
    return args, dict(cinert=t(G["cinert"]), cvel=t(G["cvel"]))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name,params", [("stand", None), ("walk", None), ("kneeling", None),
                                         ("kneeling", KNEEL_OVERRIDES)],
                         ids=["stand", "walk", "kneeling", "kneeling_overrides"])
def test_restated_builtin_programs_equal_the_builtin_ids_bitwise(model, name, params, precision):
    import torch
    from mujocoposelearning_amd.batch import reward_eval
    dt = torch.float64 if precision == "fp64" else torch.float32
    args, _ = _tensors(dt)
    a = reward_eval(model, name, *args, params=params, registry=REG)
    b = reward_eval(model, name + "_program", *args, params=params, registry=REG)
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    print(f"{name} {precision}: {int(same.sum())}/{N} bitwise, {int(np.isnan(a).sum())} NaN")
    assert np.isfinite(a).sum() > 190
    assert bits_equal(a, b), np.flatnonzero(~same)[:10]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_example_program_on_the_device_agrees_with_its_twin(model, precision):
    import torch
    from mujocoposelearning_amd.batch import reward_eval
    dt = torch.float64 if precision == "fp64" else torch.float32
    args, extra = _tensors(dt)
    for params in (None, {"target": 0.9, "w_effort": 0.2}):
        twin = twin_values(REG, "example", params)
        r = reward_eval(model, "example", *args, params=params, registry=REG, **extra).double().cpu().numpy()
        assert np.isfinite(twin).all() and np.isfinite(r).all()
        if precision == "fp64":
            rel = np.abs(r - twin) / np.abs(twin)
            print(f"example fp64: max rel {rel.max():.2e}")
            assert rel.max() <= 1e-12
        else:
            err = np.abs(r - twin) / (1 + np.abs(twin))
            print(f"example fp32: max {err.max():.2e} of (1 + |r|)")
            assert err.max() <= 2e-6
    with pytest.raises(ValueError, match="reads cvel"):
        reward_eval(model, "example", *args, registry=REG, cinert=extra["cinert"])


def _snapshot(env):
    b = env.batch
    keys = ("obs", "reward", "terminated", "truncated", "terminal_obs", "total_reward", "step_count", "episode",
            "terminal_step_count", "terminal_total_reward", "qpos", "qvel", "time")
    return {k: b.t[k].clone() for k in keys}


def _assert_same(s1, s2, step, skip=()):
    import torch
    for k in s1:
        if k not in skip:
            assert torch.equal(s1[k], s2[k]), (step, k, (s1[k].double() - s2[k].double()).abs().max().item())


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_env_steps_with_the_stand_program_equal_the_builtin_path_bitwise(model, registered, precision):
    """64 envs, duration 0.1 s: episodes end at step 7, so 20 steps cross two auto-resets."""
    import torch
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    n = 64
    e1 = HumanoidVecEnv(dict(CFG, reward_config={"type": "stand"}), n_envs=n, model=model, seed=11, precision=precision)
    e2 = HumanoidVecEnv(dict(CFG, reward_config={"type": "stand_program"}), n_envs=n, model=model, seed=11,
                        precision=precision)
    assert e2._program is not None and e2._host_reward is None
    assert torch.equal(e1.reset_tensors(), e2.reset_tensors())
    rng = np.random.default_rng(1)
    resets = 0
    for k in range(20):
        a = torch.tensor(rng.uniform(-1, 1, (n, 21)), dtype=torch.float32, device=e1.device)
        _, _, term, _ = e1.step_tensors(a)
        e2.step_tensors(a)
        _assert_same(_snapshot(e1), _snapshot(e2), k)
        resets += int(term.any())
    assert resets == 2 and (e1.batch.episode == e2.batch.episode).all() and int(e2.batch.episode.min()) >= 2
    assert bool((e2.batch.reward != 0).any())
    e1.close()
    e2.close()


def test_program_env_with_seeded_host_noise_streams_equals_the_builtin_path(model, registered):
    """After seed(s) (what SB3's PPO(seed=s) calls) env i's resets draw from np.random.RandomState(s + i) on the
    host: the program env then steps with auto-reset off and resets the finished envs itself, with the same
    draws the built-in env binds ahead of its in-kernel auto-reset.  Not graph-safe, as for built-ins."""
    import torch
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    n = 16
    e1 = HumanoidVecEnv(dict(CFG, reward_config={"type": "stand"}), n_envs=n, model=model, seed=0, precision="fp64")
    e2 = HumanoidVecEnv(dict(CFG, reward_config={"type": "stand_program"}), n_envs=n, model=model, seed=0,
                        precision="fp64")
    for e in (e1, e2):
        e.seed(100)
    assert not e2.graph_safe
    assert torch.equal(e1.reset_tensors(), e2.reset_tensors())
    assert not e2.graph_safe and e2.batch.cfg.autoreset == 1
    rng = np.random.default_rng(6)
    for k in range(16):
        a = torch.tensor(rng.uniform(-1, 1, (n, 21)), dtype=torch.float32, device=e1.device)
        e1.step_tensors(a)
        e2.step_tensors(a)
        _assert_same(_snapshot(e1), _snapshot(e2), k)
    assert int(e2.batch.episode.min()) >= 2 and e2.batch.cfg.autoreset == 1
    e1.close()
    e2.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_batch_step_program_truncation_branch_equals_the_builtin_path(model, precision):
    """max_steps = 4 with a duration beyond it: step 4 truncates -- reward 0 and the terminal rows."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    n = 64
    b1 = HsBatch(model, n, precision=precision, seed=3)
    b2 = HsBatch(model, n, precision=precision, seed=3)
    b1.configure(frame_skip=3, duration=10.0, max_steps=4, reward_id=0, autoreset=1)
    b2.configure(frame_skip=3, duration=10.0, max_steps=4, reward_id=-1, autoreset=1)
    prog = b2.compile_reward("stand_program", REG)
    b1.reset()
    b2.reset()
    rng = np.random.default_rng(2)
    keys = ("obs", "reward", "terminated", "truncated", "terminal_obs", "total_reward", "step_count", "episode",
            "terminal_step_count", "terminal_total_reward")
    for k in range(10):
        a = torch.tensor(rng.uniform(-1, 1, (n, 21)), dtype=torch.float32, device=b1.device)
        b1.step(a)
        b2.step_program(a, prog)
        for key in keys:
            assert torch.equal(b1.t[key], b2.t[key]), (k, key)
        if k in (3, 7):
            assert b2.truncated.all() and not b2.terminated.any() and (b2.reward == 0).all()
            assert (b2.terminal_step_count == 4).all() and (b2.terminal_total_reward != 0).all()
        else:
            assert not b2.truncated.any() and (b2.reward != 0).all()
    # auto-reset off: the finished envs stay where they are (the caller resets them)
    b2.configure(autoreset=0, max_steps=6)
    b2.step_program(a, prog)
    assert not b2.truncated.any() and (b2.step_count == 3).all()
    b1.close()
    b2.close()


def test_env_steps_with_a_program_equal_the_host_callable_path(model, registered):
    """The example reward registered twice: as a plain callable (the host path: fields copied out, one Python
    call per env, rewards copied back) and as a program.  Same states bitwise; rewards within the fp64 bound."""
    import torch
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    n = 64
    cfg = dict(CFG, reward_config={"type": "example", "params": {"w_effort": 0.1}})
    e1 = HumanoidVecEnv(dict(cfg, reward_config=dict(cfg["reward_config"], type="example_host")), n_envs=n, model=model,
                        seed=5, precision="fp64")
    e2 = HumanoidVecEnv(cfg, n_envs=n, model=model, seed=5, precision="fp64")
    assert e1._host_reward is not None and e2._host_reward is None and e2._program is not None
    assert torch.equal(e1.reset_tensors(), e2.reset_tensors())
    rng = np.random.default_rng(4)
    worst = 0.0
    for k in range(20):
        a = torch.tensor(rng.uniform(-1, 1, (n, 21)), dtype=torch.float32, device=e1.device)
        e1.step_tensors(a)
        e2.step_tensors(a)
        s1, s2 = _snapshot(e1), _snapshot(e2)
        _assert_same(s1, s2, k, skip=("reward", "total_reward", "terminal_total_reward"))
        for key in ("reward", "total_reward", "terminal_total_reward"):
            x, y = s1[key].cpu().numpy(), s2[key].cpu().numpy()
            rel = np.abs(x - y) / np.abs(x).clip(1e-300)
            worst = max(worst, float(rel[x != y].max(initial=0.0)))
    print(f"program vs host callable over 20 steps: max rel {worst:.2e}")
    assert worst <= 1e-12
    assert int(e2.batch.episode.min()) >= 2
    e1.close()
    e2.close()


def test_program_env_is_graph_safe_and_trains(model, registered):
    import torch
    from mujocoposelearning_amd.ppo import PPO
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    n = 64
    cfg = {"model_path": XML, "duration": 10.0, "frame_skip": 3, "reward_config": {"type": "example"}}
    env = HumanoidVecEnv(cfg, n_envs=n, model=model, seed=2, precision="fp64")
    assert env.graph_safe and env._host_reward is None and env.rollout_handle() is None
    assert env.required_outputs() == (False, False)
    env.batch.configure(aux=False, ctrl=False)         # what train_humanoid does for this program
    ppo = PPO(env, n_steps=8, batch_size=256, n_epochs=2, seed=0)
    ppo.collect_rollouts()                              # the first rollout
    rew = ppo.buf["rew"].clone()
    act = ppo.buf["act"].clamp(-1, 1).clone()
    assert not ppo.buf["done"].any()
    ppo.learn(2 * 8 * n)
    torch.cuda.synchronize()
    for k in ("policy_loss", "value_loss", "loss", "approx_kl", "entropy_loss"):
        assert np.isfinite(ppo.logger[k]), (k, ppo.logger[k])
    # the buffered rewards are the program's: a second, identically seeded env stepped by hand
    hand = HumanoidVecEnv(cfg, n_envs=n, model=model, seed=2, precision="fp64")
    hand.reset_tensors()
    for t in range(8):
        _, r, _, _ = hand.step_tensors(act[t])
        assert torch.equal(r.float(), rew[t]), t
    assert bool((rew != 0).all())
    env.close()
    hand.close()


def test_program_batch_refuses_without_the_outputs_it_reads(model):
    import torch
    from mujocoposelearning_amd import _lib
    from mujocoposelearning_amd.batch import HsBatch
    b = HsBatch(model, 8, precision="fp64", seed=1)
    b.configure(frame_skip=3, duration=10.0, reward_id=-1, autoreset=1, aux=False, ctrl=True)
    b.reset()
    a = torch.zeros(8, 21, device=b.device)
    kneel = b.compile_reward("kneeling_program", REG)       # reads subtree_com
    stand = b.compile_reward("stand_program", REG)          # does not
    before = b.step_count.clone()
    with pytest.raises(_lib.HsimError, match="subtree_com.*aux row"):
        b.step_program(a, kneel)
    assert torch.equal(b.step_count, before)                # refused before anything was launched
    b.step_program(a, stand)
    with pytest.raises(_lib.HsimError, match="subtree_com.*aux row"):
        b.compute_reward("kneeling_program", registry=REG)
    r = b.compute_reward("stand_program", registry=REG)
    assert torch.equal(r, b.reward) and torch.isfinite(r).all()
    b.configure(aux=True, ctrl=False)
    with pytest.raises(_lib.HsimError, match="reads ctrl"):
        b.step_program(a, stand)
    b.step_program(a, kneel)
    assert torch.isfinite(b.reward).all()
    assert torch.equal(b.compute_reward("kneeling_program", registry=REG), b.reward)
    b.close()
