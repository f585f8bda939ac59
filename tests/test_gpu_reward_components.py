"""Named reward components on the device (csrc/hs_reward_prog.hip RP_OUT and the outcome launch's component
rows; HsBatch, HumanoidVecEnv / StepInfos, HumanoidEnv, PPO).

Shapes: N = 65 -- two waves, one live lane in the second, so 63 lanes mirror the last env and must store
nothing -- and N = 1; fp64 and fp32.  Non-outcome mode: every row of the component block equals, bit for bit,
the device's own evaluation of a scalar program returning that expression alone (the same kernel, ops and
association).  Outcome mode: the step's components, the episode sums with their episode tag, the terminal sums,
and the zeroing on a truncated step, over episodes of three env steps.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import XML
from reward_component_cases import BREAKDOWNS, EDGE, registry

pytestmark = pytest.mark.gpu

REG = registry()
SENTINEL = -12345.678
STAND = ("velocity", "posture", "foot", "torque", "total")


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


def _same_bits(a, b):
    """Bitwise equal tensors of one float dtype, NaN positions included."""
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    na, nb = a.isnan(), b.isnan()
    return bool(torch.equal(na, nb) and torch.equal(a[~na].view(it), b[~nb].view(it)))


_STATES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_shared_batches():
    yield
    for b in _STATES.values():
        b.close()
    _STATES.clear()


def _stepped_batch(model, precision, n, full_state=False):
    """A batch one random-action step after its reset, shared by the non-outcome cases (they change no state)."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    key = (precision, n, full_state)
    if key not in _STATES:
        b = HsBatch(model, n, precision=precision, seed=17, full_state=full_state)
        b.configure(frame_skip=3, duration=10.0, reward_id=-1, autoreset=1)
        b.reset()
        rng = np.random.default_rng(3)
        b.step(torch.tensor(rng.uniform(-1, 1, (n, model.nu)), dtype=torch.float32, device=b.device))
        _STATES[key] = b
    return _STATES[key]


# -- non-outcome mode ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name", sorted(n for n in EDGE if n != "contact_forces") + ["stand_components"])
def test_component_rows_equal_the_scalar_programs_bitwise(model, name, precision, n):
    import torch
    from mujocoposelearning_amd import _lib
    b = _stepped_batch(model, precision, n)
    _check_rows(b, name, torch, _lib)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_component_rows_of_a_program_reading_cfrc_ext(model, precision):
    import torch
    from mujocoposelearning_amd import _lib
    b = _stepped_batch(model, precision, 65, full_state=True)
    rows = _check_rows(b, "contact_forces", torch, _lib)
    # the rows are the batch's own cfrc_ext, summed as rw.sum orders six terms: sequentially from 0
    for row, body in ((rows[0], 9), (rows[1], 6)):
        acc = torch.zeros(b.n, dtype=b.dtype, device=b.device)
        for j in range(6):
            acc = acc + b.cfrc_ext[:, body, j].abs()
        assert _same_bits(row, acc), body
    print(f"contact_forces {precision}: {int((rows[:2] != 0).sum())} non-zero foot forces of {2 * b.n}")


def _check_rows(b, name, torch, _lib):
    prog = b.compile_reward(name, REG)
    c, n = len(prog.outputs), b.n
    comp = torch.full((c + 1, n), SENTINEL, dtype=b.dtype, device=b.device)
    out = torch.full((n,), SENTINEL, dtype=b.dtype, device=b.device)
    _lib.check(_lib.lib().hs_reward_program_batch_components(b._h, prog.handle, prog.params(None), out.data_ptr(),
                                                             comp.data_ptr(), b.stream))
    sentinel = torch.tensor(SENTINEL, dtype=b.dtype, device=b.device)
    assert bool((comp[c] == sentinel).all()), "a row past the last component was written"
    if c == 1:
        assert not bool((comp[:c] == sentinel).any())
    for k, key in enumerate(prog.outputs):
        single = b.compute_reward(f"{name}/{key}", registry=REG)
        assert _same_bits(comp[k], single), (name, key)
    assert _same_bits(out, b.compute_reward(f"{name}/total", registry=REG))
    # the Python surface: the same launch, exactly C rows
    r2, c2 = b.compute_reward(name, registry=REG, components=True)
    assert _same_bits(r2, out) and _same_bits(c2, comp[:c])
    # and with no sink the program is the scalar program: out is written, nothing else is touched
    assert _same_bits(b.compute_reward(name, registry=REG), out)
    return comp[:c]


# -- outcome mode ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_step_program_components_sums_and_truncation(model, precision):
    """max_steps = 3: every env truncates at env step 3 and auto-resets; 5 steps of zero actions."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    n = 65
    b = HsBatch(model, n, precision=precision, seed=5)
    b.configure(frame_skip=3, duration=10.0, max_steps=3, reward_id=-1, autoreset=1)
    b.reset()
    ep0 = b.episode.clone()
    prog = b.compile_reward("stand_components", REG)
    assert prog.outputs == STAND and b.reward_component_names == ()
    with pytest.raises(AttributeError):
        b.reward_components
    a = torch.zeros(n, model.nu, device=b.device)
    ti = STAND.index("total")
    sums = torch.zeros(len(STAND), n, dtype=b.dtype, device=b.device)
    for step in range(1, 6):
        b.step_program(a, prog)
        comp, tot, term = b.reward_components, b.total_reward_components, b.terminal_total_reward_components
        assert b.reward_component_names == STAND and comp.shape == (5, n) and comp.dtype == b.dtype
        if step == 3:
            assert b.truncated.all() and not b.terminated.any()
            assert bool((comp == 0).all()) and bool((b.reward == 0).all())
            assert _same_bits(tot, sums + 0) and _same_bits(term, sums)       # the step-2 sums + 0
            assert _same_bits(term[ti], b.terminal_total_reward) and bool((term[ti] != 0).all())
            sums.zero_()
            continue
        assert not b.truncated.any() and not b.terminated.any()
        # the post-step state is the current state (no reset happened): the non-outcome evaluation of it
        r, c = b.compute_reward("stand_components", registry=REG, components=True)
        assert _same_bits(comp, c) and _same_bits(b.reward, r) and _same_bits(comp[ti], b.reward)
        sums = sums + comp                         # the sequential sum in T; at step 4 from this step's value alone
        assert _same_bits(tot, sums), step
        assert _same_bits(tot[ti], b.total_reward)
        if step < 3:
            assert bool((term == 0).all())         # nobody has finished yet
    assert bool((b.episode == ep0 + 1).all()) and bool((b.reward_components != 0).any())    # one auto-reset each
    b.close()


def test_early_termination_writes_the_terminal_sums_on_that_step(model):
    """termination "fallen" with min_height 1.3: the envs left at the reset height (1.282) end at step 1, the
    ones lifted to 1.35 do not."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    n = 65
    b = HsBatch(model, n, precision="fp64", seed=9)
    b.configure(frame_skip=3, duration=10.0, reward_id=-1, autoreset=1)
    b.reset()
    q = b.get_state()["qpos"]
    q[0::2, 2] = 1.35
    b.set_state(qpos=q)
    b.set_termination("fallen", params={"min_height": 1.3})
    prog = b.compile_reward("stand_components", REG)
    a = torch.zeros(n, model.nu, device=b.device)
    low = torch.zeros(n, dtype=torch.bool, device=b.device)
    low[1::2] = True
    b.step_program(a, prog)
    assert torch.equal(b.terminated != 0, low) and torch.equal(b.early_terminated != 0, low)
    c1 = b.reward_components.clone()
    assert bool((c1[:, low] != 0).any())                                        # an early end is rewarded as usual
    assert _same_bits(b.terminal_total_reward_components[:, low], c1[:, low])
    assert bool((b.terminal_total_reward_components[:, ~low] == 0).all())
    assert _same_bits(b.terminal_total_reward_components[4], b.terminal_total_reward)
    b.set_termination(None)
    b.step_program(a, prog)
    c2 = b.reward_components
    assert _same_bits(b.total_reward_components[:, low], c2[:, low])           # a new episode: this step alone
    assert _same_bits(b.total_reward_components[:, ~low], (c1 + c2)[:, ~low])
    b.close()


def test_output_count_mismatch_is_refused_before_the_step(model):
    import torch
    from mujocoposelearning_amd import _lib
    from mujocoposelearning_amd.batch import HsBatch
    L = _lib.lib()
    n = 8
    b = HsBatch(model, n, precision="fp64", seed=1)
    b.configure(frame_skip=3, duration=10.0, reward_id=-1, autoreset=1)
    b.reset()
    a = torch.zeros(n, model.nu, device=b.device)
    b.step_program(a, b.compile_reward("stand_components", REG))
    before = {k: b.t[k].clone() for k in ("step_count", "qpos", "reward")}
    comp = b.reward_components.clone()
    for name, count in (("shared_node", 2), ("stand_components/total", 0)):
        with pytest.raises(_lib.HsimError, match=f"the program has {count} outputs, the batch has 5 component rows"):
            b.step_program(a, b.compile_reward(name, REG))
        assert all(torch.equal(b.t[k], v) for k, v in before.items()) and torch.equal(b.reward_components, comp)
    # hs_set_reward_components checks its arguments
    p = comp.data_ptr()
    assert L.hs_set_reward_components(b._h, 17, p, p, p, p) < 0 and b"outside [0, 16]" in L.hs_last_error()
    assert L.hs_set_reward_components(b._h, -1, p, p, p, p) < 0
    assert L.hs_set_reward_components(b._h, 5, p, None, p, p) < 0 and b"all four buffers" in L.hs_last_error()
    # unbound, a scalar program steps again
    b.bind_reward_components(())
    assert b.reward_component_names == ()
    b.step_program(a, b.compile_reward("stand_components/total", REG))
    assert bool((b.step_count == before["step_count"] + 1).all())
    b.close()


# -- HumanoidVecEnv, HumanoidEnv, PPO -------------------------------------------------------------------
CFG = {"model_path": XML, "duration": 0.045, "frame_skip": 3}      # episodes of three env steps


def _vec_env(model, components, n=65, seed=4):
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    rc = {"type": "stand", "components": True} if components else {"type": "stand"}
    return HumanoidVecEnv(dict(CFG, reward_config=rc), n_envs=n, model=model, seed=seed, precision="fp64")


def test_vec_env_infos_carry_the_components(model):
    n = 65
    e0, e1 = _vec_env(model, False), _vec_env(model, True)
    assert e1.episode_length() == 3 and e1.reward_component_names == STAND and e0.reward_component_names == ()
    assert e0.terminal_total_reward_components is None and e1.rollout_handle() is None
    assert np.array_equal(e0.reset(), e1.reset())
    rng = np.random.default_rng(8)
    finished = 0
    for step in range(4):
        act = rng.uniform(-1, 1, (n, model.nu)).astype(np.float32)
        for e in (e0, e1):
            e.step_async(act)
        o0, r0, d0, i0 = e0.step_wait()
        o1, r1, d1, i1 = e1.step_wait()
        # the built-in path and the program path agree bitwise
        assert np.array_equal(o0, o1) and np.array_equal(r0, r1) and np.array_equal(d0, d1)
        comp = e1.batch.reward_components.cpu().numpy()
        term = e1.batch.terminal_total_reward_components.cpu().numpy()
        assert i1._cache is None                                        # nothing is built until somebody reads
        for i in range(n):
            assert i0[i]["reward_components"] == {} and "episode_reward_components" not in i0[i]
            assert i1[i]["reward_components"] == {k: float(comp[c, i]) for c, k in enumerate(STAND)}
            assert i1[i]["reward_components"]["total"] == r1[i]
            assert [k for k in i1[i] if k != "episode_reward_components"] == list(i0[i])
            if d1[i]:
                assert i1[i]["episode_reward_components"] == {k: float(term[c, i]) for c, k in enumerate(STAND)}
                assert i1[i]["episode_reward_components"]["total"] == i1[i]["total_reward"]
                finished += 1
            else:
                assert "episode_reward_components" not in i1[i]
        assert d1.all() == (step == 2)
    assert finished == n
    e0.close()
    e1.close()


def test_single_env_fills_reward_components(model):
    """HumanoidEnv (a GPU batch of one env, the reward's numeric twin on the host): the CPU suite constructs no
    such env, so the case lives here."""
    from mujocoposelearning_amd.env import HumanoidEnv
    cfg = dict(CFG, duration=10.0)
    e0 = HumanoidEnv(dict(cfg, reward_config={"type": "stand"}))
    e1 = HumanoidEnv(dict(cfg, reward_config={"type": "stand", "components": True}))
    e0.reset(seed=3)
    _, info = e1.reset(seed=3)
    assert list(info["reward_components"]) == ["forward", "standing", "healthy_pose", "alive", "total"]   # the reference's
    act = np.random.default_rng(0).uniform(-1, 1, model.nu).astype(np.float32)
    _, r0, *_ = e0.step(act)
    _, r1, _, _, info = e1.step(act)
    rc = info["reward_components"]
    assert list(rc) == list(STAND) and all(isinstance(v, float) for v in rc.values())
    assert rc["total"] == r1 and r1 != 0
    # the twin (numpy's libm) against the step kernel's reward (the device's): the 1e-12 relative this suite holds
    # a program's fp64 device value to against its twin (tests/test_gpu_reward_program.py)
    assert abs(r1 - r0) <= 1e-12 * abs(r0)
    assert rc["total"] == 0.4 * rc["velocity"] + 0.3 * rc["posture"] + 0.2 * rc["foot"] + 0.1 * rc["torque"]
    e1._batch.configure(max_steps=2)                  # the next step truncates: every component is 0, as the reward
    _, r2, term, trunc, info = e1.step(act)
    assert trunc and r2 == 0.0 and info["reward_components"] == {k: 0.0 for k in STAND}
    e0.close()
    e1.close()


def test_ppo_logs_the_component_means(model):
    import torch
    from mujocoposelearning_amd.ppo import PPO
    n, t = 65, 4
    env = _vec_env(model, True, seed=6)
    ppo = PPO(env, n_steps=t, batch_size=n, n_epochs=1, seed=0, stagger_episodes=False)
    assert ppo.buf["epcomp"].shape == (t, 5, n)
    ppo.collect_rollouts()
    assert len(ppo.ep_returns) == n == len(ppo.ep_components)         # every env finished its 3-step episode once
    ppo.learn(ppo.num_timesteps + t * n)                              # one more iteration
    torch.cuda.synchronize()
    means = ppo.logger["ep_components_mean"]
    assert list(means) == list(STAND) and all(np.isfinite(v) for v in means.values())
    m = ppo.logger["ep_rew_mean"]
    # ep_acc is float64 and adds each step's reward AFTER its rounding to float32 (rew.float() in the rollout
    # body), the component sums add the fp64 rewards themselves: per episode they differ by at most
    # sum |r_t| * 2^-24, and the stand reward is in [0, 1], so sum |r_t| is the return itself; 2^-40 covers the
    # float64 roundings of the sums and of the two means over <= 100 episodes
    bound = abs(m) * (2.0 ** -24 + 2.0 ** -40)
    print(f"ep_components_mean total {means['total']!r} vs ep_rew_mean {m!r}: |diff| {abs(means['total'] - m):.3e}, "
          f"bound {bound:.3e}")
    assert abs(means["total"] - m) <= bound
    # an env without components: nothing allocated, nothing logged
    env0 = _vec_env(model, False, seed=6)
    p0 = PPO(env0, n_steps=t, batch_size=n, n_epochs=1, seed=0, stagger_episodes=False)
    assert "epcomp" not in p0.buf and p0._comp_names == ()
    p0.learn(t * n)
    assert "ep_components_mean" not in p0.logger
    env.close()
    env0.close()
