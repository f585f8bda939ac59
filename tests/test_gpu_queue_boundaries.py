"""The chunk queue's item boundaries (hs_kernels.hip step_kernel_queue): a wave's
first item of a launch is item blockIdx.x, taken without the claim counter; later claims are
gridDim.x + the counter.  That only changes which wave runs which item when: every result stays
bitwise that of the direct schedule (one wave per pair), the counters are back at zero after every
launch, and the next launch finds a valid order.

Batches of 2 * resident_waves + 2 envs (and + 3: the last pair's upper half is a ghost), the
smallest that HS_SCHED_AUTO queues.  Envs end their episode in every step of the run: a pair with
both halves, one with only the lower half, one with only the upper half; the first pair (its lower
env in step 1, its upper env in step 2) and the last pair (steps T - 1 and T).
"""
import numpy as np
import pytest

from conftest import XML

pytestmark = pytest.mark.gpu

DT = 0.015          # one env step: frame_skip 3 x 0.005
T = 6               # env steps of the shared run
FIELDS = ("obs", "reward", "terminated", "truncated", "qpos", "qvel", "qacc_warmstart", "time", "step_count",
          "episode", "total_reward", "terminal_obs", "terminal_step_count", "terminal_total_reward", "warning")


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


@pytest.fixture(scope="module")
def resident(model):
    from mujocoposelearning_amd.batch import HsBatch
    b = HsBatch(model, 2, precision="fp64")
    r = b.resident_waves
    b.close()
    assert r > 0
    return r


def _batch(model, n, sched, seed=5):
    from mujocoposelearning_amd.batch import HsBatch
    b = HsBatch(model, n, precision="fp64", seed=seed)
    b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1, max_steps=750, schedule=sched)
    b.reset()
    return b


def _clock(step):
    """Episode clock, at the start of the run, of an env that terminates in its step `step`."""
    return 10.005 - DT * step


def _snap(b):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(b, k).clone() for k in FIELDS}


def _assert_equal(x, y, what):
    import torch
    for k in FIELDS:
        assert torch.equal(x[k], y[k]), f"{what}: {k} differs from the direct schedule"


def _plan(n, steps=T):
    """{step: envs that end their episode in it}."""
    npairs = (n + 1) // 2
    plan = {}
    for j in range(1, steps + 1):
        p = 1 + j * (npairs - 80) // (steps + 1)
        plan[j] = [2 * p, 2 * p + 1, 2 * (p + 37), 2 * (p + 61) + 1]
    plan[1] += [0]
    plan[2] += [1]
    last = 2 * (npairs - 1)
    if n % 2 == 0:
        plan[steps - 1] += [last]
        plan[steps] += [last + 1]
    else:
        plan[steps] += [last]            # the last pair's only real env
    flat = [e for v in plan.values() for e in v]
    assert len(flat) == len(set(flat)) and max(flat) < n
    return plan


def _set_clocks(b, plan):
    t = b.get_state()["time"]
    for j, envs in plan.items():
        t[envs] = _clock(j)
    b.set_state(time=t)


def _done(snap):
    return set(np.nonzero((snap["terminated"] | snap["truncated"]).cpu().numpy())[0].tolist())


def _acts(n, steps, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(steps, n, 21, device="cuda", generator=g) * 2 - 1


_direct_cache = {}


def _direct(model, n):
    """The direct schedule's snapshots of the T-step run at n envs (computed once per size)."""
    if n not in _direct_cache:
        acts = _acts(n, T, 21)
        b = _batch(model, n, "direct")
        _set_clocks(b, _plan(n))
        assert not b.queued()
        snaps = []
        for k in range(T):
            b.step(acts[k])
            snaps.append(_snap(b))
        b.close()
        _direct_cache[n] = snaps
    return _direct_cache[n]


@pytest.mark.parametrize("extra", [2, 3])
@pytest.mark.parametrize("sched", ["auto", "fixed_order"])
def test_queue_is_bitwise_direct_with_resets_in_every_step(model, resident, sched, extra):
    n = 2 * resident + extra
    plan = _plan(n)
    want = _direct(model, n)
    acts = _acts(n, T, 21)
    b = _batch(model, n, sched)
    _set_clocks(b, plan)
    assert b.queued()
    npairs = (n + 1) // 2
    for k in range(T):
        b.step(acts[k])
        s = _snap(b)
        assert _done(want[k]) == set(plan[k + 1]), k       # the run is what the plan says
        _assert_equal(s, want[k], f"{sched}, {n} envs, step {k + 1}")
        c = b.queue_counters()
        assert (c["head"], c["exit"], c["epoch"], c["abort"]) == (0, 0, k + 1, 0), (k, c)
        order = b.queue_order()
        if sched == "auto":
            assert sorted(order.tolist()) == list(range(npairs)), f"after step {k + 1}: not a permutation"
        else:
            assert len(order) == 0
    assert int(b.warning.sum()) == 0
    b.close()


@pytest.mark.parametrize("extra", [2, 3])
def test_tape_of_three_steps_is_bitwise_the_step_loop(model, resident, extra):
    import torch
    n, K = 2 * resident + extra, 3
    plan = _plan(n, steps=K + 1)                           # episodes end inside the tape and right after it
    acts = _acts(n, K + 1, 22)
    tape, loop = _batch(model, n, "auto"), _batch(model, n, "auto")
    for b in (tape, loop):
        _set_clocks(b, plan)
    obs, rew, term, trunc = tape.step_tape(acts[:K], outputs=True)
    for k in range(K):
        loop.step(acts[k])
        torch.cuda.synchronize()
        assert torch.equal(obs[k], loop.obs) and torch.equal(rew[k], loop.reward), k
        assert torch.equal(term[k], loop.terminated) and torch.equal(trunc[k], loop.truncated), k
        assert set(np.nonzero(term[k].cpu().numpy())[0].tolist()) == set(plan[k + 1]), k
    _assert_equal(_snap(tape), _snap(loop), "after the tape")
    c = tape.queue_counters()
    assert (c["head"], c["exit"], c["epoch"], c["abort"]) == (0, 0, 1, 0), c     # (epoch 1: one launch)
    assert tape.tape_aborts() == 0
    tape.step(acts[K])
    loop.step(acts[K])
    st, sl = _snap(tape), _snap(loop)
    _assert_equal(st, sl, "the step after the tape")
    assert _done(st) == set(plan[K + 1])
    tape.close()
    loop.close()


def test_two_env_tape_leaves_the_counters_at_zero(model):
    """2 envs, K = 2: four items in all, far fewer than a full grid's first items.  Same results as
    the step loop, and head / exit are zero afterwards, also after a second tape on the same batch."""
    import torch
    n, K = 2, 2
    acts = _acts(n, 2 * K, 23)
    tape, loop = _batch(model, n, "auto"), _batch(model, n, "direct")
    for r in range(2):
        obs, rew, term, trunc = tape.step_tape(acts[r * K:(r + 1) * K], outputs=True)
        for k in range(K):
            loop.step(acts[r * K + k])
            torch.cuda.synchronize()
            assert torch.equal(obs[k], loop.obs) and torch.equal(rew[k], loop.reward), (r, k)
            assert torch.equal(term[k], loop.terminated) and torch.equal(trunc[k], loop.truncated), (r, k)
        _assert_equal(_snap(tape), _snap(loop), f"after tape {r + 1}")
        c = tape.queue_counters()
        assert (c["head"], c["exit"], c["epoch"], c["abort"]) == (0, 0, r + 1, 0), c
    assert tape.tape_aborts() == 0 and int(tape.warning.sum()) == 0
    tape.close()
    loop.close()


def test_back_to_back_launches_see_the_counters_reset(model, resident):
    """Two queued launches with nothing between them (no host synchronisation): the second one's
    first claims start from a reset counter and its order is the one the first filed."""
    n = 2 * resident + 2
    npairs = n // 2
    acts = _acts(n, 2, 24)
    a, d = _batch(model, n, "auto"), _batch(model, n, "direct")
    a.step(acts[0])
    a.step(acts[1])
    d.step(acts[0])
    d.step(acts[1])
    _assert_equal(_snap(a), _snap(d), "second of two back-to-back launches")
    c = a.queue_counters()
    assert (c["head"], c["exit"], c["epoch"], c["abort"]) == (0, 0, 2, 0), c
    assert sorted(a.queue_order().tolist()) == list(range(npairs))
    assert int(a.warning.sum()) == 0
    a.close()
    d.close()
