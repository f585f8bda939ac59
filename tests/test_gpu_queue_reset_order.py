"""The chunk queue's reset-aware claim order (hs_kernels.hip step_kernel_queue): a
pair with an env that will auto-reset in the next env step is filed into bucket 0 and claimed first
in that step, because its last item also runs the reset's mj_step.  The rule only moves work
between waves: results stay bitwise those of the direct schedule, also when the prediction is
wrong.  Batches of 2 * resident_waves + 2 envs: the smallest that HS_SCHED_AUTO queues.
"""
import numpy as np
import pytest

from conftest import XML

pytestmark = pytest.mark.gpu

DT = 0.015          # one env step: frame_skip 3 x 0.005
T = 8               # steps of the shared run
TRUNC_STEP = 3      # the env that ends through max_steps does so in this step
FIELDS = ("obs", "reward", "terminated", "truncated", "qpos", "qvel", "qacc_warmstart", "time", "step_count",
          "episode", "total_reward", "terminal_obs", "terminal_step_count", "terminal_total_reward", "warning")


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


def _batch(model, n, sched, seed=3):
    from mujocoposelearning_amd.batch import HsBatch
    b = HsBatch(model, n, precision="fp64", seed=seed)
    b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1, max_steps=750, schedule=sched)
    b.reset()
    return b


def _n_queued(model):
    from mujocoposelearning_amd.batch import HsBatch
    b = HsBatch(model, 2, precision="fp64")
    n = 2 * b.resident_waves + 2
    b.close()
    assert b.resident_waves > 0
    return n


def _clock(step):
    """Episode clock (at the start of the run's step 1) of an env that terminates in `step`: its
    time after that step is 10.005 >= duration, after the step before it 9.99."""
    return 10.005 - DT * step


def _snap(b):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(b, k).clone() for k in FIELDS}


def _assert_equal(x, y, what):
    import torch
    for k in FIELDS:
        assert torch.equal(x[k], y[k]), f"{what}: {k} differs between the queue and the direct schedule"


def _reset_plan(n):
    """{step: envs that end their episode in it}: in every step a pair with both halves, one with
    only the lower and one with only the upper half; the first and the last pair included."""
    npairs = (n + 1) // 2
    plan = {}
    for j in range(1, T + 1):
        p = j * npairs // (T + 1)
        plan[j] = [2 * p, 2 * p + 1, 2 * (p + 37), 2 * (p + 61) + 1]
    plan[1] += [0, 1]
    plan[T] += [n - 1]
    return plan


@pytest.fixture(scope="module")
def run(model):
    """T steps on both schedules from the same clocks; per step the snapshot of both and the queue's order."""
    import torch
    n = _n_queued(model)
    plan = _reset_plan(n)
    trunc_env = 2 * ((n + 1) // 4) + 1 + 10        # ends through max_steps, not the clock
    assert all(trunc_env not in v and trunc_env ^ 1 not in v for v in plan.values())
    g = torch.Generator(device="cuda").manual_seed(11)
    acts = torch.rand(T, n, 21, device="cuda", generator=g) * 2 - 1
    out = {"n": n, "plan": plan, "trunc_env": trunc_env, "snaps": {}, "orders": []}
    for sched in ("auto", "direct"):
        b = _batch(model, n, sched)
        t = b.get_state()["time"]
        for j, envs in plan.items():
            t[envs] = _clock(j)
        b.set_state(time=t)
        b.step_count[trunc_env] = 750 - TRUNC_STEP
        assert b.queued() == (sched == "auto")
        if sched == "auto":
            assert len(b.queue_order()) == 0       # no queued launch yet: the fixed permutation
        snaps = []
        for k in range(T):
            b.step(acts[k])
            snaps.append(_snap(b))
            if sched == "auto":
                out["orders"].append(b.queue_order())
        assert len(b.queue_order()) == (n + 1) // 2 if sched == "auto" else len(b.queue_order()) == 0
        out["snaps"][sched] = snaps
        b.close()
    return out


def _done_envs(snap):
    return set(np.nonzero((snap["terminated"] | snap["truncated"]).cpu().numpy())[0].tolist())


def test_resets_happen_as_planned(run):
    """The run is what the other tests assume: in each of the T steps exactly the planned envs end
    their episode (one of them, once, through max_steps) and restart."""
    for k in range(T):
        want = set(run["plan"][k + 1]) | ({run["trunc_env"]} if k + 1 == TRUNC_STEP else set())
        s = run["snaps"]["direct"][k]
        assert _done_envs(s) == want, k
        assert (s["step_count"][sorted(want)] == 0).all() and (s["time"][sorted(want)] == 0.005).all()
    s = run["snaps"]["direct"][TRUNC_STEP - 1]
    e = run["trunc_env"]
    assert int(s["truncated"][e]) == 1 and int(s["terminated"][e]) == 0
    assert int(s["terminal_step_count"][e]) == 750


def test_queue_is_bitwise_direct_under_resets(run):
    for k in range(T):
        _assert_equal(run["snaps"]["auto"][k], run["snaps"]["direct"][k], f"step {k + 1}")
    assert int(run["snaps"]["auto"][-1]["warning"].sum()) == 0


def test_order_starts_with_the_pairs_that_reset_next(run):
    npairs = (run["n"] + 1) // 2
    for k in range(T - 1):                         # the order after step k + 1 is the one step k + 2 claims in
        order = run["orders"][k]
        assert sorted(order.tolist()) == list(range(npairs)), f"after step {k + 1}: not a permutation"
        nxt = {e // 2 for e in _done_envs(run["snaps"]["auto"][k + 1])}
        assert len(nxt) >= 3
        assert set(order[:len(nxt)].tolist()) == nxt, f"after step {k + 1}"
    assert sorted(run["orders"][-1].tolist()) == list(range(npairs))


def test_misprediction_is_harmless(model):
    """After a step, set_state moves the clocks: the pairs the queue filed first do not reset and
    others do.  The next two steps are still bitwise the direct schedule's and the order recovers."""
    import torch
    n = _n_queued(model)
    npairs = (n + 1) // 2
    A = [2 * 5, 2 * 5 + 1, 2 * 700, 2 * (npairs - 1) + 1]      # predicted to reset in step 2; they will not
    B = [2 * 9 + 1, 2 * 333, 2 * 334 + 1, n - 2]               # reset in step 2 unannounced
    Cc = [2 * 77, 2 * 612 + 1, 2 * 900, 2 * 900 + 1]           # reset in step 3, as the order after step 2 says
    g = torch.Generator(device="cuda").manual_seed(12)
    acts = torch.rand(3, n, 21, device="cuda", generator=g) * 2 - 1
    a, d = _batch(model, n, "auto"), _batch(model, n, "direct")
    for b in (a, d):
        t = b.get_state()["time"]
        t[A] = _clock(2)
        b.set_state(time=t)
        b.step(acts[0])
    assert a.queued() and not d.queued()
    order = a.queue_order()
    assert set(order[:3].tolist()) == {e // 2 for e in A} and len({e // 2 for e in A}) == 3
    for b in (a, d):
        t = b.get_state()["time"]
        t[A] -= 5.0
        t[B] = _clock(1)
        t[Cc] = _clock(2)
        b.set_state(time=t)
    for k in (1, 2):
        a.step(acts[k])
        d.step(acts[k])
        sa, sd = _snap(a), _snap(d)
        _assert_equal(sa, sd, f"step {k + 1}")
        assert _done_envs(sa) == set(B if k == 1 else Cc)
        order = a.queue_order()
        assert sorted(order.tolist()) == list(range(npairs))
        if k == 1:                                 # recovered: the pairs of Cc, and only they, in front
            want = {e // 2 for e in Cc}
            assert set(order[:len(want)].tolist()) == want
    assert int(a.warning.sum()) == 0
    a.close()
    d.close()


def test_tape_with_resets_is_bitwise_the_step_loop(model):
    """A 6-step tape at 777 envs (every env a queue unit of its own) with episodes ending inside it,
    on its last step and in the step after it, against the step loop; then one more step on both."""
    import torch
    n, K = 777, 6
    ends = {2: [0, 1, 400], 4: [5, 776], 6: [6, 7, 300], 7: [8, 301, 775]}
    g = torch.Generator(device="cuda").manual_seed(13)
    acts = torch.rand(K + 1, n, 21, device="cuda", generator=g) * 2 - 1
    tape, loop = _batch(model, n, "auto"), _batch(model, n, "auto")
    for b in (tape, loop):
        t = b.get_state()["time"]
        for j, envs in ends.items():
            t[envs] = _clock(j)
        b.set_state(time=t)
    obs, rew, term, trunc = tape.step_tape(acts[:K])
    for k in range(K):
        loop.step(acts[k])
        torch.cuda.synchronize()
        assert torch.equal(obs[k], loop.obs) and torch.equal(rew[k], loop.reward), k
        assert torch.equal(term[k], loop.terminated) and torch.equal(trunc[k], loop.truncated), k
        assert set(np.nonzero(term[k].cpu().numpy())[0].tolist()) == set(ends.get(k + 1, [])), k
    _assert_equal(_snap(tape), _snap(loop), "after the tape")
    order = tape.queue_order()                     # units are envs here: the step after the tape ends these first
    assert sorted(order.tolist()) == list(range(n))
    assert set(order[:len(ends[7])].tolist()) == set(ends[7])
    tape.step(acts[K])
    loop.step(acts[K])
    st, sl = _snap(tape), _snap(loop)
    _assert_equal(st, sl, "the step after the tape")
    assert _done_envs(st) == set(ends[7])
    tape.close()
    loop.close()
