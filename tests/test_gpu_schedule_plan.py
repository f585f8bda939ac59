"""The schedule hs_batch_schedule reports is the one the launches take (csrc/hs_schedule.h).

A queued launch, and only a queued launch, advances the chunk queue's epoch word by one (its last wave out).
Batches of R, 2R, 2R + 1 and 2R + 2 envs -- R the resident wave count, read at run time: the smallest sizes on
either side of the single / paired and the paired / queue boundaries -- take one step each with frame_skip 1 and
5, in both precisions: the epoch moves by 1 where hs_batch_schedule says "queue" and by 0 elsewhere, and
schedule_name() names the same schedule.  A tape of two steps is queued at any size, by single envs when the
batch fits the resident waves.
"""
import pytest

from conftest import XML

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


def _batch(model, n, precision):
    from mujocoposelearning_amd.batch import HsBatch
    b = HsBatch(model, n, precision=precision, seed=3)
    b.configure(frame_skip=5, duration=10.0, reward_id=0, autoreset=1, max_steps=750, schedule="auto")
    b.reset()
    return b


def _resident(model, precision):
    b = _batch(model, 2, precision)
    r = b.resident_waves
    b.close()
    assert r > 0
    return r


def _acts(n, steps=None):
    import torch
    g = torch.Generator(device="cuda").manual_seed(31)
    shape = (n, 21) if steps is None else (steps, n, 21)
    return torch.rand(*shape, device="cuda", generator=g) * 2 - 1


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_epoch_advances_exactly_when_the_plan_says_queued(model, precision):
    R = _resident(model, precision)
    # the rule, written out: more env pairs than resident waves and two substeps or more
    want = {(R, 1): "single", (R, 5): "single", (2 * R, 1): "paired", (2 * R, 5): "paired",
            (2 * R + 1, 1): "paired", (2 * R + 1, 5): "queue", (2 * R + 2, 1): "paired", (2 * R + 2, 5): "queue"}
    for n in (R, 2 * R, 2 * R + 1, 2 * R + 2):
        b = _batch(model, n, precision)
        assert b.resident_waves == R
        a = _acts(n)
        for frame_skip in (1, 5):
            b.configure(frame_skip=frame_skip)
            queued, single = b.schedule()
            name = b.schedule_name()
            assert name == ("queue" if queued else "single" if single else "paired"), (n, frame_skip)
            assert b.queued() == queued and name == want[(n, frame_skip)], (n, frame_skip, name)
            before = b.queue_counters()
            b.step(a)
            after = b.queue_counters()
            assert after["epoch"] - before["epoch"] == (1 if queued else 0), (n, frame_skip, before, after)
            assert (after["head"], after["exit"], after["abort"]) == (0, 0, 0), (n, frame_skip, after)
        assert int(b.warning.sum()) == 0
        b.close()


def test_a_tape_of_two_steps_is_queued_at_any_size(model):
    R = _resident(model, "fp64")
    for n, want_single in ((R, True), (2 * R + 2, False)):
        b = _batch(model, n, "fp64")
        assert b.schedule(n_steps=2) == (True, want_single), n
        before = b.queue_counters()
        b.step_tape(_acts(n, 2), outputs=False)
        after = b.queue_counters()
        assert after["epoch"] - before["epoch"] == 1, (n, before, after)
        assert (after["head"], after["exit"], after["abort"]) == (0, 0, 0) and b.tape_aborts() == 0, (n, after)
        assert int(b.warning.sum()) == 0
        b.close()
