"""The claim point of the chunk queue's claim-ahead, on the replay of the claim loop
(tools/probes/queue_replay.py, CPU only): a claim issued a constant time before the current item
ends is served in the same order as one issued when it ends, so the makespan is exactly that of no
lead; a claim issued when the item starts (a whole item early) turns the first chunks into a static
assignment and the launch gets longer."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools", "probes"))


@pytest.fixture(scope="module")
def launch():
    """Integer item durations (ticks) with the spread of the measured ones: first chunks about twice
    a last item, a heavy tail, a few very long items; 256 pairs on 64 waves."""
    rng = np.random.default_rng(7)
    npairs = 256
    d0 = (20000 + rng.gamma(2.0, 3000.0, npairs)).astype(np.int64)
    d1 = (10000 + rng.gamma(2.0, 2500.0, npairs)).astype(np.int64)
    d1[rng.choice(npairs, 4, replace=False)] += 15000
    return d0, d1, rng.permutation(npairs), 64


def test_lead_zero_is_the_plain_claim_loop(launch):
    from queue_replay import replay
    d0, d1, order, waves = launch
    # the claim loop written out: a free wave takes the next item, a last item waits for its first chunk
    free = np.zeros(waves)
    done0 = {}
    for p in order:
        w = int(np.argmin(free))
        free[w] += d0[p]
        done0[p] = free[w]
    for p in order:
        w = int(np.argmin(free))
        free[w] = max(free[w], done0[p]) + d1[p]
    assert replay(d0, d1, order, waves) == free.max()
    assert replay(d0, d1, order, waves, lead=0.0) == free.max()


@pytest.mark.parametrize("lead", [1, 700, 1260, 9999])
def test_constant_lead_gives_exactly_the_makespan_of_no_lead(launch, lead):
    from queue_replay import replay
    d0, d1, order, waves = launch
    assert lead < min(d0.min(), d1.min())
    assert replay(d0, d1, order, waves, lead=lead) == replay(d0, d1, order, waves)
    per_item = np.full((2, len(d0)), float(lead))
    assert replay(d0, d1, order, waves, lead=per_item) == replay(d0, d1, order, waves)


def test_whole_item_lead_is_longer(launch):
    from queue_replay import replay
    d0, d1, order, waves = launch
    base = replay(d0, d1, order, waves)
    assert replay(d0, d1, order, waves, lead=np.inf) > base
    assert replay(d0, d1, order, waves, lead=np.stack([d0, d1]).astype(float)) == replay(d0, d1, order, waves, lead=np.inf)


def test_lead_report_names_the_three_claim_points(launch):
    from queue_replay import lead_report
    d0, d1, order, waves = launch
    npairs = len(order)
    claim = np.empty(npairs, dtype=np.int64)
    claim[order] = np.arange(npairs)
    pair = np.concatenate([np.arange(npairs), np.arange(npairs)])
    z = {"pair": pair[None], "kind": np.repeat([0, 1], npairs)[None], "claim": np.concatenate([claim, claim])[None],
         "start": np.zeros((1, 2 * npairs), dtype=np.int64), "end": np.concatenate([d0, d1])[None],
         "reset": np.zeros((1, 2 * npairs), dtype=np.int64)}
    text, res = lead_report(z, waves, tail=1260.0)
    assert res["tail"] == res["none"] and res["item"] > res["none"]
    assert len(text.splitlines()) == 4
