"""tools/probes/queue_replay.py: the chunk queue's claim loop replayed on item durations, checked
on cases small enough to schedule by hand (CPU only)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probes"))
import queue_replay as qr  # noqa: E402


# three pairs on two waves; every first chunk takes 1, the last items take 1, 1 and 4
D0 = np.array([1.0, 1.0, 1.0])
D1 = np.array([1.0, 1.0, 4.0])


def test_makespan_of_a_hand_scheduled_launch():
    # order 0 1 2: t=0 w0 p0.c0 -> 1, w1 p1.c0 -> 1; t=1 w0 p2.c0 -> 2, w1 p0.last -> 2;
    # t=2 w0 p1.last -> 3, w1 p2.last -> 6
    assert qr.replay(D0, D1, [0, 1, 2], 2) == 6.0
    # the long pair first: t=0 w0 p2.c0 -> 1, w1 p0.c0 -> 1; t=1 w0 p1.c0 -> 2, w1 p2.last -> 5;
    # t=2 w0 p0.last -> 3; t=3 w0 p1.last -> 4
    assert qr.replay(D0, D1, [2, 0, 1], 2) == 5.0
    # one wave: the sum of everything
    assert qr.replay(D0, D1, [0, 1, 2], 1) == 9.0
    # more waves than items: first chunk + last item of the longest pair
    assert qr.replay(D0, D1, [0, 1, 2], 64) == 5.0


def test_last_item_waits_for_its_own_first_chunk():
    # two pairs, two waves, pair 0's first chunk is long: w1 runs p1.c0 (1), claims p0.last at t=1
    # and waits for p0.c0 until t=5, then runs it (1) -> 6; w0 claims p1.last at t=5 -> 7
    assert qr.replay(np.array([5.0, 1.0]), np.array([1.0, 2.0]), [0, 1], 2) == 7.0


def test_orders():
    used = np.array([1, 0, 3, 2])
    reset = np.array([False, False, True, False])
    prev = np.array([False, True, False, False])
    d1 = np.array([3.0, 1.0, 9.0, 4.0])
    o = qr.orders(used, reset, prev, d1)
    assert o["a"].tolist() == [1, 0, 3, 2]
    assert o["b"].tolist() == [2, 1, 0, 3]
    assert o["c"].tolist() == [2, 0, 3, 1]
    assert o["d"].tolist() == [2, 3, 0, 1]
    # a pair that reset in both launches stays in front
    o = qr.orders(used, reset, reset, d1)
    assert o["c"].tolist() == [2, 1, 0, 3]


def test_reports_on_saved_items():
    # two launches of the three-pair case in the saved layout; pair 2 resets in both, the launch
    # used order 0 1 2: (a) 6, (b) = (c) = (d) 5 (as scheduled by hand above)
    pair = np.tile(np.arange(3), 2)
    kind = np.repeat([0, 1], 3)
    claim = np.tile(np.arange(3), 2)
    start = np.array([0, 0, 1, 1, 2, 2])
    end = np.array([1, 1, 2, 2, 3, 6])
    reset = np.array([0, 0, 0, 0, 0, 1])
    z = {k: np.array([v, v]) for k, v in dict(pair=pair, kind=kind, claim=claim, start=start, end=end,
                                              reset=reset).items()}
    text, mk = qr.replay_report(z, waves=2)
    assert mk == {"a": 6.0, "b": 5.0, "c": 5.0, "d": 5.0}
    assert "(b)" in text
    rep = qr.tail_report(z, fractions=(0.1,))
    # at t = 5.4 of 6 only the reset item runs
    assert "busy waves     1.0, of them reset items   1.0" in rep
    assert "2/2 launches" in rep
