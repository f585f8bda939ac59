"""Replay of the chunk queue's claim loop on measured item durations (CPU only, numpy).

Input: the per-item arrays that ``tools/probes/gpu_timing.py fp64 tail`` saves from the timing
build -- for each of L consecutive per-step launches and each of its 2 * npairs items: pair, chunk
kind (0 = first chunk, 1 = last substep), claim index within the kind, realtime start / end (10 ns
ticks) and whether the item ran the reset pass.

The replay hands the items, in a chosen pair order (first every pair's first chunk, then every
pair's last substep, as step_kernel_queue does), to `waves` persistent waves: a wave that becomes
free claims the next item; a last-substep item starts only when its pair's first chunk has ended
(the wave that claimed it waits).  The makespan is the end of the last item.

Orders:
  a  the order the launch actually used
  b  a, with the pairs that reset in that launch moved to the front
  c  b, with the pairs that reset in the previous launch filed as cheapest (moved to the end)
  d  pairs ordered by the true duration of their last item, longest first (the ceiling of any
     rule that orders the launch's end)

Claim point (lead_report): the used order with the next claim issued 0 ticks, `tail` ticks (the
Euler + obs remainder after an item's last solve) and a whole item before the current item ends.

    python tools/probes/queue_replay.py bench_out_probes/queue_tail_fp64_4096.npz [waves [tail ticks]]
"""
import heapq
import sys

import numpy as np


def _leads(lead, d0, d1):
    """`lead` as two per-pair arrays (first chunks, last items): a constant, or an array [2][npairs]
    (kind, pair).  np.inf: the claim is issued when the item starts (a whole-item lead)."""
    lead = np.asarray(lead, dtype=float)
    if lead.ndim == 0:
        return np.full(len(d0), float(lead)), np.full(len(d1), float(lead))
    assert lead.shape == (2, len(d0)), lead.shape
    return lead[0], lead[1]


def replay(d0, d1, order, waves, lead=0.0):
    """Makespan of one launch: first-chunk durations d0[pair], last-item durations d1[pair], the
    pairs claimed in `order` for both chunk kinds, on `waves` waves.  A wave issues its next claim
    `lead` ticks before its current item ends (never before the item starts); the claims are served
    in the order they are issued and the claimed item starts when the wave's current one has ended.
    lead = 0 is the claim loop without claim-ahead."""
    l0, l1 = _leads(lead, d0, d1)
    nw = min(waves, 2 * len(order))
    claims = [(0.0, w) for w in range(nw)]      # (time the wave's pending claim was issued, wave)
    heapq.heapify(claims)
    free = [0.0] * nw                           # when the wave's current item ends
    done0 = {}
    end = 0.0
    for kind, d, l in ((0, d0, l0), (1, d1, l1)):
        for p in order:
            _, w = heapq.heappop(claims)
            start = free[w] if kind == 0 else max(free[w], done0[p])
            t = start + d[p]
            if kind == 0:
                done0[p] = t
            end = max(end, t)
            free[w] = t
            heapq.heappush(claims, (max(start, t - l[p]), w))
    return end


def front(order, sel):
    """`order` with the pairs of the boolean mask `sel` moved to the front (stable)."""
    order = np.asarray(order)
    return np.concatenate([order[sel[order]], order[~sel[order]]])


def back(order, sel):
    order = np.asarray(order)
    return np.concatenate([order[~sel[order]], order[sel[order]]])


def orders(used, reset, prev_reset, d1):
    """The four pair orders of one launch: the order it used, the pairs' reset bits in this launch
    and in the previous one (None: unknown), and the true last-item durations."""
    a = np.asarray(used)
    b = front(a, reset)
    c = b if prev_reset is None else front(back(a, prev_reset & ~reset), reset)
    d = np.argsort(-np.asarray(d1), kind="stable")
    return {"a": a, "b": b, "c": c, "d": d}


def per_pair(z, launch):
    """(used order, d0, d1, reset, start, end) of one saved launch, indexed by pair."""
    pair, kind = z["pair"][launch], z["kind"][launch]
    npairs = int(pair.max()) + 1
    out = {}
    for k in (0, 1):
        sel = kind == k
        idx = pair[sel]
        for name in ("claim", "start", "end", "reset"):
            v = np.zeros(npairs, dtype=np.int64)
            v[idx] = z[name][launch][sel]
            out[name, k] = v
    used = np.argsort(out["claim", 0], kind="stable")
    d0 = (out["end", 0] - out["start", 0]).astype(float)
    d1 = (out["end", 1] - out["start", 1]).astype(float)
    return used, d0, d1, out["reset", 1].astype(bool), out


def tail_report(z, fractions=(0.05, 0.10, 0.15)):
    """Who is busy at the end of the launch: for the last 5 / 10 / 15 % of each launch, the items
    still running at that moment and how many of them are reset items; and the last-item
    durations of reset items against the others (us).  Means over the saved launches."""
    L = z["pair"].shape[0]
    busy = {f: [] for f in fractions}
    rbusy = {f: [] for f in fractions}
    dr, dn, spans, nreset, last_is_reset = [], [], [], [], []
    for launch in range(L):
        st, en = z["start"][launch].astype(np.int64), z["end"][launch].astype(np.int64)
        rs = z["reset"][launch].astype(bool)
        span = en.max()
        spans.append(span)
        for f in fractions:
            t = span * (1 - f)
            run = (st <= t) & (en > t)
            busy[f].append(run.sum())
            rbusy[f].append((run & rs).sum())
        _, _, d1, reset, _ = per_pair(z, launch)
        nreset.append(reset.sum())
        if reset.any():
            dr.append(d1[reset].mean())
        dn.append(d1[~reset].mean())
        last_is_reset.append(bool(rs[np.argmax(en)]))
    us = 10 / 1e3
    lines = [f"launches {L}, span mean {np.mean(spans) * us:.1f} us; reset pairs per launch mean {np.mean(nreset):.1f}; "
             f"the launch's last item is a reset item in {sum(last_is_reset)}/{L} launches"]
    for f in fractions:
        lines.append(f"  last {100 * f:4.0f} % of the launch: busy waves {np.mean(busy[f]):7.1f}, of them reset items "
                     f"{np.mean(rbusy[f]):5.1f}")
    lines.append(f"  last-item duration: reset items {np.mean(dr) * us if dr else float('nan'):.1f} us, others "
                 f"{np.mean(dn) * us:.1f} us")
    return "\n".join(lines)


def replay_report(z, waves=1024):
    L = z["pair"].shape[0]
    res = {k: [] for k in "abcd"}
    measured = []
    prev = None
    for launch in range(L):
        used, d0, d1, reset, _ = per_pair(z, launch)
        measured.append(z["end"][launch].max())
        if prev is not None:   # (c) needs the previous launch's bits: the first saved launch is skipped
            for k, o in orders(used, reset, prev, d1).items():
                res[k].append(replay(d0, d1, o, waves))
        prev = reset
    us = 10 / 1e3
    a = np.mean(res["a"])
    lines = [f"replay on {waves} waves, {L - 1} launches; measured span {np.mean(measured[1:]) * us:.1f} us"]
    for k, name in (("a", "order used"), ("b", "resets first"), ("c", "resets first, last launch's resets last"),
                    ("d", "true last-item duration")):
        m = np.mean(res[k])
        lines.append(f"  ({k}) {name:42s} makespan {m * us:7.1f} us  {100 * (a - m) / a:+5.2f} % vs (a)")
    return "\n".join(lines), {k: float(np.mean(v)) for k, v in res.items()}


def lead_report(z, waves=1024, tail=1000.0):
    """The claim point of a claim-ahead: the used order replayed with the claim issued at the end of
    the item (no lead), `tail` ticks before it (the nearly constant Euler + obs / commit remainder
    after the item's last solve), and at its start (a whole item early)."""
    L = z["pair"].shape[0]
    res = {"none": [], "tail": [], "item": []}
    for launch in range(L):
        used, d0, d1, _, _ = per_pair(z, launch)
        for k, lead in (("none", 0.0), ("tail", tail), ("item", np.inf)):
            res[k].append(replay(d0, d1, used, waves, lead))
    us = 10 / 1e3
    a = np.mean(res["none"])
    lines = [f"claim point on {waves} waves, {L} launches, the order used"]
    for k, name in (("none", "claim when the item ends (lead 0)"),
                    ("tail", f"claim {tail * us:.1f} us before the item ends"),
                    ("item", "claim when the item starts (whole item)")):
        m = np.mean(res[k])
        lines.append(f"  {name:42s} makespan {m * us:7.1f} us  {100 * (a - m) / a:+5.2f} % vs lead 0")
    return "\n".join(lines), {k: float(np.mean(v)) for k, v in res.items()}


if __name__ == "__main__":
    z = np.load(sys.argv[1])
    waves = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    print(tail_report(z))
    print(replay_report(z, waves)[0])
    print(lead_report(z, waves, float(sys.argv[3]) if len(sys.argv) > 3 else 1000.0)[0])
