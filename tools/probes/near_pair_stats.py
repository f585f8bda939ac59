"""CPU statistics behind the near-pair collision of the fp64 step kernels (csrc/hs_stepper.h
collision_near, profiles/near_pairs.md): how many of humanoid.xml's static geom pairs pass the broad
tests, how they spread over the five 32-pair passes of the plain loop, and how many narrow passes a
wave of two envs needs once they are compacted.

Oracle episodes (oracle/oracle.py) of 667 env steps of 3 substeps from the env's reset pose, states
sampled every SAMPLE env steps with a fresh forward(); the broad tests are the kernel's, in numpy:
  body pairs   near iff |c2 - c1|^2 <= (r1 + h1 + r2 + h2)^2
  plane pairs  near iff (c2 - c1) . n <= (r2 + h2) (1 + 1e-9) + 1e-12
It also checks that every oracle contact belongs to a pair the tests call near.

Usage: python tools/probes/near_pair_stats.py [--episodes-random 6] [--episodes-zero 2] [--sample 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
XML = os.path.join(ROOT, "mujocoposelearning_amd", "assets", "humanoid.xml")
HL = 32


def pair_tables(M):
    """(g1, g2, is_plane, reach1, reach2) per static pair, g1 the plane of a plane pair."""
    gt, gs = np.asarray(M["geom_type"]), np.asarray(M["geom_size"], float)
    reach = np.where(gt == 3, gs[:, 0] + gs[:, 1], gs[:, 0])
    g1, g2 = np.array([[min(a, b, key=lambda g: (gt[g], g)), max(a, b, key=lambda g: (gt[g], g))]
                       for a, b in M["collision_pairs"]]).T
    return g1, g2, gt[g1] == 0, np.where(gt[g1] == 0, 0.0, reach[g1]), reach[g2]


def near_mask(o, tab):
    """The broad tests on the oracle's current (forward) geom frames: bool per static pair."""
    g1, g2, plane, R1, R2 = tab
    gx, gm = o.get("geom_xpos"), o.get("geom_xmat").reshape(-1, 3, 3)
    d = gx[g2] - gx[g1]
    far_body = (d * d).sum(1) > (R1 + R2) ** 2
    far_plane = (d * gm[g1][:, :, 2]).sum(1) > R2 * (1 + 1e-9) + 1e-12
    return ~np.where(plane, far_plane, far_body)


def episode_states(o, rng, zero_actions, sample, steps=667, nsub=3):
    """(qpos, qvel) every `sample` env steps of one oracle episode from the env's reset pose."""
    M = o.M
    o.reset_data()
    q = np.array(M["qpos0"], float)
    q[2] = 1.282
    q[3:7] = [1, 0, 0, 0]
    noise = rng.uniform(-0.01, 0.01, M["nq"])
    noise[2] *= 0.1
    noise[3:7] = 0
    o.qpos[:] = q + noise
    o.qvel[:] = rng.uniform(-0.01, 0.01, M["nv"])
    out = []
    for k in range(steps):
        a = np.zeros(M["nu"]) if zero_actions else rng.uniform(-1, 1, M["nu"]).astype(np.float32).astype(float)
        o.step(a, nsub)
        if k % sample == sample - 1:
            out.append((o.qpos.copy(), o.qvel.copy()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes-random", type=int, default=6)
    ap.add_argument("--episodes-zero", type=int, default=2)
    ap.add_argument("--sample", type=int, default=5)
    a = ap.parse_args()
    from oracle.oracle import Oracle
    o = Oracle(XML)
    tab = pair_tables(o.M)
    plane = tab[2]
    key = {frozenset(p): i for i, p in enumerate(map(tuple, o.M["collision_pairs"]))}
    rng = np.random.default_rng(0)
    states = []
    for e in range(a.episodes_random + a.episodes_zero):
        states += episode_states(o, rng, e >= a.episodes_random, a.sample)
    nnear, nplane, passes_hit, ncon, missed, checked = [], [], [], [], 0, 0
    for q, v in states:
        o.reset_data()
        o.qpos[:] = q
        o.qvel[:] = v
        o.forward()
        nm = near_mask(o, tab)
        nnear.append(int(nm.sum()))
        nplane.append(int((nm & plane).sum()))
        body = np.flatnonzero(nm & ~plane)
        passes_hit.append(len(set(body // HL)))
        ncon.append(o.d.ncon)
        for c in o.contacts():
            checked += 1
            missed += not nm[key[frozenset(c["geom"])]]
    nnear = np.array(nnear)
    pair_all_first = bool(np.all(np.diff(plane.astype(int)) <= 0))
    print(f"static pairs {len(plane)}, plane pairs {int(plane.sum())}, all plane pairs first: {pair_all_first}")
    print(f"states {len(states)} ({a.episodes_random} U(-1,1) + {a.episodes_zero} zero-action episodes, every {a.sample} env steps)")
    print(f"near pairs per env: mean {nnear.mean():.1f} p50 {np.percentile(nnear, 50):.0f} p90 {np.percentile(nnear, 90):.0f} "
          f"p99 {np.percentile(nnear, 99):.0f} max {nnear.max()}; plane pairs among them mean {np.mean(nplane):.1f}")
    print(f"states over {HL} near pairs: {100 * (nnear > HL).mean():.1f} %")
    print(f"passes of the plain loop holding a near body pair, per env: mean {np.mean(passes_hit):.2f} of 5")
    r2 = np.random.default_rng(1)
    a_, b_ = r2.integers(0, len(nnear), 20000), r2.integers(0, len(nnear), 20000)
    npass = np.ceil(np.maximum(nnear[a_], nnear[b_]) / HL)
    print(f"narrow passes of a wave of two random envs: one pass in {100 * (npass <= 1).mean():.0f} %, mean {npass.mean():.2f}")
    print(f"oracle contacts checked {checked}, in a pair called far: {missed}; mean ncon {np.mean(ncon):.1f}")


if __name__ == "__main__":
    main()
