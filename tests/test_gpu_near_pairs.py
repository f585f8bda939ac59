"""The fp64 resident-tier kernels run the collision narrow phase over a compacted list of near pairs
(csrc/hs_stepper.h collision_near): a broad pass over the 159 static pairs keeps the pairs whose bounds
overlap, ascending, in a per-env list in LDS, and the narrow phase runs ceil(max(near pairs of the wave's
two envs) / 32) passes over it.  Results must be what the five-pass loop gives: the same contacts in
MuJoCo's pair order, none dropped by a pair wrongly called far or by a list that did not survive.

States come from oracle episodes (the humanoid falls and lies on the floor); their near pairs are counted
on the CPU with the kernel's two bounds (tools/probes/near_pair_stats.py).  Bars as in
tests/test_gpu_contacts.py: ncon / nefc equal to the oracle's, qacc <= 1e-8 * scale, qpos <= 1e-12.
"""
import numpy as np
import pytest

from conftest import XML
from near_pair_stats import HL, episode_states, near_mask, pair_tables

pytestmark = pytest.mark.gpu

CAP = (32, 128)     # resident tier: contacts, rows (envs over it are re-run by the wide tier's five-pass loop)


@pytest.fixture(scope="module")
def model():
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML)


@pytest.fixture(scope="module")
def sample():
    """~660 states of five oracle episodes (four on U(-1, 1) actions, one on zeros), each with its near-pair
    count and the oracle's contact / row counts after forward().  Computed once, never modified."""
    from oracle.oracle import Oracle
    o = Oracle(XML)
    tab = pair_tables(o.M)
    rng = np.random.default_rng(11)
    states = []
    for zero in (False, False, False, False, True):
        states += episode_states(o, rng, zero, sample=5)
    q = np.stack([s[0] for s in states])
    v = np.stack([s[1] for s in states])
    nnear, ncon, nefc = [], [], []
    for i in range(len(q)):
        _forward(o, q[i], v[i])
        nnear.append(int(near_mask(o, tab).sum()))
        ncon.append(o.d.ncon)
        nefc.append(o.d.nefc)
    nnear, ncon, nefc = np.array(nnear), np.array(ncon), np.array(nefc)
    resident = (ncon <= CAP[0]) & (nefc <= CAP[1])
    out = dict(o=o, tab=tab, q=q, v=v, nnear=nnear, ncon=ncon, nefc=nefc,
               small=np.flatnonzero((nnear <= HL) & resident), big=np.flatnonzero((nnear > HL) & resident))
    # the selection holds both kinds: states whose list needs one narrow pass and states that need two
    assert len(out["small"]) >= 40 and len(out["big"]) >= 40, (len(out["small"]), len(out["big"]))
    for a in (q, v, nnear, ncon, nefc, out["small"], out["big"]):
        a.setflags(write=False)
    return out


def _forward(o, q, v):
    o.reset_data()
    o.qpos[:] = q
    o.qvel[:] = v
    o.forward()


def _oracle_step(o, q, v, c):
    o.reset_data()
    o.qpos[:] = q
    o.qvel[:] = v
    o.step(np.asarray(c, np.float64), 1)
    return o.qpos.copy(), o.qvel.copy(), o.get("qacc"), o.d.ncon, o.d.nefc


def _substep(model, q, v, c, debug=False):
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    b = HsBatch(model, len(q), precision="fp64")
    assert b.resident_capacity == CAP
    b.configure(schedule="direct")      # one wave per env pair: envs 2w and 2w + 1 share wave w
    assert b.schedule_name() == "paired"
    b.set_state(qpos=q, qvel=v, time=0.0, qacc_warmstart=0.0)
    if debug:
        b.set_debug(True)
    b.physics_step(torch.tensor(c, device=b.device), 1)
    st = b.get_state()
    aux = b.aux.double().cpu().numpy()
    warn = b.warning.cpu().numpy()
    dbg = b.get_debug() if debug else None
    reruns = b.wide_reruns()
    b.close()
    return st, aux, warn, dbg, reruns


def _spread(a, k):
    """k entries of a, evenly spaced"""
    return a[np.linspace(0, len(a) - 1, k).astype(int)]


def _ctrl(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 21)).astype(np.float32)


def test_pass_count_mix_matches_oracle(model, sample):
    """64 envs, 32 waves: the waves hold (<= 32, <= 32), (> 32, <= 32), (<= 32, > 32) and (> 32, > 32) near
    pairs in turn -- one narrow pass, two, and two with a half that idles in the second."""
    S = sample
    small, big = list(_spread(S["small"], 32)), list(_spread(S["big"], 32))
    assert len(set(small)) == 32 and len(set(big)) == 32
    idx = []
    for w in range(32):
        lo = big.pop() if w % 4 in (1, 3) else small.pop()
        hi = big.pop() if w % 4 in (2, 3) else small.pop()
        idx += [lo, hi]
    idx = np.array(idx)
    kinds = {(S["nnear"][idx[2 * w]] > HL, S["nnear"][idx[2 * w + 1]] > HL) for w in range(32)}
    assert len(kinds) == 4
    q, v, c = S["q"][idx], S["v"][idx], _ctrl(64, 21)
    st, aux, warn, _, reruns = _substep(model, q, v, c)
    assert warn.sum() == 0 and reruns == 0          # every env ran the near-pair collision
    worst_a = worst_q = 0.0
    for i in range(64):
        rq, rv, ra, ncon, nefc = _oracle_step(S["o"], q[i], v[i], c[i])
        assert (int(aux[i, 35]), int(aux[i, 36])) == (ncon, nefc), (i, aux[i, 35:37], ncon, nefc, S["nnear"][idx[i]])
        scale = 1 + np.abs(ra).max()
        worst_a = max(worst_a, np.abs(aux[i, :27] - ra).max() / scale)
        worst_q = max(worst_q, np.abs(st["qpos"][i] - rq).max())
        assert np.abs(aux[i, :27] - ra).max() <= 1e-8 * scale, i
        assert np.abs(st["qpos"][i] - rq).max() <= 1e-12, i
    print(f"near pairs {S['nnear'][idx].min()}..{S['nnear'][idx].max()}, worst qacc / scale {worst_a:.2e}, qpos {worst_q:.2e}")


def test_contact_list_through_the_stage_dump(model, sample):
    """Four states -- two with at most 32 near pairs, two with more -- placed in turn as env 0 beside a partner
    of either kind: the contact list env 0 dumps equals the oracle's, pair ids and order exactly, position,
    normal and distance to 1e-9."""
    S = sample
    o = S["o"]
    key = {frozenset(map(int, p)): i for i, p in enumerate(o.M["collision_pairs"])}
    # contact-rich states, so the order of several pairs is on show
    sm = S["small"][np.argsort(-S["ncon"][S["small"]], kind="stable")[:2]]
    bg = S["big"][np.argsort(-S["ncon"][S["big"]], kind="stable")[:2]]
    assert S["ncon"][sm].min() >= 3 and S["ncon"][bg].min() >= 3
    for e0, e1 in ((sm[0], sm[1]), (bg[0], sm[0]), (sm[1], bg[1]), (bg[1], bg[0])):
        idx = np.array([e0, e1])
        _, _, warn, dbg, reruns = _substep(model, S["q"][idx], S["v"][idx], _ctrl(2, 22), debug=True)
        assert warn.sum() == 0 and reruns == 0
        _forward(o, S["q"][e0], S["v"][e0])
        ref = o.contacts()
        assert int(dbg[2503]) == len(ref) == S["ncon"][e0]
        got = dbg[2600:2600 + 11 * len(ref)].reshape(len(ref), 11)
        assert [int(g[10]) for g in got] == [key[frozenset(c["geom"])] for c in ref], (e0, S["nnear"][e0])
        for g, c in zip(got, ref):
            assert np.abs(g[0:3] - c["pos"]).max() <= 1e-9
            assert np.abs(g[3:6] - c["frame"][:3]).max() <= 1e-9
            assert abs(g[9] - c["dist"]) <= 1e-9


def _rotation_to_z(a):
    """unit quaternion rotating unit vector a onto +z"""
    z = np.array([0.0, 0.0, 1.0])
    ax = np.cross(a, z)
    s, c = np.linalg.norm(ax), a @ z
    if s < 1e-12:
        return np.array([1.0, 0, 0, 0]) if c > 0 else np.array([0.0, 1, 0, 0])
    ang = np.arctan2(s, c)
    return np.r_[np.cos(ang / 2), np.sin(ang / 2) * ax / s]


def _qmul(a, b):
    return np.r_[a[0] * b[0] - a[1:] @ b[1:], a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:])]


def test_plane_bound_at_its_edge(model, sample):
    """A plane pair is far when the geom's centre is above the floor by more than (radius + half-length)
    (1 + 1e-9) + 1e-12.  8 states, each turned so that one capsule stands upright (its lower end then touches
    the floor exactly when its centre is at r + h) and lifted so that this centre is at (r + h) times
    1 - 1e-7, 1 - 1e-12, 1 + 1e-12 and 1 + 1e-7: ncon equals the oracle's in all 32 cases, and the oracle has
    that capsule's floor contact in the first case and not in the last."""
    S = sample
    o = S["o"]
    M = o.M
    g1, g2, plane, _, reach = S["tab"]
    caps = [int(g) for g, p in zip(g2, plane) if p and M["geom_type"][g] == 3]
    factors = (1 - 1e-7, 1 - 1e-12, 1 + 1e-12, 1 + 1e-7)
    qs, vs, hit = [], [], []
    pick = np.r_[_spread(S["small"], 4), _spread(S["big"], 4)]
    assert len(set(pick)) == 8
    for k, e in enumerate(pick):
        g = caps[(3 * k) % len(caps)]
        p = int(np.flatnonzero(plane & (g2 == g))[0])
        q = S["q"][e].copy()
        _forward(o, q, S["v"][e])
        a = o.get("geom_xmat").reshape(-1, 3, 3)[g][:, 2]
        q[3:7] = _qmul(_rotation_to_z(a), q[3:7])
        q[3:7] /= np.linalg.norm(q[3:7])
        for f in factors:
            for _ in range(2):      # the second pass removes the rounding of the first shift
                _forward(o, q, S["v"][e])
                n = o.get("geom_xmat").reshape(-1, 3, 3)[g1[p]][:, 2]
                cd = (o.get("geom_xpos")[g] - o.get("geom_xpos")[g1[p]]) @ n
                q[2] += reach[p] * f - cd
            _forward(o, q, S["v"][e])
            hit.append(any(set(c["geom"]) == {int(g1[p]), g} for c in o.contacts()))
            qs.append(q.copy())
            vs.append(S["v"][e])
    hit = np.array(hit).reshape(8, 4)
    assert hit[:, 0].all() and not hit[:, 3].any(), hit
    qs, vs, c = np.stack(qs), np.stack(vs), _ctrl(32, 23)
    _, aux, warn, _, _ = _substep(model, qs, vs, c)
    assert warn.sum() == 0
    for i in range(32):
        _, _, _, ncon, nefc = _oracle_step(o, qs[i], vs[i], c[i])
        assert int(aux[i, 35]) == ncon, (i // 4, factors[i % 4], int(aux[i, 35]), ncon)


def test_schedules_and_tape_are_bitwise_equal(model, sample):
    """5 envs (an odd count: a ghost half) from lying states with up to > 32 near pairs, 3 env steps: the
    paired schedule, the single-env schedule and a 3-step tape give the same bits."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    S = sample
    idx = np.r_[S["big"][-3:], S["small"][-2:]]
    n, steps = 5, 3
    acts = torch.tensor(np.random.default_rng(24).uniform(-1, 1, (steps, n, 21)).astype(np.float32), device="cuda")

    def make(sched):
        b = HsBatch(model, n, device=0, precision="fp64", seed=2)
        b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1, schedule=sched)
        b.reset()
        b.set_state(qpos=S["q"][idx], qvel=S["v"][idx], time=1.0, qacc_warmstart=0.0, ctrl=0.0)
        return b

    def snap(b):
        return [t.clone() for t in (b.obs, b.reward, b.terminated, b.truncated, b.qpos, b.qvel, b.qacc_warmstart,
                                    b.time, b.warning, b.aux)]

    runs = {}
    for sched in ("direct", "single"):
        b = make(sched)
        assert b.schedule_name() == ("paired" if sched == "direct" else "single")
        tr = []
        for k in range(steps):
            b.step(acts[k])
            tr.append(snap(b))
        runs[sched] = tr
        b.close()
    for k in range(steps):
        for x, y in zip(runs["direct"][k], runs["single"][k]):
            assert torch.equal(x, y), k
    b = make("auto")
    obs, rew, term, trunc = b.step_tape(acts)
    for k in range(steps):
        for x, y in zip((obs[k], rew[k], term[k], trunc[k]), runs["direct"][k][:4]):
            assert torch.equal(x, y), k
    for x, y in zip(snap(b), runs["direct"][-1]):
        assert torch.equal(x, y)
    b.close()


def test_no_contact_is_dropped(model, sample):
    """256 sampled states of every kind (the ones over the resident tier included), one substep: ncon and nefc
    equal the oracle's for every env, and no overflow is flagged where the oracle has at most 32 contacts.  A
    pair wrongly called far, or a near list overwritten before the narrow passes, would lose a contact here."""
    S = sample
    idx = np.linspace(0, len(S["q"]) - 1, 256).astype(int)
    assert (S["nnear"][idx] > HL).sum() >= 30 and (S["nnear"][idx] <= HL).sum() >= 30
    q, v, c = S["q"][idx], S["v"][idx], _ctrl(256, 25)
    _, aux, warn, _, _ = _substep(model, q, v, c)
    for i in range(256):
        _, _, _, ncon, nefc = _oracle_step(S["o"], q[i], v[i], c[i])
        assert (int(aux[i, 35]), int(aux[i, 36])) == (ncon, nefc), (i, aux[i, 35:37], ncon, nefc)
        if ncon <= 32:
            assert warn[i, 3] == 0, i           # HS_WARN_OVERFLOW
