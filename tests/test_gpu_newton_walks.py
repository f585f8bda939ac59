"""The fp64 resident-tier Newton solve walks the active contacts once per iteration for J'f and the Hessian's
contact terms (csrc/hs_contacts.h jtf_aug_lane), reads its row slots' J x operands in one batch (rows_Jx), and
takes J qacc_warmstart out of the chain walk of rows() (chain_vel2).  Every accumulator still sees its own
operations in its own order, so the bars are the ones the separate walks already met.

The states come from a seeded search with the oracle on the CPU (about a second): falling, tumbling humanoids
with the right hip and knee bent so that hamstring_right reaches its limit.  A "covering" state-substep has, all
at once and each with a nonzero force, a tendon-limit row, a joint-limit row, a floor contact and a body-body
contact, inside the resident tier (at most 32 contacts, 128 rows) and with at least 2 Newton iterations -- every
branch of the changed loops.  The tests assert that coverage from the oracle's own rows, so they cannot pass on
inputs that miss a branch.
"""
import numpy as np
import pytest

from conftest import XML

pytestmark = pytest.mark.gpu

LIMIT_JOINT, LIMIT_TENDON = 3, 4     # oracle/hsim_oracle.h (mjtConstraint)
NQ, NV, NU = 28, 27, 21


def _coverage(o, gb):
    """What the oracle's last substep exercised: rows with a nonzero force by kind, contacts with one by kind."""
    d = o.d
    nefc, ncon = d.nefc, d.ncon
    ty = np.ctypeslib.as_array(d.efc_type)[:nefc]
    f = np.ctypeslib.as_array(d.efc_force)[:nefc]
    floor = bodies = False
    for i in range(ncon):
        c = d.contact[i]
        if np.any(f[c.efc_address:c.efc_address + (4 if c.dim == 3 else 1)] != 0):
            if gb[c.geom[0]] == 0 or gb[c.geom[1]] == 0:
                floor = True
            else:
                bodies = True
    return dict(tendon=bool(np.any((ty == LIMIT_TENDON) & (f != 0))), joint=bool(np.any((ty == LIMIT_JOINT) & (f != 0))),
                floor=floor, bodies=bodies, ncon=int(ncon), nefc=int(nefc), niter=int(d.solver_niter))


def _covers(c):
    return (c["tendon"] and c["joint"] and c["floor"] and c["bodies"] and c["ncon"] <= 32 and c["nefc"] <= 128
            and c["niter"] >= 2)


@pytest.fixture(scope="module")
def oracle():
    from oracle.oracle import Oracle
    return Oracle(XML)


@pytest.fixture(scope="module")
def covering(oracle):
    """The search: default_rng(3), 300 trials of 60 substeps with zero ctrl; every covering state-substep as
    (qpos, qvel, qacc_warmstart) BEFORE the substep.  Computed once, never changed.  `seen` counts every substep
    of every trial (300 x 60), whatever became of the trial; 93 of them cover."""
    o = oracle
    M = o.M
    gb = np.asarray(M["geom_bodyid"])
    rng = np.random.default_rng(3)
    hits, seen = [], 0
    for trial in range(300):
        q = M["qpos0"].copy()
        q[2] = rng.uniform(0.25, 0.7)
        quat = rng.normal(size=4)
        q[3:7] = quat / np.linalg.norm(quat)
        q[7:] += rng.uniform(-0.8, 0.8, 21)
        q[12] = rng.uniform(-1.8, -1.0)      # hip_y_right and knee_right: the joints hamstring_right wraps
        q[13] = rng.uniform(-0.3, 0)
        v = rng.normal(0, 0.5, NV)
        o.reset_data()
        o.qpos[:] = q
        o.qvel[:] = v
        for sub in range(60):
            before = (o.qpos.copy(), o.qvel.copy(), o.arr("qacc_warmstart", NV).copy())
            o.step(None, 1)
            seen += 1
            c = _coverage(o, gb)
            if _covers(c):
                hits.append(dict(trial=trial, sub=sub, state=before, cov=c))
    assert len(hits) >= 8 and seen == 18000
    for h in hits:
        for a in h["state"]:
            a.setflags(write=False)
    return hits


def _spread(hits, k):
    """k covering states of different trials where there are as many, the largest contact counts first"""
    out, trials = [], set()
    for h in sorted(hits, key=lambda h: (-h["cov"]["ncon"], h["trial"], h["sub"])):
        if h["trial"] not in trials:
            out.append(h)
            trials.add(h["trial"])
        if len(out) == k:
            return out
    for h in hits:
        if all(h is not x for x in out):
            out.append(h)
        if len(out) == k:
            break
    return out


def _airborne(M, seed=31):
    q = M["qpos0"].copy()
    q[2] = 2.0
    rng = np.random.default_rng(seed)
    return q, rng.normal(0, 0.5, NV), np.zeros(NV)


def _standing(M):
    q = M["qpos0"].copy()
    q[2] -= 0.003
    return q, np.zeros(NV), np.zeros(NV)


def _oracle_substep(o, q, v, w):
    o.reset_data()
    o.qpos[:] = q
    o.qvel[:] = v
    o.arr("qacc_warmstart", NV)[:] = w
    o.step(None, 1)


def test_newton_stage_outputs_on_one_env_batches(oracle, covering):
    """8 one-env batches through physics_step with the stage dump -- 6 covering states, one airborne state (no
    rows) and one standing state (floor contacts only): qfrc_constraint and qacc of the dump at
    test_gpu_parity.py's stage bar (1e-9 relative), the aux row's qacc at its qacc bar (1e-8 scale), ncon and nefc
    equal to the oracle's, and the Newton iteration count within one of the oracle's.

    Why one and not zero: the two solvers share the iteration but not the stopping rules.  The oracle
    (hsim_oracle.c solve_newton) ends an iteration whose line search left the active set unchanged, whatever
    alpha, or whose cost fell by less than 1e-16, or starts none once scale |grad| < 1e-14; the kernel ends an
    iteration only if the set is unchanged AND |alpha - 1| < 1e-3, and starts none once scale |grad| < 1e-13.
    Inside the final active set the cost is quadratic and the Newton step exact, so whichever rule fires first, the
    other solver's fires at the next iteration's top at the latest: the counts differ by at most one, either
    way, and both stand at the same minimiser (the force and qacc bars above).  Without rows the oracle takes
    qacc_smooth and runs no solver (0), the kernel takes one exact Newton step from the warm start (1).
    (Measured: equal in six of the eight states; the second covering state 7 against 8, the airborne one 0
    against 1.)"""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.model import HsModel
    o = oracle
    gb = np.asarray(o.M["geom_bodyid"])
    cases = [("covering", h["state"]) for h in _spread(covering, 6)]
    cases += [("airborne", _airborne(o.M)), ("standing", _standing(o.M))]
    assert len(cases) == 8
    m = HsModel(XML)
    ctrl = torch.zeros(1, NU, device="cuda")
    for i, (kind, (q, v, w)) in enumerate(cases):
        _oracle_substep(o, q, v, w)
        c = _coverage(o, gb)
        if kind == "covering":
            assert _covers(c), (i, c)
        elif kind == "airborne":
            assert c["nefc"] == 0 and c["ncon"] == 0, c
        else:
            assert c["floor"] and not c["bodies"] and not c["tendon"] and not c["joint"] and c["niter"] >= 1, c
        rf, ra = o.get("qfrc_constraint"), o.get("qacc")
        b = HsBatch(m, 1, precision="fp64")
        b.set_state(qpos=q, qvel=v, time=0.0, qacc_warmstart=w)
        b.set_debug(True)
        b.physics_step(ctrl, 1)
        dbg = b.get_debug()
        aux = b.aux.double().cpu().numpy()[0]
        b.close()
        gf, ga = dbg[2360:2360 + NV], dbg[2400:2400 + NV]
        ef = np.abs(gf - rf).max() / (1 + np.abs(rf).max())
        ea = np.abs(ga - ra).max() / (1 + np.abs(ra).max())
        ex = np.abs(aux[:NV] - ra).max() / (1 + np.abs(ra).max())
        print(f"{kind} {i}: ncon {c['ncon']} nefc {c['nefc']} niter {c['niter']} (device {int(dbg[2505])}) "
              f"qfrc_constraint {ef:.2e} qacc {ea:.2e} aux qacc {ex:.2e}")
        assert (int(dbg[2503]), int(dbg[2504])) == (c["ncon"], c["nefc"]), (kind, i)
        assert (int(aux[35]), int(aux[36])) == (c["ncon"], c["nefc"]), (kind, i)
        assert int(dbg[2505]) == int(aux[37]) and abs(int(dbg[2505]) - c["niter"]) <= 1, (kind, i)
        assert ef <= 1e-9 and ea <= 1e-9, (kind, i, ef, ea)
        assert ex <= 1e-8, (kind, i, ex)
        if kind != "airborne":
            assert np.abs(rf).max() > 1.0


def _pair_states(o, covering):
    """8 envs: every pair (2k, 2k + 1) an airborne env beside a loaded (covering) one, the loaded half first in
    two pairs and second in the other two"""
    loaded = _spread(covering, 4)
    qs, vs, ws, kinds = [], [], [], []
    for k, h in enumerate(loaded):
        q, v, w = _airborne(o.M, seed=40 + k)
        pair = [("loaded", h["state"]), ("airborne", (q, v, w))]
        if k % 2:
            pair.reverse()
        for kind, (a, b_, c) in pair:
            qs.append(a); vs.append(b_); ws.append(c); kinds.append(kind)
    return np.stack(qs), np.stack(vs), np.stack(ws), kinds


def test_pairs_whose_halves_differ(oracle, covering):
    """A wave's two halves share the walks' control flow: 8 envs ordered so that each pair holds an airborne env
    (no rows, no contacts) beside a covering one, 4 env steps against OracleHumanoidEnv at
    test_gpu_chain_sums.py's bars (qpos 1e-8, qvel 1e-6, obs 1e-8 relative, reward rel 1e-10 / abs 1e-12)."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.model import HsModel
    from oracle.env import OracleHumanoidEnv
    o = oracle
    gb = np.asarray(o.M["geom_bodyid"])
    qs, vs, ws, kinds = _pair_states(o, covering)
    n, steps = 8, 4
    for i in range(n):      # the first substep of every env is what its kind says
        _oracle_substep(o, qs[i], vs[i], ws[i])
        c = _coverage(o, gb)
        assert _covers(c) if kinds[i] == "loaded" else (c["nefc"] == 0 and c["ncon"] == 0), (i, c)
    assert all(set(kinds[2 * k:2 * k + 2]) == {"loaded", "airborne"} for k in range(4))
    b = HsBatch(HsModel(XML), n, device=0, precision="fp64", seed=0)
    b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1, schedule="direct")
    assert b.schedule_name() == "paired"
    b.reset()
    b.set_state(qpos=qs, qvel=vs, time=0.0, qacc_warmstart=ws)
    cfg = {"model_path": XML, "duration": 10.0, "reward_config": {"type": "stand"}, "frame_skip": 3}
    refs = [OracleHumanoidEnv(cfg) for _ in range(n)]
    for i, r in enumerate(refs):
        r.reset()
        r.sim.qpos[:] = qs[i]
        r.sim.qvel[:] = vs[i]
        r.sim.arr("qacc_warmstart", NV)[:] = ws[i]
        r.sim.d.time = 0.0
    acts = np.random.default_rng(41).uniform(-1, 1, (steps, n, NU)).astype(np.float32)
    dacts = torch.tensor(acts, device="cuda")
    for k in range(steps):
        obs, rew, term, trunc = b.step(dacts[k])
        obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
        st = b.get_state()
        for i, r in enumerate(refs):
            robs, rr, *_ = r.step(acts[k, i])
            eq = np.abs(st["qpos"][i] - r.sim.qpos).max()
            ev = np.abs(st["qvel"][i] - r.sim.qvel).max()
            eo = np.abs(obs[i] - robs).max() / (1 + np.abs(robs).max())
            print(f"step {k} env {i} ({kinds[i]}): qpos {eq:.2e} qvel {ev:.2e} obs {eo:.2e} reward {abs(rew[i] - rr):.2e}")
            assert eq < 1e-8 and ev < 1e-6, (k, i, eq, ev)
            assert eo <= 1e-8, (k, i, eo)
            assert rew[i] == pytest.approx(rr, rel=1e-10, abs=1e-12), (k, i)
    b.close()


def _snapshot(b):
    return [t.clone() for t in (b.obs, b.reward, b.terminated, b.truncated, b.qpos, b.qvel, b.qacc_warmstart, b.time,
                                b.warning, b.aux)]


def test_schedules_and_tape_agree_bitwise_from_covering_states(oracle, covering):
    """5 envs (odd: the last wave's other half is a ghost), 3 env steps from covering states: the paired schedule
    bitwise equals the single-env schedule, and a 3-step tape bitwise equals the step loop."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.model import HsModel
    n, steps = 5, 3
    hits = _spread(covering, n)
    assert len(hits) == n and all(_covers(h["cov"]) for h in hits)
    qs, vs, ws = (np.stack([h["state"][j] for h in hits]) for j in range(3))
    m = HsModel(XML)
    dacts = torch.tensor(np.random.default_rng(43).uniform(-1, 1, (steps, n, NU)).astype(np.float32), device="cuda")

    def make(sched):
        b = HsBatch(m, n, device=0, precision="fp64", seed=12)
        b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1, schedule=sched)
        b.reset()
        b.set_state(qpos=qs, qvel=vs, time=0.0, qacc_warmstart=ws)
        return b

    runs = {}
    for sched in ("direct", "single"):
        b = make(sched)
        assert b.schedule_name() == ("paired" if sched == "direct" else "single")
        tr = []
        for k in range(steps):
            b.step(dacts[k])
            tr.append(_snapshot(b))
        runs[sched] = tr
        b.close()
    for k in range(steps):
        for x, y in zip(runs["direct"][k], runs["single"][k]):
            assert torch.equal(x, y), k
    assert float(runs["direct"][0][9][:, 36].min()) > 0      # every env has constraint rows after the first step
    b = make("auto")
    obs, rew, term, trunc = b.step_tape(dacts)
    for k in range(steps):
        for x, y in zip((obs[k], rew[k], term[k], trunc[k]), runs["direct"][k][:4]):
            assert torch.equal(x, y), k
    for x, y in zip(_snapshot(b), runs["direct"][-1]):
        assert torch.equal(x, y)
    b.close()
