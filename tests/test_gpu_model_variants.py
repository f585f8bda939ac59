"""The step kernels on models off humanoid.xml's constraint values (tests/model_variants.py): limit
margins with both rows of a joint active, solimp midpoints and powers other than (0.5, 2), direct solref,
friction other than 1, contact parameters mixed by priority and by solmix, pyramidal body-body contacts
(the wide tier included), frictionless floors, other geom sizes -- against the fp64 oracle on the same XML.

Bounds are tests/test_gpu_parity.py's and tests/test_gpu_contacts.py's, unchanged.  Each test prints its
worst error as a fraction of its bound (profiles/model_variants.md) and asserts, from the oracle, that its
states reach the branches the variant exists for (model_variants.check_coverage).
"""
import numpy as np
import pytest

import model_variants as mv
from test_gpu_contacts import _oracle_step
from test_gpu_parity import _run_oracle, _states

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_model_variants")
    return {name: mv.write_model_variant(d, name) for name in mv.NAMES}


def _substep_fractions(prec, qacc, qpos, qvel, ref):
    """(qacc, qpos, qvel) errors of one env as fractions of test_one_substep_many_states' bounds."""
    rq, rv, ra = ref
    scale = 1 + np.abs(ra).max()
    ea, eq, ev = np.abs(qacc - ra).max(), np.abs(qpos - rq).max(), np.abs(qvel - rv).max()
    if prec == "fp64":
        return ea / (1e-8 * scale), eq / 1e-12, ev / (1e-10 * scale)
    return ea / (2e-3 * scale), eq / (2e-6 + 1e-7 * scale), ev / (1e-5 * scale)


def _step_and_compare(o, model, prec, qs, vs, cs, oracle_step, label):
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    n = len(qs)
    b = HsBatch(model, n, precision=prec)
    b.set_state(qpos=qs, qvel=vs, time=0.0, qacc_warmstart=0.0)
    b.physics_step(torch.tensor(cs, device=b.device), 1)
    st = b.get_state()
    aux = b.aux.double().cpu().numpy()
    worst = np.zeros(3)
    for i in range(n):
        rq, rv, ra, ncon, nefc = oracle_step(o, qs[i], vs[i], cs[i])
        assert int(aux[i, 35]) == ncon and int(aux[i, 36]) == nefc, (i, aux[i, 35:37], ncon, nefc)
        f = np.array(_substep_fractions(prec, aux[i, :27], st["qpos"][i], st["qvel"][i], (rq, rv, ra)))
        assert np.isfinite(f).all(), i
        worst = np.maximum(worst, f)
    print(f"{label} {prec}: worst error / bound: qacc {worst[0]:.2g} qpos {worst[1]:.2g} qvel {worst[2]:.2g}")
    return b, worst


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("name", mv.NAMES)
def test_variant_one_substep_many_states(paths, name, prec):
    """test_gpu_parity.py::test_one_substep_many_states on each variant: its 48 states, its bounds."""
    from mujocoposelearning_amd.model import HsModel
    from oracle.oracle import Oracle
    o = Oracle(paths[name])
    states = _states(o.M, 48, seed=7)
    mv.check_coverage(name, mv.coverage(o, states))
    qs, vs, cs = (np.stack([s[k] for s in states]) for k in range(3))
    b, worst = _step_and_compare(o, HsModel(paths[name]), prec, qs, vs, cs, _run_oracle, name)
    assert (worst <= 1).all(), worst
    assert b.warning.sum().item() == 0


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_wide_tier_pyramidal_body_body_contacts(paths, prec):
    """test_gpu_contacts.py::test_wide_tier_lying_states_match_oracle on the contact variant: 16 lying states
    that overflow the resident tier, fit the wide one and have >= 2 body-body contacts, each 4 dense rows."""
    from mujocoposelearning_amd.model import HsModel
    from oracle.oracle import Oracle
    o = Oracle(paths["contact"])
    big, draws = mv.wide_body_body_states(o, 16, seed=1)
    assert draws <= 20000
    qs = np.stack(big)
    n = len(qs)
    rng = np.random.default_rng(5)
    vs = rng.normal(0, 0.3, (n, 27))
    cs = rng.uniform(-1, 1, (n, 21)).astype(np.float32)
    b, worst = _step_and_compare(o, HsModel(paths["contact"]), prec, qs, vs, cs, _oracle_step, "contact wide tier")
    assert b.wide_capacity == (64, 256) and b.resident_capacity == (32, 128)
    assert b.warning.sum().item() == 0
    assert b.wide_reruns() == 16
    assert (worst <= 1).all(), worst


@pytest.mark.parametrize("name", mv.NAMES)
def test_variant_fp64_100_substeps_within_chaos_envelope(paths, name):
    """test_gpu_parity.py::test_fp64_1000_substeps_within_chaos_envelope's rule over 100 substeps of each
    variant, one env: from qpos0 lowered 3 mm (the feet penetrate), seeded U(-1, 1) controls; every 10
    substeps |dqpos| <= max(1e-9, 20 x the oracle's own +-1e-15 perturbation envelope)."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.model import HsModel
    from oracle.oracle import Oracle
    nsub, every = 100, 10
    rng = np.random.default_rng(13)
    ref = Oracle(paths[name])
    q = ref.M["qpos0"].copy()
    q[2] -= 0.003
    v = rng.uniform(-0.01, 0.01, 27)          # nonzero, so that the relative perturbation perturbs
    tape = rng.uniform(-1, 1, (nsub, 21)).astype(np.float32)
    pert = [Oracle(paths[name]) for _ in range(2)]
    for o, p in zip([ref] + pert, (0.0, 1e-15, -1e-15)):
        o.qpos[:] = q
        o.qvel[:] = v * (1 + p)
    b = HsBatch(HsModel(paths[name]), 1, precision="fp64")
    b.set_state(qpos=q, qvel=v, time=0.0, qacc_warmstart=0.0)
    c = torch.tensor(tape, device=b.device)
    checked, worst, rows = 0, 0.0, 0
    for s in range(nsub):
        b.physics_step(c[s:s + 1], 1)
        for o in [ref] + pert:
            o.step(tape[s].astype(np.float64), 1)
        rows = max(rows, ref.d.nefc)
        if (s + 1) % every == 0:
            env = max(np.abs(o.qpos - ref.qpos).max() for o in pert)
            if env > 1e-4:
                break
            bound = max(1e-9, 20 * env)
            err = np.abs(b.get_state()["qpos"][0] - ref.qpos).max()
            assert err <= bound, (s + 1, err, bound)
            worst = max(worst, err / bound)
            checked += 1
    print(f"{name} fp64 trajectory: {checked} checkpoints, worst error / bound {worst:.3g}, max rows {rows}")
    assert checked >= 5
    assert rows > 0


def test_limits_variant_env_steps_match_the_oracle_env(paths):
    """test_gpu_lane_table.py::test_variant_model_matches_the_oracle on the limits variant, at its bars: 8
    envs, 4 env steps through HsBatch.step, so obs and reward run on a model whose limit rows differ (from
    the standing reset both rows of abdomen_x and the knees' upper rows are inside the margin)."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.model import HsModel
    from oracle.env import OracleHumanoidEnv
    n, steps = 8, 4
    m = HsModel(paths["limits"])
    b = HsBatch(m, n, device=0, precision="fp64", seed=0)
    b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1)
    rng = np.random.default_rng(5)
    pn, vn = rng.uniform(-0.01, 0.01, (n, m.nq)), rng.uniform(-0.01, 0.01, (n, m.nv))
    b.reset(qpos_noise=pn, qvel_noise=vn)
    acts = np.random.default_rng(6).uniform(-1, 1, (steps, n, 21)).astype(np.float32)
    dacts = torch.tensor(acts, device="cuda")
    cfg = {"model_path": paths["limits"], "duration": 10.0, "reward_config": {"type": "stand"}, "frame_skip": 3}
    refs = [OracleHumanoidEnv(cfg) for _ in range(n)]
    for i, r in enumerate(refs):
        r.reset(pos_noise=pn[i], vel_noise=vn[i])
    limit_rows = 0
    worst = np.zeros(3)
    for k in range(steps):
        obs, rew, term, trunc = b.step(dacts[k])
        obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
        st = b.get_state()
        for i, r in enumerate(refs):
            robs, rr, *_ = r.step(acts[k, i])
            limit_rows += int((r.sim.arr("efc_type", r.sim.d.nefc) <= mv.LIMIT_TENDON).sum())
            eq = np.abs(st["qpos"][i] - r.sim.qpos).max()
            ev = np.abs(st["qvel"][i] - r.sim.qvel).max()
            eo = np.abs(obs[i] - robs).max() / (1 + np.abs(robs).max())
            worst = np.maximum(worst, [eq / 1e-8, ev / 1e-6, eo / 1e-8])
            assert eq < 1e-8 and ev < 1e-6, (k, i, eq, ev)
            assert eo <= 1e-8, (k, i, eo)
            assert rew[i] == pytest.approx(rr, rel=1e-10, abs=1e-12), (k, i)
        assert not term.any() and not trunc.any()
    print(f"limits env steps fp64: worst error / bound: qpos {worst[0]:.3g} qvel {worst[1]:.3g} obs {worst[2]:.3g}; "
          f"{limit_rows} limit rows")
    assert limit_rows >= 2 * n * steps          # at least abdomen_x's two rows, every env and step
    b.close()
