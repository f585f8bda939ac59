"""The fp64 resident-tier step kernels read the operands of their dof-chain and subtree sums a group of
bits per LDS round trip (csrc/hs_bits.h for_bit_groups, csrc/hs_lanes.h for_bits_g): the subtree sum of
mass_matrix(), the four sums of velocity_forces(), map_vx() and post_constraint()'s subtree sum.  Every lane
still does the bit-by-bit walk's operations in its order, so the bars are the ones the walk already met.

humanoid.xml's lanes hold masks of 0 set bits (the world body), 1, and every length up to 15 dofs (a foot's
chain) and 16 bodies (the root's subtree): 15 is a multiple of a group of 3 and of no other size in {2, 3, 4}.
Two variants with the left arm moved down the left leg reach the other remainders: on the shin the longest
chain is 16 dofs (a multiple of 2 and 4, not of 3), on the foot 18 (a multiple of 2 and 3, not of 4).
"""
import numpy as np
import pytest

from conftest import XML

pytestmark = pytest.mark.gpu

ARM_ONTO = {
    # the text the arm goes in front of: the closing tags from the named body outwards
    "shin": "            </body>\n          </body>\n        </body>\n      </body>\n",
    "foot": "              </body>\n            </body>\n          </body>\n        </body>\n      </body>\n",
}
LONGEST = {"stock": 15, "shin": 16, "foot": 18}


def write_tree_variant(tmp_path, onto):
    """humanoid.xml with upper_arm_left (and its lower arm and hand) a child of shin_left / foot_left instead of
    the torso: the same bodies, joints and actuators in another tree; returns its path."""
    src = open(XML).read()
    a = src.index('      <body name="upper_arm_left"')
    e = src.index("    </body>\n  </worldbody>")
    arm, src = src[a:e], src[:a] + src[e:]
    assert src.count(ARM_ONTO[onto]) == 1
    i = src.index(ARM_ONTO[onto])
    p = tmp_path / f"humanoid_arm_on_{onto}.xml"
    p.write_text(src[:i] + arm + src[i:])
    return str(p)


@pytest.fixture(scope="module")
def xmls(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_chain_sums")
    return {"stock": XML, "shin": write_tree_variant(d, "shin"), "foot": write_tree_variant(d, "foot")}


def _mask_sizes(M):
    """Set bits of every body lane's dof-chain mask and subtree mask, from the oracle's model."""
    nb, nv = int(M["nbody"]), int(M["nv"])
    par, dofbody = np.asarray(M["dof_parentid"]), np.asarray(M["dof_bodyid"])
    depth = np.zeros(nv, int)
    for j in range(nv):
        depth[j] = 1 + (depth[par[j]] if par[j] >= 0 else 0)
    chain = [max([depth[j] for j in range(nv) if dofbody[j] == b], default=None) for b in range(nb)]
    bpar = np.asarray(M["body_parentid"])
    for b in range(1, nb):                         # a body without dofs of its own has its parent's chain
        if chain[b] is None:
            chain[b] = chain[bpar[b]]
    chain[0] = 0
    sub = np.ones(nb, int)
    for b in range(nb - 1, 0, -1):
        sub[bpar[b]] += sub[b]
    return chain, list(sub[1:])


def _actions(n, steps, seed):
    import torch
    a = np.random.default_rng(seed).uniform(-1, 1, (steps, n, 21)).astype(np.float32)
    return a, torch.tensor(a, device="cuda")


def _snapshot(b):
    return [t.clone() for t in (b.obs, b.reward, b.terminated, b.truncated, b.qpos, b.qvel, b.qacc_warmstart, b.time,
                                b.warning, b.aux)]


@pytest.mark.parametrize("which", ["stock", "shin", "foot"])
def test_env_steps_match_the_oracle(xmls, which):
    """8 envs, 4 env steps of seeded U(-1, 1) actions against OracleHumanoidEnv on the same XML, at
    test_gpu_lane_table.py's bars: qpos 1e-8, qvel 1e-6, obs 1e-8 relative, reward rel 1e-10 / abs 1e-12."""
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.model import HsModel
    from oracle.env import OracleHumanoidEnv
    from oracle.oracle import Oracle
    xml = xmls[which]
    chain, sub = _mask_sizes(Oracle(xml).M)
    assert max(chain) == LONGEST[which] and max(sub) == 16 and chain[0] == 0 and 1 in sub
    if which == "stock":                            # every chain length the humanoid has, every group boundary
        assert set(chain) >= {0, 6, 9, 12, 13, 15} and set(sub) >= {1, 2, 3, 7, 8, 16}
    n, steps = 8, 4
    m = HsModel(xml)
    b = HsBatch(m, n, device=0, precision="fp64", seed=0)
    b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1)
    rng = np.random.default_rng(15)
    pn, vn = rng.uniform(-0.01, 0.01, (n, m.nq)), rng.uniform(-0.01, 0.01, (n, m.nv))
    b.reset(qpos_noise=pn, qvel_noise=vn)
    acts, dacts = _actions(n, steps, 16)
    cfg = {"model_path": xml, "duration": 10.0, "reward_config": {"type": "stand"}, "frame_skip": 3}
    refs = [OracleHumanoidEnv(cfg) for _ in range(n)]
    for i, r in enumerate(refs):
        r.reset(pos_noise=pn[i], vel_noise=vn[i])
    for k in range(steps):
        obs, rew, term, trunc = b.step(dacts[k])
        obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
        st = b.get_state()
        for i, r in enumerate(refs):
            robs, rr, *_ = r.step(acts[k, i])
            eq = np.abs(st["qpos"][i] - r.sim.qpos).max()
            ev = np.abs(st["qvel"][i] - r.sim.qvel).max()
            eo = np.abs(obs[i] - robs).max() / (1 + np.abs(robs).max())
            print(f"{which} step {k} env {i}: qpos {eq:.2e} qvel {ev:.2e} obs {eo:.2e} reward {abs(rew[i] - rr):.2e}")
            assert eq < 1e-8 and ev < 1e-6, (k, i, eq, ev)
            assert eo <= 1e-8, (k, i, eo)
            assert rew[i] == pytest.approx(rr, rel=1e-10, abs=1e-12), (k, i)
    b.close()


@pytest.mark.parametrize("which", ["stock", "shin", "foot"])
def test_stage_dump_of_the_sums(xmls, which):
    """One state through the stage dump: cvel (the chain sum of velocity_forces), qM (from the subtree sum of
    cinert) and qfrc_smooth (the chain sums of cdof_dot and cacc and the subtree sum of cfrc) against the
    oracle at test_gpu_parity.py's stage bar, 1e-9 relative."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.model import HsModel
    from oracle.oracle import Oracle
    o = Oracle(xmls[which])
    rng = np.random.default_rng(21)
    q = o.M["qpos0"].copy()
    q[7:] += rng.uniform(-0.5, 0.5, 21)
    quat = rng.normal(size=4)
    q[3:7] = quat / np.linalg.norm(quat)
    q[2] = 1.1
    v, c = rng.normal(0, 0.5, 27), rng.uniform(-1.2, 1.2, 21).astype(np.float32)
    b = HsBatch(HsModel(xmls[which]), 1, precision="fp64")
    b.set_state(qpos=q, qvel=v, time=0.0, qacc_warmstart=0.0)
    b.set_debug(True)
    b.physics_step(torch.tensor(c[None], device=b.device), 1)
    dbg = b.get_debug()
    o.reset_data()
    o.qpos[:] = q
    o.qvel[:] = v
    o.step(c.astype(np.float64), 1)
    nb, nv = 17, 27
    for name, g, r in (("qM", dbg[700:700 + 1024].reshape(32, 32)[:nv, :nv], o.get("qM")),
                       ("cvel", dbg[1800:1800 + nb * 6].reshape(nb, 6), o.get("cvel")),
                       ("qfrc_smooth", dbg[2320:2320 + nv], o.get("qfrc_smooth"))):
        err = np.abs(g - r).max() / (1 + np.abs(r).max())
        print(f"{which} {name}: {err:.2e}")
        assert np.abs(r).max() > 0.1 and err <= 1e-9, name
    b.close()


def test_schedules_and_tape_agree_bitwise():
    """5 envs (odd count: a ghost half whose lanes hold no bits), 3 steps: the paired schedule bitwise equals the
    single-env schedule, and a 3-step tape (a queue launch) bitwise equals the step loop."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.model import HsModel
    n, steps = 5, 3
    m = HsModel(XML)
    _, dacts = _actions(n, steps, 18)

    def make(sched):
        b = HsBatch(m, n, device=0, precision="fp64", seed=12)
        b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1, schedule=sched)
        b.reset()
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
    b = make("auto")
    obs, rew, term, trunc = b.step_tape(dacts)
    for k in range(steps):
        for x, y in zip((obs[k], rew[k], term[k], trunc[k]), runs["direct"][k][:4]):
            assert torch.equal(x, y), k
    for x, y in zip(_snapshot(b), runs["direct"][-1]):
        assert torch.equal(x, y)
    b.close()


def test_full_state_sums_match_the_oracle():
    """4 full-state envs from the keyframes pressed into the floor, 3 substeps each: cfrc_ext and subtree_linvel
    (post_constraint's subtree sum of m v and of the masses) against the oracle at test_gpu_full_state.py's
    bar, 1e-8 relative."""
    import torch
    from mujocoposelearning_amd.batch import HsBatch
    from mujocoposelearning_amd.model import HsModel
    from oracle.oracle import Oracle
    n, steps = 4, 3
    M = Oracle(XML).M
    keys = list(M["keyframes"].values())
    rng = np.random.default_rng(25)
    q = np.stack([keys[i % len(keys)].copy() for i in range(n)])
    q[:, 2] -= 0.004
    q[:, 7:] += rng.uniform(-0.05, 0.05, (n, 21))
    v = rng.normal(0, 0.3, (n, 27))
    c = rng.uniform(-1, 1, (steps, n, 21)).astype(np.float32)
    b = HsBatch(HsModel(XML), n, precision="fp64", full_state=True)
    b.set_state(qpos=q, qvel=v, time=0.0, qacc_warmstart=0.0)
    refs = []
    for i in range(n):
        o = Oracle(XML)
        o.qpos[:] = q[i]
        o.qvel[:] = v[i]
        refs.append(o)
    contact = False
    for k in range(steps):
        b.physics_step(torch.tensor(c[k], device=b.device), 1)
        cf, lv = b.cfrc_ext.cpu().numpy(), b.subtree_linvel.cpu().numpy()
        for i, o in enumerate(refs):
            o.step(c[k, i].astype(np.float64), 1, full=True)
            rc, rl = o.get("cfrc_ext"), o.get("subtree_linvel")
            ec = np.abs(cf[i] - rc).max() / (1 + np.abs(rc).max())
            el = np.abs(lv[i] - rl).max() / (1 + np.abs(rl).max())
            print(f"substep {k} env {i}: cfrc_ext {ec:.2e} subtree_linvel {el:.2e}")
            assert ec <= 1e-8 and el <= 1e-8, (k, i, ec, el)
            contact |= bool(np.abs(rc).max() > 1.0)
            assert np.abs(rl).max() > 1e-3
    assert contact
    b.close()
