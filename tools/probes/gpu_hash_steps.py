"""Identity probe of the step kernels: one SHA-256 line per case, over every path step_pair has -- the
direct and single schedules, the chunk queue, tape launches, the wide tier, the fused rollout and the
fused evaluation -- at the smallest shapes that reach each.  For A/B builds that must be bitwise equal:
run once per library in fresh processes (HSIM_LIB selects it) and compare the outputs line by line.
    python tools/probes/gpu_hash_steps.py > a.txt; HSIM_LIB=.../libhsim_parent.so python tools/probes/gpu_hash_steps.py > b.txt
Every line hashes the batch's state and output tensors (STATE) plus the case's own outputs."""
import hashlib
import os
import re
import sys
import tempfile
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mujocoposelearning_amd.batch import HsBatch  # noqa: E402
from mujocoposelearning_amd.model import HsModel  # noqa: E402

XML = os.path.join(ROOT, "mujocoposelearning_amd", "assets", "humanoid.xml")
STATE = ("qpos", "qvel", "qacc_warmstart", "time", "step_count", "episode", "total_reward", "warning", "obs",
         "terminal_obs", "reward", "terminated", "truncated", "aux", "terminal_step_count", "terminal_total_reward")
DT = 0.005                  # humanoid.xml's timestep; an env step is 3 substeps
SHORT = 0.08                # duration: the clock after env step 5 (0.005 + 5 * 0.015) is the first >= it


def _add(h, x):
    if isinstance(x, dict):
        for k in sorted(x):
            _add(h, x[k])
    elif isinstance(x, (tuple, list)):
        for y in x:
            _add(h, y)
    elif torch.is_tensor(x):
        h.update(x.detach().cpu().contiguous().numpy().tobytes())
    elif isinstance(x, np.ndarray):
        h.update(np.ascontiguousarray(x).tobytes())
    else:
        h.update(repr(x).encode())


def state(h, b, *extra):
    torch.cuda.synchronize()
    for key in STATE:
        _add(h, b.t[key])
    _add(h, extra)


def emit(name, h):
    print(f"{name} {h.hexdigest()}", flush=True)


def actions(k, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(k, n, 21, generator=g) * 2 - 1).cuda()


def pgs_model(tmp):
    """<option solver="PGS"> on humanoid.xml, MuJoCo's default sweeps (as tests/test_gpu_pgs.py builds it)"""
    src = re.sub(r"<option[^>]*/>", '<option timestep="0.005" solver="PGS" iterations="100" tolerance="1e-08"/>',
                 open(XML).read(), count=1)
    p = os.path.join(tmp, "pgs.xml")
    open(p, "w").write(src)
    return HsModel(p)


def stagger(b, period=3):
    """env i's clock ahead by (i % period) env steps, so that episodes end in different steps of a run"""
    n = b.n
    k = torch.arange(n, device=b.device) % period
    b.t["time"].add_((k * 3 * DT).to(b.dtype))
    b.t["step_count"].add_(k.to(torch.int32))


def run_steps(name, b, acts, **cfg):
    b.configure(frame_skip=3, duration=SHORT, reward_id=0, **cfg)
    b.reset()
    h = hashlib.sha256()
    for a in acts:
        b.step(a)
        state(h, b)
    emit(name, h)


def small_cases(tag, model, prec):
    """n = 5 (the last wave has a ghost half): the single-env schedule (auto) and one wave per pair (direct)"""
    n = 5
    acts = actions(12, n)
    rng = np.random.default_rng(11)
    nq, nv = model.nq, model.nv
    for sched in ("auto", "direct"):
        t = f"{tag}_{sched}"
        b = HsBatch(model, n, precision=prec, seed=7)
        b.configure(frame_skip=3, duration=SHORT, reward_id=0, autoreset=1, schedule=sched)
        h = hashlib.sha256()
        b.reset()
        state(h, b)
        emit(f"{t}_reset", h)
        h = hashlib.sha256()
        b.reset(mask=[0, 1, 0, 1, 0], qpos_noise=rng.uniform(-0.01, 0.01, (n, nq)),
                qvel_noise=rng.uniform(-0.01, 0.01, (n, nv)))
        state(h, b)
        emit(f"{t}_reset_mask", h)
        run_steps(f"{t}_steps_terminate", b, acts, autoreset=1, max_steps=750)
        run_steps(f"{t}_steps_truncate", b, acts, autoreset=1, max_steps=4)
        run_steps(f"{t}_steps_no_autoreset", b, acts, autoreset=0, max_steps=750)
        for r in (0, 1, 2):     # the three reward plug-ins (each reads its own sums)
            b.configure(reward_id=r)
            b.reset()
            h = hashlib.sha256()
            for a in acts[:3]:
                b.step(a)
                state(h, b)
            emit(f"{t}_reward{r}", h)
        b.configure(reward_id=0, max_steps=750, autoreset=1)
        b.reset()
        h = hashlib.sha256()
        b.physics_step(acts[0], 2)
        state(h, b, b.t["ctrl"])
        b.physics_step(None, 3)
        state(h, b, b.t["ctrl"])
        emit(f"{t}_physics_step", h)
        qn, vn = b.set_autoreset_noise(rng.uniform(-0.01, 0.01, (n, nq)), rng.uniform(-0.01, 0.01, (n, nv)))
        run_steps(f"{t}_autoreset_noise", b, acts, autoreset=1, max_steps=750)
        b.set_autoreset_noise(None, None)
        b.close()
    b = HsBatch(model, n, precision=prec, seed=7, full_state=True)
    b.configure(frame_skip=3, duration=SHORT, reward_id=1, autoreset=1)
    b.reset()
    h = hashlib.sha256()
    for a in acts:
        b.step(a)
        state(h, b, b.t["cfrc_ext"], b.t["subtree_linvel"])
    emit(f"{tag}_full_state", h)
    b.close()


def queue_and_tape_cases(tag, model, prec):
    probe = HsBatch(model, 2, precision=prec)
    R = probe.resident_waves
    probe.close()
    nbig = 2 * R + 3
    for sched in ("auto", "fixed_order"):   # chunk queue: first chunk, hand-off, last substep, reset pass
        b = HsBatch(model, nbig, precision=prec, seed=7)
        b.configure(frame_skip=3, duration=SHORT, reward_id=0, autoreset=1, schedule=sched)
        b.reset()
        stagger(b)
        assert b.queued()
        h = hashlib.sha256()
        for a in actions(12, nbig):
            b.step(a)
            state(h, b)
        emit(f"{tag}_queue_{sched}_n{nbig}", h)
        b.close()
    for n in (5, nbig):                     # tape: single-env units / pair units
        for outputs in (True, False):
            b = HsBatch(model, n, precision=prec, seed=7)
            b.configure(frame_skip=3, duration=SHORT, reward_id=0, autoreset=1)
            b.reset()
            stagger(b)
            h = hashlib.sha256()
            for rep in range(2):            # 14 env steps: every env's episode ends inside
                res = b.step_tape(actions(7, n, seed=5 + rep), outputs=outputs)
                state(h, b, [x.clone() for x in res], b.tape_aborts())
            emit(f"{tag}_tape_n{n}_outputs{int(outputs)}", h)
            b.close()


def wide_cases(model):
    """tests/golden's pile-up states (as tests/test_gpu_contacts.py loads them): every env overflows the
    resident tier -- a per-step call defers them to step_kernel_wide, a tape launch aborts and is replayed"""
    d = np.load(os.path.join(ROOT, "tests", "golden", "pileup_states.npz"))
    qs = d["qpos"]
    n = len(qs)
    rng = np.random.default_rng(9)
    vs = rng.normal(0, 0.1, (n, 27))
    for prec in ("fp64", "fp32"):
        b = HsBatch(model, n, precision=prec)
        b.configure(frame_skip=3, duration=10.0, reward_id=0, autoreset=1)
        b.set_state(qpos=qs, qvel=vs, time=0.0, qacc_warmstart=0.0)
        h = hashlib.sha256()
        b.physics_step(actions(1, n)[0], 1)
        state(h, b, b.wide_reruns())
        b.set_state(qpos=qs, qvel=vs, time=0.0, qacc_warmstart=0.0)
        b.step(actions(1, n)[0])
        state(h, b, b.wide_reruns())
        emit(f"{prec}_wide_per_step_reruns{b.wide_reruns()}", h)
        b.set_state(qpos=qs, qvel=vs, time=0.0, qacc_warmstart=0.0)
        h = hashlib.sha256()
        res = b.step_tape(actions(3, n), outputs=True)
        state(h, b, [x.clone() for x in res], b.wide_reruns(), b.tape_aborts())
        emit(f"{prec}_wide_tape_aborts{b.tape_aborts()}", h)
        b.close()


def _vec_env(n, duration):
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    cfg = {"model_path": XML, "duration": duration, "frame_skip": 3, "reward_config": {"type": "stand"}}
    return HumanoidVecEnv(cfg, n_envs=n, model=HsModel(XML), seed=0, precision="fp64")


def _ppo(env, act, H, n_steps):
    from mujocoposelearning_amd.ppo import PPO
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return PPO(env, n_steps=n_steps, batch_size=64, n_epochs=1, seed=0,
                   policy_kwargs={"activation_fn": act, "net_arch": {"pi": [H, H], "vf": [H, H]}})


def rollout_cases():
    probe = _vec_env(2, 10.0)
    R = probe.batch.resident_waves
    probe.close()
    for act, H in (("ReLU", 64), ("Tanh", 128), ("ReLU", 256)):
        for n in (6, 2 * R + 3):
            env = _vec_env(n, 10.0)
            ppo = _ppo(env, act, H, 9)
            # env 1's clock is 4 env steps from the duration (it terminates inside the rollout), env 2's step
            # count 5 from max_steps (it truncates)
            b = env.batch
            b.t["time"][1] = 10.0 - 4 * 3 * DT + DT
            b.t["step_count"][2] = b.cfg.max_steps - 5
            h = hashlib.sha256()
            done = boot = 0
            for it in range(2):   # the second rollout continues from the first
                adv, ret = ppo.collect_rollouts()
                state(h, b, ppo.buf, ppo.ep_acc, ppo.episode_start, ppo._act_clip, ppo.obs, adv, ret)
                done, boot = done + int(ppo.buf["done"].sum()), boot + int(ppo.buf["boot"].sum())
            launches = len(getattr(ppo, "rollout_launches", []))
            emit(f"rollout_{act}{H}_n{n}_launches{launches}_fallbacks{getattr(ppo, 'fused_fallbacks', 0)}_"
                 f"done{done}_boot{boot}", h)
            env.close()


def eval_cases():
    from mujocoposelearning_amd.evaluation import evaluate_policy_device
    for deterministic in (True, False):
        env = _vec_env(6, 0.2)
        ppo = _ppo(env, "Tanh", 64, 2)
        res = evaluate_policy_device(ppo, env, 2, deterministic=deterministic, n_trace=3, seed=5)
        h = hashlib.sha256()
        state(h, env.batch, res.returns, res.lengths, res.end_step, res.trace)
        emit(f"evaluate_deterministic{int(deterministic)}_launches{res.fused_launches}_fallbacks{res.fallbacks}", h)
        env.close()


def main():
    print("# library", os.path.basename(os.environ.get("HSIM_LIB", "libhsim.so")), file=sys.stderr)
    newton = HsModel(XML)
    with tempfile.TemporaryDirectory() as tmp:
        pgs = pgs_model(tmp)
        for prec in ("fp32", "fp64"):
            small_cases(f"{prec}_newton", newton, prec)
            small_cases(f"{prec}_pgs", pgs, prec)
        for prec in ("fp64", "fp32"):
            queue_and_tape_cases(f"{prec}_newton", newton, prec)
        queue_and_tape_cases("fp64_pgs", pgs, "fp64")
    wide_cases(newton)
    rollout_cases()
    eval_cases()


if __name__ == "__main__":
    main()
