"""What a termination condition costs per env step (profiles/termination.md): 4096 fp64 envs, 'stand', a cycled
U(-1, 1) action tape, HumanoidVecEnv.step_tensors timed with HIP events over three windows of --steps steps.
python tools/probes/gpu_termination_timing.py --term 1     # with "fallen": step + outcome launch + masked reset
python tools/probes/gpu_termination_timing.py --term 0     # without a condition: the one step launch
With --term 1 the launches are then timed on their own, on the state the loop left: the outcome launch
(apply_termination), a masked reset of as many envs as ended per step on average, one with an empty mask, and the
step alone (condition cleared, auto-reset off: what launch 1 is).  --fused 1 (with --term 1) sets "fused": True and
also times the same tape as HsBatch.step_tape launches of --tape env steps (one fused launch each), per env step.
--root DIR measures another checkout of the
project (e.g. the parent commit's, with --term 0).  Prints one JSON line; times in microseconds."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--term", type=int, default=0)
ap.add_argument("--fused", type=int, default=0)
ap.add_argument("--tape", type=int, default=32)
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=667)
ap.add_argument("--warmup", type=int, default=100)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mujocoposelearning_amd.model import HsModel  # noqa: E402
from mujocoposelearning_amd.vec_env import HumanoidVecEnv  # noqa: E402

XML = os.path.join(ROOT, "mujocoposelearning_amd", "assets", "humanoid.xml")
cfg = {"model_path": XML, "duration": 10.0, "frame_skip": 3, "reward_config": {"type": "stand"}}
if args.term:
    cfg["termination"] = {"type": "fallen", "params": {"min_height": 0.8}, "grace_steps": 1}
    if args.fused:
        cfg["termination"]["fused"] = True
env = HumanoidVecEnv(cfg, n_envs=args.envs, model=HsModel(XML), seed=0, precision="fp64")
dev = env.device
tape = torch.tensor(np.random.default_rng(0).uniform(-1, 1, (64, args.envs, 21)), dtype=torch.float32, device=dev)
env.reset_tensors()


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for k in range(n):
        fn(k)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / n * 1e3      # us per call


ends = torch.zeros((), dtype=torch.int64, device=dev)


def step(k):
    _, _, te, tr = env.step_tensors(tape[k % 64])
    ends.add_(((te != 0) | (tr != 0)).sum())


timed(step, args.warmup)
ends.zero_()
windows = [timed(step, args.steps) for _ in range(3)]
res = {"root": ROOT, "term": args.term, "envs": args.envs, "steps": args.steps, "step_tensors_us": windows,
       "episode_ends_per_step": float(ends.item()) / (3 * args.steps),
       "mean_height": float(env.batch.qpos[:, 2].mean().item())}
if args.term and args.fused:      # the same tape as fused launches of --tape env steps, from the loop's end state
    b, K = env.batch, args.tape
    n_launch = max(1, args.steps // K)
    aborts = b.tape_aborts()
    timed(lambda k: b.step_tape(tape[:K], outputs=False), 3)
    res["tape_steps"] = K
    res["tape_launch_us_per_env_step"] = [timed(lambda k: b.step_tape(tape[:K], outputs=False), n_launch) / K
                                          for _ in range(3)]
    res["tape_aborts"] = b.tape_aborts() - aborts
if args.term:
    b = env.batch
    res["outcome_launch_us"] = [timed(lambda k: b.apply_termination(), 200) for _ in range(3)]
    n_end = max(1, int(round(res["episode_ends_per_step"])))
    mask = torch.zeros(args.envs, dtype=torch.uint8, device=dev)
    mask[torch.randperm(args.envs, device=dev)[:n_end]] = 1
    res["masked_reset_us"] = {"envs_reset": n_end, "us": [timed(lambda k: b.reset(mask=mask), 200) for _ in range(3)]}
    empty = torch.zeros(args.envs, dtype=torch.uint8, device=dev)
    res["masked_reset_empty_us"] = [timed(lambda k: b.reset(mask=empty), 200) for _ in range(3)]
    b.set_termination(None)
    b.configure(autoreset=0)
    res["step_alone_us"] = [timed(lambda k: b.step(tape[k % 64]), 100)]
print(json.dumps(res))
