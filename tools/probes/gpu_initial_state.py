"""What a bank of initial states costs (profiles/initial_states.md): 4096 fp64 envs, 'stand', 10 s episodes with
the episode clocks staggered (about six envs reset in every env step), PPO.collect_rollouts on the fused path
(hs_rollout launches, 32-step rollouts, the default [256, 256] ReLU nets), timed with a host clock around
synchronised windows of --rollouts rollouts.
python tools/probes/gpu_initial_state.py
Legs, each on a fresh env with the same seed: unbound, (a) the four model keyframes + default, (b) the golden
trajectory, (c) prone + supine only, unbound again.  Per leg: env steps/s of each window, the fused launches that
aborted on a resident-tier overflow and were replayed step by step (tape_aborts), the env steps the wide tier
re-ran (wide_reruns), the trainer's fallbacks, and the mean height of the envs at most two env steps into an
episode when the leg ends (where the episodes began).  Prints one JSON line per leg."""
import argparse
import json
import os
import sys
import time
import warnings

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--n-steps", type=int, default=32)
ap.add_argument("--rollouts", type=int, default=8)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--legs", default="unbound,keyframes,trajectory,floor,unbound")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from mujocoposelearning_amd.model import HsModel  # noqa: E402
from mujocoposelearning_amd.ppo import PPO  # noqa: E402
from mujocoposelearning_amd.vec_env import HumanoidVecEnv  # noqa: E402

XML = os.path.join(ROOT, "mujocoposelearning_amd", "assets", "humanoid.xml")
TRAJ = os.path.join(ROOT, "tests", "golden", "humanoid_trajectory.xml")
SPECS = {"unbound": None,
         "keyframes": {"keyframes": ["squat", "stand_on_left_leg", "prone", "supine", "default"]},
         "trajectory": {"trajectory": TRAJ},
         "floor": {"keyframes": ["prone", "supine"]}}

for leg in args.legs.split(","):
    cfg = {"model_path": XML, "duration": 10.0, "frame_skip": 3, "reward_config": {"type": "stand"}}
    if SPECS[leg] is not None:
        cfg["initial_state"] = SPECS[leg]
    env = HumanoidVecEnv(cfg, n_envs=args.envs, model=HsModel(XML), seed=0, precision="fp64")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ppo = PPO(env, n_steps=args.n_steps, batch_size=4096, n_epochs=1, seed=0)
    ppo.policy.pack_heads()
    assert ppo._fused_rollout_args() is not None, "the fused rollout does not apply"
    env.stagger_episode_clocks()
    b = env.batch
    rows = 0 if b.initial_states is None else len(b.initial_states[0])

    def window(n):
        torch.cuda.synchronize(env.device)
        t0 = time.perf_counter()
        for _ in range(n):
            ppo.collect_rollouts()
        torch.cuda.synchronize(env.device)
        return n * args.n_steps * args.envs / (time.perf_counter() - t0)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        window(args.warmup)
        aborts0, wide0, fb0 = b.tape_aborts(), b.wide_reruns(), getattr(ppo, "fused_fallbacks", 0)
        rates = [window(args.rollouts) for _ in range(args.windows)]
    fresh = b.t["step_count"] <= 2
    print(json.dumps({"leg": leg, "rows": rows, "envs": args.envs, "n_steps": args.n_steps,
                      "env_steps_per_s": [round(r) for r in rates],
                      "tape_aborts": b.tape_aborts() - aborts0, "wide_reruns": b.wide_reruns() - wide0,
                      "fused_fallbacks": getattr(ppo, "fused_fallbacks", 0) - fb0,
                      "episodes_begun": int(b.t["episode"].sum().item()),
                      "fresh_envs": int(fresh.sum().item()),
                      "fresh_height_mean": round(float(b.t["qpos"][:, 2][fresh].mean().item()), 3),
                      "warnings": b.t["warning"].sum(0).tolist()}), flush=True)
    env.close()
    del ppo, env
