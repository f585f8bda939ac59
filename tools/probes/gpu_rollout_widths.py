"""collect_rollouts at the hidden widths the fused rollout runs (64 / 128 / 256, both hidden layers,
ReLU or Tanh): 4096 envs, `stand`, fp64, staggered episode clocks, n_steps = 32 -- as hs_rollout launches
(fused) and with ppo.FUSED_ROLLOUT = False (the per-step loop), the two alternating, each repeat
synchronised.  Prints one JSON line per width and a last line with all of them.
    python tools/probes/gpu_rollout_widths.py [--repeats 5] [--warmup 2] [--widths 64,128,256]
                                              [--activation ReLU|Tanh] [--root CHECKOUT] [--label NAME]
--root: import the package from another checkout (an A/B against another build of the library; a
build without the fused Tanh rollout reports runs_fused false, and both of its columns are its
per-step path)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_ENVS, N_STEPS = 4096, 32


def measure(P, env_factory, H, repeats, warmup, activation="ReLU"):
    import torch
    env = env_factory()
    ppo = P.PPO(env, n_steps=N_STEPS, batch_size=4096, n_epochs=1, seed=0, stagger_episodes=True,
                policy_kwargs={"activation_fn": activation, "net_arch": {"pi": [H, H], "vf": [H, H]}})
    ppo.policy.pack_heads()
    runs_fused = ppo._fused_rollout_args() is not None     # False: "fused" below is the per-step path too

    def once(fused):
        P.FUSED_ROLLOUT = fused
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ppo.collect_rollouts()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        finally:
            P.FUSED_ROLLOUT = True

    for _ in range(warmup):
        once(True)
        once(False)
    t = {True: [], False: []}
    for _ in range(repeats):
        for fused in (True, False):
            t[fused].append(once(fused))
    env.close()
    steps = N_ENVS * N_STEPS

    def stats(ts):
        r = [steps / x for x in ts]
        return {"env_steps_per_s_mean": statistics.mean(r), "env_steps_per_s_min": min(r),
                "env_steps_per_s_max": max(r), "seconds": ts}

    return {"hidden": H, "activation": activation, "runs_fused": runs_fused,
            "rollout_launches": len(getattr(ppo, "rollout_launches", [])), "fused_fallbacks": getattr(ppo, "fused_fallbacks", 0),
            "fused": stats(t[True]), "per_step": stats(t[False])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--widths", default="64,128,256")
    ap.add_argument("--activation", choices=("ReLU", "Tanh"), default="ReLU")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    from mujocoposelearning_amd import ppo as P
    from mujocoposelearning_amd.model import HsModel
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    xml = os.path.join(root, "mujocoposelearning_amd", "assets", "humanoid.xml")

    def env_factory():
        return HumanoidVecEnv({"model_path": xml, "duration": 10.0, "frame_skip": 3,
                               "reward_config": {"type": "stand"}},
                              n_envs=N_ENVS, model=HsModel(xml), seed=0, precision="fp64")

    rows = []
    for H in [int(w) for w in a.widths.split(",")]:
        rows.append(measure(P, env_factory, H, max(a.repeats, 1), a.warmup, a.activation))
        print(json.dumps(dict(rows[-1], label=a.label)), flush=True)
    print(json.dumps({"label": a.label, "activation": a.activation, "n_envs": N_ENVS, "n_steps": N_STEPS, "widths": rows}), flush=True)


if __name__ == "__main__":
    main()
