"""Policy evaluation over whole episodes (evaluation.evaluate_policy_device): 4096 envs, `stand`, fp64,
duration 10 (667 env steps), one episode per env, pi nets [64, 64] and [256, 256], ReLU and Tanh -- as
hs_evaluate launches (fused) and with ppo.FUSED_ROLLOUT = False (the same loop one step_tensors at a time:
net_forward, clamp, step_tensors -- the building blocks from before hs_evaluate, so the before figure),
the two alternating, each run synchronised.  The fused runs also report the kernel time of their launches
(hs_last_tape_ms).  Prints one JSON line per net and a last line with all of them.
    python tools/probes/gpu_evaluate.py [--repeats 3] [--warmup 1] [--widths 64,256] [--activations ReLU,Tanh]
                                        [--deterministic 1]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_ENVS = 4096


def measure(P, E, env_factory, H, activation, repeats, warmup, deterministic):
    import torch
    env = env_factory()
    ppo = P.PPO(env, n_steps=2, batch_size=4096, n_epochs=1, seed=0,     # (only its policy is used)
                policy_kwargs={"activation_fn": activation, "net_arch": {"pi": [H, H], "vf": [H, H]}})
    last = {}

    def once(fused):
        P.FUSED_ROLLOUT = fused
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = E.evaluate_policy_device(ppo, env, 1, deterministic=deterministic)
            torch.cuda.synchronize()
            last[fused] = res
            return time.perf_counter() - t0, sum(res.kernel_ms) * 1e-3
        finally:
            P.FUSED_ROLLOUT = True

    for _ in range(warmup):
        once(True)
        once(False)
    t = {True: [], False: []}
    for _ in range(repeats):
        for fused in (True, False):
            t[fused].append(once(fused))
    steps = last[True].env_steps
    env.close()

    def stats(ts):
        r = [steps / x for x in ts]
        return {"env_steps_per_s_mean": statistics.mean(r), "env_steps_per_s_min": min(r),
                "env_steps_per_s_max": max(r), "seconds": ts}

    f, s = last[True], last[False]
    return {"hidden": H, "activation": activation, "deterministic": bool(deterministic), "env_steps": steps,
            "fused_launches": f.fused_launches, "fallbacks": f.fallbacks,
            "step_by_step_launches": s.fused_launches,
            "mean_return_fused": float(f.returns.mean()), "mean_return_step_by_step": float(s.returns.mean()),
            "fused": stats([x[0] for x in t[True]]), "fused_kernel": stats([x[1] for x in t[True]]),
            "step_by_step": stats([x[0] for x in t[False]])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--widths", default="64,256")
    ap.add_argument("--activations", default="ReLU,Tanh")
    ap.add_argument("--deterministic", type=int, default=1)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from mujocoposelearning_amd import evaluation as E
    from mujocoposelearning_amd import ppo as P
    from mujocoposelearning_amd.model import HsModel
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    xml = os.path.join(ROOT, "mujocoposelearning_amd", "assets", "humanoid.xml")

    def env_factory():
        return HumanoidVecEnv({"model_path": xml, "duration": 10.0, "frame_skip": 3,
                               "reward_config": {"type": "stand"}},
                              n_envs=N_ENVS, model=HsModel(xml), seed=0, precision="fp64")

    rows = []
    for act in a.activations.split(","):
        for H in [int(w) for w in a.widths.split(",")]:
            rows.append(measure(P, E, env_factory, H, act, max(a.repeats, 1), a.warmup, a.deterministic))
            print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"n_envs": N_ENVS, "episodes_per_env": 1, "nets": rows}), flush=True)


if __name__ == "__main__":
    main()
