"""The device render path against the host renderer, same process, same box (profiles/render_device.md).

Workloads:
* episode: one traced 10 s episode of an untrained [64, 64] Tanh policy (fp64, frame_skip 3, 667 env
  steps), drawn at 60 fps, 480x640, `side` camera -- the reference's video (custom_env.py:273-321).  The
  frames are picked as evaluation.record_episode picks them but not cut at a done (the env auto-resets
  and the trace goes on), so the workload is the same 601 frames (60 fps over 10.005 s) whatever the policy does.
* get_images: HumanoidVecEnv.get_images at 96x128 for 64 and for 4096 envs, 20 random steps after the
  reset.

Per workload: the host path (render.Renderer over one hs_kinematics call per frame) at its own pace --
for the episode and for the 4096 envs a sample of frames, extrapolated by the frame count and marked so
-- and the device path after a warm-up: a host clock around kinematics launch + render launch + device-to-
host copy, ending in a synchronise, and the three parts from HIP events on the stream.  The sampled
frames are also compared (max level difference device / host).  Prints one JSON line per workload.
    python tools/probes/gpu_render_timing.py [--repeats 3] [--host-frames 20] [--envs 64,4096]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def device_parts(torch, renderer, poses, camera, repeats):
    """poses() -> kinematics records.  Returns per-repeat (total_s, kin_ms, render_ms, copy_ms) and the frames."""
    out, frames = [], None
    for k in range(repeats + 1):                     # the first run is the warm-up
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        kin = poses()
        ev[1].record()
        rgb = renderer.render_kin(kin, camera=camera)
        ev[2].record()
        frames = rgb.cpu().numpy()
        ev[3].record()
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        if k:
            out.append((total, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])))
    return out, frames


def summary(parts, n_frames, nbytes):
    col = lambda i: [p[i] for p in parts]   # noqa: E731
    ms = lambda v: {"mean": statistics.mean(v), "min": min(v), "max": max(v)}   # noqa: E731
    return {"frames": n_frames, "output_bytes": nbytes, "total_s": ms(col(0)), "kinematics_ms": ms(col(1)),
            "render_ms": ms(col(2)), "copy_ms": ms(col(3))}


def host_frames(R, batch, camera, H, W, model, poses):
    """poses: a list of callables returning batch.kinematics(...) dicts.  Returns (seconds, frames)."""
    import numpy as np
    r = R.Renderer(model, height=H, width=W)
    t0 = time.perf_counter()
    out = []
    for p in poses:
        r.update_scene_pose(p(), batch, camera=camera)
        out.append(r.render())
    return time.perf_counter() - t0, np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=20)
    ap.add_argument("--envs", default="64,4096")
    ap.add_argument("--skip-episode", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import warnings

    import numpy as np
    import torch

    from mujocoposelearning_amd import evaluation as E
    from mujocoposelearning_amd import render as R
    from mujocoposelearning_amd.model import HUMANOID_XML, HsModel
    from mujocoposelearning_amd.ppo import PPO
    from mujocoposelearning_amd.vec_env import HumanoidVecEnv
    if not torch.cuda.is_available():
        raise SystemExit("gpu_render_timing: needs the GPU (no CPU fallback: a CPU time says nothing here)")
    model = HsModel(HUMANOID_XML)
    results = []

    def diff(dev, host):
        return int(np.abs(dev.astype(int) - host.astype(int)).max())

    if not a.skip_episode:
        H, W, fps, camera = 480, 640, 60, "side"
        env = HumanoidVecEnv({"model_path": HUMANOID_XML, "duration": 10.0, "frame_skip": 3,
                              "reward_config": {"type": "walk"}}, n_envs=1, model=model, precision="fp64")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ppo = PPO(env, n_steps=2, batch_size=2, n_epochs=1, seed=0,
                      policy_kwargs={"activation_fn": "Tanh", "net_arch": {"pi": [64, 64], "vf": [64, 64]}})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = E.evaluate_policy_device(ppo, env, 1, deterministic=True, n_trace=1)
        torch.cuda.synchronize()
        episode_s = time.perf_counter() - t0
        qpos = res.trace["qpos"][:, 0]
        dt = float(model.opt.timestep)
        picked = []
        for t in range(qpos.shape[0]):
            if len(picked) < dt * (1 + env.frame_skip * (t + 1)) * fps:
                picked.append(t)
        rows = qpos[torch.as_tensor(picked, device=qpos.device)].contiguous()
        r = R.DeviceRenderer(model, env.batch, height=H, width=W)
        parts, frames = device_parts(torch, r, lambda: env.batch.kinematics_batch(qpos=rows), camera, a.repeats)
        qh = rows.double().cpu().numpy()
        sample = [int(i) for i in np.linspace(0, len(picked) - 1, a.host_frames).round()]
        hs, hf = host_frames(R, env.batch, camera, H, W, model,
                             [lambda i=i: env.batch.kinematics(0, qpos=qh[i]) for i in sample])
        out = {"workload": "episode", "height": H, "width": W, "camera": camera, "episode_steps": int(qpos.shape[0]),
               "episode_eval_s": episode_s, "device": summary(parts, len(picked), frames.nbytes),
               "host": {"frames_timed": len(sample), "seconds_timed": hs, "s_per_frame": hs / len(sample),
                        "extrapolated_s": hs / len(sample) * len(picked), "extrapolated": True},
               "max_level_diff_on_sample": diff(frames[sample], hf)}
        out["host_over_device"] = out["host"]["extrapolated_s"] / out["device"]["total_s"]["mean"]
        print(json.dumps(out), flush=True)
        results.append(out)
        env.close()

    for n in [int(x) for x in a.envs.split(",") if x]:
        H, W, camera = 96, 128, "side"
        env = HumanoidVecEnv({"model_path": HUMANOID_XML, "duration": 10.0, "frame_skip": 3,
                              "reward_config": {"type": "stand"}}, n_envs=n, model=model, seed=1)
        env.reset()
        g = torch.Generator().manual_seed(1)
        for _ in range(20):
            env.step_tensors((torch.rand(n, model.nu, generator=g) * 2 - 1).to(env.device))
        torch.cuda.synchronize()
        idx = list(range(n))
        r = R.DeviceRenderer(model, env.batch, height=H, width=W)
        parts, frames = device_parts(torch, r, lambda: env.batch.kinematics_batch(envs=idx), camera, a.repeats)
        # the public call itself (its list of arrays included)
        whole = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            imgs = env.get_images(height=H, width=W)
            whole.append(time.perf_counter() - t0)
        assert len(imgs) == n and np.array_equal(np.stack(imgs), frames)
        sample = idx if n <= 64 else [int(i) for i in np.linspace(0, n - 1, 64).round()]
        hs, hf = host_frames(R, env.batch, camera, H, W, model, [lambda i=i: env.batch.kinematics(i) for i in sample])
        out = {"workload": f"get_images_{n}", "height": H, "width": W, "camera": camera,
               "precision": env.batch.precision, "device": summary(parts, n, frames.nbytes),
               "get_images_s": {"mean": statistics.mean(whole), "min": min(whole), "max": max(whole)},
               "host": {"frames_timed": len(sample), "seconds_timed": hs, "s_per_frame": hs / len(sample),
                        "extrapolated_s": hs / len(sample) * n, "extrapolated": len(sample) != n},
               "max_level_diff_on_sample": diff(frames[sample], hf)}
        out["host_over_device"] = out["host"]["extrapolated_s"] / out["get_images_s"]["mean"]
        print(json.dumps(out), flush=True)
        results.append(out)
        env.close()
    print(json.dumps({"all": results}), flush=True)


if __name__ == "__main__":
    main()
