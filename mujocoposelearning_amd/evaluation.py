"""Closed-loop policy evaluation over whole episodes.

Replaces, for envs stepped by this engine:

* ``render_policy.py:6-51`` -- play a checkpoint with ``model.predict(obs, deterministic=True)`` ("make
  deterministic (critical)") and write the video: ``render_policy``;
* ``train_sb3.py:13-61`` ``VideoRecorderCallback`` -- a video of the current policy every ``render_interval``
  finished episodes: ``VideoRecorderCallback`` (``CallbackList`` runs it beside others, train_sb3.py:217);
* SB3's ``EvalCallback`` -- whole episodes of the current policy every so often during training:
  ``EvalCallback``;
* SB3's ``evaluate_policy`` (common/evaluation.py, 2.3.2): ``evaluate_policy``.

``evaluate_policy_device`` is the engine under all three: every env plays ``n_episodes_per_env`` whole
episodes.  On the fp64 engine with a device reward and a fusable pi net (``PPO._fused_rollout_args``) it
is ``hs_evaluate`` launches of up to ``hs_rollout_max_steps`` env steps each -- the fused rollout's loop
(env step, pi net on the env's wave, action to the pair's next step) without the RolloutBuffer, so device
memory does not grow with the number of steps (the optional trace aside).  Anything else -- the fp32
engine, host reward callables, other net shapes, a CPU env -- and the rest of an evaluation whose launch
hit a resident-tier contact overflow run the same loop one ``step_tensors`` at a time.

A model trained over ``VecNormalize`` (``model.vec_normalize``) is evaluated on normalised obs: its obs
moments, frozen, are applied to the evaluation env's raw obs -- inside the kernel on the fused path
(``hs_evaluate_norm``), by ``hs_obs_norm`` step by step -- and the episode returns stay the env's raw ones.
An evaluation env that is itself wrapped is stepped through its raw env; its own moments are not used.

Evaluating never changes a training run: the noise of a stochastic evaluation is the evaluation's own
(its own Philox seed and device counter on the fused path, its own ``torch.Generator`` step by step), and
neither ``PPO._noise_ctr`` nor the global torch RNG is touched.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import numpy as np
import torch

__all__ = ["EvalResult", "evaluate_policy_device", "evaluate_policy", "EvalCallback", "render_policy", "record_episode",
           "VideoRecorderCallback", "CallbackList"]


@dataclass
class EvalResult:
    """Per-episode results of ``evaluate_policy_device``: slot ``[e, i]`` is env ``i``'s episode number
    ``e`` of the evaluation.  A slot whose episode did not end inside the evaluation (``reset=False``
    with envs in mid-episode) keeps return NaN, length 0 and end step -1."""
    returns: torch.Tensor            # [E, N] float64: the env's own sum of rewards (info["total_reward"])
    lengths: torch.Tensor            # [E, N] int32: its step count
    end_step: torch.Tensor           # [E, N] int32: the evaluation step the episode ended in
    trace: dict | None = None        # n_trace > 0: qpos / qvel / actions / rewards / dones, [T, n_trace, ...]
    fused_launches: int = 0
    fallbacks: int = 0               # launches undone after a resident-tier overflow (the rest ran step by step)
    kernel_ms: list = field(default_factory=list)    # hs_last_tape_ms of each fused launch
    env_steps: int = 0               # T x N
    noise_seed: int = 0              # the Philox key of a stochastic fused evaluation (step g: counter g)


def _eval_seed(seed):
    # the evaluation's own Philox key, never PPO._noise_seed's (a multiple of the golden ratio constant)
    return (int(seed) * 0xD1342543DE82EF95 + 0x2545F4914F6CDD1D) % 2 ** 64


def _fused_args(model, env):
    """PPO._fused_rollout_args() with ``env`` in the trainer's place: (handle, hs_policy, keep) when
    hs_evaluate can run this policy on this env, else None."""
    fn = getattr(model, "_fused_rollout_args", None)
    if fn is None or torch.device(env.device).type != "cuda":
        return None
    model.policy.pack_heads()
    saved = model.env
    model.env = env
    try:
        return fn()
    finally:
        model.env = saved


def _batch_of(env):
    return getattr(env, "batch", None)


def _policy_obs(model, obs):
    """What the policy reads of the raw fp32 obs rows: a copy normalised with the model's frozen moments
    when it was trained over VecNormalize, else the rows."""
    vn = getattr(model, "vec_normalize", None)
    if vn is None or not vn.norm_obs:
        return obs
    obs = obs.contiguous()
    return vn.normalize_obs_tensor(obs, out=torch.empty_like(obs))


def _terminal_info(env):
    """(terminal_total_reward, terminal_step_count) tensors of the env, or None: the finished episodes'
    final info (custom_env.py:216-224), from the env itself or its HsBatch."""
    for src in (env, _batch_of(env)):
        if src is not None and hasattr(src, "terminal_total_reward") and hasattr(src, "terminal_step_count"):
            return src
    return None


class _Stepwise:
    """The evaluation loop one ``step_tensors`` at a time: ``net_forward`` (+ the evaluation's own noise),
    clamp, step, and at dones the env's ``terminal_total_reward`` / ``terminal_step_count`` (an env
    without them: this loop's own float64 sum and count)."""

    def __init__(self, model, env, res, T, E, n_trace, deterministic, seed):
        self.model, self.env, self.res, self.T, self.E, self.n_trace = model, env, res, T, E, n_trace
        self.deterministic = deterministic
        dev = torch.device(env.device)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(_eval_seed(seed) % (2 ** 63))
        N = env.num_envs
        self.cols = torch.arange(N, device=dev)
        self.acc = torch.zeros(N, dtype=torch.float64, device=dev)
        self.cnt = torch.zeros(N, dtype=torch.int32, device=dev)

    @torch.no_grad()
    def action(self, obs):
        pol = self.model.policy
        mean = pol.net_forward(_policy_obs(self.model, obs.float()), 0)
        if not self.deterministic:
            noise = torch.randn(mean.shape, generator=self.gen, device=mean.device, dtype=mean.dtype)
            mean = mean + pol.log_std.detach().exp() * noise
        return mean.clamp(-1.0, 1.0).contiguous()

    @torch.no_grad()
    def run(self, obs, t_from, ep, first_action=None):
        """Steps [t_from, T).  ``ep`` [N] int64: the episode number each env is in; ``first_action``: step
        t_from's clipped action when it is already decided (after an undone fused launch)."""
        env, res, E, nt = self.env, self.res, self.E, self.n_trace
        N = env.num_envs
        info, b = _terminal_info(env), _batch_of(env)
        a = first_action
        for t in range(t_from, self.T):
            if a is None:
                a = self.action(obs)
            obs, rew, term, trunc = env.step_tensors(a)
            done = (term != 0) | (trunc != 0)
            if info is not None:
                total, count = info.terminal_total_reward.double(), info.terminal_step_count.to(torch.int32)
            else:
                self.acc += rew.double()
                self.cnt += 1
                total, count = self.acc.clone(), self.cnt.clone()
                self.acc.masked_fill_(done, 0.0)
                self.cnt.masked_fill_(done, 0)
            # slot [ep, env] of the envs that finished, no host round trip: gather, select, scatter
            sel = done & (ep < E)
            flat = ep.clamp(max=E - 1) * N + self.cols
            for dst, val in ((res.returns, total), (res.lengths, count),
                             (res.end_step, torch.full_like(count, t))):
                d = dst.view(-1)
                d[flat] = torch.where(sel, val.to(d.dtype), d[flat])
            ep = ep + done.long()
            if nt:
                tr = res.trace
                q, v = b.qpos[:nt].clone(), b.qvel[:nt].clone()
                d = done[:nt]
                # a done step's row is the terminal state: the env has auto-reset, so it comes from the
                # terminal obs (qpos[2:], qvel); the root x, y, which no obs carries, from the step before
                tob = env.terminal_obs[:nt].to(q.dtype)
                nq, nv = q.shape[1], v.shape[1]
                prev = tr["qpos"][t - 1] if t > 0 else q
                term_q = torch.cat([prev[:, :2], tob[:, :nq - 2]], dim=1)
                tr["qpos"][t] = torch.where(d[:, None], term_q, q)
                tr["qvel"][t] = torch.where(d[:, None], tob[:, nq - 2:nq - 2 + nv], v)
                tr["actions"][t] = a[:nt]
                tr["rewards"][t] = rew[:nt]
                tr["dones"][t] = d
            a = None
        return obs


@torch.no_grad()
def evaluate_policy_device(model, env, n_episodes_per_env, deterministic=True, n_trace=0, reset=True, seed=0):
    """Every env of ``env`` plays ``n_episodes_per_env`` whole episodes (``E x env.episode_length()`` env
    steps) under ``model``'s policy -- the mean action when ``deterministic``, else its Gaussian sample --
    and the per-episode results come back on the device (``EvalResult``).

    ``model``: a ``PPO`` (its ``policy`` is used; nothing of its training state is touched).  ``env``: the
    ``PPO`` env protocol plus ``episode_length()``.  ``n_trace`` > 0 also records, for envs
    ``[0, n_trace)`` and every step, the state the step's reward was computed from (qpos, qvel: on a done
    step the terminal state), the clipped action, the reward and the done flag (needs an ``HsBatch`` env; on
    the step-by-step path a done step's state comes from the terminal obs, which does not carry the root
    x, y: those two are the previous step's).
    ``reset=False`` continues from the env's current state and obs.  ``seed``: the evaluation's own noise.
    """
    from .vec_normalize import unwrap
    env, _ = unwrap(env)             # raw obs and rewards; the moments applied are the model's
    vn = getattr(model, "vec_normalize", None)
    norm = vn.norm_args() if vn is not None and vn.norm_obs and torch.device(env.device).type == "cuda" else None
    E, N, nt = int(n_episodes_per_env), int(env.num_envs), int(n_trace)
    if E < 1:
        raise ValueError("n_episodes_per_env must be >= 1")
    if not 0 <= nt <= N:
        raise ValueError(f"n_trace={nt} must lie in [0, num_envs={N}]")
    dev = torch.device(env.device)
    b = _batch_of(env)
    if nt and b is None:
        raise ValueError("n_trace > 0 needs an env over an HsBatch (its qpos / qvel)")
    T = E * int(env.episode_length())
    if reset:
        obs = env.reset_tensors()
    elif b is not None:
        obs = b.obs
    else:
        obs = env.current_obs()
    res = EvalResult(returns=torch.full((E, N), float("nan"), dtype=torch.float64, device=dev),
                     lengths=torch.zeros(E, N, dtype=torch.int32, device=dev),
                     end_step=torch.full((E, N), -1, dtype=torch.int32, device=dev), env_steps=T * N,
                     noise_seed=_eval_seed(seed))
    if nt:
        f = b.dtype
        res.trace = dict(qpos=torch.zeros(T, nt, b.model.nq, dtype=f, device=dev),
                         qvel=torch.zeros(T, nt, b.model.nv, dtype=f, device=dev),
                         actions=torch.zeros(T, nt, env.act_dim, dtype=torch.float32, device=dev),
                         rewards=torch.zeros(T, nt, dtype=f, device=dev),
                         dones=torch.zeros(T, nt, dtype=torch.bool, device=dev))
    step = _Stepwise(model, env, res, T, E, nt, deterministic, seed)
    ep = torch.zeros(N, dtype=torch.int64, device=dev)
    fused = _fused_args(model, env)
    if fused is None:
        step.run(obs, 0, ep)
        return res

    import ctypes as C

    from . import _lib
    from .ppo_ops import ppo_act
    handle, cpol, keep = fused
    pol, A = model.policy, env.act_dim
    f32 = torch.float32
    key = _eval_seed(seed)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)            # the evaluation's own Philox counter
    act_clip = torch.zeros(N, A, dtype=f32, device=dev)
    scratch = [torch.zeros(N, A, dtype=f32, device=dev)] + [torch.zeros(N, dtype=f32, device=dev) for _ in range(4)]
    # step 0's action on the first obs: the per-step sampler, as PPO._rollout_fused
    mean = pol.net_forward(_policy_obs(model, obs.float()), 0)
    ppo_act(mean, scratch[1], pol.log_std.detach(), scratch[2], key, 0, deterministic, scratch[0], act_clip,
            scratch[3], scratch[4], scratch[2].clone(), counter_base=ctr)
    episode0 = b.episode.clone()
    tr = res.trace or {}
    eb = _lib.hs_eval_bufs()
    eb.actions_clipped, eb.episode0 = act_clip.data_ptr(), episode0.data_ptr()
    eb.max_episodes, eb.n_trace = E, nt
    eb.ep_return, eb.ep_length, eb.ep_end_step = res.returns.data_ptr(), res.lengths.data_ptr(), res.end_step.data_ptr()
    if nt:
        eb.trace_qpos, eb.trace_qvel = tr["qpos"].data_ptr(), tr["qvel"].data_ptr()
        eb.trace_actions, eb.trace_rewards = tr["actions"].data_ptr(), tr["rewards"].data_ptr()
        eb.trace_dones = tr["dones"].data_ptr()
    eb.counter_base, eb.seed, eb.deterministic = ctr.data_ptr(), key, int(bool(deterministic))
    L = _lib.check(_lib.lib().hs_rollout_max_steps(handle))
    stream = torch.cuda.current_stream(dev).cuda_stream
    t0 = 0
    while t0 < T:
        k = min(L, T - t0)
        if norm is not None:
            rc = _lib.check(_lib.lib().hs_evaluate_norm(handle, C.byref(cpol), pol._act_id(), C.byref(eb),
                                                        C.byref(norm), t0, k, T, stream))
        else:
            rc = _lib.check(_lib.lib().hs_evaluate(handle, C.byref(cpol), pol._act_id(), C.byref(eb), t0, k, T,
                                                   stream))
        if rc == 1:
            # resident-tier overflow: the library restored the env state and act_clip; whatever the undone
            # launch wrote into the result slots is dropped, and the rest runs step by step from t0
            res.fallbacks += 1
            stale = res.end_step >= t0
            res.returns.masked_fill_(stale, float("nan"))
            res.lengths.masked_fill_(stale, 0)
            res.end_step.masked_fill_(stale, -1)
            step.run(None, t0, (b.episode - episode0).long(), first_action=act_clip)
            break
        ms = C.c_double(0)
        _lib.check(_lib.lib().hs_last_tape_ms(handle, C.byref(ms)))
        res.kernel_ms.append(ms.value)
        res.fused_launches += 1
        t0 += k
    del keep
    return res


def evaluate_policy(model, env, n_eval_episodes=10, deterministic=True, return_episode_rewards=False, seed=0):
    """SB3 ``evaluate_policy`` (common/evaluation.py, 2.3.2) on a vectorised env: env ``i`` contributes its
    first ``(n_eval_episodes + i) // n_envs`` episodes, the episodes are ordered by (the step they ended
    in, env index) -- the order SB3's loop appends them in -- and the result is ``(np.mean, np.std)`` of
    the episode rewards, or with ``return_episode_rewards`` the two lists (rewards, lengths)."""
    n = int(env.num_envs)
    targets = np.array([(int(n_eval_episodes) + i) // n for i in range(n)], dtype=int)
    if targets.max() < 1:
        raise ValueError("n_eval_episodes must be >= 1")
    res = evaluate_policy_device(model, env, int(targets.max()), deterministic=deterministic, seed=seed)
    ret, length, end = (x.cpu().numpy() for x in (res.returns, res.lengths, res.end_step))
    e, i = np.nonzero(np.arange(ret.shape[0])[:, None] < targets[None, :])
    if (end[e, i] < 0).any():
        raise RuntimeError("evaluate_policy: an episode did not end within episode_length() steps")
    order = np.lexsort((i, end[e, i]))
    rewards = [float(x) for x in ret[e, i][order]]
    lengths = [int(x) for x in length[e, i][order]]
    if return_episode_rewards:
        return rewards, lengths
    return float(np.mean(rewards)), float(np.std(rewards))


class EvalCallback:
    """SB3 ``EvalCallback`` for ``PPO.learn(callback=...)`` (what train_sb3.py:52-60's
    VideoRecorderCallback does with whole episodes of the current policy): each time ``num_timesteps`` has
    advanced by ``eval_freq`` since the last evaluation, ``evaluate_policy`` on ``eval_env``; the mean
    reward and episode length go to ``model.logger`` (``eval/mean_reward``, ``eval/mean_ep_length``) and
    ``evaluations`` gets (timesteps, mean, std).  Rank 0 saves ``best_model`` under
    ``best_model_save_path`` when the mean improves.  Every rank evaluates on its own eval env, with no
    collective.  Always returns True (training goes on)."""

    def __init__(self, eval_env, eval_freq, n_eval_episodes, deterministic=True, best_model_save_path=None):
        self.eval_env, self.eval_freq, self.n_eval_episodes = eval_env, int(eval_freq), int(n_eval_episodes)
        self.deterministic, self.best_model_save_path = deterministic, best_model_save_path
        self.evaluations = []
        self.best_mean_reward = -np.inf
        self.last_mean_reward = -np.inf
        self._last_eval = 0

    def __call__(self, model):
        if model.num_timesteps - self._last_eval < self.eval_freq:
            return True
        self._last_eval = model.num_timesteps
        rewards, lengths = evaluate_policy(model, self.eval_env, self.n_eval_episodes, self.deterministic,
                                           return_episode_rewards=True, seed=len(self.evaluations))
        mean, std = float(np.mean(rewards)), float(np.std(rewards))
        self.last_mean_reward = mean
        model.logger["eval/mean_reward"] = mean
        model.logger["eval/mean_ep_length"] = float(np.mean(lengths))
        self.evaluations.append((model.num_timesteps, mean, std))
        if mean > self.best_mean_reward:
            self.best_mean_reward = mean
            if self.best_model_save_path is not None and getattr(model, "rank", 0) == 0:
                os.makedirs(self.best_model_save_path, exist_ok=True)
                model.save(os.path.join(self.best_model_save_path, "best_model"))
        return True


def record_episode(model, env, out_path, *, deterministic=True, camera="side", height=480, width=640, framerate=60,
                   num_steps=1000, renderer="device", seed=0):
    """One episode of env 0 of ``env`` under ``model``'s policy (at most ``num_steps`` steps of it) as a
    video at ``out_path``: one traced ``evaluate_policy_device`` run; a frame is taken after a step while
    ``len(frames) < time x framerate`` (custom_env.py:273-289), its pose from the traced qpos.
    ``renderer="device"``: the selected qpos rows go from the trace to ``render.DeviceRenderer.render_qpos``
    on the device -- one kinematics launch, one ray-cast launch, one copy of the uint8 frames
    [F, H, W, 3]; ``renderer="host"``: ``render.Renderer`` frame by frame.  Returns the written path (None:
    no frame)."""
    from . import render
    from .vec_normalize import unwrap
    if renderer not in ("device", "host"):
        raise ValueError(f"renderer must be 'device' or 'host', got {renderer!r}")
    env, _ = unwrap(env)
    res = evaluate_policy_device(model, env, 1, deterministic=deterministic, n_trace=1, seed=seed)
    qpos = res.trace["qpos"][:, 0]
    dones = res.trace["dones"][:, 0].cpu().numpy()
    dt = float(env.model.opt.timestep)
    picked = []
    for t in range(min(int(num_steps), len(dones))):
        time = dt * (1 + env.frame_skip * (t + 1))        # data.time after step t (the reset took one mj_step)
        if len(picked) < time * framerate:
            picked.append(t)
        if dones[t]:
            break
    if not picked:
        return None
    if renderer == "device":
        r = render.DeviceRenderer(env.model, env.batch, height=height, width=width)
        rows = qpos[torch.as_tensor(picked, device=qpos.device)]
        frames = r.render_qpos(rows, camera=camera).cpu().numpy()
    else:
        r = render.Renderer(env.model, height=height, width=width)
        q = qpos.double().cpu().numpy()
        frames = []
        for t in picked:
            r.update_scene_pose(env.batch.kinematics(0, qpos=q[t]), env.batch, camera=camera)
            frames.append(r.render())
        r.close()
    return str(render.write_video(str(out_path), frames, fps=framerate))


def render_policy(model_path, out_path, num_steps=1000, camera="side", height=480, width=640, framerate=60, device=0,
                  env_config=None, renderer="device"):
    """render_policy.py:6-51: load an SB3-layout checkpoint (ours or SB3's own zip), play one
    deterministic episode of one env (at most ``num_steps`` steps of it) and write the video
    (``record_episode``: the frames drawn on the GPU, or with ``renderer="host"`` by ``render.Renderer``).
    ``env_config`` overrides the env's keys (train.py's defaults: duration 10.0, frame_skip 3, reward
    'walk').  Returns the written path."""
    import json
    import zipfile

    from .ppo import PPO
    from .sb3_format import load_sb3_zip, read_member
    from .vec_env import HumanoidVecEnv
    from .vec_normalize import VecNormalize
    xml = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", "humanoid.xml")
    cfg = {"model_path": xml, "framerate": framerate, "duration": 10.0, "reward_config": {"type": "walk"},
           "frame_skip": 3}
    cfg.update(env_config or {})
    zp = str(model_path) if str(model_path).endswith(".zip") else str(model_path) + ".zip"
    with zipfile.ZipFile(zp) as z:
        data = json.loads(z.read("data")) if "data" in z.namelist() else {}
    pk = data.get("policy_kwargs") if isinstance(data.get("policy_kwargs"), dict) else {}
    env = HumanoidVecEnv(cfg, n_envs=1, device=device, precision="fp64")
    try:
        stats = read_member(zp, "vec_normalize.npz")     # a model trained over VecNormalize: frozen moments
        penv = VecNormalize(env, training=False) if stats is not None else env
        model = PPO(penv, n_steps=2, batch_size=2, n_epochs=1,
                    policy_kwargs={"net_arch": pk.get("net_arch", {"pi": [64, 64], "vf": [64, 64]}),
                                   "activation_fn": pk.get("activation_fn", "Tanh")})
        load_sb3_zip(zp, model.policy, map_location=model.device)
        if stats is not None:
            penv.from_bytes(stats)
            penv.training = False
        return record_episode(model, env, out_path, deterministic=True, camera=camera, height=height, width=width,
                              framerate=framerate, num_steps=num_steps, renderer=renderer)
    finally:
        env.close()


class VideoRecorderCallback:
    """train_sb3.py:13-61's ``VideoRecorderCallback`` for ``PPO.learn(callback=...)``: after an iteration, when
    the number of finished episodes (``len(model.ep_returns)``) has crossed one or more multiples of
    ``render_interval`` since the last call, record ONE episode of the current policy on the callback's own
    1-env evaluation env (``env_config_from_kwargs(env_kwargs)``, frames at ``env_kwargs["framerate"]``) and
    write ``<out_dir>/<run_name>/episode_<largest multiple crossed>.gif``.  Stochastic by default, as the
    reference's callback (it dropped ``deterministic=True``); a model trained over VecNormalize is played on
    its frozen obs moments (``evaluate_policy_device``).  Rank 0 only; always returns True; the written
    paths are kept in ``videos``."""

    def __init__(self, render_interval, env_kwargs, run_name=None, out_dir="recordings", deterministic=False,
                 height=480, width=640, camera="side", device=0):
        if int(render_interval) < 1:
            raise ValueError("render_interval must be >= 1")
        self.render_interval = int(render_interval)
        self.env_kwargs = dict(env_kwargs or {})
        self.run_name = str(run_name) if run_name is not None else "run"
        self.out_dir, self.deterministic = str(out_dir), bool(deterministic)
        self.height, self.width, self.camera, self.device = int(height), int(width), camera, device
        self.videos = []
        self._seen = 0          # finished episodes at the last call
        self._env = None

    def _eval_env(self):
        if self._env is None:
            from .train import env_config_from_kwargs
            from .vec_env import HumanoidVecEnv
            self._env = HumanoidVecEnv(env_config_from_kwargs(self.env_kwargs), n_envs=1, device=self.device,
                                       precision="fp64")
        return self._env

    def _record(self, model, path):
        return record_episode(model, self._eval_env(), path, deterministic=self.deterministic, camera=self.camera,
                              height=self.height, width=self.width,
                              framerate=self.env_kwargs.get("framerate", 60), num_steps=10 ** 9,
                              renderer="device", seed=len(self.videos))

    def __call__(self, model):
        done = len(model.ep_returns)
        k = self.render_interval
        crossed = done // k > self._seen // k
        self._seen = done
        if not crossed or getattr(model, "rank", 0) != 0:
            return True
        d = os.path.join(self.out_dir, self.run_name)
        os.makedirs(d, exist_ok=True)
        path = self._record(model, os.path.join(d, f"episode_{done // k * k}.gif"))
        if path is not None:
            self.videos.append(path)
        return True

    def close(self):
        if self._env is not None:
            self._env.close()
            self._env = None


class CallbackList:
    """SB3's ``CallbackList`` for ``PPO.learn(callback=...)`` (train_sb3.py:217): calls every callback with
    the model, each one every time, and returns False if any returned False (training then stops)."""

    def __init__(self, callbacks):
        self.callbacks = list(callbacks)

    def __call__(self, model):
        go = True
        for cb in self.callbacks:
            if cb(model) is False:
                go = False
        return go
