"""On-device PPO (PyTorch-ROCm) restating SB3 2.3.2's PPO/MlpPolicy semantics (the reference's
trainer, train_sb3.py:208-231) so rollouts never leave HBM.

* ActorCritic: separate pi / vf MLPs (net_arch dict, ReLU -- main.py:16,100 -- or Tanh), diagonal Gaussian
  with state-independent log_std (init 0), orthogonal init (gain sqrt(2) hidden, 0.01 action
  head, 1 value head) -- SB3 ActorCriticPolicy defaults.
* Rollout: n_steps x n_envs on device; actions clipped to the action space before stepping
  (SB3 collect_rollouts); time-limit truncation bootstraps r += gamma V(terminal_obs).
* GAE(gamma, lambda) reverse scan; per-minibatch advantage normalisation; clipped surrogate,
  value MSE (vf_coef 0.5), entropy bonus, clip_grad_norm(max_grad_norm 0.5), Adam(eps 1e-5).
* Multi-GPU: envs are sharded per rank; each optimizer step all-reduces the flattened gradient
  bucket ONCE (RCCL over xGMI, ~1.27 MB at [256,256]) -- no other collective on the data path
  (SURVEY.md 8e).  Ranks stay in lockstep for ANY shard sizes (train_sb3.py:203 accepts any
  n_envs): at construction the ranks agree once on every rank's env count, so all of them run the
  same number of rollout timesteps, minibatches per epoch and all-reduces; each rank's gradient is
  weighted by its share of the rollout samples before the sum.
"""
from __future__ import annotations

import math
import time

import numpy as np
import torch
import torch.nn as nn


from . import _lib
from . import batch as _batch_mod
from ._lib import HS_ACT_RELU, HS_ACT_TANH
from .ppo_ops import (FUSED_WIDTHS, Linear, _GaussLogpFn, _PPOLossFn, _SplitKLinearFn, _SplitKLinearReLUFn,  # noqa: F401
                      _SPLITK_ROWS, adam_clip_step, colsum, gae_device, activation_id, mlp2_forward,
                      mlp_forward, mlp_head_forward, ppo_act, ppo_kl_stop, ppo_loss, ppo_loss_ex, ppo_post,
                      ppo_stats_size)

FUSED_MLP = True      # rollout forward through the fused hs_mlp2_forward kernel where it applies
FUSED_ROLLOUT = True  # whole rollouts as hs_rollout launches (policy inside the env kernel) where they apply


def _fused_width(w1, mid):
    """The hidden width H of a packed pi / vf pair (pack_heads: w1 [D, 2H], mid) that the fused kernels
    run -- two hidden layers of the same width, 64, 128 or 256 -- else None."""
    H = w1.shape[1] // 2
    if len(mid) != 1 or w1.shape[1] != 2 * H or H not in FUSED_WIDTHS or tuple(mid[0][0].shape) != (2, H, H):
        return None
    return H


def _schedule_value(x, progress_remaining):
    """SB3's schedules: a constant, or a callable of progress_remaining (1 at the start of learn(),
    falling to 0 at total_timesteps); None stays None."""
    if x is None:
        return None
    return float(x(progress_remaining)) if callable(x) else float(x)


def _flat_packed(pk):
    w1, b1, mid, w3, b3 = pk
    return [w1, b1] + [t for wb in mid for t in wb] + [w3, b3]


def _mlp(inp, sizes, act=nn.ReLU):
    layers, d = [], inp
    for s in sizes:
        layers += [Linear(d, s), act()]
        d = s
    return nn.Sequential(*layers), d


class ActorCritic(nn.Module):
    def __init__(self, obs_dim, act_dim, pi=(64, 64), vf=None, activation=nn.ReLU, log_std_init=0.0):
        super().__init__()
        vf = pi if vf is None else vf
        self.pi_net, dp = _mlp(obs_dim, pi, activation)
        self.vf_net, dv = _mlp(obs_dim, vf, activation)
        self.action_net = Linear(dp, act_dim)
        self.value_net = Linear(dv, 1)
        self.log_std = nn.Parameter(torch.full((act_dim,), float(log_std_init)))
        self._packed = None      # pack_heads() cache, rebuilt at the start of every rollout
        self._packed_act = None  # the packed nets' activation (HS_ACT_RELU / HS_ACT_TANH), set with _packed
        for mod, gain in ((self.pi_net, math.sqrt(2)), (self.vf_net, math.sqrt(2)), (self.action_net, 0.01),
                          (self.value_net, 1.0)):
            for m in mod.modules() if isinstance(mod, nn.Sequential) else [mod]:
                if isinstance(m, nn.Linear):
                    nn.init.orthogonal_(m.weight, gain=gain)
                    nn.init.zeros_(m.bias)

    def forward(self, obs):
        return (mlp_head_forward(self.pi_net, self.action_net, obs),
                mlp_head_forward(self.vf_net, self.value_net, obs).squeeze(-1))

    def _logp(self, mean, actions):
        """DiagGaussian log_prob; on a device through hs_gauss_logp (+ its HIP backward)."""
        if mean.is_cuda and mean.shape[-1] <= 32:
            return _GaussLogpFn.apply(mean, actions, self.log_std)
        return self._logp_torch(mean, actions)

    def _logp_torch(self, mean, actions):
        std = self.log_std.exp()
        z = (actions - mean) / std
        return (-0.5 * z * z - self.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)

    def entropy(self):
        """DiagGaussian entropy (state-independent std, so the same for every sample)."""
        return (0.5 + 0.5 * math.log(2 * math.pi) + self.log_std).sum()

    @torch.no_grad()
    def act(self, obs, deterministic=False):
        mean, value = self(obs)
        a = mean if deterministic else mean + self.log_std.exp() * torch.randn_like(mean)
        return a, self._logp(mean, a), value

    def evaluate(self, obs, actions):
        mean, value = self(obs)
        ent = (0.5 + 0.5 * math.log(2 * math.pi) + self.log_std).sum().expand(obs.shape[0])
        return self._logp(mean, actions), ent, value

    @torch.no_grad()
    def value(self, obs):
        return self.value_net(self.vf_net(obs)).squeeze(-1)

    # -- rollout-time forward (no autograd) -------------------------------------------------------
    def _hidden(self, net):
        return [m for m in net if isinstance(m, nn.Linear)]

    @torch.no_grad()
    def pack_heads(self):
        """Stack the pi and vf MLPs into one chain of batched GEMMs for the rollout forward
        (weights are constant over a rollout, so this runs once per collect_rollouts): layer 1 is
        one [obs_dim x (h_pi + h_vf)] GEMM (both nets read the same obs), deeper layers one
        2-batch GEMM each, and the heads one 2-batch GEMM whose vf half carries the value column
        in column 0 of an A-wide block.  Needs equal pi/vf widths and one activation throughout,
        nn.ReLU or nn.Tanh (recorded in _packed_act); otherwise None and heads() runs the two nets."""
        lp, lv = self._hidden(self.pi_net), self._hidden(self.vf_net)
        act = activation_id([m for m in list(self.pi_net) + list(self.vf_net) if not isinstance(m, nn.Linear)])
        same = len(lp) == len(lv) >= 1 and all(a.weight.shape == b.weight.shape for a, b in zip(lp, lv))
        if not same or act is None:
            self._packed = self._packed_act = None
            return None
        self._packed_act = act
        A, H = self.action_net.out_features, lp[-1].out_features
        w1 = torch.cat([lp[0].weight, lv[0].weight]).t().contiguous()
        b1 = torch.cat([lp[0].bias, lv[0].bias])
        mid = [(torch.stack([a.weight.t(), b.weight.t()]).contiguous(), torch.stack([a.bias, b.bias])[:, None, :])
               for a, b in zip(lp[1:], lv[1:])]
        w3 = torch.zeros(2, H, A, device=w1.device, dtype=w1.dtype)
        w3[0] = self.action_net.weight.t()
        w3[1, :, 0] = self.value_net.weight[0]
        b3 = torch.zeros(2, 1, A, device=w1.device, dtype=w1.dtype)
        b3[0, 0] = self.action_net.bias
        b3[1, 0, 0] = self.value_net.bias[0]
        new = (w1, b1, mid, w3, b3)
        old = self._packed
        if old is not None and all(a.shape == b.shape for a, b in zip(_flat_packed(old), _flat_packed(new))):
            for a, b in zip(_flat_packed(old), _flat_packed(new)):    # in place: captured graphs stay valid
                a.copy_(b)
            return old
        self._packed = new
        return self._packed

    def _act_id(self):
        """The packed nets' activation (a module packed before the attribute existed: ReLU)."""
        act = getattr(self, "_packed_act", None)
        return HS_ACT_RELU if act is None else act

    def _act_addmm(self, b, x, w):
        """act(x w + b) of the packed chain: ReLU in the GEMM epilogue on a device, Tanh in place."""
        if self._act_id() == HS_ACT_TANH:
            return torch.addmm(b, x, w).tanh_()
        return torch._addmm_activation(b, x, w) if x.is_cuda else torch.addmm(b, x, w).relu_()

    @torch.no_grad()
    def heads(self, obs):
        """Rollout forward: (mean [N, A] view, value [N] strided view) from the packed GEMM chain
        (pack_heads) or, for unequal pi/vf nets, the two MLPs."""
        pk = getattr(self, "_packed", None)
        if pk is None:
            mean, value = self(obs)
            return mean, value
        if self._fused_mlp_ok(obs):                               # two fused launches beat the chain here
            return self.net_forward(obs, 0), self.net_forward(obs, 1)
        w1, b1, mid, w3, b3 = pk
        n = obs.shape[0]
        # [N, 2H]: layer 1 of both nets, ReLU in the GEMM epilogue on a device (Tanh: in place)
        tanh = self._act_id() == HS_ACT_TANH
        h = self._act_addmm(b1, obs, w1)
        h = h.view(n, 2, -1).transpose(0, 1)                      # [2, N, H] (strided)
        for w, b in mid:
            h = torch.baddbmm(b, h, w)
            h = h.tanh_() if tanh else h.relu_()
        out = torch.baddbmm(b3, h, w3)                            # [2, N, A]
        return out[0], out[1, :, 0]

    def _fused_mlp_ok(self, obs):
        """The fused hs_mlp2_forward_act kernel applies: packed equal pi / vf nets of two hidden layers of
        the same width, 64, 128 or 256 (ReLU or Tanh: _packed_act), <= 512 inputs and <= 32 actions, fp32 rows
        with unit stride on a device."""
        pk = getattr(self, "_packed", None)
        if pk is None or not FUSED_MLP or not obs.is_cuda:
            return False
        w1, _, mid, w3, _ = pk
        return (_fused_width(w1, mid) is not None and obs.shape[1] <= 512 and w3.shape[2] <= 32
                and obs.dtype == torch.float32 and obs.stride(1) == 1)

    @torch.no_grad()
    def net_forward(self, obs, which):
        """One of the two nets on its own from the packed weights (which = 0: pi -> mean [N, A],
        1: vf -> value [N]); hidden layers with the ReLU in the GEMM epilogue on a device (Tanh nets: an
        in-place tanh after each GEMM).  The
        device rollout samples with the pi net per step and evaluates the vf net once per rollout
        over the whole [T*N] buffer (the policy is fixed during a rollout)."""
        pk = getattr(self, "_packed", None)
        if pk is None:
            return self(obs)[which]
        w1, b1, mid, w3, b3 = pk
        H = w1.shape[1] // 2
        if self._fused_mlp_ok(obs):
            # one fused MFMA launch (ppo_mlp.hip mlp2_fwd_kernel) instead of three GEMMs, reading the
            # nn.Linear weights as they are ([out][in]: the reduction index contiguous)
            net, head = (self.pi_net, self.action_net) if which == 0 else (self.vf_net, self.value_net)
            l1, l2 = self._hidden(net)
            out = mlp2_forward(obs, l1.weight, l1.bias, l2.weight, l2.bias, head.weight, head.bias,
                               act=self._act_id())
            return out if which == 0 else out[:, 0]
        act = self._act_addmm
        h = act(b1[which * H:(which + 1) * H], obs, w1[:, which * H:(which + 1) * H])
        for w, b in mid:
            h = act(b[which, 0], h, w[which])
        out = torch.addmm(b3[which, 0], h, w3[which])
        return out if which == 0 else out[:, 0]


def gae(rewards, values, dones, last_values, last_dones, gamma, lam):
    """SB3 RolloutBuffer.compute_returns_and_advantage (stable_baselines3 2.3.2 common/buffers.py):
    reverse scan over time, vectorised over envs.  rewards/values/dones: [T, N] (dones[t] = the
    episode_start flag of step t, as SB3 stores it).  Returns (advantages, returns).

    On a GPU the scan is the HIP kernel ``hs_gae`` (gae.hip, one launch per rollout); on the CPU
    (tests, toy envs) it is this torch loop."""
    if rewards.is_cuda:
        return gae_device(rewards, values, dones, last_values, last_dones, gamma, lam)
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    last = torch.zeros_like(last_values)
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            nonterm = 1.0 - last_dones
            nv = last_values
        else:
            nonterm = 1.0 - dones[t + 1]
            nv = values[t + 1]
        delta = rewards[t] + gamma * nv * nonterm - values[t]
        last = delta + gamma * lam * nonterm * last
        adv[t] = last
    return adv, adv + values


def minibatch_weights(counts, rank, n_steps, n_minibatches):
    """Gradient weight of each of rank ``rank``'s minibatches in the world-plan of
    PPO._plan_minibatches: rank r splits its n_steps * counts[r] samples into n_minibatches
    chunks at (j * M_r) // n_minibatches, and minibatch j's weight is its chunk's share of the
    global minibatch j (the sum over ranks), so the all-reduced sum is the global mean."""
    nmb = n_minibatches
    def size(c, j):
        m = n_steps * c
        return ((j + 1) * m) // nmb - (j * m) // nmb
    return [size(counts[rank], j) / sum(size(c, j) for c in counts) for j in range(nmb)]


class PPO:
    """PPO over a device vec-env (HumanoidVecEnv's fast path).

    The env protocol: ``num_envs``, ``obs_dim``, ``act_dim``, ``device``, ``reset_tensors()``,
    ``step_tensors(actions) -> (obs, reward, terminated, truncated)`` on device, and
    ``terminal_obs`` (pre-reset obs of envs that just finished).  ``world_size``/``rank``
    default to the initialised torch.distributed group (one process per GPU, envs sharded).
    """

    def __init__(self, env, learning_rate=3e-4, n_steps=2048, batch_size=64, n_epochs=10, gamma=0.99,
                 gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 policy_kwargs=None, seed=0, world_size=None, rank=None, sync_grads=None, stagger_episodes=False,
                 normalize_advantage=True, target_kl=None, clip_range_vf=None):
        import torch.distributed as dist
        if world_size is None:
            world_size = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if rank is None:
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        # sync_grads: all-reduce the gradient bucket every optimizer step (default: world > 1; True
        # with a world-1 group runs the collective anyway -- the RCCL smoke test of tests/)
        self.sync_grads = world_size > 1 if sync_grads is None else bool(sync_grads)
        if self.sync_grads and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("PPO: gradient sync needs an initialised torch.distributed process group "
                               f"(world_size={world_size}); see train.init_distributed")
        pk = dict(policy_kwargs or {})
        net = pk.get("net_arch", {"pi": [64, 64], "vf": [64, 64]})
        if isinstance(net, (list, tuple)):
            net = {"pi": list(net), "vf": list(net)}
        act = pk.get("activation_fn", nn.Tanh)
        if isinstance(act, str):
            act = getattr(nn, act)
        self.env = env
        # PPO(VecNormalize(venv)): the wrapper's moments normalise what the policy sees;
        # self.obs, ep_returns and the logger's ep_rew_mean stay raw
        from .vec_normalize import VecNormalize
        self.vec_normalize = env if isinstance(env, VecNormalize) else None
        self.policy_kwargs, self.net_arch, self.learning_rate = pk, net, learning_rate
        self.device = torch.device(env.device)
        torch.manual_seed(seed)          # identical initial weights on every rank
        self.policy = ActorCritic(env.obs_dim, env.act_dim, net["pi"], net["vf"], act,
                                  pk.get("log_std_init", 0.0)).to(self.device)
        torch.manual_seed(seed + 7919 * rank)   # per-rank exploration noise / minibatch order
        # fused (single-kernel) Adam on a device; the same update rule and state_dict as foreach Adam
        cuda = self.device.type == "cuda"
        # SB3 2.3.2's train controls: target_kl (None: no early stop), clip_range_vf (None: no value
        # clipping); learning_rate, clip_range and clip_range_vf may be schedules f(progress_remaining),
        # evaluated at the start of every train() (_update_hyperparameters)
        self.target_kl, self.clip_range_vf = target_kl, clip_range_vf
        self.n_updates = 0
        self._total_timesteps = None     # set while learn() runs: progress_remaining = 1 - steps / total
        self._lr_now = _schedule_value(learning_rate, 1.0)
        self._clip_now = _schedule_value(clip_range, 1.0)
        self._clip_vf_now = _schedule_value(clip_range_vf, 1.0)
        self.opt = torch.optim.Adam(self.policy.parameters(), lr=self._lr_now, eps=1e-5,
                                    fused=True if cuda else None, capturable=cuda)
        # on a device the minibatch step replays as HIP graphs (see _build_graphs); the update is
        # launch-bound without them (~1.3 ms of kernels per 32768-sample step, ~1.7 ms eager)
        self.graphs = cuda
        self._graphs = self._epoch_graph = None
        self.n_steps, self.batch_size, self.n_epochs = n_steps, batch_size, n_epochs
        self.gamma, self.gae_lambda, self.clip_range = gamma, gae_lambda, clip_range
        self.ent_coef, self.vf_coef, self.max_grad_norm = ent_coef, vf_coef, max_grad_norm
        # SB3 PPO's normalize_advantage (default True): per-minibatch mean / std; with world > 1 each
        # rank normalises its own chunk of the global minibatch (tests/test_ppo.py equal-result test)
        self.normalize_advantage = bool(normalize_advantage)
        self.world_size, self.rank = world_size, rank
        N, T, D, A = env.num_envs, n_steps, env.obs_dim, env.act_dim
        self._plan_minibatches(N)
        f, dev = torch.float32, self.device
        self.buf = dict(obs=torch.zeros(T, N, D, dtype=f, device=dev), act=torch.zeros(T, N, A, dtype=f, device=dev),
                        rew=torch.zeros(T, N, dtype=f, device=dev), start=torch.zeros(T, N, dtype=f, device=dev),
                        val=torch.zeros(T, N, dtype=f, device=dev), logp=torch.zeros(T, N, dtype=f, device=dev),
                        done=torch.zeros(T, N, dtype=torch.bool, device=dev),
                        epret=torch.zeros(T, N, dtype=torch.float64, device=dev))
        if dev.type == "cuda":   # device rollout: deferred TimeLimit bootstrap (flags + terminal obs rows)
            self.buf.update(boot=torch.zeros(T, N, dtype=torch.bool, device=dev),
                            tobs=torch.zeros(T, N, D, dtype=f, device=dev))
        self.obs = env.reset_tensors().float().clone()
        # stagger_episodes: spread the envs' episode clocks after this first reset (not an SB3 option;
        # HumanoidVecEnv.stagger_episode_clocks) so that short rollouts see every episode phase
        if stagger_episodes:
            if not hasattr(env, "stagger_episode_clocks"):
                raise ValueError("stagger_episodes=True needs an env with stagger_episode_clocks() (HumanoidVecEnv)")
            env.stagger_episode_clocks()
        elif hasattr(env, "episode_length") and N > 1 and 2 * n_steps < env.episode_length():
            import warnings
            warnings.warn(f"PPO: rollouts of n_steps={n_steps} cover a small part of the {env.episode_length()}-step "
                          "episode and every env resets together, so each rollout sees one phase of it; "
                          "stagger_episodes=True spreads the envs' episode clocks (profiles/learning_curve_r5.md)",
                          RuntimeWarning, stacklevel=2)
        self.episode_start = torch.ones(N, dtype=f, device=dev)
        self.num_timesteps = 0
        self.ep_returns = []
        self.ep_acc = torch.zeros(N, dtype=torch.float64, device=dev)
        # a reward with named components (HumanoidVecEnv.terminal_total_reward_components, [C, N]): the finished
        # episodes' component sums are copied per step -- one device copy, graph-capturable -- and gathered under
        # the done mask with ep_returns.  No components: nothing is allocated, launched or logged.
        self._comp_names = ()
        self.ep_components = []
        if getattr(env, "terminal_total_reward_components", None) is not None:
            self._comp_names = tuple(env.reward_component_names)
            self.buf["epcomp"] = torch.zeros(T, len(self._comp_names), N, dtype=torch.float64, device=dev)
        self.flat = [p for p in self.policy.parameters()]
        # device rollout: the clipped actions the env steps with, and the Philox noise stream
        self._act_clip = torch.zeros(N, A, dtype=f, device=dev)
        self._zero_n = torch.zeros(N, dtype=f, device=dev)        # value input of hs_ppo_act (values are
        self._val_scratch = torch.zeros(N, dtype=f, device=dev)   # filled once per rollout, see below)
        self._noise_seed = (int(seed) + 7919 * rank) * 0x9E3779B97F4A7C15 % 2 ** 64
        self._noise_ctr = torch.zeros(1, dtype=torch.int64, device=dev)    # Philox step counter (device)
        self._rollout_graph = None
        self._rollout_graph_gen = 0             # the env batch's launch_generation the graph was recorded at
        if self.vec_normalize is not None:      # normalised copies: one step's obs, the rollout's last obs
            self._obs_step = torch.zeros(N, D, dtype=f, device=dev)
            self._obs_last_n = torch.zeros(N, D, dtype=f, device=dev)
        self.logger = {}
        # with world > 1 the stop decision is taken from the global minibatch's approx_kl, which rides
        # as one extra element of the gradient bucket (only when target_kl is set: the bucket is the
        # parameters alone otherwise, and the logged approx_kl is then this rank's)
        self._kl_sync = self.sync_grads and target_kl is not None
        if cuda:
            # device-resident train controls (include/hsim.h HS_PPO_*): the hyperparameter block every
            # update kernel reads (so captured graphs follow schedules), the stop word + epoch index,
            # and the stats block read back once per train()
            self._hp = torch.zeros(_lib.HS_PPO_HP_SIZE, dtype=f, device=dev)
            self._hp_host = torch.zeros(_lib.HS_PPO_HP_SIZE, dtype=f).pin_memory()   # staging: an async copy
            # control words and stats in one allocation, so one launch zeroes both before a train()
            self._blk = torch.zeros(2 + ppo_stats_size(n_epochs), dtype=f, device=dev)
            self._ctl = self._blk[:2].view(torch.int32)
            self._stats = self._blk[2:]
            self._kl_local = torch.zeros(1, dtype=f, device=dev)
            self._upload_hyperparameters()

    # -- SB3's per-iteration hyperparameters ------------------------------------------------------
    def _update_hyperparameters(self):
        """SB3's _update_current_progress_remaining + _update_learning_rate + the clip schedules of
        PPO.train: evaluate learning_rate / clip_range / clip_range_vf at progress_remaining
        (1 - num_timesteps / total_timesteps inside learn(), 1.0 for a bare train()) and hand them to
        the optimizer (CPU) and, in one small copy, to the device block (GPU)."""
        total = self._total_timesteps
        progress = 1.0 if not total else 1.0 - float(self.num_timesteps) / float(total)
        self._lr_now = _schedule_value(self.learning_rate, progress)
        self._clip_now = _schedule_value(self.clip_range, progress)
        self._clip_vf_now = _schedule_value(self.clip_range_vf, progress)
        for grp in self.opt.param_groups:
            grp["lr"] = self._lr_now
        if self.device.type == "cuda":
            self._upload_hyperparameters()

    def _upload_hyperparameters(self):
        cvf, tkl = self._clip_vf_now, self.target_kl
        # the pinned staging buffer is rewritten only here, and every train() ends in a device -> host
        # read of the stats block, so the previous copy has long completed
        self._hp_host.copy_(torch.tensor([self._lr_now, self._clip_now, -1.0 if cvf is None else cvf,
                                          -1.0 if tkl is None else 1.5 * tkl], dtype=torch.float32))
        self._hp.copy_(self._hp_host, non_blocking=True)

    def collect_rollouts(self):
        if self.device.type == "cuda":
            return self._collect_rollouts_device()
        return self._collect_rollouts_torch()

    def _collect_rollouts_device(self):
        """collect_rollouts on the GPU: per env step the packed policy GEMM chain, one hs_ppo_act
        launch (sample, log-prob, clip, buffer writes), the env kernel and one hs_ppo_post launch
        (dones, returns, obs -> slot t+1, and the TimeLimit.truncated envs' flags and terminal obs).
        No host synchronisation inside the loop.  The bootstrap r += gamma V(terminal obs) of the
        truncated envs is applied once after the loop, with one value forward over just those rows
        (the policy is fixed during the rollout, so this equals SB3's per-step evaluation)."""
        b, env, pol = self.buf, self.env, self.policy
        T, N = self.n_steps, env.num_envs
        pol.pack_heads()
        vn = self.vec_normalize
        if vn is not None:
            vn.begin_rollout()
        if self._fused_rollout_args() is not None:
            self._rollout_fused()
        else:
            # a recorded env launch holds the launch arguments of its time: a bank of initial states bound since
            # (HsBatch.set_initial_states) is not in it, so the graph is dropped and recorded again
            gen = getattr(getattr(env, "batch", None), "launch_generation", 0)
            if self._rollout_graph is not None and gen != self._rollout_graph_gen:
                self._rollout_graph = None
            if self.graphs and self._rollout_graph is None and getattr(env, "graph_safe", False):
                self._rollout_graph_gen = gen
                self._capture_rollout()                   # on failure: graphs off, eager body below
            if self._rollout_graph is not None:
                self._rollout_graph.replay()
            else:
                self._rollout_body()
        if vn is not None:
            self._normalize_rollout()                     # buffer obs, values, rewards (before the bootstrap)
        boot = b["boot"].view(-1).nonzero().squeeze(1)
        if boot.numel():                                        # deferred TimeLimit bootstrap
            tobs = b["tobs"].view(T * N, -1)[boot]
            if self._norm_obs():
                vn.normalize_obs_tensor(tobs)                   # with the rollout-start moments
            b["rew"].view(-1)[boot] += self.gamma * pol.value(tobs)
        return self._finish_rollout()

    def _norm_obs(self):
        vn = self.vec_normalize
        return vn is not None and vn.norm_obs

    def _policy_obs(self, obs, out):
        """What the policy reads of the raw rows ``obs``: the rows themselves, or with VecNormalize their
        normalised copy in ``out`` (hs_obs_norm with the rollout-start moments)."""
        return self.vec_normalize.normalize_obs_tensor(obs, out=out) if self._norm_obs() else obs

    def _normalize_rollout(self):
        """After a rollout over a VecNormalize env (the buffers hold RAW obs and rewards): normalise the
        buffered obs in place with the rollout-start moments -- the same pass yields the batch moments of the
        returned obs obs_1 .. obs_T (and, in the first rollout, of the reset obs) --, a normalised copy of the
        last obs for the last value, V(obs_t) over the buffer (device), and VecNormalize's reward path as a
        post-pass.  The running moments absorb the batch moments in _finish_rollout."""
        vn, b, T = self.vec_normalize, self.buf, self.n_steps
        if vn.norm_obs:
            train = vn.training
            first = train and vn.absorb_reset()
            vn.normalize_obs_tensor(b["obs"][0], moments_slot=0 if first else None)
            if T > 1:
                vn.normalize_obs_tensor(b["obs"][1:], moments_slot=1 if train else None)
            vn.normalize_obs_tensor(self.obs, out=self._obs_last_n, moments_slot=2 if train else None)
            if self.device.type == "cuda":
                self._rollout_values()
        vn.normalize_rewards_rollout(b["rew"], b["done"], self.world_size if self.sync_grads else 1,
                                     self._comm_device() if self.sync_grads and self.world_size > 1 else None)

    def _finish_rollout(self):
        """The end of collect_rollouts on either path: finished-episode returns, the timestep count,
        the value of the last obs and GAE."""
        b = self.buf
        if "epcomp" not in b:
            self.ep_returns += b["epret"][b["done"]].tolist()      # one device -> host transfer per rollout
        else:     # the same transfer carries the finished episodes' component sums: rows of (return, components)
            T, C, N = b["epcomp"].shape
            idx = b["done"].view(-1).nonzero().squeeze(1)
            rows = torch.cat([b["epret"].view(-1)[idx][:, None],
                              b["epcomp"].permute(0, 2, 1).reshape(T * N, C)[idx]], dim=1).tolist()
            self.ep_returns += [r[0] for r in rows]
            self.ep_components += [r[1:] for r in rows]
        self.num_timesteps += self.n_steps * self.n_envs_global
        last_v = self.policy.value(self._obs_last_n if self._norm_obs() else self.obs)
        vn = self.vec_normalize
        if vn is not None and vn.norm_obs and vn.training:     # between rollouts: the moments move
            vn.merge_obs_moments(self.world_size if self.sync_grads else 1,
                                 self._comm_device() if self.sync_grads and self.world_size > 1 else None)
        return gae(b["rew"], b["val"], b["start"], last_v, self.episode_start, self.gamma, self.gae_lambda)

    def _fused_rollout_args(self):
        """(batch handle, hs_policy) when the whole rollout can run as hs_rollout_act launches -- the env's
        fp64 engine with the device reward (HumanoidVecEnv.rollout_handle) and a pi net of two ReLU or
        two Tanh layers (policy._packed_act, passed beside the struct) of the same width, 64, 128 or 256
        (the reference's config.py net_arch is [64, 64] with ReLU, its README.md:44-50 results'
        [256, 256]; Tanh is the default of SB3's MlpPolicy and of PPO here) -- else None."""
        if not FUSED_ROLLOUT or self.device.type != "cuda":
            return None
        handle = self.env.rollout_handle() if hasattr(self.env, "rollout_handle") else None
        pk = self.policy._packed
        if handle is None or pk is None:
            return None
        w1, b1, mid, w3, b3 = pk
        D, A = w1.shape[0], w3.shape[2]
        H = _fused_width(w1, mid)
        if (H is None or D != self.env.obs_dim or D % 4 or D > 512 or A > 32
                or A != self.env.act_dim):
            return None
        from . import _lib
        ls = self.policy.log_std.detach()
        keep = (w1, b1, mid[0][0][0], mid[0][1][0, 0], w3[0], b3[0, 0], ls)
        if not all(t.is_contiguous() for t in keep):
            return None
        pol = _lib.hs_policy(*[t.data_ptr() for t in keep], w1.shape[1], D, A, H)
        return handle, pol, keep

    def _rollout_fused(self):
        """collect_rollouts as hs_rollout_act launches: this method samples step 0's action on the first obs
        (the per-step sampler, as _rollout_body), then each launch runs up to hs_rollout_max_steps env
        steps with the policy forward, sampling and buffer bookkeeping inside the env kernel
        (hs_env_step.h step_pair: rollout_rows, next_action; hs_policy.h), each env pair's step t + 1 starting when its own step t is done.
        The noise is hs_ppo_act's Philox stream, so the draws are those of the per-step path; the
        policy means agree with the GEMM chain to fp32 rounding (tests/test_gpu_ppo.py).  A launch
        that hits a resident-tier contact overflow is undone by the library, and the rest of the
        rollout runs step by step."""
        import ctypes as C

        from . import _lib
        b, env, pol = self.buf, self.env, self.policy
        T = self.n_steps
        handle, cpol, keep = self._fused_rollout_args()
        b["obs"][0].copy_(self.obs)
        mean = pol.net_forward(self._policy_obs(b["obs"][0], getattr(self, "_obs_step", None)), 0)
        ppo_act(mean, self._zero_n, pol.log_std.detach(), self.episode_start, self._noise_seed, 0, False,
                b["act"][0], self._act_clip, b["logp"][0], self._val_scratch, b["start"][0],
                counter_base=self._noise_ctr)
        norm = self.vec_normalize.norm_args() if self._norm_obs() else None
        rb = _lib.hs_rollout_bufs(b["obs"].data_ptr(), self.obs.data_ptr(), b["act"].data_ptr(), b["logp"].data_ptr(),
                                  b["start"].data_ptr(), b["rew"].data_ptr(), b["done"].data_ptr(),
                                  b["epret"].data_ptr(), b["boot"].data_ptr(), b["tobs"].data_ptr(),
                                  self.ep_acc.data_ptr(), self.episode_start.data_ptr(), self._act_clip.data_ptr(),
                                  self._noise_ctr.data_ptr(), self._noise_seed, 0)
        L = _lib.check(_lib.lib().hs_rollout_max_steps(handle))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        t0 = 0
        while t0 < T:
            k = min(L, T - t0)
            if norm is not None:       # the policy inside the kernel normalises its obs on load
                rc = _lib.check(_lib.lib().hs_rollout_norm(handle, C.byref(cpol), pol._act_id(), C.byref(rb),
                                                           C.byref(norm), t0, k, T, stream))
            else:
                rc = _lib.check(_lib.lib().hs_rollout_act(handle, C.byref(cpol), pol._act_id(), C.byref(rb), t0, k, T,
                                                          stream))
            if rc == 0:                       # (env steps, kernel ms by HIP events) of the last launches
                ms = C.c_double(0)
                _lib.check(_lib.lib().hs_last_tape_ms(handle, C.byref(ms)))
                self.rollout_launches = (getattr(self, "rollout_launches", []) + [(k * self.env.num_envs, ms.value)])[-64:]
            if rc == 1:                       # resident-tier overflow: state restored, step by step from t0
                self.fused_fallbacks = getattr(self, "fused_fallbacks", 0) + 1
                self._rollout_body(t_from=t0)
                return
            t0 += k
        del keep
        self._rollout_tail()

    def _rollout_body(self, t_from=0):
        """The T env steps of a device rollout (what the rollout graph captures); t_from > 0: the
        rest of a rollout whose steps [0, t_from) are in the buffers (the fused path's fallback)."""
        b, env, pol = self.buf, self.env, self.policy
        T, N = self.n_steps, env.num_envs
        gamma = float(self.gamma)
        if t_from == 0:
            b["obs"][0].copy_(self.obs)
        for t in range(t_from, T):
            x = self._policy_obs(b["obs"][t], getattr(self, "_obs_step", None))
            mean = pol.net_forward(x, 0) if pol._packed is not None else pol.heads(x)[0]
            ppo_act(mean, self._zero_n, pol.log_std.detach(), self.episode_start, self._noise_seed, t, False,
                    b["act"][t], self._act_clip, b["logp"][t], self._val_scratch, b["start"][t],
                    counter_base=self._noise_ctr)
            obs, rew, term, trunc = env.step_tensors(self._act_clip)
            nxt = b["obs"][t + 1] if t + 1 < T else self.obs
            ppo_post(rew.float(), term.to(torch.uint8), trunc.to(torch.uint8), None, gamma, obs.float(), nxt,
                     b["rew"][t], b["done"][t], self.ep_acc, b["epret"][t], self.episode_start,
                     terminal_obs=env.terminal_obs.float(), boot_obs_out=b["tobs"][t], boot_out=b["boot"][t])
            if "epcomp" in b:
                b["epcomp"][t].copy_(env.terminal_total_reward_components)
        self._rollout_tail()

    def _rollout_tail(self):
        self._noise_ctr.add_(self.n_steps)
        if not self._norm_obs():       # (VecNormalize: after the buffer's in-place pass, _normalize_rollout)
            self._rollout_values()

    def _rollout_values(self):
        b, pol = self.buf, self.policy
        T, N = self.n_steps, self.env.num_envs
        # values of every buffered obs in one batched vf forward (SB3 stores V(obs_t) per step;
        # the policy does not change inside a rollout, so this is the same quantity)
        b["val"].view(-1).copy_(pol.net_forward(b["obs"].view(T * N, -1), 1) if pol._packed is not None
                                else pol.value(b["obs"].view(T * N, -1)))

    def _capture_rollout(self):
        """Capture the whole T-step device rollout as one HIP graph (policy GEMMs, hs_ppo_act, the
        env kernel, hs_ppo_post per step): one host call per rollout.  Every pointer it uses is
        persistent (rollout buffers, the env batch's buffers, pack_heads' weight copies) and the
        noise counter lives in device memory, so replays are exactly the eager loop.  Only the
        side-effect-free policy forward is warmed up (GEMM library handles); the env steps are
        recorded, not executed, during capture."""
        pol, b, dev = self.policy, self.buf, self.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                pol.heads(b["obs"][0])
                pol.value(self.obs)
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._rollout_body()
            self._rollout_graph = g
        except RuntimeError as e:                  # nothing ran during capture: stay eager
            import warnings
            warnings.warn(f"rollout graph capture failed ({e}); collecting rollouts eagerly")
            self.graphs = False

    def _collect_rollouts_torch(self):
        """SB3 PPO.collect_rollouts on device.  No host synchronisation inside the loop: the
        timeout bootstrap r += gamma V(terminal_obs) is evaluated for every env and masked, and
        finished-episode returns are recorded in device buffers and read back once at the end."""
        b, env, pol = self.buf, self.env, self.policy
        if self.vec_normalize is not None:
            return self._collect_rollouts_torch_norm()
        for t in range(self.n_steps):
            a, logp, v = pol.act(self.obs)
            b["obs"][t] = self.obs
            b["act"][t] = a
            b["val"][t] = v
            b["logp"][t] = logp
            b["start"][t] = self.episode_start
            obs, rew, term, trunc = env.step_tensors(a.clamp(-1.0, 1.0))
            term, trunc = term.bool(), trunc.bool()
            boot = (trunc & ~term).float()          # TimeLimit.truncated: bootstrap from V(terminal obs)
            tv = pol.value(env.terminal_obs.float())
            b["rew"][t] = rew.float() + self.gamma * torch.where(boot > 0, tv, torch.zeros_like(tv))
            done = term | trunc
            self.ep_acc += rew.double()
            b["done"][t] = done
            b["epret"][t] = self.ep_acc
            self.ep_acc.masked_fill_(done, 0.0)
            if "epcomp" in b:
                b["epcomp"][t].copy_(env.terminal_total_reward_components)
            self.obs = obs.float().clone()
            self.episode_start = done.float()
        return self._finish_rollout()

    def _collect_rollouts_torch_norm(self):
        """_collect_rollouts_torch over a VecNormalize env, with the device path's semantics: the policy
        reads obs normalised with the rollout-start moments, the buffers hold raw obs and rewards until
        _normalize_rollout, and the TimeLimit bootstrap is added to the already normalised reward."""
        b, env, pol, vn = self.buf, self.env, self.policy, self.vec_normalize
        vn.begin_rollout()
        tv_all = torch.zeros_like(b["rew"])
        for t in range(self.n_steps):
            a, logp, v = pol.act(self._policy_obs(self.obs, self._obs_step))
            b["obs"][t] = self.obs
            b["act"][t] = a
            b["val"][t] = v
            b["logp"][t] = logp
            b["start"][t] = self.episode_start
            obs, rew, term, trunc = env.step_tensors(a.clamp(-1.0, 1.0))
            term, trunc = term.bool(), trunc.bool()
            boot = trunc & ~term
            tv = pol.value(self._policy_obs(env.terminal_obs.float().contiguous(), self._obs_last_n))
            tv_all[t] = torch.where(boot, tv, torch.zeros_like(tv))
            b["rew"][t] = rew.float()
            done = term | trunc
            self.ep_acc += rew.double()
            b["done"][t] = done
            b["epret"][t] = self.ep_acc
            self.ep_acc.masked_fill_(done, 0.0)
            if "epcomp" in b:
                b["epcomp"][t].copy_(env.terminal_total_reward_components)
            self.obs = obs.float().clone()
            self.episode_start = done.float()
        self._normalize_rollout()
        b["rew"] += self.gamma * tv_all
        return self._finish_rollout()

    # -- multi-rank lockstep ---------------------------------------------------------------------
    def _comm_device(self):
        import torch.distributed as dist
        return self.device if dist.get_backend() == "nccl" else torch.device("cpu")

    def _plan_minibatches(self, n_local):
        """Agree (one all-reduce at construction) on every rank's env count, then fix the per-epoch
        minibatch plan so that every rank issues the same number of gradient all-reduces:

        * world 1: SB3's plan -- ceil(M / batch_size) minibatches of batch_size, the last one short;
        * world > 1: n_mb = max over ranks of ceil(M_r / batch_size) minibatches per epoch on EVERY
          rank, each rank splitting its own permutation of M_r = n_steps * N_r samples into n_mb
          near-equal chunks (sizes differ by at most one; equal to batch_size for even shards whose
          M_r is a multiple of it, i.e. the usual case).  Gradients are weighted by the rank's share
          M_r / M_total before the sum, so uneven shards count per sample.
        """
        world, T, bs = self.world_size, self.n_steps, self.batch_size
        if self.sync_grads:      # independent trainers (sync_grads=False) plan locally, no collective
            import torch.distributed as dist
            counts = torch.zeros(world, dtype=torch.int64, device=self._comm_device())
            counts[self.rank] = n_local
            dist.all_reduce(counts)
            counts = [int(c) for c in counts.cpu()]
            if counts[self.rank] != n_local or min(counts) <= 0:
                raise RuntimeError(f"PPO: inconsistent env counts across ranks: {counts}")
        else:
            counts = [n_local]
        self.env_counts = counts
        self.n_envs_global = sum(counts)
        M = T * n_local
        if world == 1 or not self.sync_grads:
            self.n_minibatches = -(-M // bs)
            self._mb_bounds = [min(s, M) for s in range(0, M + bs, bs)][: self.n_minibatches + 1]
            self._mb_bounds[-1] = M
        else:
            self.n_minibatches = max(-(-(T * c) // bs) for c in counts)
            if T * min(counts) < self.n_minibatches:
                raise ValueError(f"batch_size={bs} is too small for env shards {counts} x n_steps={T}: "
                                 "a rank would get an empty minibatch")
            self._mb_bounds = [(j * M) // self.n_minibatches for j in range(self.n_minibatches + 1)]
        sizes = {b - a for a, b in zip(self._mb_bounds, self._mb_bounds[1:])}
        self._chunk = sizes.pop() if len(sizes) == 1 else None     # uniform minibatch size (graphable)
        # minibatch j's gradient is weighted by this rank's share of the global minibatch j,
        # s_r(j) / sum_r' s_r'(j) (every rank's chunk sizes follow from the agreed counts), so the
        # summed bucket is the mean over the global minibatch for even and uneven shards alike
        self._mb_weight = (minibatch_weights(counts, self.rank, T, self.n_minibatches)
                           if self.sync_grads and world > 1 else [1.0] * self.n_minibatches)
        self.grad_weight = self._mb_weight[0]

    def _agree_stop(self, stop):
        """Every rank leaves learn() at the same iteration (a callback may stop one rank only)."""
        if self.world_size == 1:
            return stop
        import torch.distributed as dist
        f = torch.tensor([1 if stop else 0], dtype=torch.int32, device=self._comm_device())
        dist.all_reduce(f, op=dist.ReduceOp.MAX)
        return bool(f.item())

    def _allreduce_flat(self, flat):
        import torch.distributed as dist
        if flat.is_cuda and dist.get_backend() == "gloo":     # multi-rank rehearsal without RCCL
            host = flat.cpu()
            dist.all_reduce(host)
            flat.copy_(host)
        else:
            dist.all_reduce(flat)        # ONE RCCL all-reduce per optimizer step (xGMI ring)

    def _allreduce_grads(self, kl=None):
        """All-reduce the weighted gradient bucket; with ``kl`` (this rank's approx_kl of the minibatch,
        when target_kl is set) it rides as one extra element, weighted like the gradients, and the
        global minibatch's approx_kl is returned (a one-element view of the reduced bucket)."""
        if not self.sync_grads:
            return kl
        grads = [p.grad for p in self.flat]
        flat = torch.cat([g.reshape(-1) for g in grads] + ([] if kl is None else [kl.detach().reshape(1).to(grads[0])]))
        flat.mul_(self.grad_weight)      # this rank's share of the samples (1/world for even shards)
        self._allreduce_flat(flat)
        o = 0
        for g in grads:
            n = g.numel()
            g.copy_(flat[o:o + n].view_as(g))
            o += n
        return None if kl is None else flat[o:o + 1]

    def _minibatch_loss(self, obs, act, old_logp, adv, ret, idx, old_val=None):
        """SB3 PPO.train's per-minibatch loss (clipped surrogate + vf_coef MSE - ent_coef entropy), the
        value loss on old_v + clamp(v - old_v, +-clip_range_vf) when clip_range_vf is set (old_val: the
        rollout values, the buffer's by default).  The minibatch's approx_kl and clip_fraction: on a
        device they go straight into the stats block (hs_ppo_loss_ex), on the CPU into _mb_extra."""
        mean, v = self.policy(obs[idx])
        logp = self.policy._logp(mean, act[idx])
        if old_val is None:
            old_val = self.buf["val"].reshape(-1)
        if logp.is_cuda:                            # fused HIP loss (same formulas as below)
            pg, vf = ppo_loss_ex(logp, v, idx, adv, ret, old_logp, old_val, self._hp, self.policy.log_std.detach(),
                                 self.vf_coef, self.ent_coef, self._stats, self.n_epochs, self._ctl,
                                 self._kl_local if self._kl_sync else None, self.normalize_advantage)
            loss = torch.add(pg, vf, alpha=self.vf_coef)
            if self.ent_coef:                       # SB3's default ent_coef 0: no term, no launches
                loss = loss - self.ent_coef * self.policy.entropy()
            return loss, pg, vf
        ent_mean = self.policy.entropy()            # = evaluate()'s per-sample entropy, averaged
        a = adv[idx]
        if self.normalize_advantage and a.numel() > 1:
            a = (a - a.mean()) / (a.std() + 1e-8)
        clip, clip_vf = self._clip_now, self._clip_vf_now
        log_ratio = logp - old_logp[idx]
        ratio = torch.exp(log_ratio)
        pg = -torch.min(a * ratio, a * ratio.clamp(1 - clip, 1 + clip)).mean()
        if clip_vf is not None:
            ov = old_val[idx]
            v = ov + torch.clamp(v - ov, -clip_vf, clip_vf)
        vf = torch.nn.functional.mse_loss(ret[idx], v)
        with torch.no_grad():                       # SB3: approx_kl_div and clip_fraction of the minibatch
            self._mb_extra = (((ratio - 1) - log_ratio).mean(), ((ratio - 1).abs() > clip).float().mean(), ent_mean)
        return pg + self.ent_coef * (-ent_mean) + self.vf_coef * vf, pg, vf

    @staticmethod
    def _explained_variance(val, ret):
        """SB3 utils.explained_variance: 1 - Var(ret - val) / Var(ret) (population variances), nan when
        Var(ret) == 0; a 0-dim tensor on the inputs' device."""
        y, yp = ret.reshape(-1), val.reshape(-1)
        var_y = y.var(unbiased=False)
        return torch.where(var_y == 0, torch.full_like(var_y, float("nan")), 1 - (y - yp).var(unbiased=False) / var_y)

    def _train_stats(self, st, epochs_entered):
        """The logger entries of one train() from a stats block (a list laid out as HS_PPO_STAT_*)."""
        L = _lib
        n = max(st[L.HS_PPO_STAT_COUNT], 1.0)
        e = max(epochs_entered - 1, 0)      # SB3 resets approx_kl_divs every epoch: the last one entered
        kl_sum, kl_n = st[L.HS_PPO_STAT_KL + 2 * e], st[L.HS_PPO_STAT_KL + 2 * e + 1]
        out = dict(policy_loss=st[L.HS_PPO_STAT_POLICY_LOSS] / n, value_loss=st[L.HS_PPO_STAT_VALUE_LOSS] / n,
                   approx_kl=kl_sum / kl_n if kl_n else float("nan"),
                   clip_fraction=st[L.HS_PPO_STAT_CLIP_FRACTION] / n, entropy_loss=-st[L.HS_PPO_STAT_ENTROPY] / n,
                   explained_variance=st[L.HS_PPO_STAT_EXPLAINED_VARIANCE], loss=st[L.HS_PPO_STAT_LOSS_LAST],
                   std=st[L.HS_PPO_STAT_STD], n_updates=self.n_updates, learning_rate=self._lr_now,
                   clip_range=self._clip_now)
        if self._clip_vf_now is not None:
            out["clip_range_vf"] = self._clip_vf_now
        self.last_kl = st[L.HS_PPO_STAT_KL_LAST]       # the approx_kl the last stop decision was taken from
        self.logger.update(out)
        return out

    def train(self, adv, ret):
        """SB3 PPO.train: n_epochs passes over the rollout in minibatches; with target_kl, the first
        minibatch whose approx_kl exceeds 1.5 target_kl takes no optimizer step and ends the update
        (its statistics are recorded, n_updates counts its epoch).  The epoch loop is this one; a path
        (CPU, device eager, device graphed) supplies one epoch's minibatches, the stop test after it
        and the finish that turns its statistics into the logger entries."""
        M = self.n_steps * self.env.num_envs
        cuda = self.device.type == "cuda"
        self._update_hyperparameters()
        if not cuda:
            run_epoch, stopped, finish = self._train_path_cpu(adv, ret)
        else:
            # one stats block per train(): zeroed here (with the control words), filled by the loss
            # kernels, read once at the end
            self._blk.zero_()
            graphed = self.graphs and self._chunk is not None
            run_epoch = self._train_path_graphed(adv, ret) if graphed else self._train_path_eager(adv, ret)
            stopped, finish = self._stopped, lambda entered: self._finish_device_train(entered, ret)
        entered = 0
        for epoch in range(self.n_epochs):
            perm = torch.randperm(M, device=self.device)
            entered += 1
            self.n_updates += 1
            run_epoch(epoch, perm)
            if stopped():
                break
            if cuda:
                self._ctl[_lib.HS_PPO_CTL_EPOCH].add_(1)
        return finish(entered)

    def _rollout_views(self, adv, ret):
        """(obs, act, old_logp, adv, ret, old_val) of the rollout, flattened over [T, N]."""
        b, M = self.buf, self.n_steps * self.env.num_envs
        return (b["obs"].reshape(M, -1), b["act"].reshape(M, -1), b["logp"].reshape(-1), adv.reshape(-1),
                ret.reshape(-1), b["val"].reshape(-1))

    def _train_path_cpu(self, adv, ret):
        """train() on the CPU (toy envs, tests): the torch restatement, its statistics in a host list
        laid out as the stats block, the stop decision taken on the host before the optimizer step."""
        obs, act, old_logp, adv, ret, old_val = self._rollout_views(adv, ret)
        st = [0.0] * (_lib.HS_PPO_STAT_KL + 2 * self.n_epochs)
        st[_lib.HS_PPO_STAT_EXPLAINED_VARIANCE] = float(self._explained_variance(old_val, ret))
        stop = False

        def run_epoch(epoch, perm):
            nonlocal stop
            for j, (s, e) in enumerate(zip(self._mb_bounds, self._mb_bounds[1:])):
                self.grad_weight = self._mb_weight[j]
                loss, pg, vf = self._minibatch_loss(obs, act, old_logp, adv, ret, perm[s:e], old_val)
                kl, cf, ent = self._mb_extra
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                # world > 1: the decision value is the global minibatch's approx_kl (same on every rank)
                red = self._allreduce_grads(kl if self._kl_sync else None)
                kl = float(kl if red is None else red)
                for k, x in ((_lib.HS_PPO_STAT_POLICY_LOSS, pg), (_lib.HS_PPO_STAT_VALUE_LOSS, vf),
                             (_lib.HS_PPO_STAT_CLIP_FRACTION, cf), (_lib.HS_PPO_STAT_ENTROPY, ent),
                             (_lib.HS_PPO_STAT_LOSS, loss)):
                    st[k] += float(x.detach())
                st[_lib.HS_PPO_STAT_LOSS_LAST] = float(loss.detach())
                st[_lib.HS_PPO_STAT_COUNT] += 1.0
                st[_lib.HS_PPO_STAT_KL + 2 * epoch] += kl
                st[_lib.HS_PPO_STAT_KL + 2 * epoch + 1] += 1.0
                st[_lib.HS_PPO_STAT_KL_LAST] = kl
                if self.target_kl is not None and kl > 1.5 * self.target_kl:
                    stop = True                      # SB3: break before the optimizer step
                    return
                self._clip_and_step()

        def finish(entered):
            st[_lib.HS_PPO_STAT_STD] = float(self.policy.log_std.detach().exp().mean())
            return self._train_stats(st, entered)
        return run_epoch, lambda: stop, finish

    def _stopped(self):
        """The device stop word, read by the host once after an epoch (only with target_kl set)."""
        return self.target_kl is not None and bool(self._ctl[_lib.HS_PPO_CTL_STOP].item())

    def _finish_device_train(self, entered, ret):
        """The per-iteration statistics (queued behind the update's kernels, so the host's launches
        hide under them; the rollout values and returns are untouched by the update) and the read."""
        self._stats[_lib.HS_PPO_STAT_EXPLAINED_VARIANCE].copy_(self._explained_variance(self.buf["val"], ret))
        self._stats[_lib.HS_PPO_STAT_STD].copy_(self.policy.log_std.detach().exp().mean())
        return self._train_stats(self._stats.tolist(), entered)      # the one device -> host read

    def _train_path_eager(self, adv, ret):
        """train() on a device without graphs (capture refused, or ragged minibatches): the same
        kernels and device predicates as the graphed update -- after the stop word is set the rest of
        that epoch's minibatches run and are discarded -- with the stop word read once per epoch."""
        obs, act, old_logp, adv, ret, old_val = self._rollout_views(adv, ret)

        def run_epoch(epoch, perm):
            for j, (s, e) in enumerate(zip(self._mb_bounds, self._mb_bounds[1:])):
                self.grad_weight = self._mb_weight[j]
                loss, pg, vf = self._minibatch_loss(obs, act, old_logp, adv, ret, perm[s:e], old_val)
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                kl = self._allreduce_grads(self._kl_local if self._kl_sync else None)
                if self._kl_sync:
                    ppo_kl_stop(kl, self._hp, self._stats, self.n_epochs, self._ctl)
                self._clip_and_step()
        return run_epoch

    def _clip_and_step(self):
        """clip_grad_norm_(max_grad_norm) + Adam step: hs_adam_clip_ex on a device (lr from the device
        block, skipped when the stop word is set), torch on the CPU."""
        params = self.flat
        if params[0].is_cuda:
            self._adam_ws = adam_clip_step(self.opt, params, self.max_grad_norm, getattr(self, "_adam_ws", None),
                                           hp=self._hp, skip=self._ctl)
        else:
            torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm)
            self.opt.step()

    # -- HIP-graph update ----------------------------------------------------------------------
    def _build_graphs(self):
        """Capture one minibatch step as two HIP graphs over static buffers: G1 = gather by the
        static index buffer + forward + loss + backward (gradients land in graph-owned .grad
        tensors and, for world > 1, are packed into one flat bucket), G2 = unpack/average the
        bucket + clip_grad_norm + capturable fused Adam.  The per-step RCCL all-reduce of the
        bucket (world > 1) is the one eager call between the two replays.  The warm-up steps
        capture needs are undone (parameters and Adam state restored in place), so graphed
        training takes exactly the eager path's optimizer steps.
        Every per-iteration hyperparameter is read from the device block (_hp) and the target_kl stop
        is a device predicate (the stop word of _ctl: set by the loss's final kernel -- with world > 1
        by hs_ppo_kl_stop in G2, from the bucket's all-reduced extra element, before the Adam kernels
        -- and read by hs_adam_clip_ex), so the graphs are captured once and follow the schedules."""
        b, M, bs = self.buf, self.n_steps * self.env.num_envs, self._chunk
        dev = self.device
        self._g_idx = torch.zeros(bs, dtype=torch.long, device=dev)
        self._g_adv = torch.zeros(M, dtype=torch.float32, device=dev)
        self._g_ret = torch.zeros(M, dtype=torch.float32, device=dev)
        src = (b["obs"].view(M, -1), b["act"].view(M, -1), b["logp"].view(-1), self._g_adv, self._g_ret)
        old_val = b["val"].view(-1)
        params = list(self.policy.parameters())

        sync, kl_sync = self.sync_grads, self._kl_sync
        n_par = sum(p.numel() for p in params)
        self._g_flat = torch.zeros(n_par + (1 if kl_sync else 0), dtype=torch.float32, device=dev) if sync else None
        self._g_w = torch.full((1,), float(self._mb_weight[0]), dtype=torch.float32, device=dev)

        def g1_body():
            loss, pg, vf = self._minibatch_loss(*src, self._g_idx, old_val)
            loss.backward()
            if sync:                     # the weighted gradient bucket the eager all-reduce sends
                torch.cat([p.grad.reshape(-1) for p in params] + ([self._kl_local] if kl_sync else []),
                          out=self._g_flat)
                self._g_flat.mul_(self._g_w)     # minibatch weight, refreshed before each replay

        def g2_body():
            if sync:                     # summed bucket back into the .grad tensors
                o = 0
                for p in params:
                    n = p.numel()
                    p.grad.copy_(self._g_flat[o:o + n].view_as(p.grad))
                    o += n
                if kl_sync:              # the global minibatch's approx_kl: stop decision before Adam
                    ppo_kl_stop(self._g_flat[n_par:], self._hp, self._stats, self.n_epochs, self._ctl)
            self._clip_and_step()

        saved_p = [p.detach().clone() for p in params]
        saved_s = {id(p): {k: v.clone() for k, v in self.opt.state[p].items()} for p in params if p in self.opt.state}
        self._g_idx.copy_(torch.arange(bs, device=dev))
        self._ctl.zero_()                # the warm-up steps below must not meet a set stop word
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                self.opt.zero_grad(set_to_none=True)
                g1_body()
                g2_body()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.opt.zero_grad(set_to_none=True)
        pool = torch.cuda.graph_pool_handle()
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        try:
            # thread_local: RCCL's proxy threads (world > 1) may touch the runtime meanwhile
            with torch.cuda.graph(g1, pool=pool, capture_error_mode="thread_local"):
                g1_body()
            with torch.cuda.graph(g2, pool=pool, capture_error_mode="thread_local"):
                g2_body()
            self._graphs = (g1, g2)
            self._epoch_graph = None
            if not sync:
                # world 1: the whole epoch -- every minibatch's gather, forward, loss, backward, clip and
                # Adam, indices read from slices of one static permutation buffer -- as ONE graph, so
                # small minibatches (README.md:23-53: batch 128, 128 steps per epoch) cost one replay
                # per epoch instead of two per minibatch.  Each step starts from .grad = None, so its
                # backward writes fresh gradients exactly as G1 does.  After a minibatch trips the
                # target_kl stop the rest of the epoch still runs forward and backward inside the graph
                # and is discarded by the stop word (no statistics, no optimizer step).
                self._g_perm = torch.zeros(M, dtype=torch.long, device=dev)
                ge = torch.cuda.CUDAGraph()
                with torch.cuda.graph(ge, pool=pool, capture_error_mode="thread_local"):
                    for s0, e0 in zip(self._mb_bounds, self._mb_bounds[1:]):
                        self.opt.zero_grad(set_to_none=True)
                        loss, pg, vf = self._minibatch_loss(*src, self._g_perm[s0:e0], old_val)
                        loss.backward()
                        self._clip_and_step()
                self._epoch_graph = ge
        except RuntimeError as e:                  # capture refused: train eagerly from here on
            import warnings
            warnings.warn(f"PPO update graph capture failed ({e}); falling back to the eager update")
            self.graphs = False
            self._graphs = None
            self.opt.zero_grad(set_to_none=True)
        finally:
            with torch.no_grad():                  # undo the warm-up steps in place
                for p, q in zip(params, saved_p):
                    p.copy_(q)
                for p in params:
                    st, old = self.opt.state.get(p, {}), saved_s.get(id(p))
                    for k, v in st.items():
                        if old is not None and k in old:
                            v.copy_(old[k])
                        elif torch.is_tensor(v):
                            v.zero_()
                self._blk.zero_()    # the warm-up's statistics and stop word: back to the start of train()

    def _train_path_graphed(self, adv, ret):
        """train() on a device as graph replays (captured on first use): one replay per epoch with
        world 1, else G1 / all-reduce / G2 per minibatch."""
        if self._graphs is None:
            self._build_graphs()
            if self._graphs is None:
                return self._train_path_eager(adv, ret)         # capture failed: self.graphs is now False
        g1, g2 = self._graphs
        self._g_adv.copy_(adv.reshape(-1))
        self._g_ret.copy_(ret.reshape(-1))
        ge = getattr(self, "_epoch_graph", None)

        def run_epoch(epoch, perm):
            if ge is not None:                    # world 1: one replay per epoch
                self._g_perm.copy_(perm)
                ge.replay()
                return
            for j, (s, e) in enumerate(zip(self._mb_bounds, self._mb_bounds[1:])):
                self._g_idx.copy_(perm[s:e])
                if self.sync_grads:
                    self._g_w.fill_(self._mb_weight[j])
                g1.replay()
                if self.sync_grads:
                    self._allreduce_flat(self._g_flat)
                g2.replay()
        return run_epoch

    WARN_KINDS = _batch_mod.WARN_KINDS

    def _check_env_warnings(self):
        """Once per rollout: the env's warning counters (include/hsim.h HS_WARN_*) since the last
        check, summed over ranks.  Bad-state resets are reported the way MuJoCo's mj_step reports
        them (mju_warning: the state was reset with mj_resetData and the run goes on; custom_env.py:160);
        a lost chunk-queue hand-off is a scheduling failure, not physics, so it raises on every
        rank (batch.report_warnings).  Returns the new counts (also in ``logger["env_warnings"]``)."""
        fn = getattr(self.env, "warning_counts", None)
        if fn is None:
            return None
        tot = np.asarray(fn(), dtype=np.int64)
        prev = getattr(self, "_warn_seen", None)
        new = np.maximum(tot - prev, 0) if prev is not None and prev.shape == tot.shape else tot
        self._warn_seen = tot
        if self.world_size > 1:
            import torch.distributed as dist
            t = torch.as_tensor(new, dtype=torch.int64, device=self._comm_device())
            dist.all_reduce(t)
            new = t.cpu().numpy()
        self._warn_new = new
        _batch_mod.report_warnings(new, "rollout")
        return new

    def learn(self, total_timesteps, callback=None, log_interval=1):
        it = 0
        self._total_timesteps = total_timesteps      # schedules: progress_remaining = 1 - steps / total
        try:
            return self._learn(total_timesteps, callback, it)
        finally:
            self._total_timesteps = None

    def _learn(self, total_timesteps, callback, it):
        while self.num_timesteps < total_timesteps:
            t0 = time.perf_counter()
            adv, ret = self.collect_rollouts()
            warn = self._check_env_warnings()
            t1 = time.perf_counter()
            st = self.train(adv, ret)
            t2 = time.perf_counter()
            it += 1
            mean_ret = float(np.mean(self.ep_returns[-100:])) if self.ep_returns else float("nan")
            self.logger = dict(self.logger, iteration=it, timesteps=self.num_timesteps, rollout_s=t1 - t0,
                               train_s=t2 - t1, ep_rew_mean=mean_ret, **st)
            if warn is not None:
                self.logger["env_warnings"] = [int(x) for x in warn]
            if self._comp_names and self.ep_components:   # the reward's named components, as ep_rew_mean is
                means = np.mean(np.asarray(self.ep_components[-100:], dtype=np.float64), axis=0)
                self.logger["ep_components_mean"] = {k: float(v) for k, v in zip(self._comp_names, means)}
            if self._agree_stop(callback is not None and callback(self) is False):
                break
        return self

    @torch.no_grad()
    def predict(self, observation, state=None, episode_start=None, deterministic=False):
        """SB3 BaseAlgorithm.predict (render_policy.py:30): obs (obs_dim,) or (n, obs_dim) ->
        (actions clipped to [-1, 1] as numpy, None)."""
        obs = torch.as_tensor(np.asarray(observation), dtype=torch.float32, device=self.device)
        single = obs.dim() == 1
        obs = (obs[None] if single else obs).contiguous()
        if self._norm_obs():         # frozen moments: predict never updates them
            obs = self.vec_normalize.normalize_obs_tensor(obs, out=torch.empty_like(obs))
        a, _, _ = self.policy.act(obs, deterministic=deterministic)
        a = a.clamp(-1.0, 1.0).cpu().numpy()
        return (a[0] if single else a), None

    def _data(self):
        act = self.policy_kwargs.get("activation_fn", nn.Tanh)
        return {"n_steps": self.n_steps, "batch_size": self.batch_size, "n_epochs": self.n_epochs,
                "gamma": self.gamma, "gae_lambda": self.gae_lambda,
                "clip_range": _schedule_value(self.clip_range, 1.0),     # a schedule: its value at the start
                "clip_range_vf": _schedule_value(self.clip_range_vf, 1.0), "target_kl": self.target_kl,
                "ent_coef": self.ent_coef, "vf_coef": self.vf_coef, "max_grad_norm": self.max_grad_norm,
                "learning_rate": _schedule_value(self.learning_rate, 1.0), "num_timesteps": self.num_timesteps,
                "n_updates": self.n_updates,
                "n_envs": self.n_envs_global,
                "policy_kwargs": {"net_arch": self.net_arch,
                                  "activation_fn": act if isinstance(act, str) else act.__name__}}

    def save(self, path):
        """SB3 checkpoint layout (train_sb3.py:234 ``model.save``): writes ``path``.zip."""
        from .sb3_format import save_sb3_zip
        vn = self.vec_normalize
        extra = {"vec_normalize.npz": vn.to_bytes()} if vn is not None else None
        return save_sb3_zip(path, self.policy, self.opt, self._data(), extra=extra)

    def load(self, path):
        """Load weights + optimizer state from an SB3-layout zip (ours or SB3's own)."""
        from .sb3_format import load_sb3_zip, read_member
        raw = read_member(path, "vec_normalize.npz")
        if raw is not None and self.vec_normalize is None:
            raise ValueError(f"{path}: the model was saved with VecNormalize (vec_normalize.npz), but this PPO's env "
                             "is not wrapped: build it as PPO(VecNormalize(env), ...) so the policy sees the obs "
                             "it was trained on")
        data = load_sb3_zip(path, self.policy, self.opt, map_location=self.device)
        if raw is not None:
            self.vec_normalize.from_bytes(raw)
        self._graphs = None          # optimizer state tensors were replaced: recapture
        self.num_timesteps = int(data.get("num_timesteps", 0))
        self.n_updates = int(data.get("n_updates", 0))           # absent in older checkpoints
        if "target_kl" in data:
            self.target_kl = data["target_kl"]
            self._kl_sync = self.sync_grads and self.target_kl is not None
        if "clip_range_vf" in data and not callable(self.clip_range_vf):   # a schedule stays the caller's
            self.clip_range_vf = data["clip_range_vf"]
        self._update_hyperparameters()
        return self
