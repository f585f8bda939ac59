"""VecNormalize: running-moment normalisation of observations and rewards (SB3 2.3.2
``common/vec_env/vec_normalize.py`` and ``common/running_mean_std.py``) with the state on the env's device.

Two surfaces over one state:

* the numpy VecEnv surface (``reset`` / ``step_async`` / ``step_wait``) follows SB3's ``VecNormalize`` step by
  step, ``infos[i]["terminal_observation"]`` included, so SB3's own PPO can sit on it unchanged;
* the device surface is what ``ppo.PPO`` and ``evaluation`` use: the observation moments are
  frozen within a rollout and absorb the rollout's obs batches between rollouts (Chan's merge, exact in exact
  arithmetic, so after every rollout they equal SB3's step-by-step moments to float64 rounding); rewards are
  normalised exactly as SB3 does, step by step, in a post-pass over the rollout's [T][N] rewards and dones.

On a GPU the work is the HIP kernels of csrc/ppo_norm.hip (``hs_obs_norm``, ``hs_rms_merge``,
``hs_return_moments``, ``hs_reward_scale``) and the fused policy's obs load (``hs_rollout_norm``,
``hs_evaluate_norm``); on the CPU (toy envs, tests) numpy / torch restate the same arithmetic.
"""
from __future__ import annotations

import io

import numpy as np
import torch

__all__ = ["VecNormalize", "RunningMeanStd"]

_OPTIONS = ("training", "norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma", "epsilon")


class RunningMeanStd:
    """SB3's ``RunningMeanStd`` as a view of device state: ``state`` is one float64 tensor (count, mean[D],
    var[D]), starting at count 1e-4, mean 0, var 1.  ``mean`` / ``var`` / ``count`` are float64 numpy: views
    of the state on the CPU, fresh copies of it on a GPU."""

    def __init__(self, dim, device, shape=None):
        self.dim = int(dim)
        self.shape = (self.dim,) if shape is None else tuple(shape)
        self.state = torch.zeros(1 + 2 * self.dim, dtype=torch.float64, device=device)
        self.state[0] = 1e-4
        self.state[1 + self.dim:] = 1.0

    def _host(self):
        s = self.state
        return s.numpy() if s.device.type == "cpu" else s.cpu().numpy()

    @property
    def count(self):
        return float(self._host()[0])

    @property
    def mean(self):
        return self._host()[1:1 + self.dim].reshape(self.shape)

    @property
    def var(self):
        return self._host()[1 + self.dim:].reshape(self.shape)

    def set(self, mean, var, count):
        h = np.concatenate([[float(count)], np.asarray(mean, dtype=np.float64).reshape(-1),
                            np.asarray(var, dtype=np.float64).reshape(-1)])
        if h.shape[0] != 1 + 2 * self.dim:
            raise ValueError(f"running stats of {h.shape[0] // 2} values do not fit a dimension of {self.dim}")
        self.state.copy_(torch.as_tensor(h))

    def merge_sets(self, sets):
        """``update_from_moments`` (running_mean_std.py) for each (count, mean[D], M2[D]) row of the host
        array ``sets``, in order; rows with count 0 are skipped.  Host arithmetic (the CPU path and the
        numpy surface); the device path is hs_rms_merge."""
        h = self._host().copy()
        D = self.dim
        count, mean, var = h[0], h[1:1 + D], h[1 + D:]
        for s in np.asarray(sets, dtype=np.float64).reshape(-1, 1 + 2 * D):
            bn = s[0]
            if not bn > 0:
                continue
            delta = s[1:1 + D] - mean
            tot = count + bn
            new_mean = mean + delta * bn / tot
            m2 = var * count + s[1 + D:] + np.square(delta) * count * bn / tot
            mean, var, count = new_mean, m2 / tot, tot
        self.set(mean, var, count)

    def update(self, arr):
        """SB3's ``update``: absorb the batch ``arr`` [n, D] (numpy)."""
        arr = np.asarray(arr, dtype=np.float64).reshape(-1, self.dim)
        n = arr.shape[0]
        self.merge_sets(np.concatenate([[float(n)], arr.mean(0), arr.var(0) * n])[None])


def _batch_set(x):
    """(count, mean[D], M2[D]) of the rows of the host array x, float64 two-pass."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], -1)
    m = x.mean(0)
    return np.concatenate([[float(x.shape[0])], m, np.square(x - m).sum(0)])


class VecNormalize:
    """``VecNormalize(venv, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0,
    gamma=0.99, epsilon=1e-8)`` over a device vec-env (``HumanoidVecEnv`` or anything with the PPO env
    protocol).  Everything of the protocol that is not normalisation is the wrapped env's."""

    def __init__(self, venv, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0,
                 gamma=0.99, epsilon=1e-8):
        if isinstance(venv, VecNormalize):
            raise ValueError("VecNormalize: the env is already wrapped")
        if not clip_obs > 0 or not clip_reward > 0:
            raise ValueError("VecNormalize: clip_obs and clip_reward must be positive")
        self.venv = venv
        self.training, self.norm_obs, self.norm_reward = bool(training), bool(norm_obs), bool(norm_reward)
        self.clip_obs, self.clip_reward = float(clip_obs), float(clip_reward)
        self.gamma, self.epsilon = float(gamma), float(epsilon)
        dev = torch.device(venv.device)
        D, N = int(venv.obs_dim), int(venv.num_envs)
        self._dev, self._D, self._N = dev, D, N
        self.obs_rms = RunningMeanStd(D, dev)
        self.ret_rms = RunningMeanStd(1, dev, shape=())
        # what the kernels read: fp32 mean and 1 / sqrt(var + eps), refreshed after every moments change
        self._mean32 = torch.zeros(D, dtype=torch.float32, device=dev)
        self._inv32 = torch.ones(D, dtype=torch.float32, device=dev)
        self._ret_carry = torch.zeros(N, dtype=torch.float64, device=dev)      # SB3's self.returns
        # batch moment sets of one rollout: the reset obs (first rollout), obs_1 .. obs_{T-1}, obs_T
        self._sets = torch.zeros(3, 1 + 2 * D, dtype=torch.float64, device=dev)
        self._absorbed_reset = False
        self._ws = {}
        self.old_obs = self.old_reward = None
        self._refresh()

    # ------------------------------------------------------------------ delegation
    def __getattr__(self, name):
        if name in ("venv", "__setstate__"):
            raise AttributeError(name)
        return getattr(self.venv, name)

    @property
    def returns(self):
        """SB3's ``self.returns``: the per-env discounted return carry (float64 numpy)."""
        c = self._ret_carry
        return c.numpy() if c.device.type == "cpu" else c.cpu().numpy()

    @returns.setter
    def returns(self, value):
        self._ret_carry.copy_(torch.as_tensor(np.asarray(value, dtype=np.float64)))

    # ------------------------------------------------------------------ state
    def _refresh(self):
        """The fp32 mean / inv_std arrays from the float64 state (after the state was set from the host)."""
        if self._dev.type == "cuda":
            from . import _lib
            _lib.check(_lib.lib().hs_rms_merge(self.obs_rms.state.data_ptr(), self._D, None, 0, 0, self.epsilon,
                                               self._mean32.data_ptr(), self._inv32.data_ptr(), self._stream()))
        else:
            h = self.obs_rms._host()
            self._mean32.copy_(torch.as_tensor(h[1:1 + self._D].astype(np.float32)))
            self._inv32.copy_(torch.as_tensor((1.0 / np.sqrt(h[1 + self._D:] + self.epsilon)).astype(np.float32)))

    def _stream(self):
        return torch.cuda.current_stream(self._dev).cuda_stream

    def _buf(self, key, shape, dtype):
        t = self._ws.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._ws[key] = torch.zeros(shape, dtype=dtype, device=self._dev)
        return t

    def norm_args(self):
        """The hs_obs_norm_args of a fused launch (and the tensors it points into)."""
        from . import _lib
        return _lib.hs_obs_norm_args(self._mean32.data_ptr(), self._inv32.data_ptr(), self.clip_obs, self._D)

    # ------------------------------------------------------------------ device surface (PPO, evaluation)
    def normalize_obs_tensor(self, x, out=None, moments_slot=None):
        """clamp((x - mean) inv_std, +-clip_obs) over the rows of the fp32 tensor ``x`` [..., D] (unit column
        stride, equal row strides) into ``out`` (default: in place); ``moments_slot`` 0..2: also the raw
        rows' batch moments into that set of the rollout.  hs_obs_norm on a GPU."""
        D = self._D
        out = x if out is None else out
        x2, o2 = x.reshape(-1, D) if x.is_contiguous() else x, out.reshape(-1, D) if out.is_contiguous() else out
        if x2.dim() != 2 or o2.dim() != 2 or x2.stride(1) != 1 or o2.stride(1) != 1 or x2.dtype != torch.float32:
            raise ValueError("normalize_obs_tensor: need fp32 rows of obs_dim values with unit column stride")
        R = x2.shape[0]
        if x2.device.type == "cuda":
            from . import _lib
            L = _lib.lib()
            mom = ws = None
            if moments_slot is not None:
                nbytes = int(L.hs_obs_norm_workspace(R, D))
                ws = self._buf("obs_ws", (nbytes // 8,), torch.float64).data_ptr()
                mom = self._sets[moments_slot].data_ptr()
            _lib.check(L.hs_obs_norm(x2.data_ptr(), x2.stride(0), R, D, self._mean32.data_ptr(), self._inv32.data_ptr(),
                                     self.clip_obs, o2.data_ptr(), o2.stride(0), mom, ws, self._stream()))
            return out
        if moments_slot is not None:
            self._sets[moments_slot].copy_(torch.as_tensor(_batch_set(x2.numpy())))
        o2.copy_(((x2 - self._mean32) * self._inv32).clamp(-self.clip_obs, self.clip_obs))
        return out

    def begin_rollout(self):
        self._sets[:, 0] = 0.0

    def absorb_reset(self):
        """True once: the first rollout also absorbs the reset obs, as VecNormalize.reset does."""
        first = not self._absorbed_reset
        self._absorbed_reset = True
        return first

    def merge_obs_moments(self, world_size=1, comm_device=None):
        """obs_rms absorbs the rollout's batch moment sets; with world_size > 1 every rank's sets are
        all-gathered first and merged in rank order, so all ranks end with bitwise the same moments."""
        sets = self._sets
        if world_size > 1:
            sets = _all_gather(sets, world_size, comm_device).to(self._dev)
        n = sets.numel() // (1 + 2 * self._D)
        if self._dev.type == "cuda":
            from . import _lib
            sets = sets.contiguous()
            _lib.check(_lib.lib().hs_rms_merge(self.obs_rms.state.data_ptr(), self._D, sets.data_ptr(), n,
                                               1 + 2 * self._D, self.epsilon, self._mean32.data_ptr(),
                                               self._inv32.data_ptr(), self._stream()))
        else:
            self.obs_rms.merge_sets(sets.numpy())
            self._refresh()

    def normalize_rewards_rollout(self, rew, done, world_size=1, comm_device=None):
        """VecNormalize.step_wait's reward path over a rollout's [T][N] fp32 rewards (in place) and bool /
        uint8 dones, step by step: returns advance, ret_rms absorbs the step's returns, the step's rewards are
        scaled with the updated variance and clipped, the done envs' returns are zeroed."""
        T, N = rew.shape
        training = self.training
        if rew.device.type == "cuda":
            from . import _lib
            L = _lib.lib()
            d8 = done.view(torch.uint8) if done.dtype == torch.bool else done
            sets = self._buf("ret_sets", (T, 3), torch.float64)
            sets.zero_()
            if training:
                ws = self._buf("ret_ws", (T, N), torch.float64)
                _lib.check(L.hs_return_moments(rew.data_ptr(), d8.data_ptr(), T, N, self.gamma,
                                               self._ret_carry.data_ptr(), ws.data_ptr(), sets.data_ptr(),
                                               self._stream()))
            else:
                self._ret_carry.masked_fill_(done.bool().any(0), 0.0)
            if not self.norm_reward and not training:
                return
            nsets = 1
            if world_size > 1 and training:
                sets = _all_gather(sets, world_size, comm_device).to(self._dev).contiguous()
                nsets = world_size
            if self.norm_reward:
                scale = self._buf("ret_scale", (T,), torch.float64)
                _lib.check(L.hs_reward_scale(rew.data_ptr(), T, N, self.ret_rms.state.data_ptr(), sets.data_ptr(),
                                             nsets, 3 * T, self.epsilon, self.clip_reward, scale.data_ptr(),
                                             self._stream()))
            else:      # SB3 updates ret_rms while training even with norm_reward off
                self._merge_return_sets(sets.cpu().numpy().reshape(nsets, T, 3), None)
            return
        # CPU: the same arithmetic in numpy
        r, d = rew.numpy(), done.numpy().astype(bool)
        sets = np.zeros((T, 3))
        if training:
            carry = self._ret_carry.numpy()
            for t in range(T):
                carry[:] = carry * self.gamma + r[t].astype(np.float64)
                m = carry.mean()
                sets[t] = (N, m, np.square(carry - m).sum())
                carry[d[t]] = 0.0
        else:
            self._ret_carry[torch.as_tensor(d.any(0))] = 0.0
        sets = sets[None]
        if world_size > 1 and training:
            sets = _all_gather(torch.as_tensor(sets[0]), world_size, comm_device).numpy().reshape(world_size, T, 3)
        self._merge_return_sets(sets, r if self.norm_reward else None)

    def _merge_return_sets(self, sets, r):
        """Host restatement of hs_reward_scale: sets [n_sets][T][3]; r: the [T][N] fp32 rewards to scale in
        place, or None (moments only)."""
        h = self.ret_rms._host()
        count, mean, var = float(h[0]), float(h[1]), float(h[2])
        for t in range(sets.shape[1]):
            bn = bm = bq = 0.0
            for k in range(sets.shape[0]):
                n, m, q = (float(v) for v in sets[k, t])
                if not n > 0:
                    continue
                if bn == 0.0:
                    bn, bm, bq = n, m, q
                    continue
                delta, tot = m - bm, bn + n
                bq = bq + q + delta * delta * bn * n / tot
                bm = bm + delta * n / tot
                bn = tot
            if bn > 0:
                delta, tot = bm - mean, count + bn
                new_mean = mean + delta * bn / tot
                m2 = var * count + bq + delta * delta * count * bn / tot
                mean, var, count = new_mean, m2 / tot, tot
            if r is not None:
                y = r[t].astype(np.float64) / np.sqrt(var + self.epsilon)
                r[t] = np.clip(y, -self.clip_reward, self.clip_reward).astype(np.float32)
        self.ret_rms.set(mean, var, count)

    # ------------------------------------------------------------------ SB3's numpy surface
    def normalize_obs(self, obs):
        """SB3 ``normalize_obs``: float32 of clip((obs - mean) / sqrt(var + eps), +-clip_obs) in float64."""
        obs = np.asarray(obs)
        if not self.norm_obs:
            return obs.copy()
        y = np.clip((obs - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon), -self.clip_obs, self.clip_obs)
        return y.astype(np.float32)

    def normalize_reward(self, reward):
        reward = np.asarray(reward)
        if not self.norm_reward:
            return reward
        return np.clip(reward / np.sqrt(self.ret_rms.var + self.epsilon), -self.clip_reward, self.clip_reward)

    def unnormalize_obs(self, obs):
        if not self.norm_obs:
            return np.asarray(obs)
        return np.asarray(obs) * np.sqrt(self.obs_rms.var + self.epsilon) + self.obs_rms.mean

    def unnormalize_reward(self, reward):
        if not self.norm_reward:
            return np.asarray(reward)
        return np.asarray(reward) * np.sqrt(self.ret_rms.var + self.epsilon)

    def get_original_obs(self):
        return None if self.old_obs is None else np.array(self.old_obs, copy=True)

    def get_original_reward(self):
        return None if self.old_reward is None else np.array(self.old_reward, copy=True)

    def _obs_changed(self):
        self._absorbed_reset = True
        self._refresh()

    def reset(self):
        obs = self.venv.reset()
        self.old_obs = obs
        self.returns = np.zeros(self._N)
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
            self._obs_changed()
        return self.normalize_obs(obs)

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        obs, rewards, dones, infos = self.venv.step_wait()
        self.old_obs, self.old_reward = obs, rewards
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
            self._obs_changed()
        obs = self.normalize_obs(obs)
        ret = self.returns.copy()
        if self.training:          # _update_reward
            ret = ret * self.gamma + rewards
            self.ret_rms.update(ret.reshape(-1, 1))
        rewards = self.normalize_reward(rewards)
        dones = np.asarray(dones)
        infos = list(infos)
        for i in np.flatnonzero(dones):
            if "terminal_observation" in infos[i]:
                infos[i] = dict(infos[i])
                infos[i]["terminal_observation"] = self.normalize_obs(infos[i]["terminal_observation"])
        ret[dones.astype(bool)] = 0
        self.returns = ret
        return obs, rewards, dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        """Both moment sets, the options and the return carry (numpy; ``vec_normalize.npz`` of PPO.save)."""
        d = {"obs_mean": self.obs_rms.mean.copy(), "obs_var": self.obs_rms.var.copy(),
             "obs_count": np.float64(self.obs_rms.count), "ret_mean": np.float64(self.ret_rms.mean),
             "ret_var": np.float64(self.ret_rms.var), "ret_count": np.float64(self.ret_rms.count),
             "returns": self.returns.copy(), "absorbed_reset": np.bool_(self._absorbed_reset)}
        for k in _OPTIONS:
            d[k] = np.asarray(getattr(self, k))
        return d

    def load_state_dict(self, d, options=True):
        self.obs_rms.set(d["obs_mean"], d["obs_var"], d["obs_count"])
        self.ret_rms.set(d["ret_mean"], d["ret_var"], d["ret_count"])
        if "returns" in d and np.asarray(d["returns"]).shape == (self._N,):
            self.returns = d["returns"]
        if options:
            for k in _OPTIONS:
                if k in d:
                    setattr(self, k, type(getattr(self, k))(np.asarray(d[k]).item()))
        self._absorbed_reset = bool(np.asarray(d.get("absorbed_reset", True)).item())
        self._refresh()

    def load_running_stats(self, stats):
        """Arrays copied from an SB3 ``VecNormalize``: ``{"obs_rms": {"mean", "var", "count"}, "ret_rms":
        {...}}`` (either may be missing), or objects with those attributes."""
        def parts(x):
            get = (lambda k: x[k]) if isinstance(x, dict) else (lambda k: getattr(x, k))
            return get("mean"), get("var"), get("count")
        get = (lambda k: stats.get(k)) if isinstance(stats, dict) else (lambda k: getattr(stats, k, None))
        if get("obs_rms") is not None:
            self.obs_rms.set(*parts(get("obs_rms")))
        if get("ret_rms") is not None:
            self.ret_rms.set(*parts(get("ret_rms")))
        self._absorbed_reset = True
        self._refresh()

    def to_bytes(self):
        f = io.BytesIO()
        np.savez(f, **self.state_dict())
        return f.getvalue()

    def from_bytes(self, raw):
        with np.load(io.BytesIO(raw), allow_pickle=False) as z:
            self.load_state_dict({k: z[k] for k in z.files})


def _all_gather(t, world_size, comm_device):
    """[world][...] of every rank's ``t`` (the same shape everywhere), on the communication device."""
    import torch.distributed as dist
    src = t.to(comm_device).contiguous()
    out = [torch.empty_like(src) for _ in range(world_size)]
    dist.all_gather(out, src)
    return torch.stack(out)


def unwrap(env):
    """(raw env, VecNormalize or None)."""
    return (env.venv, env) if isinstance(env, VecNormalize) else (env, None)
