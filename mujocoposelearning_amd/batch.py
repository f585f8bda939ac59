"""A batch of humanoid envs resident in HBM, stepped by the HIP kernels through the C ABI.

``HsBatch`` allocates every per-env buffer as a torch tensor on the chosen GPU and binds them
to the native batch (``hs_batch_create(..., external=buffers)``), so observations / rewards /
dones are device tensors that a PyTorch policy consumes without leaving HBM.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, lib

KNEEL_DEFAULTS = (1.282, 0.85, math.pi / 6, 0.1, 0.3, 0.3, 0.2, 0.1, 0.1)
KNEEL_KEYS = ("target_height", "min_height", "max_roll_pitch", "com_radius", "energy_weight", "posture_weight",
              "com_weight", "foot_weight", "alive_weight")


def _torch():
    import torch
    return torch


# MuJoCo's own warning texts for the three bad-state resets (mjWARN_BADQPOS / QVEL / QACC)
WARN_KINDS = ("Nan, Inf or huge value in QPOS", "Nan, Inf or huge value in QVEL", "Nan, Inf or huge value in QACC",
              "contacts dropped past the wide contact tier", "chunk-queue hand-off lost")


def report_warnings(new, where="step"):
    """Surface new warning counts (include/hsim.h HS_WARN_*, one value per kind) the way the reference
    run surfaces them: MuJoCo's mj_step prints mju_warning and resets a bad state (mj_resetData) and the
    run goes on (custom_env.py:160) -- here one RuntimeWarning per call with the counts; a lost
    chunk-queue hand-off is a scheduling failure of the step kernel, not physics, so it raises."""
    new = np.asarray(new, dtype=np.int64)
    if len(new) > 4 and new[4] > 0:
        raise _lib.HsimError(f"{WARN_KINDS[4]} in {int(new[4])} env step(s) of this {where}: a scheduling failure of "
                             "the step kernel (e.g. more concurrent queued batches than the GPU holds waves for), "
                             "not physics -- those envs were reset and the results are not valid")
    parts = [f"{WARN_KINDS[k]} in {int(new[k])} env step(s) of this {where}" for k in range(min(4, len(new)))
             if new[k] > 0]
    if parts:
        import warnings
        warnings.warn("mj_step warning: " + "; ".join(parts) + (" -- those envs were reset (mj_resetData)"
                      if new[:3].any() else ""), RuntimeWarning, stacklevel=3)


class _DeviceBytes:
    """A [n] uint8 buffer of the native library as torch sees it (``torch.as_tensor`` reads the interface)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "|u1", "data": (int(ptr), False),
                                         "strides": None, "version": 2}


def reward_eval(model, name, qpos, qvel, ctrl, time, subtree_com0, subtree_linvel0, cfrc_ext, qfrc_actuator,
                params=None, registry=None, cinert=None, cvel=None):
    """``REWARD_FUNCTIONS[name](data, params)`` for n states at once, computed by the device reward
    code of the step kernel (``hs_reward_eval``; reward_functions.py:66-269).  Arguments are CUDA
    tensors of one float dtype (float64 = the fp64 engine's formulas, float32 = the fp32 engine's):
    qpos [n][nq], qvel [n][nv], ctrl [n][nu], time [n], subtree_com0 / subtree_linvel0 [n][3],
    cfrc_ext [n][nbody][6], qfrc_actuator [n][nv].  ``params`` are the kneeling reward's overrides
    (merged over its defaults like reward_functions.py:83).  Returns a [n] tensor.  Unknown names raise
    ValueError like custom_env.py:268-269; plain user callables have no device formula (HsimError).
    A reward registered as a program (``reward_program.register_device_reward``) runs through
    ``hs_reward_program_eval``; ``params`` are then its parameter overrides, ``cinert`` [n][nbody][10] and
    ``cvel`` [n][nbody][6] the two further fields a program may read, and of ``subtree_linvel`` a program
    sees row 0 as given and zeros elsewhere."""
    from .reward_functions import device_reward_id
    torch = _torch()
    rid = device_reward_id(name, registry)
    if rid is None:
        from .reward_program import device_reward_program
        rec = device_reward_program(name, registry)
        if rec is None:
            raise _lib.HsimError(f"reward {name!r} is a host callable: no device formula")
        return _reward_program_eval(model, rec, params, qpos=qpos, qvel=qvel, ctrl=ctrl, time=time,
                                    subtree_com=subtree_com0, subtree_linvel0=subtree_linvel0, cfrc_ext=cfrc_ext,
                                    qfrc_actuator=qfrc_actuator, cinert=cinert, cvel=cvel)
    args = [qpos, qvel, ctrl, time, subtree_com0, subtree_linvel0, cfrc_ext, qfrc_actuator]
    dt = qpos.dtype
    if dt not in (torch.float32, torch.float64):
        raise TypeError("reward_eval: float32 or float64 tensors")
    n = qpos.shape[0]
    shapes = [(n, model.nq), (n, model.nv), (n, model.nu), (n,), (n, 3), (n, 3), (n, model.nbody, 6),
              (n, model.nv)]
    for a, s in zip(args, shapes):
        if not a.is_cuda or a.dtype != dt or tuple(a.shape) != s or not a.is_contiguous():
            raise ValueError(f"reward_eval: expected a contiguous CUDA {dt} tensor of shape {s}, got "
                             f"{tuple(a.shape)} {a.dtype} on {a.device}")
    kn = None
    if rid == 1:
        p = {**dict(zip(KNEEL_KEYS, KNEEL_DEFAULTS)), **(params or {})}
        kn = (C.c_double * 9)(*[float(p[k]) for k in KNEEL_KEYS])
    out = torch.empty(n, dtype=dt, device=qpos.device)
    with torch.cuda.device(qpos.device):
        st = torch.cuda.current_stream().cuda_stream
        check(lib().hs_reward_eval(model.handle, 1 if dt == torch.float64 else 0, rid,
                                   C.cast(kn, C.c_void_p) if kn is not None else None, n,
                                   *[a.data_ptr() for a in args], out.data_ptr(), st))
    return out


def _reward_program_eval(model, rec, params, subtree_linvel0=None, **fields):
    """``reward_eval`` for a reward program: the fields it reads, checked, through hs_reward_program_eval."""
    torch = _torch()
    prog = rec.compile(model)
    qpos = fields["qpos"]
    dt, n = qpos.dtype, qpos.shape[0]
    if dt not in (torch.float32, torch.float64):
        raise TypeError("reward_eval: float32 or float64 tensors")
    if "subtree_linvel" in prog.fields:
        lv = torch.zeros(n, model.nbody, 3, dtype=dt, device=qpos.device)
        lv[:, 0] = subtree_linvel0
        fields["subtree_linvel"] = lv
    shapes = dict(qpos=(n, model.nq), qvel=(n, model.nv), ctrl=(n, model.nu), time=(n,), subtree_com=(n, 3),
                  subtree_linvel=(n, model.nbody, 3), cfrc_ext=(n, model.nbody, 6), qfrc_actuator=(n, model.nv),
                  cinert=(n, model.nbody, 10), cvel=(n, model.nbody, 6))
    f = _lib.hs_reward_fields()
    for k in prog.fields:
        a = fields.get(k)
        if a is None:
            raise ValueError(f"reward_eval: the program reads {k}, which was not given")
        if not a.is_cuda or a.dtype != dt or tuple(a.shape) != shapes[k] or not a.is_contiguous():
            raise ValueError(f"reward_eval: expected a contiguous CUDA {dt} tensor of shape {shapes[k]} for {k}, got "
                             f"{tuple(a.shape)} {a.dtype} on {a.device}")
        setattr(f, _lib.REWARD_FIELD_MEMBER[k], a.data_ptr())
    out = torch.empty(n, dtype=dt, device=qpos.device)
    with torch.cuda.device(qpos.device):
        st = torch.cuda.current_stream().cuda_stream
        check(lib().hs_reward_program_eval(prog.handle, 1 if dt == torch.float64 else 0, prog.params(params), n,
                                           C.byref(f), out.data_ptr(), st))
    return out


class HsBatch:
    def __init__(self, model, n_envs, device=0, seed=0, precision="fp32", full_state=False, groups=1):
        """``groups`` > 1 splits the envs into that many native sub-batches (contiguous env ranges
        bound to slices of the same tensors), each launched on its own HIP stream: a group's
        Newton-iteration tail can overlap the other groups' next launches.  That needs the groups
        to run free (``step(..., join=False)`` then ``join()``): a per-step join (the default, what
        a policy that reads every env's obs needs) makes each step as long as its slowest group.
        Results per env are identical; reset-noise streams differ (per-group seeds)."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("HsBatch needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.model = model
        self.n = int(n_envs)
        self.device = torch.device("cuda", int(device))
        self.precision = precision
        prec = _lib.HS_FP64 if precision == "fp64" else _lib.HS_FP32
        self.dtype = torch.float64 if prec == _lib.HS_FP64 else torch.float32
        nq, nv, nu, nb = model.nq, model.nv, model.nu, model.nbody
        self.full_state = bool(full_state)
        # custom_env.py:242-256 (352 for humanoid.xml); full_state adds cfrc_ext[1:] (their :247)
        self.obs_dim = (nq - 2) + nv + 10 * nb + 6 * nb + nv + (6 * (nb - 1) if self.full_state else 0)
        N, f, i32, u8 = self.n, self.dtype, torch.int32, torch.uint8
        z = lambda *s, dt=f: torch.zeros(*s, dtype=dt, device=self.device)  # noqa: E731
        self.t = dict(qpos=z(N, nq), qvel=z(N, nv), qacc_warmstart=z(N, nv), ctrl=z(N, nu), time=z(N),
                      step_count=z(N, dt=i32), episode=z(N, dt=i32), total_reward=z(N),
                      warning=z(N, _lib.HS_NWARN, dt=i32), obs=z(N, self.obs_dim), terminal_obs=z(N, self.obs_dim),
                      reward=z(N), terminated=z(N, dt=u8), truncated=z(N, dt=u8), aux=z(N, _lib.HS_AUXDIM),
                      cfrc_ext=z(N, nb, 6), subtree_linvel=z(N, nb, 3), terminal_step_count=z(N, dt=i32),
                      terminal_total_reward=z(N))
        torch.cuda.synchronize(self.device)
        flags = prec | (_lib.HS_FULL_STATE if self.full_state else 0)
        G = max(1, min(int(groups), self.n))
        bounds = [self.n * g // G for g in range(G + 1)]
        self._groups = []                       # (handle, lo, hi)
        self._seed = int(seed)
        # counts the changes of what a launch is given beyond the batch's buffers (set_initial_states): a launch
        # recorded into a graph holds the old arguments, so whoever replays one compares this number first
        self.launch_generation = 0
        for g in range(G):
            lo, hi = bounds[g], bounds[g + 1]
            bufs = _lib.hs_buffers(**{k: v.data_ptr() + lo * v.stride(0) * v.element_size() for k, v in self.t.items()})
            gseed = self._group_seed(g)
            h = lib().hs_batch_create(model.handle, hi - lo, self.device.index, gseed, flags, C.byref(bufs))
            if not h:
                self.close()
                raise _lib.HsimError(lib().hs_last_error().decode())
            self._groups.append((h, lo, hi))
        self._h = self._groups[0][0]
        # group 0 runs on the caller's current stream, groups 1.. on their own: G groups use exactly G
        # streams (a process has GPU_MAX_HW_QUEUES = 4 hardware queues; two streams sharing one serialise)
        self._streams = [None] + [torch.cuda.Stream(self.device) for _ in range(G - 1)] if G > 1 else None
        self._events = [torch.cuda.Event()] if G > 1 else None
        self._free = False
        self.cfg = _lib.hs_env_config()
        check(lib().hs_get_config(self._h, C.byref(self.cfg)))
        info = _lib.hs_batch_info()
        check(lib().hs_batch_get_info(self._h, C.byref(info)))
        # per-env (contacts, constraint rows) of the resident kernel tier and of the wide re-run tier
        self.resident_capacity = (info.resident_con, info.resident_efc)
        self.wide_capacity = (info.wide_con, info.wide_efc)
        self.resident_waves = info.resident_waves
        # static worst case (contacts, rows) of one env: every pair touching / every geom on the floor
        self.contact_bound_all = (info.bound_con_all, info.bound_efc_all)
        self.contact_bound_floor = (info.bound_con_floor, info.bound_efc_floor)

    def queued(self, nsub=None):
        """True when an env step of this batch runs on the chunk-queue schedule (HS_SCHED_AUTO, more
        env pairs than resident waves, >= 2 substeps; include/hsim.h)."""
        return self.schedule(nsub)[0]

    def schedule_name(self, nsub=None):
        """The schedule an env step of this batch runs on (the largest group's; hs_batch_schedule):
        "queue" (chunk queue), "single" (one wave per env) or "paired"."""
        queue, single = self.schedule(nsub)
        return "queue" if queue else "single" if single else "paired"

    def schedule(self, nsub=None, n_steps=1):
        """(queued, single) of the largest group's launch of n_steps env steps (hs_batch_schedule)."""
        h = max(self._groups, key=lambda g: g[2] - g[1])[0]
        queue, single = C.c_int(0), C.c_int(0)
        check(lib().hs_batch_schedule(h, int(self.cfg.frame_skip if nsub is None else nsub), int(n_steps),
                                      C.byref(queue), C.byref(single)))
        return bool(queue.value), bool(single.value)

    # -- tensors (device views, valid until the next call) ---------------------------------
    def __getattr__(self, name):
        t = self.__dict__.get("t")
        if t is not None and name in t:
            return t[name]
        raise AttributeError(name)

    @property
    def stream(self):
        return _torch().cuda.current_stream(self.device).cuda_stream

    # -- configuration ---------------------------------------------------------------------
    def configure(self, frame_skip=None, duration=None, reward_id=None, max_steps=None, autoreset=None,
                  max_newton=None, init_height=None, noise_scale=None, kneel_params=None, aux=None, ctrl=None,
                  schedule=None):
        """``schedule``: "auto" (default: one wave per env when every env fits the resident waves, a
        chunk queue when the env pairs outnumber them, else one wave per env pair; include/hsim.h
        HS_SCHED_AUTO), "direct" (one wave per env pair), "single" (one wave per env) or
        "fixed_order" (auto with the chunk queue's claims in a fixed permutation instead of cost
        order); results are bitwise identical.
        ``aux`` / ``ctrl``: write the optional aux row (qacc, subtree com, contact / row counts,
        solver iterations) and the data.ctrl copy at every commit (both on by default; data views,
        host rewards and statistics read them, the on-device trainer does not)."""
        c = self.cfg
        if aux is not None:
            c.outputs = (c.outputs & ~_lib.HS_OUT_AUX) | (_lib.HS_OUT_AUX if aux else 0)
        if ctrl is not None:
            c.outputs = (c.outputs & ~_lib.HS_OUT_CTRL) | (_lib.HS_OUT_CTRL if ctrl else 0)
        if schedule is not None:
            c.schedule = {"auto": _lib.HS_SCHED_AUTO, "direct": _lib.HS_SCHED_DIRECT,
                          "single": _lib.HS_SCHED_SINGLE, "fixed_order": _lib.HS_SCHED_FIXED_ORDER}[schedule]
        if frame_skip is not None:
            c.frame_skip = int(frame_skip)
        if duration is not None:
            c.duration = float(duration)
        if reward_id is not None:
            c.reward_id = int(reward_id)
        if max_steps is not None:
            c.max_steps = int(max_steps)
        if autoreset is not None:
            c.autoreset = int(bool(autoreset))
        if max_newton is not None:
            c.max_newton = int(max_newton)
        if init_height is not None:
            c.init_height = float(init_height)
        if noise_scale is not None:
            c.noise_scale = float(noise_scale)
        if kneel_params is not None:
            p = {**dict(zip(KNEEL_KEYS, KNEEL_DEFAULTS)), **kneel_params}
            for k, key in enumerate(KNEEL_KEYS):
                c.kneel_params[k] = float(p[key])
        for h, _, _ in self._groups:
            check(lib().hs_set_config(h, C.byref(c)))

    def set_seed(self, seed):
        self._seed = int(seed)
        for g, (h, _, _) in enumerate(self._groups):
            check(lib().hs_set_seed(h, self._group_seed(g)))

    def _launch(self, fn, *tensors, join=True):
        """fn(handle, lo, hi, stream) per group; multi-group launches fan out to the group streams
        and (join=True) join back into the caller's current stream.  A free-running session
        (join=False) waits on the caller's stream once, at its first launch (inputs produced before
        it); later free launches add no cross-stream waits (5 streams share the 4 hardware queues
        of a process, GPU_MAX_HW_QUEUES=4, and per-step waits would serialise them again)."""
        if self._streams is None:
            h, lo, hi = self._groups[0]
            fn(h, lo, hi, self.stream)
            return
        torch = _torch()
        cur = torch.cuda.current_stream(self.device)
        if join or not self._free:
            self._events[0].record(cur)
            for st in self._streams[1:]:
                st.wait_event(self._events[0])
        self._free = not join
        for (h, lo, hi), st in zip(self._groups, self._streams):
            if st is not None:
                for t in tensors:
                    if t is not None:
                        t.record_stream(st)
            fn(h, lo, hi, (cur if st is None else st).cuda_stream)
        if join:
            self.join()

    def join(self):
        """Make the caller's current stream wait for every group's last launch."""
        if self._streams is None:
            return
        cur = _torch().cuda.current_stream(self.device)
        for st in self._streams[1:]:
            cur.wait_stream(st)
        self._free = False

    # -- stepping --------------------------------------------------------------------------
    def reset(self, mask=None, qpos_noise=None, qvel_noise=None):
        """custom_env.py:97-150 for the envs selected by ``mask`` (None = all)."""
        torch = _torch()
        keep = []
        def dev(x, dt):
            if x is None:
                return None
            x = torch.as_tensor(x, device=self.device).to(dt).contiguous()
            keep.append(x)
            return x
        mk, qn, vn = dev(mask, torch.uint8), dev(qpos_noise, self.dtype), dev(qvel_noise, self.dtype)

        def off(x, lo):
            return None if x is None else x.data_ptr() + lo * x.stride(0) * x.element_size()
        self._launch(lambda h, lo, hi, st: check(lib().hs_reset(h, off(mk, lo), off(qn, lo), off(vn, lo), st)),
                     mk, qn, vn)
        return self.t["obs"]

    def set_autoreset_noise(self, qpos_noise=None, qvel_noise=None):
        """Bind [N, nq] / [N, nv] device tensors (batch dtype) holding each env's NEXT reset noise
        for the auto-reset inside ``step`` (None: the on-device counter RNG).  The tensors are
        kept referenced; refresh the rows of envs that reset (hs_set_autoreset_noise)."""
        torch = _torch()
        if qpos_noise is None:
            self._ar_noise = None
            for h, _, _ in self._groups:
                check(lib().hs_set_autoreset_noise(h, None, None))
            return
        qn = torch.as_tensor(qpos_noise, device=self.device).to(self.dtype).contiguous()
        vn = torch.as_tensor(qvel_noise, device=self.device).to(self.dtype).contiguous()
        assert qn.shape == (self.n, self.model.nq) and vn.shape == (self.n, self.model.nv)
        self._ar_noise = (qn, vn)
        for h, lo, hi in self._groups:
            check(lib().hs_set_autoreset_noise(h, qn.data_ptr() + lo * qn.stride(0) * qn.element_size(),
                                               vn.data_ptr() + lo * vn.stride(0) * vn.element_size()))
        return qn, vn

    # -- where episodes begin (hs_set_initial_states) ------------------------------------------
    def set_initial_states(self, qpos=None, qvel=None):
        """Bind the bank of initial states every reset of this batch draws its start from: ``qpos`` [K, nq] and
        ``qvel`` [K, nv] (None: zeros) as host arrays, e.g. ``initial_state.build_bank(model, spec)``; ``qpos``
        None unbinds, and resets are the reference's again.  Each group gets the same bank and draws with its own
        seed.  A row's free-joint quaternion is normalised by the library.  The call waits for the batch's pending
        launches; a trainer that replays a recorded per-step graph re-records it (``launch_generation``).
        HsimError: rows of the wrong length, a value that is not finite, a zero quaternion, more than
        ``HS_MAX_INITIAL_STATES`` rows."""
        from .initial_state import normalize_quaternions
        self.launch_generation += 1
        if qpos is None:
            for h, _, _ in self._groups:
                check(lib().hs_set_initial_states(h, 0, None, None))
            self._initial_states = None
            return None
        nq, nv = self.model.nq, self.model.nv
        q = np.ascontiguousarray(np.asarray(qpos, dtype=np.float64))
        q = q[None] if q.ndim == 1 else q
        if q.ndim != 2 or q.shape[1] != nq or q.shape[0] < 1:
            raise _lib.HsimError(f"set_initial_states: qpos must be [K, {nq}] with K >= 1, got {q.shape}")
        v = None
        if qvel is not None:
            v = np.ascontiguousarray(np.asarray(qvel, dtype=np.float64))
            v = v[None] if v.ndim == 1 else v
            if v.shape != (q.shape[0], nv):
                raise _lib.HsimError(f"set_initial_states: qvel must be [{q.shape[0]}, {nv}], got {v.shape}")
        for h, _, _ in self._groups:
            check(lib().hs_set_initial_states(h, q.shape[0], q.ctypes.data, None if v is None else v.ctypes.data))
        # the rows as the library holds them (fp64; an fp32 batch rounds them once more)
        self._initial_states = (normalize_quaternions(q), np.zeros((q.shape[0], nv)) if v is None else v.copy())
        return self._initial_states

    @property
    def initial_states(self):
        """(qpos [K, nq], qvel [K, nv]) float64 host arrays of the bound bank as the library holds it (quaternions
        normalised; an fp32 batch holds them rounded to float32), or None when none is bound."""
        return self.__dict__.get("_initial_states")

    def initial_state_index(self):
        """[N] int64 host array: the bank row each env's current episode started from, restated on the host from
        the ``episode`` counters and the group seeds (``initial_state.draw_index``).  Meaningful for the episodes
        that began with this bank bound; -1 for an env that was never reset, and for every env with no bank."""
        from .initial_state import draw_index
        out = np.full(self.n, -1, dtype=np.int64)
        bank = self.initial_states
        if bank is None:
            return out
        ep = self.t["episode"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        for g, (_, lo, hi) in enumerate(self._groups):
            out[lo:hi] = draw_index(self._group_seed(g), np.arange(hi - lo), ep[lo:hi], len(bank[0]))
        out[ep == 0] = -1
        return out

    # -- what rewards and termination conditions compare against (hs_set_reference_motion) ------
    def set_reference_motion(self, qpos=None, qvel=None, key_dt=None, end="hold", start="zero"):
        """Bind the reference motion that reward and termination programs read as ``d.ref_qpos`` / ``d.ref_qvel``
        (``reference_motion.py``): ``qpos`` [K, nq] and ``qvel`` [K, nv] (None: zeros) as host arrays, ``key_dt``
        seconds between rows (required with K > 1), ``end`` ``"hold"`` | ``"loop"``, ``start`` ``"zero"`` |
        ``"drawn"`` -- or one ``reference_motion.Reference`` as the first argument.  ``qpos`` None unbinds.  Each
        group gets the same rows and draws with its own seed.  ``start="drawn"`` needs a bank of initial states of
        the same K bound by the time a program that reads the reference is launched (checked then, before the
        launch).  The call waits for the batch's pending launches; a trainer that replays a recorded per-step graph
        re-records it (``launch_generation``).  A batch whose programs do not read the reference runs exactly the
        launches it ran before.  ValueError / HsimError: rows of the wrong length, a value that is not finite, a zero
        quaternion, more than ``HS_MAX_REFERENCE_ROWS`` rows, a missing ``key_dt``, an unknown mode."""
        from .reference_motion import Reference
        if qpos is None:
            self.launch_generation += 1
            for h, _, _ in self._groups:
                check(lib().hs_set_reference_motion(h, 0, None, None, 0.0, 0))
            self._reference_motion = None
            return None
        nq, nv = self.model.nq, self.model.nv
        ref = qpos if isinstance(qpos, Reference) else Reference(qpos, qvel, key_dt, end, start, nv=nv)
        if ref.qpos.shape[1] != nq or ref.qvel.shape[1] != nv:
            raise _lib.HsimError(f"set_reference_motion: rows must be [K, {nq}] / [K, {nv}], got "
                                 f"{ref.qpos.shape} / {ref.qvel.shape}")
        self.launch_generation += 1
        q, v = np.ascontiguousarray(ref.qpos), np.ascontiguousarray(ref.qvel)
        for h, _, _ in self._groups:
            check(lib().hs_set_reference_motion(h, ref.K, q.ctypes.data, v.ctypes.data,
                                                1.0 if ref.key_dt is None else ref.key_dt, ref.flags))
        # the rows as the library holds them: it normalises the quaternions of what it is given once more, by the
        # expression of initial_state.normalize_quaternions, which moves an already normalised one by an ulp at most
        self._reference_motion = Reference(ref.qpos, ref.qvel, ref.key_dt, ref.end, ref.start)
        return self._reference_motion

    @property
    def reference_motion(self):
        """The bound ``reference_motion.Reference``, or None: the float64 rows as the library holds them (it
        normalises the quaternions once more when it binds them, so they may differ from the rows given in the last
        bit; an fp32 batch holds them rounded to float32).  ``reference_motion.sample`` of THIS object is bitwise
        what the device reads."""
        return self.__dict__.get("_reference_motion")

    def _group_seeds_env(self):
        """Per env: its group's seed (a list of ints) and its index within the group ([N] int64)."""
        seeds, env = [0] * self.n, np.zeros(self.n, dtype=np.int64)
        for g, (_, lo, hi) in enumerate(self._groups):
            seeds[lo:hi] = [self._group_seed(g)] * (hi - lo)
            env[lo:hi] = np.arange(hi - lo)
        return seeds, env

    def reference_phase(self):
        """[N] float64 host array: each env's phase x on the bound reference at its current ``episode`` and ``time``
        -- start row + time / key_dt after its clamps, the value whose floor indexes the rows
        (``reference_motion.phase``, the host restatement of what the kernel computes).  HsimError with none bound."""
        from .reference_motion import phase
        ref = self.reference_motion
        if ref is None:
            raise _lib.HsimError("reference_phase: the batch has no reference motion bound (set_reference_motion)")
        seeds, env = self._group_seeds_env()
        return phase(ref, self.t["time"].cpu().numpy(), self.t["episode"].cpu().numpy(), seeds, env)[0]

    def reference_sample(self):
        """(ref_qpos [N, nq], ref_qvel [N, nv]) host arrays of the batch dtype: what a program launched now would read
        (``reference_motion.sample`` at the envs' current ``episode`` and ``time``)."""
        from .reference_motion import sample
        ref = self.reference_motion
        if ref is None:
            raise _lib.HsimError("reference_sample: the batch has no reference motion bound (set_reference_motion)")
        seeds, env = self._group_seeds_env()
        return sample(ref, self.t["time"].cpu().numpy(), self.t["episode"].cpu().numpy(), seeds, env,
                      dtype=np.float64 if self.precision == "fp64" else np.float32)

    def _group_seed(self, g):
        return (int(self._seed) + 0x9E3779B97F4A7C15 * g) & (2 ** 64 - 1)

    def step(self, actions, join=True):
        """custom_env.py:152-230 batched; ``actions`` [N, nu] float32 on device.  With stream
        groups and join=False the groups run free; call ``join()`` before reading outputs."""
        torch = _torch()
        a = torch.as_tensor(actions, device=self.device).to(torch.float32).contiguous()
        assert a.shape == (self.n, self.model.nu), a.shape
        row = a.stride(0) * a.element_size()
        self._launch(lambda h, lo, hi, st: check(lib().hs_step(h, a.data_ptr() + lo * row, st)), a, join=join)
        return self.t["obs"], self.t["reward"], self.t["terminated"], self.t["truncated"]

    def compile_reward(self, name, registry=None):
        """The native program of the registered program reward ``name`` for this batch's model, resident on
        this batch's GPU (``reward_program.DeviceReward.compile``); None for any other entry."""
        from .reward_program import device_reward_program
        rec = device_reward_program(name, registry)
        if rec is None:
            return None
        with _torch().cuda.device(self.device):
            return rec.compile(self.model)

    def step_program(self, actions, program, params=None):
        """One env step with a program reward (``hs_step_program``): the step without reward and auto-reset,
        the program on the post-step state (reward, total_reward, a finished env's terminal rows), then --
        with auto-reset configured -- the masked reset, all as launches.  ``program``: a
        ``reward_program.CompiledProgram`` (``compile_reward``); ``params``: its parameter overrides.
        One stream group only."""
        torch = _torch()
        if len(self._groups) != 1:
            raise NotImplementedError("step_program: one stream group only")
        a = torch.as_tensor(actions, device=self.device).to(torch.float32).contiguous()
        assert a.shape == (self.n, self.model.nu), a.shape
        if program.outputs and self.__dict__.get("_comp") is None:
            self.bind_reward_components(program.outputs)
        check(lib().hs_step_program(self._h, a.data_ptr(), program.handle, program.params(params), self.stream))
        return self.t["obs"], self.t["reward"], self.t["terminated"], self.t["truncated"]

    # -- named reward components (hs_set_reward_components) -----------------------------------
    def bind_reward_components(self, names):
        """Allocate and bind the component rows of a program reward with the components ``names`` (the
        program's ``outputs``): ``reward_components``, ``total_reward_components`` and
        ``terminal_total_reward_components``, [C, N] tensors of the batch's dtype, component-major (one
        component is one contiguous row: the kernel's store of a component is coalesced), and the sums' [N] int32
        episode tag.  ``step_program`` does this once, at the first step with such a program; from then on a
        program with another number of outputs is refused before the step.  ``names`` empty: unbind."""
        torch = _torch()
        if len(self._groups) != 1:
            raise NotImplementedError("reward components: one stream group only")
        names = tuple(names)
        if not names:
            check(lib().hs_set_reward_components(self._h, 0, None, None, None, None))
            self._comp = None
            return
        c, n = len(names), self.n
        z = lambda *s, dt=self.dtype: torch.zeros(*s, dtype=dt, device=self.device)  # noqa: E731
        comp = dict(names=names, step=z(c, n), total=z(c, n), terminal=z(c, n), episode=z(n, dt=torch.int32))
        torch.cuda.synchronize(self.device)
        check(lib().hs_set_reward_components(self._h, c, comp["step"].data_ptr(), comp["total"].data_ptr(),
                                             comp["episode"].data_ptr(), comp["terminal"].data_ptr()))
        self._comp = comp

    def _comp_view(self, key):
        comp = self.__dict__.get("_comp")
        if comp is None:
            raise AttributeError(f"{key}: no component rows are bound (step_program with a program whose function "
                                 "returns a dict binds them)")
        return comp[key]

    @property
    def reward_component_names(self):
        """The names of the bound component rows, in row order; () when none are bound."""
        comp = self.__dict__.get("_comp")
        return comp["names"] if comp is not None else ()

    @property
    def reward_components(self):
        """[C, N] device tensor: the last ``step_program``'s value of every component (0 for a truncated env)."""
        return self._comp_view("step")

    @property
    def total_reward_components(self):
        """[C, N] device tensor: every component's running sum over the env's current episode, as of the last
        ``step_program`` (for an env that just auto-reset: the finished episode's; read them together with the
        episode tag's meaning in include/hsim.h -- the next step restarts them)."""
        return self._comp_view("total")

    @property
    def terminal_total_reward_components(self):
        """[C, N] device tensor: the episode sums of the envs that finished in the last ``step_program``, beside
        ``terminal_total_reward`` (other envs' columns keep what an earlier end left)."""
        return self._comp_view("terminal")

    # -- termination conditions (hs_set_termination) -----------------------------------------
    def set_termination(self, condition=None, params=None, grace_steps=1, registry=None, fused=False):
        """End episodes on a condition of the state (``hs_set_termination``).  ``condition``: the name of an entry
        of ``reward_program.TERMINATION_FUNCTIONS`` (``"fallen"``, ``"lost_balance"``, or one registered with
        ``register_device_termination``), or None to clear it; ``params``: its parameter overrides (unknown key:
        ValueError); ``grace_steps`` >= 1: the episode ends at the first env step at which the predicate has held
        for that many consecutive env steps of the episode.  From then on ``step`` (with a device reward) and
        ``step_program`` are three launches -- the step without auto-reset, one outcome launch (reward program,
        predicate, grace counter, terminated |= early, ``early_terminated``, the terminal rows), the masked
        reset when auto-reset is configured -- and the fused launches are refused (``step_tape`` falls back to
        one ``step`` per tape row).  With ``reward_id`` -1 (a host reward) ``step`` stays the step alone and the
        caller runs ``apply_termination()`` after writing reward / total_reward.  The grace counter belongs to
        the episode: every reset clears it, ``set_state`` leaves it alone.  One stream group only.

        ``fused=True`` (the built-ins ``"fallen"`` / ``"lost_balance"`` only; anything else: ValueError) sets the
        condition with ``hs_set_termination_builtin``: ``step`` stays the three launches above, and the fused
        launches -- ``step_tape``, ``hs_rollout*``, ``hs_evaluate*`` -- run kernel instances that evaluate the
        built-in themselves, bitwise the per-step results.  An env may end several episodes in such a launch, so
        the terminal rows (``terminal_obs``, ``terminal_step_count``, ``terminal_total_reward``) are then written
        by the launch's last step only: defined for the envs that were done on that step."""
        if condition is None:
            for h, _, _ in self._groups:
                check(lib().hs_set_termination(h, None, None, 1))
            self._termination = None
            self._termination_fused = False
            self.__dict__.pop("_early_view", None)
            return None
        if len(self._groups) != 1:
            raise NotImplementedError("set_termination: one stream group only")
        from .reward_program import (builtin_termination_kind, termination_from_config,
                                     termination_fused_from_config)
        config = {"type": condition, "params": params, "grace_steps": grace_steps, "fused": fused}
        rec, params, grace = termination_from_config(config, registry)
        fused = termination_fused_from_config(config, registry)
        with _torch().cuda.device(self.device):
            prog = rec.compile(self.model)
            if fused:
                vals = dict(zip(rec.param_keys, rec.params(params)))
                check(lib().hs_set_termination_builtin(
                    self._h, prog.handle, prog.params(params), grace, builtin_termination_kind(rec),
                    vals["min_height"], vals.get("max_roll_pitch", 0.0)))
            else:
                check(lib().hs_set_termination(self._h, prog.handle, prog.params(params), grace))
        self._termination = (prog, params, grace)      # the native batch does not own the predicate: keep it alive
        self._termination_fused = fused
        self.__dict__.pop("_early_view", None)
        return prog

    @property
    def termination(self):
        """(compiled predicate, parameter overrides, grace_steps) of the condition set, or None."""
        return self.__dict__.get("_termination")

    @property
    def termination_fused(self):
        """True when the condition set is fused-capable (``set_termination(..., fused=True)``)."""
        return bool(self.__dict__.get("_termination_fused", False))

    def apply_termination(self):
        """The outcome launch alone on the batch's current state, no reset (``hs_apply_termination``): for a
        caller that steps with ``reward_id`` -1 and writes the reward itself.  Once per env step: it advances
        the grace counter."""
        check(lib().hs_apply_termination(self._h, self.stream))
        return self.t["terminated"], self.early_terminated

    @property
    def early_terminated(self):
        """[N] uint8 device view: 1 for the envs whose episode the condition ended in the last outcome launch
        (valid until the next step; the buffer is the native batch's)."""
        v = self.__dict__.get("_early_view")
        if v is None:
            if self.termination is None:
                raise _lib.HsimError("early_terminated: the batch has no termination condition (set_termination)")
            p = C.c_void_p()
            check(lib().hs_termination_state(self._h, None, C.byref(p), None, None))
            v = self._early_view = _torch().as_tensor(_DeviceBytes(p.value, self.n), device=self.device)
        return v

    def grace_counts(self):
        """[N] int32 device tensor (a copy): each env's effective grace count -- the consecutive env steps of
        its current episode at which the condition has held; a stored count that belongs to another episode
        reads as 0 (``hs_termination_state``)."""
        if self.termination is None:
            raise _lib.HsimError("grace_counts: the batch has no termination condition (set_termination)")
        torch = _torch()
        cnt, tag = C.c_void_p(), C.c_void_p()
        check(lib().hs_termination_state(self._h, None, None, C.byref(cnt), C.byref(tag)))
        view = lambda p: torch.as_tensor(_DeviceBytes(p.value, 4 * self.n), device=self.device).view(torch.int32)
        return torch.where(view(tag) == self.episode.to(torch.int32), view(cnt), torch.zeros_like(view(cnt)))

    def step_tape(self, actions, outputs=True):
        """K consecutive ``step`` calls over an action tape [K, N, nu] (float32, on device) in one
        launch (hs_step_tape: a pair's step t + 1 starts once its own step t is committed, so the
        launch does not end every step on its slowest pair).  Bitwise the results of K ``step``
        calls.  outputs=True returns the per-step (obs [K, N, obs_dim], reward [K, N], terminated,
        truncated [K, N] uint8); the batch's own buffers hold the last step either way.  With a termination
        condition set (``set_termination``) without ``fused=True`` the tape is stepped one ``step`` at a time
        instead: the same results, slower; with ``fused=True`` it is hs_step_tape as ever.  Open loop:
        benchmarks, trajectory evaluation -- a policy in the loop steps with ``step`` (or, for the PPO pi
        net, inside the launch: hs_rollout, PPO._rollout_fused).  Synchronous;
        one stream group only."""
        torch = _torch()
        if len(self._groups) != 1:
            raise NotImplementedError("step_tape: one stream group only")
        a = torch.as_tensor(actions, device=self.device).to(torch.float32).contiguous()
        if a.dim() != 3 or a.shape[1:] != (self.n, self.model.nu):
            raise ValueError(f"step_tape: actions must be [K, {self.n}, {self.model.nu}], got {tuple(a.shape)}")
        K = a.shape[0]
        res, out = None, None
        if outputs:
            res = (torch.empty(K, self.n, self.obs_dim, dtype=self.dtype, device=self.device),
                   torch.empty(K, self.n, dtype=self.dtype, device=self.device),
                   torch.empty(K, self.n, dtype=torch.uint8, device=self.device),
                   torch.empty(K, self.n, dtype=torch.uint8, device=self.device))
            out = _lib.hs_tape_out(*[x.data_ptr() for x in res])
        if self.termination is not None and not self.termination_fused:
            # a termination condition that is not fused-capable: hs_step_tape refuses (a fused launch is bounded by the shortest possible
            # episode), so the tape is stepped one ``step`` at a time -- the same results, slower
            for k in range(K):
                step = self.step(a[k])
                if outputs:
                    for dst, src in zip(res, step):
                        dst[k].copy_(src)
            return res if outputs else step
        h = self._groups[0][0]
        check(lib().hs_step_tape(h, a.data_ptr(), K, C.byref(out) if out is not None else None, self.stream))
        if outputs:
            return res
        return self.t["obs"], self.t["reward"], self.t["terminated"], self.t["truncated"]

    # -- host copies of a step's outputs (the Gym / SB3 numpy surfaces) ----------------------
    _HOST_COLS = ("reward", "terminated", "truncated", "total_reward", "step_count", "terminal_step_count",
                  "terminal_total_reward")

    def host_outputs(self, ncols=3, warnings=False, components=False):
        """One step's outputs on the host in ONE device-to-host copy: the obs and the first ``ncols``
        of (reward, terminated, truncated, total_reward, step_count, terminal_step_count,
        terminal_total_reward), packed on the device into one float64 buffer, copied into pinned
        host memory and synchronized once.  Returns (obs [N, obs_dim] float64, cols [ncols, N]
        float64), views of a fresh pinned block (torch's caching host allocator recycles it once
        both are dropped).  ``warnings=True`` also packs the warning counters summed over the envs
        (HS_NWARN values, cumulative since the batch was created) and returns them third, as int64.
        One native pack launch (hs_pack_outputs) for a single-group batch.  ``components=True`` appends one more
        result: with component rows bound, a [2, C, N] float64 block -- ``reward_components`` and
        ``terminal_total_reward_components`` -- that joins the same copy (two device copies behind the pack);
        with none bound, None, and nothing more is copied."""
        torch = _torch()
        N, D = self.n, self.obs_dim
        nwr = N * _lib.HS_NWARN if warnings else 0          # per-env warning rows (summed on the host)
        comp = self.__dict__.get("_comp") if components else None
        ncomp = 2 * len(comp["names"]) * N if comp is not None else 0
        size = N * D + ncols * N + nwr + ncomp
        dev = self.__dict__.get("_pack_dev")
        if dev is None or dev.numel() != size:
            dev = self._pack_dev = torch.empty(size, dtype=torch.float64, device=self.device)
        st = torch.cuda.current_stream(self.device)
        if len(self._groups) == 1:   # one pack launch (hs_pack_outputs)
            check(lib().hs_pack_outputs(self._h, dev.data_ptr(), int(ncols), 1 if warnings else 0, st.cuda_stream))
        else:
            dev[:N * D].view(N, D).copy_(self.t["obs"])
            cols = dev[N * D:N * D + ncols * N].view(ncols, N)
            for k in range(ncols):
                cols[k].copy_(self.t[self._HOST_COLS[k]])
            if nwr:
                dev[N * D + ncols * N:size - ncomp].view(_lib.HS_NWARN, N).copy_(self.t["warning"].t())
        if ncomp:     # the component rows ride in the same copy, behind everything else
            tail = dev[size - ncomp:].view(2, len(comp["names"]), N)
            tail[0].copy_(comp["step"])
            tail[1].copy_(comp["terminal"])
        host = torch.empty(size, dtype=torch.float64, pin_memory=True)
        host.copy_(dev, non_blocking=True)
        st.synchronize()
        a = host.numpy()
        obs, c = a[:N * D].reshape(N, D), a[N * D:N * D + ncols * N].reshape(ncols, N)
        res = (obs, c)
        if nwr:
            res += (a[N * D + ncols * N:size - ncomp].reshape(_lib.HS_NWARN, N).sum(1).astype(np.int64),)
        if components:
            res += (a[size - ncomp:].reshape(2, -1, N) if ncomp else None,)
        return res

    def tape_aborts(self):
        """Tape launches replayed step by step because an env overflowed the resident tier."""
        v = C.c_uint64(0)
        check(lib().hs_tape_aborts(self._groups[0][0], C.byref(v)))
        return int(v.value)

    def compute_reward(self, name, params=None, registry=None, components=False):
        """``REWARD_FUNCTIONS[name](data_i, params)`` for every env's current state on the device
        (``hs_reward``: the step kernel's reward code on the batch's own buffers; custom_env.py:263-271
        ``_compute_reward``; ``self.reward`` stays the last step's reward buffer).
        Needs the aux row and the data.ctrl copy (``configure(aux=True, ctrl=True)``, the default).
        Returns an [N] tensor of the batch precision.  ``components=True`` (a reward program only): (reward [N],
        components [C, N]), the rows in the order of the program's ``outputs`` ([0, N] for a scalar function)."""
        from .reward_functions import device_reward_id
        torch = _torch()
        rid = device_reward_id(name, registry)
        if rid is None:
            prog = self.compile_reward(name, registry)
            if prog is None:
                raise _lib.HsimError(f"reward {name!r} is a host callable: no device formula")
            if len(self._groups) != 1:
                raise NotImplementedError("compute_reward with a reward program: one stream group only")
            out = torch.empty(self.n, dtype=self.dtype, device=self.device)
            if not components:
                check(lib().hs_reward_program_batch(self._h, prog.handle, prog.params(params), out.data_ptr(),
                                                    self.stream))
                return out
            comp = torch.empty(len(prog.outputs), self.n, dtype=self.dtype, device=self.device)
            check(lib().hs_reward_program_batch_components(self._h, prog.handle, prog.params(params), out.data_ptr(),
                                                           comp.data_ptr() if comp.numel() else None, self.stream))
            return out, comp
        if components:
            raise _lib.HsimError(f"reward {name!r} is a built-in id: only a reward program has named components")
        kn = None
        if params is not None:
            p = {**dict(zip(KNEEL_KEYS, KNEEL_DEFAULTS)), **params}
            kn = (C.c_double * 9)(*[float(p[k]) for k in KNEEL_KEYS])
        out = torch.empty(self.n, dtype=self.dtype, device=self.device)

        def go(h, lo, hi, st):
            check(lib().hs_reward(h, rid, C.cast(kn, C.c_void_p) if kn is not None else None,
                                  out.data_ptr() + lo * out.element_size(), st))
        self._launch(go, out)
        return out

    def last_tape_ms(self):
        """Duration (ms, HIP events on its stream) of the last tape / fused-rollout kernel launch."""
        v = C.c_double(0)
        check(lib().hs_last_tape_ms(self._groups[0][0], C.byref(v)))
        return float(v.value)

    def stream_orders(self):
        """Cross-stream waits the library inserted because calls of this batch came on different
        streams (include/hsim.h: one batch's launches are always ordered)."""
        tot = 0
        for h, _, _ in self._groups:
            v = C.c_uint64(0)
            check(lib().hs_stream_orders(h, C.byref(v)))
            tot += int(v.value)
        return tot

    def physics_step(self, ctrl=None, nsub=1):
        """nsub raw mj_step's with the given ctrl [N, nu] (None keeps the current ctrl)."""
        torch = _torch()
        c = None
        if ctrl is not None:
            c = torch.as_tensor(ctrl, device=self.device).to(torch.float32).contiguous()
            assert c.shape == (self.n, self.model.nu), c.shape
            self._keep = c

        def go(h, lo, hi, st):
            p = None if c is None else c.data_ptr() + lo * c.stride(0) * c.element_size()
            check(lib().hs_physics_step(h, p, int(nsub), st))
        self._launch(go, c)

    # -- host state access (through the C ABI, synchronous, fp64) ---------------------------
    def get_state(self):
        """qpos / qvel / qacc_warmstart / time (and ctrl, while the data.ctrl copy is written:
        ``configure(ctrl=True)``, the default) as fp64 host arrays."""
        N, m = self.n, self.model
        out = dict(qpos=np.zeros((N, m.nq)), qvel=np.zeros((N, m.nv)), qacc_warmstart=np.zeros((N, m.nv)),
                   time=np.zeros(N), ctrl=np.zeros((N, m.nu)))
        keys = ("qpos", "qvel", "qacc_warmstart", "time", "ctrl")
        if not self.cfg.outputs & _lib.HS_OUT_CTRL:
            del out["ctrl"]
        for h, lo, hi in self._groups:
            check(lib().hs_state_io(h, 0, *[out[k][lo:hi].ctypes.data if k in out else None for k in keys]))
        return out

    def set_state(self, qpos=None, qvel=None, qacc_warmstart=None, time=None, ctrl=None):
        """Overwrite the given state fields from fp64 host arrays (broadcast to every env).  The episode number
        is not part of the state, so a termination condition's grace counter is left alone."""
        def p(x, shape):
            if x is None:
                return None, None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), shape))
            return a, a.ctypes.data
        N, m = self.n, self.model
        keep = [p(qpos, (N, m.nq)), p(qvel, (N, m.nv)), p(qacc_warmstart, (N, m.nv)), p(time, (N,)), p(ctrl, (N, m.nu))]
        for h, lo, hi in self._groups:
            check(lib().hs_state_io(h, 1, *[None if a is None else a[lo:hi].ctypes.data for a, _ in keep]))

    def kinematics(self, env=0, qpos=None):
        """mj_kinematics + mj_comPos of one env on the GPU (hs_kinematics): body xpos / xmat,
        geom_xpos / geom_zaxis and the root subtree COM, fp64 on the host.  ``qpos`` poses that
        configuration instead of the env's current one.  Visualisation only (one sync launch)."""
        env = int(env)
        for h, lo, hi in self._groups:
            if lo <= env < hi:
                break
        else:
            raise IndexError(f"env {env} out of range [0, {self.n})")
        m = self.model
        out = {"xpos": np.zeros((m.nbody, 3)), "xmat": np.zeros((m.nbody, 9)), "geom_xpos": np.zeros((m.ngeom, 3)),
               "geom_zaxis": np.zeros((m.ngeom, 3)), "com": np.zeros(3)}
        q = None if qpos is None else np.ascontiguousarray(qpos, np.float64)
        if q is not None and q.shape != (m.nq,):
            raise ValueError(f"qpos must have shape ({m.nq},)")
        check(lib().hs_kinematics(h, env - lo, None if q is None else q.ctypes.data,
                                  *[out[k].ctypes.data for k in ("xpos", "xmat", "geom_xpos", "geom_zaxis", "com")]))
        return out

    def kinematics_batch(self, envs=None, qpos=None):
        """``kinematics`` for n poses in one launch, device to device (hs_kinematics_batch): a
        ``[n, HS_KINDIM]`` tensor of the batch's dtype, record i = [xpos 20*3][xmat 20*9][geom_xpos 24*3]
        [geom z-axis 24*3][com 3] of pose i (rows past nbody / ngeom are zero).  The poses are the current
        states of the envs ``envs`` (a sequence of ids) or the rows of ``qpos`` [n, nq]; exactly one of
        the two.  The env states are only read.  What ``render.DeviceRenderer`` draws."""
        torch = _torch()
        if (envs is None) == (qpos is None):
            raise ValueError("kinematics_batch: exactly one of envs / qpos")
        if envs is not None:
            ids = np.ascontiguousarray(np.asarray(envs, dtype=np.int64).reshape(-1))
            if ids.size and (ids.min() < 0 or ids.max() >= self.n):
                bad = ids[(ids < 0) | (ids >= self.n)][0]
                raise IndexError(f"env {int(bad)} out of range [0, {self.n})")
            n = ids.size
        else:
            q = torch.as_tensor(qpos, device=self.device).to(self.dtype)
            if q.dim() == 1:
                q = q[None]
            if q.dim() != 2 or q.shape[1] != self.model.nq:
                raise ValueError(f"qpos must have shape (n, {self.model.nq})")
            q = q.contiguous()
            n = q.shape[0]
        if n < 1:
            raise ValueError("kinematics_batch: no poses")
        out = torch.zeros(n, _lib.HS_KINDIM, dtype=self.dtype, device=self.device)
        row = out.stride(0) * out.element_size()
        if envs is None:
            check(lib().hs_kinematics_batch(self._h, n, None, q.data_ptr(), out.data_ptr(), self.stream))
            return out
        if len(self._groups) == 1:
            loc = ids.astype(np.int32)
            check(lib().hs_kinematics_batch(self._h, n, loc.ctypes.data, None, out.data_ptr(), self.stream))
            return out
        # stream groups: each group poses its own envs (group-local ids) into a scratch block on its
        # stream; the rows go to their places once the groups have joined
        order = np.argsort(ids, kind="stable")
        tmp = torch.zeros_like(out)
        spans = {}
        for g, (h, lo, hi) in enumerate(self._groups):
            a, b_ = np.searchsorted(ids[order], [lo, hi])
            if b_ > a:
                spans[h] = (int(a), int(b_), np.ascontiguousarray(ids[order][a:b_] - lo, dtype=np.int32))

        def go(h, lo, hi, st):
            if h in spans:
                a, b_, loc = spans[h]
                check(lib().hs_kinematics_batch(h, b_ - a, loc.ctypes.data, None, tmp.data_ptr() + a * row, st))
        self._launch(go, tmp)
        out[torch.as_tensor(order, device=self.device)] = tmp
        return out

    def set_debug(self, on=True):
        check(lib().hs_set_debug(self._h, int(bool(on))))

    def debug_lose_handoff(self, env):
        """Test hook (hs_debug_lose_handoff): the chunk-queue hand-off of ``env``'s pair is treated
        as lost in the following queued launches (the pair is reset as mj_checkPos resets a bad state
        and counted in the HS_WARN_HANDOFF column of ``warning``);
        ``env=None`` turns it off."""
        for h, lo, hi in self._groups:
            inside = env is not None and lo <= int(env) < hi
            check(lib().hs_debug_lose_handoff(h, int(env) - lo if inside else -1))

    def queue_order(self):
        """Tests only (hs_debug_queue_order): the env pairs in the order the next chunk-queue launch
        of the first group will claim them -- pairs with an env about to auto-reset first, then by
        the last launch's measured cost; empty while that launch would use the fixed permutation.
        Synchronous."""
        out = np.zeros(self._groups[0][2] - self._groups[0][1], dtype=np.int32)
        cnt = lib().hs_debug_queue_order(self._h, out.ctypes.data, len(out))
        if cnt < 0:
            raise _lib.HsimError(lib().hs_last_error().decode())
        return out[:cnt].copy()

    def queue_counters(self):
        """Tests only (hs_debug_queue_counters): the first group's chunk-queue sync words as
        {"head", "exit", "epoch", "abort"}; head and exit are 0 between launches.  Synchronous."""
        out = np.zeros(4, dtype=np.int32)
        check(lib().hs_debug_queue_counters(self._h, out.ctypes.data))
        return dict(zip(("head", "exit", "epoch", "abort"), out.tolist()))

    def get_debug(self):
        out = np.zeros(_lib.DBGDIM)
        check(lib().hs_get_debug(self._h, out.ctypes.data, _lib.DBGDIM))
        return out

    def wide_reruns(self):
        """Env steps re-run by the wide contact tier so far (resident tier overflowed; see
        hs_model.h).  Synchronous."""
        tot = 0
        for h, _, _ in self._groups:
            v = C.c_uint64(0)
            check(lib().hs_batch_counters(h, C.byref(v)))
            tot += int(v.value)
        return tot

    def synchronize(self):
        for h, _, _ in self._groups:
            check(lib().hs_synchronize(h))

    def close(self):
        for h, _, _ in self.__dict__.get("_groups", []):
            if h:
                lib().hs_batch_destroy(h)
        self._groups = []
        self._h = None
        self.__dict__.pop("_early_view", None)       # a view of the native batch's buffer, gone with it

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
