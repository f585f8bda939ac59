"""Reference motions: the recording a reward or a termination condition compares the state against.

``env_config["initial_state"]`` starts episodes from the rows of a recording; a *reference motion* bound to the
batch (``HsBatch.set_reference_motion``, ``env_config["reference_motion"]``) lets reward and termination programs
(``reward_program``) see the recording: ``d.ref_qpos`` [nq] and ``d.ref_qvel`` [nv] are the recording's rows,
linearly interpolated at the env's own phase.  The registered reward ``"track"`` and the termination condition
``"off_track"`` are written over them.

A reference is ``K >= 1`` rows ``qpos [K, nq]`` / ``qvel [K, nv]``, ``key_dt`` seconds apart, an end mode
(``"hold"`` the last row, or ``"loop"``) and a start mode (``"zero"``: every episode starts at row 0;
``"drawn"``: at the row its initial state drew, which needs a bank of initial states of the same ``K`` bound).
The sample is a pure function of ``(seed, env, episode[env], time[env])`` and the rows -- nothing is carried
between steps -- with ONE definition, stated in csrc/hs_reward_prog.h (``rp_ref_start``, ``rp_ref_phase``,
``rp_ref_value``: the kernel and the host interpreter share them) and restated here in numpy (``phase``,
``sample``), bit for bit::

    j0 = 0                                           start "zero", or episode 0 (never reset)
       = initial_state.draw_index(seed, env, ep, K)  start "drawn"
    x  = float64(j0) + float64(t) / key_dt           always float64; NaN or negative: 0
    hold:  x = min(x, K - 1);  i = floor(x);  i1 = min(i + 1, K - 1)
    loop:  x = min(x, 2**52);  i = floor(x) mod K;  i1 = (i + 1) mod K
    w  = T(x - floor(x));   ref[k] = a + w * (b - a),   a = row_i[k], b = row_i1[k]

each operation rounded in the batch dtype ``T``.  ``K == 1`` is the row itself and ignores ``key_dt``.  The free
joint's quaternion of every row is normalised when the reference is built or bound; the INTERPOLATED quaternion
is not renormalised (between two unit quaternions its norm dips below 1): a program divides by the norm where it
matters, as ``"track"`` does.

``key_dt`` is explicit and required with more than one row: the ``time`` attributes of recorded ``<key>``
elements are not trusted (the reference project's writer stamps env-step indices times the substep length).
"""
from __future__ import annotations

import numpy as np

from . import initial_state as _is

END_MODES = ("hold", "loop")
START_MODES = ("zero", "drawn")
HS_REF_HOLD, HS_REF_LOOP, HS_REF_START_ZERO, HS_REF_START_DRAWN = 0, 1, 0, 2     # include/hsim.h
MAX_ROWS = 4096                                                                   # HS_MAX_REFERENCE_ROWS
ROW_KEYS = ("keyframe", "keyframes", "trajectory", "stride", "states")           # initial_state.build_bank's sources
SPEC_KEYS = ROW_KEYS + ("key_dt", "end", "start", "from_initial_state")
_TWO52 = 4503599627370496.0


class Reference:
    """A reference motion on the host: ``qpos`` [K, nq] / ``qvel`` [K, nv] float64 (quaternions normalised),
    ``key_dt`` (None with one row), ``end`` and ``start``.  ``qvel`` None: zeros, ``nv`` columns (default nq - 1,
    a model with one free joint and otherwise scalar joints).  Checked on construction (ValueError)."""

    def __init__(self, qpos, qvel=None, key_dt=None, end="hold", start="zero", nv=None):
        q = np.array(qpos, dtype=np.float64, copy=True)
        q = q[None] if q.ndim == 1 else q
        if q.ndim != 2 or q.shape[0] < 1:
            raise ValueError(f"reference_motion: qpos must be [K, nq] with K >= 1, got shape {q.shape}")
        if q.shape[0] > MAX_ROWS:
            raise ValueError(f"reference_motion: {q.shape[0]} rows, the limit is {MAX_ROWS}")
        if qvel is None:
            v = np.zeros((q.shape[0], q.shape[1] - 1 if nv is None else int(nv)))
        else:
            v = np.array(qvel, dtype=np.float64, copy=True)
            v = v[None] if v.ndim == 1 else v
            if v.ndim != 2 or v.shape[0] != q.shape[0] or (nv is not None and v.shape[1] != int(nv)):
                raise ValueError(f"reference_motion: {q.shape[0]} qpos rows but qvel of shape {v.shape}")
        if not np.isfinite(q).all() or not np.isfinite(v).all():
            raise ValueError("reference_motion: the rows hold a value that is not finite")
        if end not in END_MODES:
            raise ValueError(f"reference_motion: end must be one of {', '.join(map(repr, END_MODES))}, got {end!r}")
        if start not in START_MODES:
            raise ValueError(f"reference_motion: start must be one of {', '.join(map(repr, START_MODES))}, "
                             f"got {start!r}")
        if q.shape[0] > 1:
            if key_dt is None:
                raise ValueError("reference_motion: key_dt (the seconds between consecutive rows) is required with "
                                 "more than one row")
            key_dt = float(key_dt)
            if not (np.isfinite(key_dt) and key_dt > 0):
                raise ValueError(f"reference_motion: key_dt must be finite and > 0, got {key_dt}")
        else:
            key_dt = None if key_dt is None else float(key_dt)
        self.qpos = _is.normalize_quaternions(q) if q.shape[1] >= 7 else q
        self.qvel = v
        self.key_dt, self.end, self.start = key_dt, end, start

    @property
    def K(self):
        return self.qpos.shape[0]

    @property
    def flags(self):
        """The HS_REF_* flags of include/hsim.h."""
        return (HS_REF_LOOP if self.end == "loop" else HS_REF_HOLD) | \
               (HS_REF_START_DRAWN if self.start == "drawn" else HS_REF_START_ZERO)

    def __repr__(self):
        return f"Reference(K={self.K}, key_dt={self.key_dt}, end={self.end!r}, start={self.start!r})"


def build_reference(model, spec, initial_state=None):
    """The ``Reference`` that ``spec`` describes: ``initial_state.build_bank``'s row sources (``keyframe``,
    ``keyframes``, ``trajectory`` + ``stride``, ``states``) plus ``key_dt``, ``end`` (``"hold"`` | ``"loop"``) and
    ``start`` (``"zero"`` | ``"drawn"``).  ``{"from_initial_state": True, "key_dt": ...}`` takes the rows of
    ``initial_state`` (the env config's ``initial_state`` spec) instead and ``start="drawn"``: the reference an
    episode is compared against is the recording it started from.  CPU only.  ValueError: an unknown key (the
    message lists the valid ones), what ``build_bank`` refuses, a missing or non-positive ``key_dt`` with more than
    one row, an unknown mode."""
    if not isinstance(spec, dict):
        raise ValueError(f"reference_motion: a dict with some of {', '.join(SPEC_KEYS)}; got {type(spec).__name__}")
    unknown = sorted(set(spec) - set(SPEC_KEYS))
    if unknown:
        raise ValueError(f"reference_motion: unknown key(s) {', '.join(map(repr, unknown))}; "
                         f"valid: {', '.join(SPEC_KEYS)}")
    rows = {k: spec[k] for k in ROW_KEYS if k in spec}
    start = spec.get("start")
    if spec.get("from_initial_state"):
        if rows:
            raise ValueError("reference_motion: 'from_initial_state' takes the rows of the initial_state spec; "
                             f"it does not go with {', '.join(map(repr, rows))}")
        if initial_state is None:
            raise ValueError("reference_motion: 'from_initial_state' needs an initial_state spec in the env config")
        if start not in (None, "drawn"):
            raise ValueError("reference_motion: 'from_initial_state' means start='drawn'")
        rows = {k: initial_state[k] for k in ROW_KEYS if k in initial_state}
        start = "drawn"
    try:
        qpos, qvel = _is.build_bank(model, rows)
    except ValueError as e:
        raise ValueError(str(e).replace("initial_state:", "reference_motion:")) from None
    return Reference(qpos, qvel, spec.get("key_dt"), spec.get("end", "hold"), start or "zero")


def reference_from_config(model, cfg):
    """``env_config["reference_motion"]`` checked against the rest of the config, on the CPU, before any batch or
    native program exists: the ``Reference`` (None when the key is absent or None).  ValueError: what
    ``build_reference`` refuses; a reward or termination condition of the config that reads ``ref_qpos`` /
    ``ref_qvel`` with no reference configured; ``start="drawn"`` without an ``initial_state`` bank of the same K."""
    from . import reward_program as rw
    spec, init = cfg.get("reference_motion"), cfg.get("initial_state")
    ref = None if spec is None else build_reference(model, spec, init)
    dims = (model.nq, model.nv, model.nu, model.nbody)
    readers = []
    rc = cfg.get("reward_config") or {}
    rtype = rc.get("type", "default")
    if not rc.get("components"):
        try:
            rec = rw.device_reward_program(rtype)
        except ValueError:
            rec = None          # an unknown type is the env's own error to raise
        if rec is not None:
            readers.append(("reward", rtype, rec))
    term = cfg.get("termination")
    if isinstance(term, dict) and term.get("type") in rw.TERMINATION_FUNCTIONS:
        readers.append(("termination", term["type"], rw.device_termination(term["type"])))
    for kind, name, rec in readers:
        read = sorted(set(rec.trace(dims).fields) & set(rw.REFERENCE_FIELDS))
        if read and ref is None:
            raise ValueError(f"{kind} {name!r} reads {', '.join(read)}, but the env config has no 'reference_motion' "
                             "(e.g. {\"trajectory\": path, \"key_dt\": 0.05} or {\"from_initial_state\": True, "
                             "\"key_dt\": ...})")
    if ref is not None and ref.start == "drawn":
        k = None if init is None else len(_is.build_bank(model, {k: v for k, v in init.items() if k in ROW_KEYS})[0])
        if k != ref.K:
            raise ValueError(f"reference_motion: start='drawn' needs an 'initial_state' bank of the same {ref.K} rows "
                             f"(the episode starts from the row it is compared against); "
                             + ("the config has none" if k is None else f"the bank has {k}"))
    return ref


def start_rows(ref, n, episode=None, seed=0, env=None):
    """[n] int64: each state's start row j0 -- zeros, or for ``start="drawn"`` the initial-state draw's own row
    (``initial_state.draw_index``; 0 for episode 0, which no reset began).  ``seed``: one integer, or [n] per-state
    seeds (a batch with stream groups draws with one seed per group); ``env`` [n]: each state's env index within
    its group (default 0 .. n-1)."""
    j0 = np.zeros(n, dtype=np.int64)
    if ref.start != "drawn":
        return j0
    if episode is None:
        raise ValueError("reference_motion: start='drawn' needs the episode numbers")
    ep = np.broadcast_to(np.asarray(episode, dtype=np.int64), (n,))
    env = np.arange(n, dtype=np.int64) if env is None else np.broadcast_to(np.asarray(env, dtype=np.int64), (n,))
    seeds = np.broadcast_to(np.asarray(seed, dtype=object), (n,))
    for s in set(int(x) for x in seeds):
        m = np.array([int(x) == s for x in seeds])
        j0[m] = _is.draw_index(s, env[m], ep[m], ref.K)
    j0[ep == 0] = 0
    return j0


def phase(ref, time, episode=None, seed=0, env=None):
    """The phase of n states, float64 whatever the batch dtype: (x [n], i [n], i1 [n], frac [n]) with ``x`` the
    phase after its clamps (the value whose floor indexes), ``i`` / ``i1`` the two rows, both in [0, K - 1] for
    every input, and ``frac = x - floor(x)``."""
    t = np.atleast_1d(np.asarray(time)).astype(np.float64)
    n, K = len(t), ref.K
    if K == 1:
        z = np.zeros(n, dtype=np.int64)
        return np.zeros(n), z, z.copy(), np.zeros(n)
    j0 = start_rows(ref, n, episode, seed, env)
    with np.errstate(all="ignore"):
        x = j0.astype(np.float64) + t / np.float64(ref.key_dt)
        x = np.where(x >= 0.0, x, 0.0)
        if ref.end == "loop":
            x = np.where(x < _TWO52, x, _TWO52)
            f = np.floor(x)
            i = f.astype(np.int64) % K
            i1 = (i + 1) % K
        else:
            x = np.where(x < float(K - 1), x, float(K - 1))
            f = np.floor(x)
            i = f.astype(np.int64)
            i1 = np.minimum(i + 1, K - 1)
        return x, i, i1, x - f


def sample(ref, time, episode=None, seed=0, env=None, dtype=np.float64):
    """(ref_qpos [n, nq], ref_qvel [n, nv]) in ``dtype``: what ``d.ref_qpos`` / ``d.ref_qvel`` are for n states with
    the times ``time`` [n] (the batch's ``time`` values), episode numbers ``episode`` and seed(s) ``seed`` -- the
    numpy restatement of the device's sample, bitwise its result in the batch dtype."""
    T = np.dtype(dtype).type
    _, i, i1, frac = phase(ref, time, episode, seed, env)
    w = frac.astype(T)[:, None]

    def lerp(rows):
        rows = rows.astype(T)
        a, b = rows[i], rows[i1]
        d = b - a
        s = w * d
        return a + s
    with np.errstate(all="ignore"):
        return lerp(ref.qpos), lerp(ref.qvel)
