"""Where an episode begins: banks of initial states, and the numpy restatement of the device's draw.

The reference's reset (custom_env.py:97-130) always starts from ``qpos0`` at z = 1.282, upright.  With a bank of
states bound to a batch (``HsBatch.set_initial_states``, ``env_config["initial_state"]``) every reset -- the
explicit one and every auto-reset inside a step, tape, fused rollout or fused evaluation -- starts from one row
of the bank instead, drawn per episode inside the step kernel's reset pass (csrc/hs_env_step.h ``reset_draw``),
plus the usual reset noise.  ``build_bank`` makes the bank on the CPU from a spec:

* ``{"keyframe": "squat"}``: one keyframe of the model (``assets/humanoid.xml`` ships ``squat``,
  ``stand_on_left_leg``, ``prone``, ``supine``);
* ``{"keyframes": ["squat", "prone", "default"]}``: several, qvel zeros; ``"default"`` is the reference's own
  start pose (``qpos0``, z = 1.282, upright quaternion);
* ``{"trajectory": path}``: every ``<key>`` of an MJCF keyframe file that carries qpos and qvel -- what
  ``trajectories.write_trajectory_xml`` writes (the model's own keyframes in such a file have no qvel and are
  not part of the recording); ``"stride": s`` keeps every s-th of them;
* ``{"states": (qpos, qvel)}``: arrays [K, nq] / [K, nv] (qvel may be None: zeros).

Several keys may be combined; their rows are concatenated in the order keyframe, keyframes, trajectory, states.
The draw is uniform over the rows: repeat a row to weight it.  ``"noise_scale"`` is not a row source: the env
surfaces map it onto the reset noise's scale (``HsBatch.configure(noise_scale=...)``).

``draw_index`` / ``uniform_pm`` restate the device's counter hash in uint64 numpy arithmetic, so a host program
can tell which row an episode started from (``HsBatch.initial_state_index``) and what noise it got.
"""
from __future__ import annotations

import xml.etree.ElementTree as ET

import numpy as np

DEFAULT_HEIGHT = 1.282      # custom_env.py:59 init_height
INIT_SLOT = 128             # the draw's slot of the counter hash (qpos noise: 0..nq-1, qvel noise: 64..64+nv-1)
QVEL_SLOT0 = 64
MODEL_KEYFRAMES = ("squat", "stand_on_left_leg", "prone", "supine")
SPEC_KEYS = ("keyframe", "keyframes", "trajectory", "stride", "states", "noise_scale")


# ------------------------------------------------------------------ the device's counter hash, restated
def _splitmix(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hash_bits(seed, env, episode, slot):
    """The 53 random bits of the counter hash at (seed, env, episode, slot), as uint64 (broadcast over the
    arguments): ``splitmix(seed ^ splitmix(env << 32 ^ episode << 8 ^ slot)) >> 11``.  ``episode`` is the number
    of the episode the reset begins (the batch's ``episode`` counter after that reset)."""
    seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    env = np.asarray(env, dtype=np.int64).astype(np.uint64)
    episode = (np.asarray(episode, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint64)
    slot = np.asarray(slot, dtype=np.int64).astype(np.uint64)
    h = _splitmix(seed ^ _splitmix((env << np.uint64(32)) ^ (episode << np.uint64(8)) ^ slot))
    return h >> np.uint64(11)


def uniform01(seed, env, episode, slot):
    """The hash's value in [0, 1): 53 bits times 2^-53 (exact in float64)."""
    return hash_bits(seed, env, episode, slot).astype(np.float64) * (1.0 / 9007199254740992.0)


def uniform_pm(seed, env, episode, slot, scale, fused=True):
    """The device's ``uniform_pm``: the U(-scale, scale) reset-noise value at (seed, env, episode, slot), float64.
    ``scale`` is the batch precision's noise scale as a float64 (``float(np.float32(0.01))`` for an fp32 batch);
    an fp32 batch rounds the result to float32.  The device evaluates ``-scale + (2 scale) u`` as one fused
    multiply-add (``fused=True``): with u = m 2^-53 that is scale (m - 2^52) 2^-52 rounded once, which numpy
    states exactly because m - 2^52 is an integer a float64 holds.  ``fused=False`` rounds the product first."""
    scale = np.float64(scale)
    if not fused:
        return -scale + 2.0 * scale * uniform01(seed, env, episode, slot)
    d = hash_bits(seed, env, episode, slot).astype(np.int64) - np.int64(1 << 52)
    return scale * d.astype(np.float64) * 2.0 ** -52


def draw_index(seed, env, episode, K):
    """The bank row the device draws for (seed, env, episode): ``min(K - 1, floor(u K))`` with u the hash's
    [0, 1) value at slot 128.  Vectorised over ``env`` / ``episode``; int64."""
    K = int(K)
    if K < 1:
        raise ValueError("draw_index: K must be >= 1")
    u = uniform01(seed, env, episode, INIT_SLOT)
    return np.minimum(K - 1, np.floor(u * float(K)).astype(np.int64))


# ------------------------------------------------------------------ banks
def normalize_quaternions(qpos):
    """``qpos`` [K, nq] with every row's free-joint quaternion divided by its norm, the expression the native
    library applies to the rows it is given (``q / sqrt(w w + x x + y y + z z)``, summed left to right).  A zero
    quaternion raises ValueError."""
    q = np.array(qpos, dtype=np.float64, copy=True)
    w, x, y, z = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
    norm = np.sqrt(((w * w + x * x) + y * y) + z * z)
    if not np.all(norm >= 1e-15):
        raise ValueError(f"initial state row {int(np.flatnonzero(~(norm >= 1e-15))[0])} has a zero quaternion")
    q[:, 3:7] /= norm[:, None]
    return q


def default_pose(model):
    """The reference's own start pose: qpos0 at z = 1.282 with the upright quaternion (custom_env.py:104-107)."""
    q = np.array(model.qpos0, dtype=np.float64)
    q[2] = DEFAULT_HEIGHT
    q[3:7] = (1.0, 0.0, 0.0, 0.0)
    return q


def _keyframe_row(model, name):
    if name == "default":
        return default_pose(model)
    if not isinstance(name, str):
        raise ValueError(f"keyframe names are strings, got {name!r}")
    try:
        q = np.asarray(model.keyframe(name), dtype=np.float64)
    except Exception:
        q = np.zeros(0)
    if q.size == 0:
        valid = [k for k in MODEL_KEYFRAMES if _has_keyframe(model, k)] + ["default"]
        raise ValueError(f"unknown keyframe {name!r}; valid names: {', '.join(valid)}")
    return q


def _has_keyframe(model, name):
    try:
        return np.asarray(model.keyframe(name)).size > 0
    except Exception:
        return False


def load_trajectory(path, stride=1):
    """(qpos [K, nq'], qvel [K, nv']) of every ``<key>`` of the MJCF file ``path`` that carries both attributes,
    in file order, every ``stride``-th of them."""
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be >= 1")
    keys = [k for k in ET.parse(path).getroot().iter("key") if k.get("qpos") is not None and k.get("qvel") is not None]
    if not keys:
        raise ValueError(f"{path}: no <key> with qpos and qvel")
    keys = keys[::stride]
    try:
        qpos = [np.array(k.get("qpos").split(), dtype=np.float64) for k in keys]
        qvel = [np.array(k.get("qvel").split(), dtype=np.float64) for k in keys]
    except ValueError as e:
        raise ValueError(f"{path}: a <key> holds a value that is no number ({e})") from None
    if len({len(q) for q in qpos}) != 1 or len({len(v) for v in qvel}) != 1:
        raise ValueError(f"{path}: the <key> elements differ in length")
    return np.stack(qpos), np.stack(qvel)


def _check_rows(what, a, n, name):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or a.shape[1] != n:
        raise ValueError(f"{what}: {name} rows must have length {n}, got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: {name} holds a value that is not finite")
    return a


def build_bank(model, spec):
    """(qpos [K, nq], qvel [K, nv]) float64 of the bank ``spec`` describes (module docstring), the free joint's
    quaternions normalised.  CPU only.  ValueError: an unknown spec key or keyframe name (the message lists the
    valid ones), rows of the wrong length, values that are not finite, a zero quaternion, an empty bank."""
    if not isinstance(spec, dict):
        raise ValueError(f"initial_state: a dict with some of {', '.join(SPEC_KEYS[:5])}; got {type(spec).__name__}")
    unknown = sorted(set(spec) - set(SPEC_KEYS))
    if unknown:
        raise ValueError(f"initial_state: unknown key(s) {', '.join(map(repr, unknown))}; "
                         f"valid: {', '.join(SPEC_KEYS)}")
    if "stride" in spec and "trajectory" not in spec:
        raise ValueError("initial_state: 'stride' goes with 'trajectory'")
    nq, nv = model.nq, model.nv
    qs, vs = [], []

    def add(what, q, v=None):
        q = _check_rows(what, q, nq, "qpos")
        v = np.zeros((len(q), nv)) if v is None else _check_rows(what, v, nv, "qvel")
        if len(v) != len(q):
            raise ValueError(f"{what}: {len(q)} qpos rows but {len(v)} qvel rows")
        qs.append(q)
        vs.append(v)

    if "keyframe" in spec:
        add("keyframe", _keyframe_row(model, spec["keyframe"]))
    if "keyframes" in spec:
        names = spec["keyframes"]
        if isinstance(names, str) or not len(names):
            raise ValueError("initial_state: 'keyframes' is a non-empty list of names")
        add("keyframes", np.stack([_keyframe_row(model, n) for n in names]))
    if "trajectory" in spec:
        add(f"trajectory {spec['trajectory']}", *load_trajectory(spec["trajectory"], spec.get("stride", 1)))
    if "states" in spec:
        st = spec["states"]
        if not isinstance(st, (tuple, list)) or len(st) != 2:
            raise ValueError("initial_state: 'states' is a pair (qpos, qvel); qvel may be None")
        add("states", st[0], st[1])
    if not qs:
        raise ValueError("initial_state: the spec names no states (keyframe, keyframes, trajectory or states)")
    return normalize_quaternions(np.concatenate(qs)), np.concatenate(vs)


def noise_scale_of(spec, default=None):
    """The spec's optional ``"noise_scale"`` (a finite value >= 0), or ``default``."""
    if "noise_scale" not in spec:
        return default
    s = float(spec["noise_scale"])
    if not np.isfinite(s) or s < 0:
        raise ValueError(f"initial_state: noise_scale must be finite and >= 0, got {s}")
    return s
