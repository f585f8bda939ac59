"""Shared by tests/test_reference_motion.py and tests/test_gpu_reference_motion.py: fixed pseudo-random reference
rows, the edge times, and a 16-component probe program that writes reference values out unchanged."""
import numpy as np

from mujocoposelearning_amd import reference_motion as rm
from mujocoposelearning_amd import reward_program as rw

NQ, NV, NU, NBODY = 28, 27, 21, 17
DIMS = (NQ, NV, NU, NBODY)
KEY_DT = 0.25
SEED = 0x5EED1234ABCD


def rows(K, seed=3):
    """(qpos [K, nq], qvel [K, nv]): values of mixed sign and magnitude, unit-free quaternions (normalised on bind)."""
    rng = np.random.default_rng(seed + K)
    q = rng.normal(size=(K, NQ)) * 10.0 ** rng.integers(-2, 2, size=(K, NQ))
    q[:, 3:7] = rng.normal(size=(K, 4)) + np.array([2.0, 0, 0, 0])
    v = rng.normal(size=(K, NV)) * 3.0
    return q, v


def reference(K, end="hold", start="zero", seed=3):
    q, v = rows(K, seed)
    return rm.Reference(q, v, key_dt=KEY_DT if K > 1 else None, end=end, start=start)


def edge_times(K):
    """Exact key boundaries, mid-interval, the last interval, beyond the end, 0, negative, NaN, +inf, 1e300."""
    last = (K - 1) * KEY_DT
    t = [0.0, KEY_DT, 2 * KEY_DT, last, 0.5 * KEY_DT, 0.1, 1.37 * KEY_DT, last - 0.25 * KEY_DT, last - 1e-9,
         last + 1e-9, last + 0.6 * KEY_DT, K * KEY_DT, (K + 0.5) * KEY_DT, 37.3, 1e6 + 0.1, -0.0, -1e-300, -0.5,
         -np.inf, np.nan, np.inf, 1e300, 2.0 ** 52 * KEY_DT, 2.0 ** 60]
    return np.array(t, dtype=np.float64)


PROBE_NAMES = tuple([f"q{k}" for k in range(7)] + ["q_last", "v0", "v5", "v_last", "sum_q", "sum_v", "dot", "mix",
                                                    "total"])


def probe(d, p):
    """16 components: reference values unchanged (so a wrong row, weight or offset shows bitwise) and a few sums."""
    q, v = d.ref_qpos, d.ref_qvel
    out = {f"q{k}": q[k] for k in range(7)}
    out["q_last"] = q[NQ - 1]
    out["v0"], out["v5"], out["v_last"] = v[0], v[5], v[NV - 1]
    out["sum_q"] = rw.sum(q[7:])
    out["sum_v"] = rw.sum(v[6:])
    out["dot"] = rw.sum(q[3:7] * q[3:7])
    out["mix"] = q[2] * 2.0 - v[1]
    out["total"] = q[2] + v[0]
    return out


def probe_expected(ref_q, ref_v):
    """The probe's [16, n] components from sampled (ref_qpos, ref_qvel) of dtype T, every operation rounded in T
    in the program's own order (rw.sum's pairwise order through the numeric helpers is float64 only, so the sums
    are restated here with the same association)."""
    T = ref_q.dtype.type

    def psum(x):                    # reward_program.sum's order, in T
        n = x.shape[1]
        if n < 8:
            res = np.zeros(len(x), dtype=T)
            i = 0
        else:
            nb = n - n % 8
            r = [x[:, j].copy() for j in range(8)]
            for i in range(8, nb, 8):
                for j in range(8):
                    r[j] = r[j] + x[:, i + j]
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            i = nb
        for j in range(i, n):
            res = res + x[:, j]
        return res
    with np.errstate(all="ignore"):
        out = [ref_q[:, k] for k in range(7)] + [ref_q[:, NQ - 1], ref_v[:, 0], ref_v[:, 5], ref_v[:, NV - 1],
                                                 psum(ref_q[:, 7:]), psum(ref_v[:, 6:]),
                                                 psum(ref_q[:, 3:7] * ref_q[:, 3:7]),
                                                 ref_q[:, 2] * T(2.0) - ref_v[:, 1], ref_q[:, 2] + ref_v[:, 0]]
    return np.stack(out)


def scalar_probe(d, p):
    """A program without components (the sanitizer harness validates with none): first, middle and last columns of
    both fields and the time, behind a few operations."""
    return (d.ref_qpos[0] + d.ref_qpos[NQ - 1] * d.ref_qvel[NV - 1]) - rw.sum(d.ref_qvel[:5]) * d.ref_qpos[13] + d.time


def probe_registry():
    reg = {}
    rw.register_device_reward("ref_probe", probe, registry=reg)
    rw.register_device_reward("ref_scalar", scalar_probe, registry=reg)
    return reg


def times_of(K, dtype):
    """The edge times as a batch of ``dtype`` can hold them, float64 (1e300 is +inf in float32)."""
    with np.errstate(over="ignore"):
        return edge_times(K).astype(dtype).astype(np.float64)
