"""What correctly rounded fp32 costs on the model variants (tests/model_variants.py), on the CPU: the
oracle's fp32 emulation (oracle/precision.py: every stage rounded to float, model, state and ctrl rounded
to float) against the fp64 oracle, one substep on the 48 states of the GPU test, as a fraction of the fp32
one-substep bounds of tests/test_gpu_parity.py.  The table of profiles/model_variants.md.

Run:  python tools/probes/model_variants_emulation.py
"""
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import model_variants as mv  # noqa: E402
from oracle import precision as pe  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402
from test_gpu_parity import _run_oracle, _states  # noqa: E402


def main():
    tmp = pathlib.Path(tempfile.mkdtemp())
    print("| variant | qacc / bound | qpos / bound | qvel / bound | worst state | counts equal |")
    print("|---|---|---|---|---|---|")
    for name in mv.NAMES:
        p = mv.write_model_variant(tmp, name)
        o = Oracle(p)
        e = pe.PrecOracle(M=pe.round_model(o.M))
        pe.set_mask(pe.ALL)
        worst, at, same = np.zeros(3), 0, 0
        states = _states(o.M, 48, seed=7)
        for i, (q, v, c) in enumerate(states):
            rq, rv, ra, ncon, nefc = _run_oracle(o, q, v, c)
            f32 = lambda x: x.astype(np.float32).astype(np.float64)   # noqa: E731
            eq, ev, ea, encon, enefc = _run_oracle(e, f32(q), f32(v), c)
            same += (ncon, nefc) == (encon, enefc)
            s = 1 + np.abs(ra).max()
            f = np.array([np.abs(ea - ra).max() / (2e-3 * s), np.abs(eq - rq).max() / (2e-6 + 1e-7 * s),
                          np.abs(ev - rv).max() / (1e-5 * s)])
            if f.max() > worst.max():
                at = i
            worst = np.maximum(worst, f)
        print(f"| {name} | {worst[0]:.3f} | {worst[1]:.3f} | {worst[2]:.3f} | {at} | {same} of {len(states)} |")


if __name__ == "__main__":
    main()
