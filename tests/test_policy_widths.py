"""The hidden width of the fused rollout-time kernels is a parameter (64, 128 or 256): hs_policy
carries it in a trailing `hidden` field that costs no size, and hs_mlp2_forward_h validates it
before touching the device (CPU only: nothing is launched)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_policy_and_rollout_struct_layouts_match_the_c_compiler(tmp_path):
    """Size and every field offset of the ctypes mirrors of hs_policy and hs_rollout_bufs equal what
    gcc lays out for include/hsim.h; hs_policy has `hidden` in its former tail padding (size 72)."""
    from mujocoposelearning_amd import _lib
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    structs = {"hs_policy": _lib.hs_policy, "hs_rollout_bufs": _lib.hs_rollout_bufs}
    assert "hidden" in [f for f, _ in _lib.hs_policy._fields_]
    assert C.sizeof(_lib.hs_policy) == 72
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hsim.h"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append(f'  printf("{name} size %zu\\n", sizeof({name}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{name} {f} %zu\\n", offsetof({name}, {f}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l}
    assert got[("hs_policy", "size")] == 72
    for name, cls in structs.items():
        assert got[(name, "size")] == C.sizeof(cls), name
        for f, _ in cls._fields_:
            assert got[(name, f)] == getattr(cls, f).offset, (name, f)
    # positional construction without the new field leaves it 0 (= 256)
    assert _lib.hs_policy(1, 2, 3, 4, 5, 6, 7, 512, 352, 21).hidden == 0


def test_mlp2_forward_h_validates_arguments():
    """hs_mlp2_forward_h rejects a hidden width outside {64, 128, 256} and ld2 / ld3 < H with a
    message, and reaches the null-buffer check for the widths it runs."""
    from mujocoposelearning_amd import _lib
    L = _lib.lib()

    def err(rc):
        assert rc < 0
        return L.hs_last_error().decode()

    def mlp(H, ld2=None, ld3=None, N=8, D=352, A=21):
        return L.hs_mlp2_forward_h(None, D, D, N, H, None, D, None, None, H if ld2 is None else ld2, None, None,
                                   H if ld3 is None else ld3, None, A, None, A, None)

    for H in (0, 32, 96, 512):
        assert "H = 64, 128 or 256" in err(mlp(H))
    for H in (64, 128, 256):
        assert f"ld2 >= {H}" in err(mlp(H, ld2=H - 4))
        assert f"ld3 >= {H}" in err(mlp(H, ld3=H - 4))
        assert "null buffer" in err(mlp(H))
        assert "A <= 32" in err(mlp(H, A=33))
        assert mlp(H, N=0) == 0          # an empty problem is a no-op
