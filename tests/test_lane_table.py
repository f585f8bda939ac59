"""The model's lane table (csrc/hs_model.h LaneTable): the host packer, checked entry by entry.

The fp64 step kernels read the model's per-lane constants from an LDS copy of this table instead of
from the compiled model, so an entry the packer gets wrong is a wrong simulation.  No GPU needed: the
table, its layout description and the compiled model's own fields come through the C ABI
(hs_model_lane_table, hs_lane_layout, hs_model_lane_source).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import XML

HS_FP32, HS_FP64 = 0, 1
KIND_DTYPE = {0: None, 1: np.uint32, 2: np.int8}     # 0: the precision's real

# what the variant changes in humanoid.xml: (old text, new text), each old text occurring exactly once
VARIANT_EDITS = (
    ('<joint type="hinge" damping=".2" stiffness="1" armature=".01"',
     '<joint type="hinge" damping=".35" stiffness="1" armature=".02"'),                     # damping, armature
    ('<motor name="knee_right"      gear="80"', '<motor name="knee_right"      gear="60"'),  # gear
    ('<motor name="elbow_left"      gear="40"', '<motor name="elbow_left"      ctrlrange="-0.4 0.6" gear="40"'),
    ('<joint name="abdomen_x" pos="0 0 .1" axis="1 0 0" range="-35 35"',
     '<joint name="abdomen_x" pos="0 0 .1" axis="1 0 0" range="-25 30"'),                   # one joint range
    ('<fixed name="hamstring_left" limited="true" range="-0.3 2">',
     '<fixed name="hamstring_left" limited="true" range="-0.2 1.5">'),                      # one tendon range
    ('<joint pos="0 0 .08" axis="0 1 0" stiffness="6"/>', '<joint pos="0 0 .08" axis="0 1 0" stiffness="8"/>'),
)
# the table entries those edits must change (and the only ones they may)
VARIANT_CHANGES = {"dof_damping", "dof_armature", "dof_invweight0", "body_invweight_tran", "act_gear",
                   "act_ctrlrange", "jnt_range", "ten_range", "dof_stiffness"}


def write_variant(tmp_path):
    """humanoid.xml with other damping, armature, one gear, one ctrlrange, one joint range, one tendon
    range and one stiffness; returns its path."""
    src = open(XML).read()
    for old, new in VARIANT_EDITS:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    p = tmp_path / "humanoid_variant.xml"
    p.write_text(src)
    return str(p)


def _layout(prec):
    from mujocoposelearning_amd._lib import lib
    L = lib()
    n = L.hs_lane_layout(prec, -1, None, 0, None, None, None)
    assert n > 0
    out = []
    for i in range(n):
        name = C.create_string_buffer(64)
        off, cnt, kind = C.c_int(), C.c_int(), C.c_int()
        assert L.hs_lane_layout(prec, i, name, 64, C.byref(off), C.byref(cnt), C.byref(kind)) == n
        out.append((name.value.decode(), off.value, cnt.value, kind.value))
    return out


def _table(model, prec):
    from mujocoposelearning_amd._lib import lib
    L = lib()
    size = L.hs_model_lane_table(model.handle, prec, None, 0)
    assert size > 0 and size % 16 == 0
    raw = np.zeros(size, np.uint8)
    assert L.hs_model_lane_table(model.handle, prec, raw.ctypes.data, size) == size
    return raw


def _source(model, prec, name):
    from mujocoposelearning_amd._lib import lib
    L = lib()
    n = L.hs_model_lane_source(model.handle, prec, name.encode(), None, 0)
    assert n > 0, name
    out = np.zeros(n, np.float64)
    assert L.hs_model_lane_source(model.handle, prec, name.encode(), out.ctypes.data, n) == n
    return out


def _decode(raw, prec, entry):
    _, off, cnt, kind = entry
    dt = KIND_DTYPE[kind] or (np.float64 if prec == HS_FP64 else np.float32)
    return raw[off:off + cnt * np.dtype(dt).itemsize].view(dt)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from mujocoposelearning_amd.model import HsModel
    return HsModel(XML), HsModel(write_variant(tmp_path_factory.mktemp("lane_table")))


@pytest.mark.parametrize("prec", [HS_FP64, HS_FP32])
def test_layout_covers_the_table_without_overlap(models, prec):
    lay = _layout(prec)
    raw = _table(models[0], prec)
    real = 8 if prec == HS_FP64 else 4
    used = np.zeros(raw.size, bool)
    for name, off, cnt, kind in lay:
        w = {0: real, 1: 4, 2: 1}[kind]
        assert off % w == 0 and off + cnt * w <= raw.size, name
        assert not used[off:off + cnt * w].any(), name
        used[off:off + cnt * w] = True
    assert len({e[0] for e in lay}) == len(lay)
    assert raw.size - used.sum() < 16          # only the struct's tail padding is outside every entry
    if prec == HS_FP64:                        # the fp64 kernels' LDS budget (4 workgroups per CU)
        assert raw.size <= 5208


@pytest.mark.parametrize("prec", [HS_FP64, HS_FP32])
@pytest.mark.parametrize("which", [0, 1])
def test_every_entry_equals_the_compiled_model_field(models, prec, which):
    m = models[which]
    raw = _table(m, prec)
    for entry in _layout(prec):
        got = _decode(raw, prec, entry).astype(np.float64)
        want = _source(m, prec, entry[0])
        assert got.shape == want.shape, entry[0]
        assert np.array_equal(got, want), entry[0]


def test_entries_agree_with_the_mjcf_fields(models):
    """The entries a reader can check against the MJCF by eye, against hs_model_field (MuJoCo's names)."""
    for m in models:
        raw = _table(m, HS_FP64)
        t = {e[0]: _decode(raw, HS_FP64, e) for e in _layout(HS_FP64)}
        nv, nu, nj, nb, nq = m.nv, m.nu, m.njnt, m.nbody, m.nq
        assert np.array_equal(t["dof_damping"][:nv], m.field("dof_damping"))
        assert np.array_equal(t["dof_armature"][:nv], m.field("dof_armature"))
        assert np.array_equal(t["dof_invweight0"][:nv], m.field("dof_invweight0"))
        assert np.array_equal(t["act_gear"][:nu], m.field("actuator_gear").reshape(nu, -1)[:, 0])
        assert np.array_equal(t["act_ctrlrange"][:2 * nu], m.field("actuator_ctrlrange").ravel())
        assert np.array_equal(t["jnt_range"][:2 * nj], m.field("jnt_range").ravel())
        assert np.array_equal(t["ten_range"][:2 * m.ntendon], m.field("tendon_range").ravel())
        assert np.array_equal(t["body_mass"][:nb], m.field("body_mass"))
        assert np.array_equal(t["qpos0"][:nq], m.field("qpos0"))
        assert np.array_equal(t["body_pos"][:3 * nb], m.field("body_pos").ravel())
        assert np.array_equal(t["body_quat"][:4 * nb], m.field("body_quat").ravel())
        jstiff = m.field("jnt_stiffness")
        jid = t["dof_jntid"][:nv]
        hinge = t["jnt_type"][jid] == 3
        assert np.array_equal(t["dof_stiffness"][:nv][hinge], jstiff[jid[hinge]])


def test_variant_changes_exactly_the_edited_entries(models):
    stock, var = (_table(m, HS_FP64) for m in models)
    changed = {e[0] for e in _layout(HS_FP64)
               if not np.array_equal(_decode(stock, HS_FP64, e), _decode(var, HS_FP64, e))}
    assert changed == VARIANT_CHANGES
    t0 = {e[0]: _decode(stock, HS_FP64, e) for e in _layout(HS_FP64)}
    t1 = {e[0]: _decode(var, HS_FP64, e) for e in _layout(HS_FP64)}
    for name, k in (("act_gear", 1), ("act_ctrlrange", 2), ("jnt_range", 2), ("ten_range", 2)):
        assert (t0[name] != t1[name]).sum() == k, name       # ONE gear, ctrlrange, joint range, tendon range
    assert (t0["dof_stiffness"] != t1["dof_stiffness"]).sum() == 2   # the ankle_y class: both ankles
