"""The model variants of tests/model_variants.py on the CPU: both MJCF compilers agree on them, the lane
table carries them entry by entry in both precisions, the states the GPU tests step them on do reach the
branches the variants exist for (counted from the fp64 oracle alone), and a geom ``gap`` -- which neither
the step kernels nor the oracle honour -- is rejected by both compilers.
"""
import numpy as np
import pytest

import model_variants as mv
from conftest import XML
from test_lane_table import HS_FP32, HS_FP64, _decode, _layout, _source, _table
from test_model import FIELDS


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("model_variants")
    return {name: mv.write_model_variant(d, name) for name in mv.NAMES}


@pytest.mark.parametrize("name", mv.NAMES)
def test_compilers_agree_on_the_variant(paths, name):
    """tests/test_model.py's field-by-field comparison and tolerances, on the variant."""
    from mujocoposelearning_amd.model import HsModel
    from oracle.model import compile_mjcf
    P, O = HsModel(paths[name]), compile_mjcf(paths[name])
    assert (P.nq, P.nv, P.nu) == (28, 27, 21) == (O["nq"], O["nv"], O["nu"])
    for k in FIELDS:
        a = np.asarray(P.field(k), float).reshape(-1)
        b = np.asarray(O[k], float).reshape(-1)
        assert a.shape == b.shape, k
        assert np.allclose(a, b, rtol=1e-10, atol=1e-12), (k, np.abs(a - b).max())
    assert np.allclose(P.field("body_inertia_full").reshape(-1, 3, 3), O["body_inertia_full"], atol=1e-14)
    assert P.field("stat_meaninertia")[0] == pytest.approx(O["stat_meaninertia"], rel=1e-12)


@pytest.mark.parametrize("name", mv.NAMES)
def test_variant_differs_from_the_shipped_model_where_it_says(paths, name, oracle_model):
    """The edits took: the oracle compiler's fields differ from humanoid.xml's in the edited places."""
    from oracle.model import compile_mjcf
    S, V = oracle_model, compile_mjcf(paths[name])
    differ = {k for k in FIELDS + ["jnt_margin", "tendon_margin", "tendon_solref", "tendon_solimp", "geom_priority",
                                   "geom_solmix"]
              if not np.array_equal(np.asarray(S[k], float), np.asarray(V[k], float))}
    want = {"limits": {"jnt_margin", "jnt_solimp", "tendon_margin", "tendon_solref", "jnt_limited", "jnt_range"},
            "contact": {"geom_condim", "geom_friction", "geom_solimp", "geom_solref", "geom_priority", "geom_solmix"},
            "frictionless_direct": {"geom_condim", "geom_solref"},
            "shape": {"geom_solmix", "geom_solimp", "jnt_solimp", "tendon_solimp", "geom_size", "geom_pos",
                      "geom_rbound", "actuator_ctrllimited", "qpos_spring", "body_mass"}}[name]
    assert want <= differ, want - differ
    if name == "limits":
        j = V["jnt_name"].index("abdomen_x")
        assert V["jnt_range"][j][1] - V["jnt_range"][j][0] < 2 * V["jnt_margin"][j]
        assert V["jnt_limited"].sum() == S["jnt_limited"].sum() - 2          # the two elbows
        assert list(V["jnt_solimp"][j]) == [0.1, 0.95, 0.02, 0.3, 3]
        assert list(V["tendon_solref"][1]) == [-800, -30] and list(V["tendon_margin"]) == [0, 0.2]
    if name == "shape":
        assert V["actuator_ctrllimited"].sum() == 20
        assert V["jnt_solimp"][1][4] == 1 and V["tendon_solimp"][1][0] == V["tendon_solimp"][1][1]


@pytest.mark.parametrize("prec", [HS_FP64, HS_FP32])
@pytest.mark.parametrize("name", mv.NAMES)
def test_lane_table_equals_its_sources(paths, name, prec):
    """tests/test_lane_table.py's entry-by-entry check on the variant, and the one margin the table holds
    (jnt_margin) against the oracle compiler's."""
    from mujocoposelearning_amd.model import HsModel
    from oracle.model import compile_mjcf
    m = HsModel(paths[name])
    raw = _table(m, prec)
    t = {}
    for entry in _layout(prec):
        got = _decode(raw, prec, entry).astype(np.float64)
        want = _source(m, prec, entry[0])
        assert got.shape == want.shape, entry[0]
        assert np.array_equal(got, want), entry[0]
        t[entry[0]] = got
    O = compile_mjcf(paths[name])
    real = np.float64 if prec == HS_FP64 else np.float32
    nj = O["njnt"]
    assert np.array_equal(t["jnt_margin"][:nj], O["jnt_margin"].astype(real).astype(np.float64))
    assert np.array_equal(t["jnt_limited"][:nj], O["jnt_limited"])
    assert np.array_equal(t["act_ctrllimited"][:O["nu"]], O["actuator_ctrllimited"])
    assert np.allclose(t["jnt_range"][:2 * nj], O["jnt_range"].ravel(), rtol=1e-6 if prec == HS_FP32 else 1e-12)
    if name == "limits":
        assert (t["jnt_margin"][1:nj] != 0).all()


@pytest.mark.parametrize("name", mv.NAMES)
def test_the_48_states_reach_the_variant_branches(paths, name):
    """The coverage conditions of the GPU one-substep test, from the oracle alone (no state skipped)."""
    from oracle.oracle import Oracle
    from test_gpu_parity import _states
    o = Oracle(paths[name])
    states = _states(o.M, 48, seed=7)
    assert len(states) == 48
    c = mv.coverage(o, states)
    print(name, c)
    mv.check_coverage(name, c)


def test_wide_tier_generator_finds_its_states(paths):
    """The pyramidal body-body wide-tier states of the GPU test exist within the generator's 20 000 draws."""
    from oracle.oracle import Oracle
    o = Oracle(paths["contact"])
    qs, draws = mv.wide_body_body_states(o, 16, seed=1)
    assert len(qs) == 16 and draws <= 20000
    print("draws", draws)


@pytest.mark.parametrize("where", ["floor", "body"])
def test_geom_gap_fails_loudly_in_both_compilers(tmp_path, where):
    from mujocoposelearning_amd._lib import HsimError
    from mujocoposelearning_amd.model import HsModel
    from oracle.model import compile_mjcf
    old = mv.FLOOR if where == "floor" else mv.BODY_GEOM
    src = open(XML).read()
    assert src.count(old) == 1
    p = tmp_path / "gap.xml"
    p.write_text(src.replace(old, old.replace("<geom ", '<geom gap="0.01" ')))
    with pytest.raises(HsimError, match="gap"):
        HsModel(str(p))
    with pytest.raises(ValueError, match="gap"):
        compile_mjcf(str(p))
    zero = tmp_path / "gap0.xml"                       # gap="0" is MuJoCo's default and still compiles
    zero.write_text(src.replace(old, old.replace("<geom ", '<geom gap="0" ')))
    assert HsModel(str(zero)).nv == 27 == compile_mjcf(str(zero))["nv"]
