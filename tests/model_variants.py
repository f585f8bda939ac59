"""Named variants of the shipped humanoid.xml whose constraint parameters leave the values the shipped
model pins: limit margins, solimp midpoints and powers, direct solref, friction other than 1, contact
parameter mixing by priority and by solmix, condim combinations, other geom sizes.

Each variant is a list of (old text, new text) edits, applied as tests/test_lane_table.py's
write_variant applies its own: the old text must occur exactly once.  Every variant keeps nq = 28,
nv = 27, nu = 21.  Variants are written into a test's tmp_path; no XML is committed.

coverage() counts, from the fp64 oracle alone, how often the states of a test reach the branches a
variant exists for, so the CPU suite and the GPU suite assert the same conditions.
"""
import numpy as np

from conftest import XML

JOINT_DEFAULT = '<joint type="hinge" damping=".2" stiffness="1" armature=".01" limited="true" solimplimit="0 .99 .01"/>'
BODY_GEOM = '<geom type="capsule" condim="1" friction=".7" solimp=".9 .99 .003" solref=".015 1" material="body" group="1"/>'
FLOOR = '<geom name="floor" size="0 0 .05" type="plane" material="grid" condim="3"/>'
HAMSTRING_LEFT = '<fixed name="hamstring_left" limited="true" range="-0.3 2">'

VARIANTS = {
    # joint margin 0.05 rad and a 5-number solimp (midpoint 0.3, power 3) on every hinge limit; tendon margin
    # 0.2 with a direct solref; the elbows unlimited; abdomen_x's range (4 deg = 0.0698 rad) narrower than
    # twice the margin, so both of its rows are active for every q inside the range
    "limits": (
        (JOINT_DEFAULT,
         '<joint type="hinge" damping=".2" stiffness="1" armature=".01" limited="true" margin="0.05" '
         'solimplimit="0.1 .95 .02 0.3 3"/>'),
        (HAMSTRING_LEFT, '<fixed name="hamstring_left" limited="true" range="-0.3 2" margin="0.2" solreflimit="-800 -30">'),
        ('<joint range="-100 50" stiffness="0"/>', '<joint range="-100 50" stiffness="0" limited="false"/>'),
        ('<joint name="abdomen_x" pos="0 0 .1" axis="1 0 0" range="-35 35"',
         '<joint name="abdomen_x" pos="0 0 .1" axis="1 0 0" range="-2 2"'),
    ),
    # pyramidal body-body contacts at mu = 1.3; the floor wins by priority: mu = 0.4 and the floor's own
    # (default) solref and solimp, whatever its solmix
    "contact": (
        (BODY_GEOM,
         '<geom type="capsule" condim="3" friction="1.3" solimp=".8 .97 .004 0.4 2.5" solref=".02 0.9" '
         'material="body" group="1"/>'),
        (FLOOR, '<geom name="floor" size="0 0 .05" type="plane" material="grid" condim="3" friction="0.4" '
                'priority="1" solmix="3"/>'),
    ),
    # every contact one frictionless row; floor contacts through the direct solref branch, mixed by the
    # min rule (a non-positive solref on either geom)
    "frictionless_direct": (
        (FLOOR, '<geom name="floor" size="0 0 .05" type="plane" material="grid" condim="1" solref="-4000 -60"/>'),
    ),
    # equal priorities with solmix 3 : 0.5 (floor contacts: mix 6/7, so a solimp power of 13/7 and a midpoint
    # of 0.5 + 0.2/7); body-body contacts with power exactly 1; joint limits with power 1; a tendon solimp
    # with d0 == dmax; thicker, tilted, shorter shins, bigger hands; an unclamped knee motor; a springref
    "shape": (
        (FLOOR, '<geom name="floor" size="0 0 .05" type="plane" material="grid" condim="3" solmix="3"/>'),
        (BODY_GEOM,
         '<geom type="capsule" condim="1" friction=".7" solimp=".9 .99 .003 0.7 1" solref=".015 1" solmix="0.5" '
         'material="body" group="1"/>'),
        (JOINT_DEFAULT,
         '<joint type="hinge" damping=".2" stiffness="1" armature=".01" limited="true" solimplimit="0 .99 .01 0.5 1"/>'),
        (HAMSTRING_LEFT, '<fixed name="hamstring_left" limited="true" range="-0.3 2" solimplimit=".95 .95 .01">'),
        ('<geom fromto="0 0 0 0 0 -.3"  size=".049"/>', '<geom fromto="0 0 0 .02 0 -.27"  size=".055"/>'),
        ('<geom name="shin_left" fromto="0 0 0 0 0 -.3" class="shin"/>',
         '<geom name="shin_left" fromto="0 0 0 .02 0 -.27" class="shin"/>'),
        ('<geom type="sphere" size=".04"/>', '<geom type="sphere" size=".055"/>'),
        ('<motor name="knee_left"       gear="80"  joint="knee_left"/>',
         '<motor name="knee_left"       gear="80"  joint="knee_left" ctrllimited="false"/>'),
        ('<joint name="abdomen_y" pos="0 0 .065" axis="0 1 0" range="-75 30" class="joint_big"/>',
         '<joint name="abdomen_y" pos="0 0 .065" axis="0 1 0" range="-75 30" springref="10" class="joint_big"/>'),
    ),
}
NAMES = tuple(VARIANTS)

# oracle/hsim_oracle.h: efc_type
LIMIT_JOINT, LIMIT_TENDON, CONTACT_FRICTIONLESS, CONTACT_PYRAMIDAL = 3, 4, 5, 6


def write_model_variant(tmp_path, name):
    """humanoid.xml with the edits of VARIANTS[name]; returns its path."""
    src = open(XML).read()
    for old, new in VARIANTS[name]:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    p = tmp_path / f"humanoid_{name}.xml"
    p.write_text(src)
    return str(p)


def forward_rows(o, q, v):
    """The oracle's constraint rows and contacts at (q, v): (efc_type, efc_id, efc_pos, contacts)."""
    o.reset_data()
    o.qpos[:] = q
    o.qvel[:] = v
    o.forward()
    n = o.d.nefc
    return (o.arr("efc_type", n).copy(), o.arr("efc_id", n).copy(), o.arr("efc_pos", n).copy(), o.contacts())


def coverage(o, states):
    """Counts over ``states`` ((qpos, qvel, ...) tuples, none skipped) of what the variants exist to reach."""
    c = dict(joint_rows_in_margin=0, tendon_rows_in_margin=0, states_with_both_rows_of_a_joint=0, contacts=0,
             contacts_dim3_mu_not_1=0, body_body_contacts=0, frictionless_rows=0, contact_rows=0, direct_solref_contacts=0,
             power1_contacts=0, pow_contacts=0, joint_rows=0, tendon_rows=0, tendon1_rows=0)
    for s in states:
        typ, ids, pos, cons = forward_rows(o, s[0], s[1])
        jl = typ == LIMIT_JOINT
        c["joint_rows_in_margin"] += int((jl & (pos > 0)).sum())
        c["tendon_rows_in_margin"] += int(((typ == LIMIT_TENDON) & (pos > 0)).sum())
        c["states_with_both_rows_of_a_joint"] += int(len(set(ids[jl])) < jl.sum())
        c["contacts"] += len(cons)
        c["contacts_dim3_mu_not_1"] += sum(k["dim"] == 3 and k["friction"][0] != 1 for k in cons)
        c["body_body_contacts"] += sum(o.M["geom_bodyid"][k["geom"][0]] != 0 for k in cons)
        c["frictionless_rows"] += int((typ == CONTACT_FRICTIONLESS).sum())
        c["contact_rows"] += int((typ >= CONTACT_FRICTIONLESS).sum())
        c["direct_solref_contacts"] += sum(k["solref"][0] <= 0 for k in cons)
        c["power1_contacts"] += sum(k["solimp"][4] == 1 for k in cons)
        c["pow_contacts"] += sum(k["solimp"][4] not in (1, 2) for k in cons)
        c["joint_rows"] += int(jl.sum())
        c["tendon_rows"] += int((typ == LIMIT_TENDON).sum())
        c["tendon1_rows"] += int(((typ == LIMIT_TENDON) & (ids == 1)).sum())
    return c


def check_coverage(name, c):
    """The conditions a variant's states must meet for its test to mean anything.  Each is about half the
    count the fp64 oracle gives on test_gpu_parity._states(M, 48, seed=7), written next to it."""
    if name == "limits":
        # 71, not the 40 of a wider abdomen_x range: "-2 2" puts both of its rows inside the margin in every
        # standing state; the bound is half of what these edits give
        assert c["joint_rows_in_margin"] >= 35, c                    # 71
        assert c["tendon_rows_in_margin"] >= 5, c                    # 10
        assert c["states_with_both_rows_of_a_joint"] >= 1, c         # 17
    elif name == "contact":
        assert c["contacts"] > 0 and c["contacts_dim3_mu_not_1"] == c["contacts"], c     # 186 of 186
        assert c["body_body_contacts"] >= 10, c                      # 26
    elif name == "frictionless_direct":
        assert c["contact_rows"] > 0 and c["frictionless_rows"] == c["contact_rows"] == c["contacts"], c   # 186 rows
        assert c["direct_solref_contacts"] >= 80, c                  # 160 (the floor's)
    elif name == "shape":
        assert c["power1_contacts"] >= 13, c                         # 26 (body-body)
        assert c["pow_contacts"] >= 80, c                            # 160 (floor: power 13/7)
        assert c["joint_rows"] >= 40, c                              # 85 (power 1)
        assert c["tendon1_rows"] >= 1, c                             # 3 (d0 == dmax)


def wide_body_body_states(o, n, seed, resident=(32, 128), wide=(64, 256), min_body_body=2):
    """n lying poses (tests/test_gpu_contacts.py's pose generator) that overflow the resident tier, fit the
    wide tier and have at least ``min_body_body`` body-body contacts, by the oracle; (poses, draws used)."""
    from test_gpu_contacts import lying_poses
    out = []
    for k, q in enumerate(lying_poses(o.M, seed)):
        o.reset_data()
        o.qpos[:] = q
        o.qvel[:] = 0
        o.forward()
        ncon, nefc = o.d.ncon, o.d.nefc
        if (ncon > resident[0] or nefc > resident[1]) and ncon <= wide[0] and nefc <= wide[1] and \
                sum(o.M["geom_bodyid"][c["geom"][0]] != 0 for c in o.contacts()) >= min_body_body:
            out.append(q)
            if len(out) == n:
                return out, k + 1
    raise AssertionError(f"only {len(out)} of {n} states in 20000 draws")
