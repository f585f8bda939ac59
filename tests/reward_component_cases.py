"""Shared by tests/test_reward_components.py and tests/test_gpu_reward_components.py: reward functions that
return a dict of named components, chosen for the tracer's and the interpreter's edge cases, and a private
registry holding each of them, each of their components alone as a scalar program, and the built-ins'
breakdowns."""
from mujocoposelearning_amd import reward_functions as rf
from mujocoposelearning_amd import reward_program as rw

DIMS = (28, 27, 21, 17)


def dead_output(d, p):
    """``extra`` feeds nothing: it is alive only because it is an output."""
    extra = d.qvel[0] * d.qvel[1] - 3.0
    return {"total": d.qpos[2] * 2.0, "extra": extra}


def shared_node(d, p):
    """Two names bound to one node."""
    x = d.qpos[2] * d.qpos[2] + d.qvel[0]
    return {"a": x, "total": x}


def leaf_outputs(d, p):
    """Outputs that are a bare constant, a bare parameter and a bare load; ``unused`` is a load nothing else reads."""
    return {"const": 1.5, "param": p["w"], "load": d.qvel[1], "unused": d.qvel[5], "total": d.qvel[1] / p["w"]}


def total_first(d, p):
    """``total`` is not the last entry."""
    up = d.qpos[2] - 1.282
    lean = d.qpos[3] * d.qpos[3]
    return {"total": rw.where(d.qpos[2] < 0.8, 0.0, lean - up * up), "up": up, "lean": lean, "low": d.qpos[2] < 0.8}


def sixteen(d, p):
    """The limit: 16 outputs."""
    out = {f"q{i}": d.qpos[i] * float(i + 1) + d.qvel[i] for i in range(15)}
    out["total"] = rw.sum([out[f"q{i}"] for i in range(15)])
    return out


def slot_reuse(d, p):
    """``early`` is produced and written out first; the chain that follows is long enough to reuse its slot."""
    early = d.qpos[2] * d.qvel[2]
    acc = d.qpos[0]
    for i in range(1, 12):
        acc = acc * 0.5 + d.qpos[i]
    return {"early": early, "total": acc}


def arith_ops(d, p):
    """+ - * /, comparisons and where only: the host interpreter must equal the twin bit for bit."""
    a, b = d.qvel[3], d.qpos[2]
    return {"sum": a + b, "diff": a - b, "prod": a * b, "quot": a / b, "lt": a < b, "ge": a >= b, "ne": a != b,
            "sel": rw.where(a < b, a * 2.0, b / 3.0), "total": (a + b) * (a - b) / (b * b + 1.0)}


def libm_ops(d, p):
    """One libm op per component, on a plain load (scaled into the op's domain): each within the host
    interpreter's 1 ulp of the numeric twin."""
    x = d.qvel[4] * 0.25
    u = d.qpos[3]                      # a unit quaternion's w: in [-1, 1]
    return {"exp": rw.exp(x), "log": rw.log(abs(x) + 0.5), "sin": rw.sin(x), "cos": rw.cos(x), "tanh": rw.tanh(x),
            "arcsin": rw.arcsin(u), "arccos": rw.arccos(u), "arctan2": rw.arctan2(x, u), "sqrt": rw.sqrt(abs(x)),
            "total": x}


def only_total(d, p):
    """One component: the reward itself."""
    return {"total": d.qpos[2] * d.qpos[2] - d.qvel[2]}


def contact_forces(d, p):
    """Reads cfrc_ext (the two feet, bodies 9 and 6 of humanoid.xml): zeros unless the batch computes the full
    state."""
    lf, rf_ = rw.sum(abs(d.cfrc_ext[9])), rw.sum(abs(d.cfrc_ext[6]))
    return {"left": lf, "right": rf_, "total": lf - rf_}


# name -> (function, parameter defaults)
EDGE = {"dead_output": (dead_output, None), "shared_node": (shared_node, None), "leaf_outputs": (leaf_outputs, {"w": 0.75}),
        "total_first": (total_first, None), "sixteen": (sixteen, None), "slot_reuse": (slot_reuse, None),
        "arith_ops": (arith_ops, None), "libm_ops": (libm_ops, None), "only_total": (only_total, None),
        "contact_forces": (contact_forces, None)}
BREAKDOWNS = {"stand_components": (rw.stand_components_program, None),
              "walk_components": (rw.walk_components_program, None),
              "kneeling_components": (rw.kneeling_components_program, rw.KNEEL_DEFAULTS)}


def _one(fn, key):
    def single(d, p):
        return fn(d, p)[key]
    single.__name__ = f"{fn.__name__}_{key}"
    return single


def registry():
    """A private registry: every function above under its name, and component ``k`` of function ``f`` alone, as a
    scalar program, under ``"f/k"``."""
    reg = dict(rf.REWARD_FUNCTIONS)
    for name, (fn, defaults) in {**EDGE, **BREAKDOWNS}.items():
        rw.register_device_reward(name, fn, defaults=defaults, registry=reg)
        for key in rw.device_reward_program(name, reg).trace(DIMS).outputs:
            rw.register_device_reward(f"{name}/{key}", _one(fn, key), defaults=defaults, registry=reg)
    return reg
