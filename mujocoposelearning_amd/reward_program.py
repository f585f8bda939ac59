"""Reward programs: user-defined reward functions that run on the device.

The reference's extension point is one more entry in ``REWARD_FUNCTIONS`` (reward_functions.py:264-269).
Here such a function is written ONCE, over this module's small expression namespace::

    from mujocoposelearning_amd import reward_program as rw

    @rw.register_device_reward("lean", defaults={"target": 1.2, "w": 0.1})
    def lean(d, p):
        up = rw.exp(-4.0 * (d.qpos[2] - p["target"]) ** 2)
        return rw.where(d.qpos[2] < 0.8, 0.0, up - p["w"] * rw.sum(rw.square(d.ctrl)))

``d`` is the ``env_data`` view with the reference's field names, ``p`` the float parameters (the
defaults overlaid with ``reward_config["params"]``).  Called with symbols, the function is TRACED into a
flat, branch-free instruction list that ``reward_program_kernel`` (csrc/hs_reward_prog.hip) evaluates for
every env of a batch; called with numbers, the same function is the host callable registered in
``REWARD_FUNCTIONS`` (its *numeric twin*), which ``HumanoidEnv`` and every host surface use and which
is the device code's reference in the tests.

Fields: ``qpos``, ``qvel``, ``ctrl``, ``time``, ``qfrc_actuator[nv]``, ``cinert[nbody][10]``,
``cvel[nbody][6]``, ``subtree_com[0]`` (only the root's row: the batch keeps that one, in its aux row),
``cfrc_ext[nbody][6]`` and ``subtree_linvel[nbody][3]`` (zeros unless ``full_state``, as the built-in
rewards see them); and ``ref_qpos[nq]`` / ``ref_qvel[nv]``, the batch's reference motion sampled at the env's own
episode and time (``reference_motion.py``; the batch must have one bound).  Indexing and slicing give object arrays of scalars, so a vector expression unrolls
into scalar instructions; negative and slice indices are resolved against the model at trace time.

Operators: ``+ - * /``, unary minus, ``abs``, ``**`` with a constant exponent 2, 3 or 4 (repeated
multiplication), comparisons and ``& | ~`` on their results; the functions below (``where``, ``minimum``,
``maximum``, ``sqrt``, ``exp``, ``log``, ``sin``, ``cos``, ``tanh``, ``arctan2``, ``arcsin``, ``arccos``,
``square``, ``sum``, ``quaternion_to_euler``); ``np.exp(x)`` and the like work too (numpy calls the
method of the same name on an object scalar).  ``bool(x)`` raises: a Python ``if`` or the builtin ``min``
cannot be traced, use ``where`` / ``minimum``.

Semantics, identical in the numeric twin, the host interpreter (``hs_reward_program_eval_host``) and
the kernel: every operation is rounded on its own (no FMA contraction) in the association the function
wrote; a comparison with a NaN is false; ``where`` selects, both arms are always evaluated;
``minimum(a, b)`` is ``where(b < a, b, a)``, the Python ``min(a, b)`` the reference's rewards use;
``sum`` adds in numpy's pairwise order (n < 8: sequentially from 0; else eight strided accumulators over
the whole blocks of 8, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail in order) -- the
tracer emits that add tree itself.  Programs are pure: the ``params["previous_qpos"]`` side effect of
the built-in callables is not part of the language.

Named components: a function may return a ``dict`` of name -> scalar expression instead of one expression.  It
must contain ``"total"``, which is the reward; every entry, ``"total"`` included, is a component, in dict order
(at most ``MAX_OUTPUTS`` = 16, names non-empty ``str``; otherwise ValueError).  The twin in ``REWARD_FUNCTIONS``
still returns the reward as a float; ``DeviceReward.twin_components`` gives ``{name: float}`` and the program
carries one ``out`` instruction per component (csrc/hs_reward_prog.h RP_OUT), which the kernel stores into
component-major ``[C, N]`` rows: ``info["reward_components"]`` of the env surfaces, ``HsBatch.reward_components``.
A function that returns a scalar traces exactly as before.  ``stand_components_program`` and its two siblings at
the end of this module break the built-ins down; ``reward_config={"type": "stand", "components": True}`` runs one.

Limits (include/hsim.h HS_RP_MAX_*): 4096 instructions, 64 LIVE values (the tracer allocates value slots
by liveness, so a long program is fine as long as few values are alive at once), 256 constants,
32 parameters.  A program over a limit is refused at trace time with the figure in the message.

Termination conditions are predicates in the same language (``register_device_termination``,
``TERMINATION_FUNCTIONS``, the built-ins ``"fallen"`` and ``"lost_balance"``): see the section at the end of
this module and ``env_config["termination"]``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import reward_functions as _rf

MAX_INSTR, MAX_SLOTS, MAX_CONSTS, MAX_PARAMS = 4096, 64, 256, 32

# csrc/hs_reward_prog.h RpOp
_OPS = ("const", "param", "load",
        "add", "sub", "mul", "div", "arctan2", "lt", "le", "gt", "ge", "eq", "ne", "and", "or",
        "neg", "abs", "sqrt", "exp", "log", "sin", "cos", "tanh", "arcsin", "arccos", "not",
        "where", "result", "out")
OP = {n: i for i, n in enumerate(_OPS)}
MAX_OUTPUTS = 16
_ARITY = {**{n: 2 for n in _OPS[3:16]}, **{n: 1 for n in _OPS[16:27]}, "where": 3}
# csrc/hs_reward_prog.h RpField, and each field's row shape from (nq, nv, nu, nbody)
FIELDS = ("qpos", "qvel", "ctrl", "time", "qfrc_actuator", "cinert", "cvel", "subtree_com", "cfrc_ext",
          "subtree_linvel")
# ``FIELDS`` are the state fields, which a caller supplies as arrays (the members of hs_reward_fields, one each).
# The two REFERENCE_FIELDS come after them in the id space, in a block of their own (RP_F_REF_QPOS = 16,
# RP_F_REF_QVEL = 17; the ids 10 .. 15 stay unknown): the sample of the batch's reference motion at the env's own
# phase (reference_motion.py), which no caller supplies as an array.
REFERENCE_FIELDS = ("ref_qpos", "ref_qvel")
ALL_FIELDS = FIELDS + REFERENCE_FIELDS
FIELD_ID = {**{n: i for i, n in enumerate(FIELDS)}, "ref_qpos": 16, "ref_qvel": 17}
_FIELD_NAME = {i: n for n, i in FIELD_ID.items()}


def _field_shape(name, nq, nv, nu, nbody):
    return {"qpos": (nq,), "qvel": (nv,), "ctrl": (nu,), "time": (), "qfrc_actuator": (nv,), "cinert": (nbody, 10),
            "cvel": (nbody, 6), "subtree_com": (3,), "cfrc_ext": (nbody, 6), "subtree_linvel": (nbody, 3),
            "ref_qpos": (nq,), "ref_qvel": (nv,)}[name]


# ------------------------------------------------------------------ scalars
class Scalar:
    """One value of a reward function: a number (numeric twin) or a node of the traced program.  All
    arithmetic goes through its context, so the two runs of a function perform the same operations."""
    __slots__ = ("ctx", "v")
    __hash__ = None

    def __init__(self, ctx, v):
        self.ctx = ctx
        self.v = v

    def __bool__(self):
        raise TypeError("the truth value of a reward-program scalar is not available while the function is traced: "
                        "a Python `if`, `and`/`or` or the builtin min/max cannot become device code -- use "
                        "rw.where(cond, a, b), rw.minimum / rw.maximum and & | ~ instead")

    def _b(self, op, o, swap=False):
        if isinstance(o, np.ndarray):
            return NotImplemented
        o = self.ctx.lift(o)
        return self.ctx.op(op, o, self) if swap else self.ctx.op(op, self, o)

    def __add__(self, o): return self._b("add", o)
    def __radd__(self, o): return self._b("add", o, True)
    def __sub__(self, o): return self._b("sub", o)
    def __rsub__(self, o): return self._b("sub", o, True)
    def __mul__(self, o): return self._b("mul", o)
    def __rmul__(self, o): return self._b("mul", o, True)
    def __truediv__(self, o): return self._b("div", o)
    def __rtruediv__(self, o): return self._b("div", o, True)
    def __lt__(self, o): return self._b("lt", o)
    def __le__(self, o): return self._b("le", o)
    def __gt__(self, o): return self._b("gt", o)
    def __ge__(self, o): return self._b("ge", o)
    def __eq__(self, o): return self._b("eq", o)
    def __ne__(self, o): return self._b("ne", o)
    def __and__(self, o): return self._b("and", o)
    def __rand__(self, o): return self._b("and", o, True)
    def __or__(self, o): return self._b("or", o)
    def __ror__(self, o): return self._b("or", o, True)
    def __neg__(self): return self.ctx.op("neg", self)
    def __pos__(self): return self
    def __abs__(self): return self.ctx.op("abs", self)
    def __invert__(self): return self.ctx.op("not", self)

    def __pow__(self, k):
        if isinstance(k, Scalar) or float(k) not in (2.0, 3.0, 4.0):
            raise TypeError("reward programs support ** only with a constant integer exponent of 2, 3 or 4 "
                            "(repeated multiplication)")
        r = self
        for _ in range(int(k) - 1):
            r = r * self
        return r

    # numpy calls the method named like the ufunc on an object scalar: np.exp(x) -> x.exp()
    def sqrt(self): return self.ctx.op("sqrt", self)
    def exp(self): return self.ctx.op("exp", self)
    def log(self): return self.ctx.op("log", self)
    def sin(self): return self.ctx.op("sin", self)
    def cos(self): return self.ctx.op("cos", self)
    def tanh(self): return self.ctx.op("tanh", self)
    def arcsin(self): return self.ctx.op("arcsin", self)
    def arccos(self): return self.ctx.op("arccos", self)
    def arctan2(self, o): return self._b("arctan2", o)
    def square(self): return self * self
    def fabs(self): return abs(self)
    def absolute(self): return abs(self)

    def __repr__(self):
        return f"Scalar({self.v!r})"


_F = np.float64
_NUM = {
    "add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "div": lambda a, b: a / b,
    "arctan2": np.arctan2,
    "lt": lambda a, b: _F(a < b), "le": lambda a, b: _F(a <= b), "gt": lambda a, b: _F(a > b),
    "ge": lambda a, b: _F(a >= b), "eq": lambda a, b: _F(a == b), "ne": lambda a, b: _F(a != b),
    "and": lambda a, b: _F(a != 0 and b != 0), "or": lambda a, b: _F(a != 0 or b != 0),
    "neg": lambda a: -a, "abs": np.abs, "sqrt": np.sqrt, "exp": np.exp, "log": np.log, "sin": np.sin, "cos": np.cos,
    "tanh": np.tanh, "arcsin": np.arcsin, "arccos": np.arccos, "not": lambda a: _F(a == 0),
    "where": lambda c, a, b: a if c != 0 else b,
}


class _Numeric:
    """The numeric twin's context: float64, numpy's libm (what the reference's rewards call)."""

    def lift(self, x):
        if isinstance(x, Scalar):
            return x
        return Scalar(self, _F(x))

    def op(self, name, *args):
        return Scalar(self, _F(_NUM[name](*[a.v for a in args])))


_NUMERIC = _Numeric()


class _Tracer:
    """The tracing context: a DAG of (op, a, b, c) nodes, identical pure nodes shared."""

    def __init__(self, param_keys):
        self.nodes = []           # (op name, a, b, c)
        self.index = {}
        self.consts = []          # float64 values; node ("const", k, 0, 0)
        self.const_index = {}
        self.param_keys = list(param_keys)

    def _node(self, key):
        i = self.index.get(key)
        if i is None:
            i = self.index[key] = len(self.nodes)
            self.nodes.append(key)
        return Scalar(self, i)

    def lift(self, x):
        if isinstance(x, Scalar):
            if x.ctx is not self:
                raise TypeError("a reward-program scalar of another trace (or a number of the numeric twin) was mixed in")
            return x
        if not isinstance(x, (int, float, np.floating, np.integer, bool, np.bool_)):
            raise TypeError(f"reward programs compute on scalars, not on {type(x).__name__}")
        v = float(x)
        bits = np.float64(v).tobytes()
        k = self.const_index.get(bits)
        if k is None:
            k = self.const_index[bits] = len(self.consts)
            self.consts.append(v)
        return self._node(("const", k, 0, 0))

    def param(self, k):
        return self._node(("param", k, 0, 0))

    def load(self, field, idx):
        return self._node(("load", FIELD_ID[field], int(idx), 0))

    def op(self, name, *args):
        ids = [self.lift(a).v for a in args]
        return self._node((name, *ids, *([0] * (3 - len(ids)))))


# ------------------------------------------------------------------ the env_data view and the parameters
class _ComRows:
    """``subtree_com``: only row 0."""

    def __init__(self, row0):
        self._row0 = row0

    def __getitem__(self, i):
        if isinstance(i, (int, np.integer)) and int(i) == 0:
            return self._row0
        raise ValueError("a reward program can read subtree_com[0] only: the batch keeps the root's subtree centre of "
                         "mass (its aux row) and no other body's, so subtree_com[%r] has no device source" % (i,))


class _View:
    """``d``: the env_data fields as object arrays of scalars (built on first access)."""

    def __init__(self, make):
        self._make = make

    def __getattr__(self, name):
        if name not in FIELD_ID:
            raise AttributeError(f"env_data.{name} is not a field a reward program can read (available: "
                                 + ", ".join(ALL_FIELDS) + ")")
        v = self._make(name)
        self.__dict__[name] = v
        return v


def _object_array(vals, shape):
    a = np.empty(len(vals), dtype=object)
    for i, v in enumerate(vals):
        a[i] = v
    return a.reshape(shape)


def _trace_view(tr, dims):
    def make(name):
        shape = _field_shape(name, *dims)
        if shape == ():
            return tr.load(name, 0)
        n = int(np.prod(shape))
        arr = _object_array([tr.load(name, i) for i in range(n)], shape)
        return _ComRows(arr) if name == "subtree_com" else arr
    return _View(make)


def _numeric_view(env_data):
    def make(name):
        if name in REFERENCE_FIELDS and not hasattr(env_data, name):
            raise AttributeError(f"env_data.{name}: this env_data carries no reference sample (HumanoidEnv's data view "
                                 "does with env_config['reference_motion']; elsewhere set ref_qpos / ref_qvel from "
                                 "reference_motion.sample)")
        x = getattr(env_data, name)
        if name == "time":
            return Scalar(_NUMERIC, _F(x))
        a = np.asarray(x, dtype=np.float64)
        if name == "subtree_com":
            a = a[0] if a.ndim == 2 else a
        arr = _object_array([Scalar(_NUMERIC, v) for v in a.reshape(-1)], a.shape)
        return _ComRows(arr) if name == "subtree_com" else arr
    return _View(make)


class _Params(dict):
    def __missing__(self, key):
        raise ValueError(f"unknown reward parameter {key!r} (the program's parameters: {sorted(self)})")


def _merge_params(defaults, overrides, name, kind="reward"):
    vals = dict(defaults)
    for k, v in (overrides or {}).items():
        if k not in defaults:
            raise ValueError(f"unknown parameter {k!r} for {kind} {name!r} (its parameters: {sorted(defaults)})")
        vals[k] = v
    return vals


# ------------------------------------------------------------------ the namespace
def _ctx_of(*xs):
    for x in xs:
        if isinstance(x, Scalar):
            return x.ctx
        if isinstance(x, (np.ndarray, list, tuple)):
            for y in np.asarray(x, dtype=object).reshape(-1):
                if isinstance(y, Scalar):
                    return y.ctx
    return _NUMERIC


def _unary(name):
    def f(x):
        if isinstance(x, (np.ndarray, list, tuple)):
            a = np.asarray(x, dtype=object)
            return _object_array([f(v) for v in a.reshape(-1)], a.shape)
        return getattr(_ctx_of(x).lift(x), name)()
    f.__name__ = name
    f.__doc__ = f"``np.{name}`` on a scalar, or elementwise on an array of scalars."
    return f


sqrt, exp, log, sin, cos, tanh, arcsin, arccos, square = (_unary(n) for n in (
    "sqrt", "exp", "log", "sin", "cos", "tanh", "arcsin", "arccos", "square"))


def arctan2(y, x):
    ctx = _ctx_of(y, x)
    return ctx.op("arctan2", ctx.lift(y), ctx.lift(x))


def where(c, a, b):
    """``a`` where ``c`` holds, else ``b``: a select, both arms are always evaluated."""
    ctx = _ctx_of(c, a, b)
    return ctx.op("where", ctx.lift(c), ctx.lift(a), ctx.lift(b))


def minimum(a, b):
    """Python's ``min(a, b)``: ``b if b < a else a`` (a NaN first operand is returned as is)."""
    ctx = _ctx_of(a, b)
    a, b = ctx.lift(a), ctx.lift(b)
    return where(b < a, b, a)


def maximum(a, b):
    """Python's ``max(a, b)``: ``b if b > a else a``."""
    ctx = _ctx_of(a, b)
    a, b = ctx.lift(a), ctx.lift(b)
    return where(b > a, b, a)


def sum(x):   # noqa: A001 - the namespace mirrors numpy's names
    """``np.sum`` of a list / array of scalars in numpy's pairwise order (see the module docstring)."""
    ctx = _ctx_of(x)
    xs = [ctx.lift(v) for v in np.asarray(x, dtype=object).reshape(-1)]
    n = len(xs)
    if n < 8:
        res = ctx.lift(0.0)
        i = 0
    else:
        nb = n - n % 8
        r = list(xs[:8])
        for i in range(8, nb, 8):
            for j in range(8):
                r[j] = r[j] + xs[i + j]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        i = nb
    for v in xs[i:]:
        res = res + v
    return res


def quaternion_to_euler(quat):
    """utils.py:3-21: (w, x, y, z) -> (roll, pitch, yaw); the pitch is NOT clamped (NaN beyond |sin| = 1)."""
    w, x, y, z = quat
    roll = arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y))
    pitch = arcsin(2 * (w * y - z * x))
    yaw = arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    return roll, pitch, yaw


# ------------------------------------------------------------------ tracing
class TracedProgram:
    """A reward function traced for one model: ``code`` [n, 5] int32 (op, dst, a, b, c), ``consts`` float64,
    ``param_keys`` (the parameter slots' names, in order), ``n_slots`` and the set of ``fields`` read."""

    def __init__(self, code, consts, param_keys, n_slots, fields, outputs=()):
        self.code, self.consts, self.param_keys, self.n_slots, self.fields = code, consts, param_keys, n_slots, fields
        self.outputs = tuple(outputs)     # the component names in dict order; () for a scalar function

    @property
    def n_instr(self):
        return len(self.code)


def _components(ret, lift):
    """What a reward function returned, checked: (total, [(name, scalar), ...]).  A dict is the reward's named
    components, ``"total"`` the reward itself; anything else is the reward alone and has no components."""
    if not isinstance(ret, dict):
        return lift(ret), []
    for k in ret:
        if not isinstance(k, str) or not k:
            raise ValueError(f"reward components: the names must be non-empty str, got {k!r}")
    if "total" not in ret:
        raise ValueError(f'reward components: the dict must contain the key "total" (the reward); got {list(ret)}')
    if len(ret) > MAX_OUTPUTS:
        raise ValueError(f"reward components: {len(ret)} entries, the limit is {MAX_OUTPUTS}")
    comps = [(k, lift(v)) for k, v in ret.items()]
    return dict(comps)["total"], comps


def trace(fn, dims, param_keys=()):
    """Run ``fn(d, p)`` on symbols for a model of ``dims`` = (nq, nv, nu, nbody) and encode it."""
    param_keys = list(param_keys)
    if len(param_keys) > MAX_PARAMS:
        raise ValueError(f"reward program: {len(param_keys)} parameters, the limit is {MAX_PARAMS}")
    tr = _Tracer(param_keys)
    p = _Params({k: tr.param(i) for i, k in enumerate(param_keys)})
    res, comps = _components(fn(_trace_view(tr, tuple(int(x) for x in dims)), p), tr.lift)
    nodes = tr.nodes
    # node -> the indices of the components it is (two names may be bound to one node); an ``out`` is the
    # order entry ("out", node, index): it reads the node's slot and writes none
    outs = {}
    for c, (_, s) in enumerate(comps):
        outs.setdefault(s.v, []).append(c)
    # dead code out: only what the result and the components depend on
    need = np.zeros(len(nodes), dtype=bool)
    stack = [res.v] + list(outs)
    while stack:
        i = stack.pop()
        if need[i]:
            continue
        need[i] = True
        op, *args = nodes[i]
        stack.extend(args[:_ARITY.get(op, 0)])
    # order: computed nodes as the function made them; a leaf (constant, parameter, load) right before its first use
    # a component's ``out`` right after the instruction that produces its value, so that its slot is free again
    # as early as it can be
    order, placed = [], set()

    def place(i):
        placed.add(i)
        order.append(i)
        order.extend(("out", i, c) for c in outs.get(i, ()))
    for i, (op, *args) in enumerate(nodes):
        if not need[i] or op in ("const", "param", "load"):
            continue
        for a in args[:_ARITY[op]]:
            if a not in placed and nodes[a][0] in ("const", "param", "load"):
                place(a)
        place(i)
    for i in outs:                      # a component that is a bare leaf nothing else uses
        if i not in placed:
            place(i)
    if res.v not in placed:
        order.append(res.v)
    if len(order) + 1 > MAX_INSTR:
        raise ValueError(f"reward program: {len(order) + 1} instructions, the limit is {MAX_INSTR}")
    last = {}
    for pos, i in enumerate(order):
        if isinstance(i, tuple):        # an out keeps its value's slot alive until here
            last[i[1]] = pos
            continue
        op, *args = nodes[i]
        for a in args[:_ARITY.get(op, 0)]:
            last[a] = pos
    last[res.v] = len(order)
    # value slots by liveness: an operand's slot is free again at its last use (the destination may take it:
    # an instruction reads before it writes)
    const_map, consts = {}, []
    slot, free, n_slots = {}, [], 0
    code = np.zeros((len(order) + 1, 5), dtype=np.int32)
    for pos, i in enumerate(order):
        if isinstance(i, tuple):
            code[pos] = [OP["out"], 0, slot[i[1]], i[2], 0]
            if last[i[1]] == pos:
                free.append(slot.pop(i[1]))
            continue
        op, *args = nodes[i]
        ar = _ARITY.get(op, 0)
        ops = [slot[a] for a in args[:ar]]
        for a in set(args[:ar]):
            if last[a] == pos:
                free.append(slot.pop(a))
        if free:
            free.sort(reverse=True)
            s = free.pop()
        else:
            s = n_slots
            n_slots += 1
            if n_slots > MAX_SLOTS:
                raise ValueError(f"reward program: more than {MAX_SLOTS} values alive at once (at instruction {pos} of "
                                 f"{len(order)}); the limit is {MAX_SLOTS} live values -- reduce sums as you go")
        slot[i] = s
        if op == "const":
            k = const_map.get(args[0])
            if k is None:
                k = const_map[args[0]] = len(consts)
                consts.append(tr.consts[args[0]])
            row = [k, 0, 0]
        elif op in ("param", "load"):
            row = list(args)
        else:
            row = ops + [0] * (3 - ar)
        code[pos] = [OP[op], s] + row
    if len(consts) > MAX_CONSTS:
        raise ValueError(f"reward program: {len(consts)} constants, the limit is {MAX_CONSTS}")
    code[len(order)] = [OP["result"], 0, slot[res.v], 0, 0]
    fields = sorted({_FIELD_NAME[nodes[i][1]] for i in order if not isinstance(i, tuple) and nodes[i][0] == "load"})
    return TracedProgram(code, np.asarray(consts, dtype=np.float64), param_keys, max(n_slots, 1), fields,
                         [k for k, _ in comps])


# ------------------------------------------------------------------ registration
class DeviceReward:
    """The record of a device-capable reward: its function, parameter defaults, numeric twin, and the
    traces / native programs made of it per model."""

    kind = "reward"
    components_allowed = True      # a function may return a dict of named components (DeviceTermination: no)

    def __init__(self, name, fn, defaults):
        self.name = name
        self.fn = fn
        self.defaults = {k: float(v) for k, v in (defaults or {}).items()}
        self.param_keys = list(self.defaults)
        self._traced = {}
        self._compiled = {}
        self._names = None

        def twin(env_data, params=None):
            return self._twin_value(self.twin_with_components(env_data, params)[0])
        twin.__name__ = getattr(fn, "__name__", name)
        twin.__doc__ = fn.__doc__
        twin.device_reward = self
        self.twin = twin

    @staticmethod
    def _twin_value(v):
        return v

    def twin_with_components(self, env_data, params=None):
        """The function on numbers, one evaluation: (the twin's value before ``_twin_value``, a float;
        ``{component name: float}``, empty for a function that returns a scalar)."""
        vals = _merge_params(self.defaults, params, self.name, self.kind)
        p = _Params({k: Scalar(_NUMERIC, _F(v)) for k, v in vals.items()})
        with np.errstate(all="ignore"):
            total, comps = _components(self.fn(_numeric_view(env_data), p), _NUMERIC.lift)
        self._note_names([k for k, _ in comps])
        return float(total.v), {k: float(s.v) for k, s in comps}

    def _note_names(self, names):
        if names and not self.components_allowed:
            raise ValueError(f"{self.kind} {self.name!r} returns a dict of components {list(names)}: a termination "
                             "predicate is one truth value and has no components")
        self._names = tuple(names)

    def twin_components(self, env_data, params=None):
        """The named components ``{name: float}`` of the reward on ``env_data``, evaluated in the numeric twin's
        context: ``twin_components(d)["total"]`` is the twin's own return value, bit for bit.  ``{}`` for a
        function that returns a scalar."""
        return self.twin_with_components(env_data, params)[1]

    @property
    def component_names(self):
        """The component names in dict order, a tuple; () for a function that returns a scalar.  Known from the
        function's last trace or evaluation; before either, from a trace for the packaged humanoid's dimensions."""
        if self._names is None:
            self.trace((28, 27, 21, 17))
        return self._names

    def params(self, overrides=None):
        """The parameter values in slot order: the defaults overlaid with ``overrides`` (unknown key: ValueError)."""
        vals = _merge_params(self.defaults, overrides, self.name, self.kind)
        return np.asarray([float(vals[k]) for k in self.param_keys], dtype=np.float64)

    def trace(self, dims):
        dims = tuple(int(x) for x in dims)
        t = self._traced.get(dims)
        if t is None:
            t = trace(self.fn, dims, self.param_keys)
            self._note_names(t.outputs)
            self._traced[dims] = t
        return t

    def compile(self, model):
        """The native program (``hs_reward_program_create``) for ``model``, made once per model."""
        c = self._compiled.get(id(model))
        if c is None or c.model is not model:
            c = self._compiled[id(model)] = CompiledProgram(self, model)
        return c


class CompiledProgram:
    """A validated native reward program of one model (``hs_reward_program_*``)."""

    def __init__(self, reward, model):
        from ._lib import check, lib
        self.reward = reward
        self.model = model
        self.traced = t = reward.trace((model.nq, model.nv, model.nu, model.nbody))
        self.fields = t.fields
        self.outputs = t.outputs            # the component names, row by row of the [C, N] component tensors
        code = np.ascontiguousarray(t.code, dtype=np.int32)
        h = C.c_void_p()
        check(lib().hs_reward_program_create_components(model.handle, code.ctypes.data, len(code),
                                                        t.consts.ctypes.data if len(t.consts) else None, len(t.consts),
                                                        len(t.param_keys), len(t.outputs), C.byref(h)))
        self.handle = h
        self._pcache = {}

    def params(self, overrides=None):
        """A ctypes double array of the parameter slots (None when the program has none)."""
        key = tuple(sorted((overrides or {}).items()))
        a = self._pcache.get(key)
        if a is None:
            v = self.reward.params(overrides)
            a = self._pcache[key] = (C.c_double * max(len(v), 1))(*v)
        return a

    def eval_host(self, fields, params=None, components=False, reference=None):
        """The program interpreted on the CPU (``hs_reward_program_eval_host``): ``fields`` maps field names to
        float64 arrays [n, ...] (``subtree_com``: [n, 3] or [n, nbody, 3], row 0 is used); returns [n] float64.
        ``components=True``: (reward [n], components [C, n]), the rows in the order of ``self.outputs``.
        ``reference``: for a program that reads ``ref_qpos`` / ``ref_qvel``, a dict ``{"motion":
        reference_motion.Reference, "episode": [n] (start "drawn" only), "seed": int or [n], "env": [n] or None,
        "dtype": np.float64 | np.float32}`` -- the sample is taken at ``fields["time"]``
        (``hs_reward_program_eval_host_reference``); without it such a program is refused."""
        from . import _lib
        f, keep, n = self._host_fields(fields, with_time=reference is not None)
        out = np.zeros(n, dtype=np.float64)
        if reference is not None:
            ref, keep_ref = self._host_reference(reference, n)
            comp = np.zeros((len(self.outputs), n), dtype=np.float64)
            _lib.check(_lib.lib().hs_reward_program_eval_host_reference(
                self.handle, self.params(params), n, C.byref(f), C.byref(ref), out.ctypes.data,
                comp.ctypes.data if components and comp.size else None))
            return (out, comp) if components else out
        if not components:
            _lib.check(_lib.lib().hs_reward_program_eval_host(self.handle, self.params(params), n, C.byref(f),
                                                             out.ctypes.data))
            return out
        comp = np.zeros((len(self.outputs), n), dtype=np.float64)
        _lib.check(_lib.lib().hs_reward_program_eval_host_components(
            self.handle, self.params(params), n, C.byref(f), out.ctypes.data, comp.ctypes.data if comp.size else None))
        return out, comp

    @staticmethod
    def _host_reference(reference, n):
        """The ``hs_reference_host`` of ``eval_host``'s ``reference`` dict, and the arrays it points into."""
        from . import _lib
        unknown = sorted(set(reference) - {"motion", "episode", "seed", "env", "dtype"})
        if unknown or "motion" not in reference:
            raise ValueError(f"reference: a dict with 'motion' and optionally 'episode', 'seed', 'env', 'dtype'; "
                             f"got {sorted(reference)}")
        m = reference["motion"]
        dt = np.dtype(reference.get("dtype", np.float64))
        if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError(f"reference: dtype must be float64 or float32, got {dt}")
        # the rows as a batch of that dtype holds them
        keep = [np.ascontiguousarray(m.qpos.astype(dt).astype(np.float64)),
                np.ascontiguousarray(m.qvel.astype(dt).astype(np.float64))]
        ep = seed = env = None
        if reference.get("episode") is not None:
            ep = np.ascontiguousarray(np.broadcast_to(np.asarray(reference["episode"], dtype=np.int64), (n,)),
                                      dtype=np.int32)
        if m.start == "drawn":
            if ep is None:
                raise ValueError("reference: start='drawn' needs 'episode'")
            s = np.broadcast_to(np.asarray(reference.get("seed", 0), dtype=object), (n,))
            seed = np.array([int(x) & (2 ** 64 - 1) for x in s], dtype=np.uint64)
        if reference.get("env") is not None:
            env = np.ascontiguousarray(np.broadcast_to(np.asarray(reference["env"], dtype=np.int64), (n,)),
                                       dtype=np.int32)
        keep += [ep, seed, env]
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        ref = _lib.hs_reference_host(n_rows=m.K, qpos=ptr(keep[0]), qvel=ptr(keep[1]),
                                     key_dt=1.0 if m.key_dt is None else m.key_dt, flags=m.flags,
                                     precision=_lib.HS_FP32 if dt == np.dtype(np.float32) else _lib.HS_FP64,
                                     episode=ptr(ep), seed=ptr(seed), env=ptr(env))
        return ref, keep

    def _host_fields(self, fields, with_time=False):
        from . import _lib
        keep, n = {}, None
        names = [k for k in self.fields if k not in REFERENCE_FIELDS]
        if with_time and "time" not in names:     # a reference is sampled at the state's time
            names.append("time")
        for name in names:
            a = np.asarray(fields[name], dtype=np.float64)
            if name == "subtree_com" and a.ndim == 3:
                a = a[:, 0]
            keep[name] = a = np.ascontiguousarray(a)
            n = len(a)
        if n is None:
            n = len(next(iter(fields.values())))
        f = _lib.hs_reward_fields(**{_lib.REWARD_FIELD_MEMBER[k]: v.ctypes.data for k, v in keep.items()})
        return f, keep, n

    def termination_eval_host(self, fields, episode, count, episode_tag, params=None, grace_steps=1, reference=None):
        """The program as a termination predicate on the CPU (``hs_termination_eval_host``): the predicate on n
        states (``fields`` as for ``eval_host``) and one grace-counter update per state.  ``episode`` [n] int32 are
        the envs' current episode numbers; ``count`` and ``episode_tag`` [n] int32 (contiguous) are read and
        UPDATED IN PLACE.  Returns the [n] bool array of the envs whose episode ends.  ``reference``: as for
        ``eval_host`` (``hs_termination_eval_host_reference``)."""
        from . import _lib
        f, keep, n = self._host_fields(fields, with_time=reference is not None)
        episode = np.ascontiguousarray(episode, dtype=np.int32)
        for a in (count, episode_tag):
            if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous and a.shape == (n,)):
                raise ValueError(f"count / episode_tag: contiguous int32 arrays of shape ({n},)")
        if episode.shape != (n,):
            raise ValueError(f"episode: shape ({n},)")
        early = np.zeros(n, dtype=np.uint8)
        if reference is not None:
            ref, keep_ref = self._host_reference(reference, n)
            _lib.check(_lib.lib().hs_termination_eval_host_reference(
                self.handle, self.params(params), int(grace_steps), n, C.byref(f), C.byref(ref), episode.ctypes.data,
                count.ctypes.data, episode_tag.ctypes.data, early.ctypes.data))
            return early != 0
        _lib.check(_lib.lib().hs_termination_eval_host(self.handle, self.params(params), int(grace_steps), n,
                                                      C.byref(f), episode.ctypes.data, count.ctypes.data,
                                                      episode_tag.ctypes.data, early.ctypes.data))
        return early != 0

    def close(self):
        h, self.handle = self.handle, None
        if h:
            from ._lib import lib
            lib().hs_reward_program_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_BY_TWIN = {}


def register_device_reward(name, fn=None, defaults=None, registry=None):
    """Register ``fn(d, p)`` as the reward ``name``: its numeric twin ``(env_data, params=None)`` goes into
    ``REWARD_FUNCTIONS`` (or ``registry``) and the function is recorded as device-capable.  Usable as a decorator:
    ``@register_device_reward("name", defaults={...})``.  Returns ``fn``."""
    if fn is None:
        return lambda f: register_device_reward(name, f, defaults, registry)
    rec = DeviceReward(name, fn, defaults)
    reg = _rf.REWARD_FUNCTIONS if registry is None else registry
    reg[name] = rec.twin
    _BY_TWIN[rec.twin] = rec
    return fn


def device_reward_program(name, registry=None):
    """The ``DeviceReward`` record of ``REWARD_FUNCTIONS[name]``, or None when that entry is a built-in or a plain
    host callable.  Unknown names raise ValueError like custom_env.py:268-269."""
    reg = _rf.REWARD_FUNCTIONS if registry is None else registry
    if name not in reg:
        if registry is None and name in _rf.PROGRAM_REWARDS:      # the package's own program rewards ("track")
            return _BY_TWIN.get(_rf.PROGRAM_REWARDS[name])
        raise ValueError(f"Unknown reward type: {name}")
    return _BY_TWIN.get(reg[name])


# ------------------------------------------------------------------ termination conditions
# The fall conditions the reference holds commented out (custom_env.py:167-200): a predicate written in this
# language, evaluated on the device after every env step (hs_set_termination); when it has held for
# ``grace_steps`` consecutive env steps of an episode, the step returns terminated = True and the env resets.
TERMINATION_FUNCTIONS = {}


class DeviceTermination(DeviceReward):
    """The record of a termination condition: a ``DeviceReward`` whose value is read as a truth value --
    terminated iff the result is non-zero and not NaN (a comparison with a NaN is false, as in Python)."""

    kind = "termination"
    components_allowed = False     # a dict-returning predicate raises ValueError when traced or evaluated

    @staticmethod
    def _twin_value(v):
        return bool(v != 0.0 and v == v)


def register_device_termination(name, fn=None, defaults=None, registry=None):
    """Register ``fn(d, p)`` as the termination condition ``name``, the counterpart of ``register_device_reward``:
    the same ``env_data`` view ``d`` and parameter dict ``p``, the same tracer and limits.  Its numeric twin
    ``(env_data, params=None) -> bool`` goes into ``TERMINATION_FUNCTIONS`` (or ``registry``).  Usable as a
    decorator.  Returns ``fn``."""
    if fn is None:
        return lambda f: register_device_termination(name, f, defaults, registry)
    rec = DeviceTermination(name, fn, defaults)
    reg = TERMINATION_FUNCTIONS if registry is None else registry
    reg[name] = rec.twin
    _BY_TWIN[rec.twin] = rec
    return fn


def device_termination(name, registry=None):
    """The ``DeviceTermination`` record of ``TERMINATION_FUNCTIONS[name]``; an unknown type raises ValueError like
    an unknown reward type."""
    reg = TERMINATION_FUNCTIONS if registry is None else registry
    rec = _BY_TWIN.get(reg[name]) if name in reg else None
    if rec is None:
        raise ValueError(f"Unknown termination type: {name}")
    return rec


# the built-in conditions the step kernel's fused instances evaluate themselves (include/hsim.h HS_TERM_*,
# csrc/hs_term_builtin.h): the registered function -> its kind
TERM_FALLEN, TERM_LOST_BALANCE = 1, 2


def builtin_termination_kind(rec):
    """HS_TERM_FALLEN / HS_TERM_LOST_BALANCE when ``rec`` is the record of one of the two registered built-ins
    (the function itself, under whatever name), else None."""
    return {fallen: TERM_FALLEN, lost_balance: TERM_LOST_BALANCE}.get(rec.fn)


def builtin_termination_eval_host(kind, qpos, min_height=0.8, max_roll_pitch=np.pi / 4):
    """The built-in predicate ``kind`` on the rows of ``qpos`` [n, >= 7] float64 (``hs_termination_builtin_eval_host``:
    the function the fused kernel instances run, on the CPU, needing no batch and no GPU).  Returns [n] bool."""
    from . import _lib
    q = np.ascontiguousarray(qpos, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] < 7:
        raise ValueError("builtin_termination_eval_host: qpos must be [n, >= 7]")
    out = np.zeros(len(q), dtype=np.uint8)
    _lib.check(_lib.lib().hs_termination_builtin_eval_host(int(kind), float(min_height), float(max_roll_pitch), len(q),
                                                          q.ctypes.data, q.shape[1], out.ctypes.data))
    return out != 0


def termination_fused_from_config(termination, registry=None):
    """The ``"fused"`` flag of ``env_config["termination"]`` (default False), checked: a non-bool, or True with a
    condition that is not one of the two registered built-ins, raises ValueError.  None config: False."""
    if termination is None:
        return False
    checked = termination_from_config(termination, registry)
    fused = termination.get("fused", False)
    if not isinstance(fused, (bool, np.bool_)):
        raise ValueError(f"termination: fused must be a bool, got {fused!r}")
    if fused and builtin_termination_kind(checked[0]) is None:
        raise ValueError(f"termination: fused=True needs one of the built-in conditions 'fallen' / 'lost_balance': "
                         f"{checked[0].name!r} is a user-registered predicate, which only the interpreter of the "
                         "per-step path can evaluate")
    return bool(fused)


def termination_from_config(termination, registry=None):
    """``env_config["termination"]`` -- ``{"type": name, "params": {...}, "grace_steps": k, "fused": bool}`` or None
    -- checked: returns (record, parameter overrides, grace_steps) or None.  Unknown type, unknown parameter key or a
    grace period that is not an integer >= 1: ValueError.  The ``"fused"`` flag is ``termination_fused_from_config``'s."""
    if termination is None:
        return None
    if not isinstance(termination, dict) or "type" not in termination:
        raise ValueError('termination: expected {"type": name, "params": {...}, "grace_steps": k} or None')
    unknown = set(termination) - {"type", "params", "grace_steps", "fused"}
    if unknown:
        raise ValueError(f"termination: unknown key(s) {sorted(unknown)}")
    if not isinstance(termination.get("fused", False), (bool, np.bool_)):
        raise ValueError(f"termination: fused must be a bool, got {termination['fused']!r}")
    rec = device_termination(termination["type"], registry)
    params = termination.get("params") or None
    rec.params(params)
    g = termination.get("grace_steps", 1)
    if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or g < 1:
        raise ValueError(f"termination: grace_steps must be an integer >= 1, got {g!r}")
    return rec, params, int(g)


@register_device_termination("fallen", defaults={"min_height": 0.8})
def fallen(d, p):
    """custom_env.py:169 (and reward_functions.py's own ``height < 0.8``): the torso is below ``min_height``."""
    return d.qpos[2] < p["min_height"]


@register_device_termination("lost_balance", defaults={"min_height": 0.8, "max_roll_pitch": np.pi / 4})
def lost_balance(d, p):
    """custom_env.py:183-200: fallen, or rolled / pitched beyond ``max_roll_pitch`` (45 degrees).  The pitch is
    the unclamped ``arcsin`` of ``quaternion_to_euler``: a NaN pitch compares false and does not terminate."""
    roll, pitch, _ = quaternion_to_euler(d.qpos[3:7])
    return (d.qpos[2] < p["min_height"]) | (abs(roll) > p["max_roll_pitch"]) | (abs(pitch) > p["max_roll_pitch"])


# ------------------------------------------------------------------ reference-motion targets
# Written over d.ref_qpos / d.ref_qvel (reference_motion.py): they need a reference motion bound to the batch
# (env_config["reference_motion"], HsBatch.set_reference_motion) and run on the program path -- three launches per
# step, rollout_handle() None -- like any user program.  "track" is registered in reward_functions.PROGRAM_REWARDS,
# which every lookup by name consults after REWARD_FUNCTIONS (that one keeps the reference's four keys).
TRACK_DEFAULTS = {"k_pose": 2.0, "k_vel": 0.1, "k_root": 5.0, "w_pose": 0.5, "w_vel": 0.1, "w_root": 0.4}


@register_device_reward("track", defaults=TRACK_DEFAULTS, registry=_rf.PROGRAM_REWARDS)
def track(d, p):
    """Follow the reference motion (DeepMimic-style exponentials of squared errors), components ``pose``,
    ``velocity``, ``root``, ``total``:

        pose     = exp(-k_pose sum((qpos[7:] - ref_qpos[7:])^2))          the joint angles
        velocity = exp(-k_vel  sum((qvel[6:] - ref_qvel[6:])^2))          the joint velocities
        root     = exp(-k_root (sum((qpos[:3] - ref_qpos[:3])^2) + 1 - (q . q_ref)^2 / sum(q_ref^2)))
        total    = w_pose pose + w_vel velocity + w_root root

    ``q`` is the root quaternion (unit: the step normalises it); the interpolated ``q_ref`` is not renormalised, so
    its squared norm divides.  Every constant is a parameter.  The defaults are a starting point, not a tuned
    claim: nothing has been trained with them."""
    pose = exp(-p["k_pose"] * sum(square(d.qpos[7:] - d.ref_qpos[7:])))
    velocity = exp(-p["k_vel"] * sum(square(d.qvel[6:] - d.ref_qvel[6:])))
    q, qr = d.qpos[3:7], d.ref_qpos[3:7]
    dot = sum(q * qr)
    root = exp(-p["k_root"] * (sum(square(d.qpos[:3] - d.ref_qpos[:3])) + 1.0 - dot * dot / sum(square(qr))))
    return {"pose": pose, "velocity": velocity, "root": root,
            "total": p["w_pose"] * pose + p["w_vel"] * velocity + p["w_root"] * root}


@register_device_termination("off_track", defaults={"max_root_dist": 0.5})
def off_track(d, p):
    """The root has drifted more than ``max_root_dist`` from the reference's: sum((qpos[:3] - ref_qpos[:3])^2) >
    max_root_dist^2.  With ``grace_steps`` the drift must last that many env steps."""
    return sum(square(d.qpos[:3] - d.ref_qpos[:3])) > p["max_root_dist"] ** 2


# ------------------------------------------------------------------ the built-in rewards, restated
KNEEL_DEFAULTS = {'target_height': 1.282, 'min_height': 0.85, 'max_roll_pitch': np.pi / 6, 'com_radius': 0.1,
                  'energy_weight': 0.3, 'posture_weight': 0.3, 'com_weight': 0.2, 'foot_weight': 0.1,
                  'alive_weight': 0.1}


def kneeling_program(d, p):
    """reward_functions.py:66-154 (``robust_kneeling_reward``) in the language."""
    return kneeling_components_program(d, p)["total"]


def stand_program(d, p):
    """reward_functions.py:156-211 (``stand_reward``, the 'default' and 'stand' entries) in the language."""
    return stand_components_program(d, p)["total"]


def walk_program(d, p):
    """reward_functions.py:213-261 (``walk_reward``) in the language."""
    return walk_components_program(d, p)["total"]


# The same three with their terms named: the reference's own term names (reward_functions.py's velocity_reward,
# posture_reward, foot_reward, torque_penalty, ... without the suffix), each the UNWEIGHTED term as the reference
# computes it, and "total" the reward -- the very expression the *_program functions above return.  They are not
# registry entries either; reward_config={"type": "stand", "components": True} selects one (components_reward).
def kneeling_components_program(d, p):
    """``kneeling_program`` with its terms: posture, com, foot, energy, alive (each before its weight), total."""
    qpos, qvel = d.qpos, d.qvel
    h = qpos[2]
    roll, pitch, _ = quaternion_to_euler(qpos[3:7])
    orientation_error = (roll ** 2 + pitch ** 2) / (p['max_roll_pitch'] ** 2)
    posture = 0.7 * exp(-5.0 * orientation_error) + 0.3 * exp(-5.0 * square(h - p['target_height']))
    com_pos, com_vel = d.subtree_com[0], d.subtree_linvel[0]
    dist = sqrt(com_pos[0] ** 2 + com_pos[1] ** 2)
    com = 0.7 * exp(-10.0 * (dist / p['com_radius'])) + 0.3 * exp(-0.1 * sum(com_vel ** 2))
    lf, rf = sum(abs(d.cfrc_ext[-2])), sum(abs(d.cfrc_ext[-1]))
    foot = minimum(lf, rf) / (lf + rf + 1e-8)
    av = qvel[6:]
    af = d.qfrc_actuator[-len(av):]
    energy = exp(-0.01 * sum(square(af * av)))
    alive = 1.0 - exp(-0.5 * d.time)
    total = (p['posture_weight'] * posture + p['com_weight'] * com + p['foot_weight'] * foot +
             p['energy_weight'] * energy + p['alive_weight'] * alive)
    return {"posture": posture, "com": com, "foot": foot, "energy": energy, "alive": alive,
            "total": where(h < p['min_height'], h ** 2, total)}


def stand_components_program(d, p):
    """``stand_program`` with its terms: velocity, posture, foot, torque (weights 0.4, 0.3, 0.2, 0.1), total."""
    h = d.qpos[2]
    vx = d.qvel[0]
    roll, pitch, _ = quaternion_to_euler(d.qpos[3:7])
    lf, rf = sum(abs(d.cfrc_ext[-2])), sum(abs(d.cfrc_ext[-1]))
    vel = exp(-2.0 * ((vx - 1.0) ** 2))
    posture = 0.5 * exp(-2.0 * ((h - 1.282) ** 2)) + 0.5 * exp(-3.0 * (roll ** 2 + pitch ** 2))
    torque = exp(-0.05 * sum(square(d.ctrl)))
    foot = 1.0 - minimum(lf, rf) / (lf + rf + 1e-8)
    reward = 0.4 * vel + 0.3 * posture + 0.2 * foot + 0.1 * torque
    return {"velocity": vel, "posture": posture, "foot": foot, "torque": torque, "total": where(h < 0.8, 0.0, reward)}


def walk_components_program(d, p):
    """``walk_program`` with its terms: velocity, posture, torque (total = velocity + posture * torque), total."""
    h = d.qpos[2]
    vx = d.qvel[0]
    roll, pitch, _ = quaternion_to_euler(d.qpos[3:7])
    vel = exp(-0.5 * ((vx - 10.0) ** 2))
    posture = 0.5 * exp(-2.0 * ((h - 1.282) ** 2)) + 0.5 * exp(-3.0 * (roll ** 2 + pitch ** 2))
    torque = exp(-0.05 * sum(square(d.ctrl)))
    return {"velocity": vel, "posture": posture, "torque": torque,
            "total": where(h < 0.8, 0.1 * h / 0.8, vel + posture * torque)}


COMPONENT_PROGRAMS = {"default": (stand_components_program, None), "stand": (stand_components_program, None),
                      "kneeling": (kneeling_components_program, KNEEL_DEFAULTS),
                      "walk": (walk_components_program, None)}
_COMPONENT_RECORDS = {}


def components_reward(rtype):
    """The ``DeviceReward`` record of the built-in reward ``rtype`` with its terms named -- what
    ``reward_config={"type": rtype, "components": True}`` runs, on the program path (hs_step_program: three
    launches per step, never a fused launch).  The records are kept here, not in ``REWARD_FUNCTIONS``, whose keys
    stay the reference's four.  A type without a breakdown raises ValueError."""
    if rtype not in COMPONENT_PROGRAMS:
        raise ValueError(f'reward_config "components": True needs one of the built-in types {sorted(COMPONENT_PROGRAMS)} '
                         f"(got {rtype!r}); a registered program reward has components when its function returns a dict")
    rec = _COMPONENT_RECORDS.get(rtype)
    if rec is None:
        fn, defaults = COMPONENT_PROGRAMS[rtype]
        rec = _COMPONENT_RECORDS[rtype] = DeviceReward(rtype, fn, defaults)
    return rec


# (The *_program functions are worked examples and the feature's yardstick, not registry entries: REWARD_FUNCTIONS
# keeps the reference's four keys, whose built-in names run inside the step kernel.  To use one as a program:
# register_device_reward("stand_program", stand_program), and for kneeling defaults=KNEEL_DEFAULTS; the breakdowns
# are reached through reward_config["components"], or registered the same way under a name of your own.)
