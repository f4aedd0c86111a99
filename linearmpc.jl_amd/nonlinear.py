"""A nonlinear true plant for the scenario loop: a Python function of (x, u, d, q), traced ONCE into the straight-line
program `lmpc_plant_program` of include/lmpc_hip.h, which `lmpc_simulate_scenario_nonlinear_device` interprets on the
GPU, one scenario per lane.  The program is data: nothing is compiled at run time.

    plant = NonlinearPlant(f, nx, nu, nd=0, nq=0, Ts=0.01)      # x+ = x + Ts * f(x, u, d, q)   (reference model.jl:87)
    plant = NonlinearPlant(f, nx, nu)                           # Ts=None: f returns x+ itself
    Simulation(mpc, scenario, plant, params=q)                  # q: (nq,) shared or (N_scen, nq)

`f` receives four lists of traced values and returns nx expressions built from them with + - * /, unary minus, `**` by
a small non-negative integer (left-to-right products) and this module's `sin cos fma minimum maximum abs_` (also
reachable as `abs(value)`).  Every operation becomes ONE binary64 operation of the program, in the order written: the
tracer never reorders or reassociates.  It merges structurally identical operations (same opcode, same operands in the
same order) and folds an operation whose operands are all constants -- both leave every bit of the result unchanged,
the fold being computed with the same restated operations the interpreter runs.  Slots are allocated by liveness.
Anything else -- a comparison or `if` on a traced value, a numpy ufunc, sqrt / exp / tanh -- raises `TraceError`
naming the operation.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import struct

import numpy as np

__all__ = ["NonlinearPlant", "TraceError", "sin", "cos", "fma", "minimum", "maximum", "abs_", "OPS", "MAX_INS",
           "MAX_SLOTS", "MAX_CONSTS"]

OPS = {"LOADX": 1, "LOADU": 2, "LOADD": 3, "LOADQ": 4, "CONST": 5, "ADD": 6, "SUB": 7, "MUL": 8, "DIV": 9, "NEG": 10,
       "ABS": 11, "FMA": 12, "MIN": 13, "MAX": 14, "SIN": 15, "COS": 16}
MAX_INS, MAX_SLOTS, MAX_CONSTS = 1024, 64, 256
_LOADS = ("LOADX", "LOADU", "LOADD", "LOADQ")

def _load_libm():
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lib.fma.restype = ctypes.c_double
    lib.fma.argtypes = [ctypes.c_double] * 3
    lib.rint.restype = ctypes.c_double
    lib.rint.argtypes = [ctypes.c_double]
    return lib


_libm = _load_libm()


class TraceError(TypeError):
    """An operation the plant program cannot express; the message starts with the operation's name."""


def _bits(h):
    return struct.unpack("<d", struct.pack("<Q", h))[0]


# the constants of sin_ / cos_ as include/lmpc_hip.h lists them
_TWO_OVER_PI = _bits(0x3FE45F306DC9C883)
_P = tuple(_bits(h) for h in (0x3FF921FB54400000, 0x3DD0B4611A600000, 0x3BA3198A2E037073))
_S = tuple(_bits(h) for h in (0xBFC5555555555549, 0x3F8111111110F8A6, 0xBF2A01A019C161D5, 0x3EC71DE357B1FE7D,
                              0xBE5AE5E68A2B9CEB, 0x3DE5D93A5ACFD57C))
_C = tuple(_bits(h) for h in (0x3FA555555555554C, 0xBF56C16C16C15177, 0x3EFA01A019CB1590, 0xBE927E4F809C52AD,
                              0x3E21EE9EBDB4B1C4, 0xBDA8FAE9BE8838D4))


def _sincos(t):
    """the header's sequence on one Python float (used to fold sin / cos of a constant): sn, cs, m"""
    f, np64 = _libm.fma, np.float64
    with np.errstate(all="ignore"):
        t = np64(t)
        kd = np64(_libm.rint(float(t * np64(_TWO_OVER_PI))))
        r = t
        for p in _P:
            r = np64(f(float(-kd), p, float(r)))
        z = r * r
        ps = np64(_S[5])
        for c in _S[4::-1]:
            ps = np64(f(float(ps), float(z), c))
        sn = np64(f(float(r * z), float(ps), float(r)))
        pc = np64(_C[5])
        for c in _C[4::-1]:
            pc = np64(f(float(pc), float(z), c))
        hz = np64(0.5) * z
        w = np64(1.0) - hz
        cs = w + np64(f(float(z * z), float(pc), float((np64(1.0) - w) - hz)))
        m = kd - np64(4.0) * np64(_libm.rint(float(np64(0.25) * kd)))
    return float(sn), float(cs), float(m)


def _fold(op, vals):
    """one program operation on Python floats, bit for bit what the interpreter computes"""
    a = np.float64(vals[0])
    b = np.float64(vals[1]) if len(vals) > 1 else None
    with np.errstate(all="ignore"):
        if op == "ADD":
            return float(a + b)
        if op == "SUB":
            return float(a - b)
        if op == "MUL":
            return float(a * b)
        if op == "DIV":
            return float(a / b)
        if op == "NEG":
            return float(-a)
        if op == "ABS":
            return float(np.abs(a))
        if op == "FMA":
            return float(_libm.fma(*[float(v) for v in vals]))
        if op == "MIN":
            return float(a) if a < b else float(b)
        if op == "MAX":
            return float(a) if a > b else float(b)
        sn, cs, m = _sincos(a)
        if op == "SIN":
            return sn if m == 0 else cs if m == 1 else -cs if m == -1 else -sn
        return cs if m == 0 else -sn if m == 1 else sn if m == -1 else -cs


class _Tracer:
    """the graph under construction: nodes are (op, operands) with operands node ids (or an index for loads, a bit
    pattern for constants); identical nodes are one node"""

    def __init__(self):
        self.nodes, self.index = [], {}

    def node(self, op, args):
        key = (op, args)
        if key not in self.index:
            self.index[key] = len(self.nodes)
            self.nodes.append(key)
        return Value(self, self.index[key])

    def const(self, v):
        return self.node("CONST", (struct.pack("<d", float(v)),))           # keyed by bits: -0.0 is not +0.0

    def value_of(self, nid):
        op, args = self.nodes[nid]
        return struct.unpack("<d", args[0])[0] if op == "CONST" else None

    def lift(self, v, opname):
        if isinstance(v, Value):
            if v.tr is not self:
                raise TraceError(f"{opname}: operand comes from another trace")
            return v
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TraceError(f"{opname}: operand of type {type(v).__name__} is not a traced value or a real number")
        return self.const(float(v))

    def apply(self, op, *operands):
        vs = [self.lift(v, op) for v in operands]
        consts = [self.value_of(v.nid) for v in vs]
        if all(c is not None for c in consts):
            return self.const(_fold(op, consts))
        return self.node(op, tuple(v.nid for v in vs))


def _refuse(name):
    def method(self, *a, **k):
        raise TraceError(f"{name}: not an operation of the plant program")
    return method


class Value:
    """A traced binary64 value."""
    __slots__ = ("tr", "nid")
    __array_priority__ = 1000.0

    def __init__(self, tr, nid):
        self.tr, self.nid = tr, nid

    def __add__(self, o): return self.tr.apply("ADD", self, o)
    def __radd__(self, o): return self.tr.apply("ADD", o, self)
    def __sub__(self, o): return self.tr.apply("SUB", self, o)
    def __rsub__(self, o): return self.tr.apply("SUB", o, self)
    def __mul__(self, o): return self.tr.apply("MUL", self, o)
    def __rmul__(self, o): return self.tr.apply("MUL", o, self)
    def __truediv__(self, o): return self.tr.apply("DIV", self, o)
    def __rtruediv__(self, o): return self.tr.apply("DIV", o, self)
    def __neg__(self): return self.tr.apply("NEG", self)
    def __pos__(self): return self
    def __abs__(self): return self.tr.apply("ABS", self)

    def __pow__(self, n, mod=None):
        if mod is not None or isinstance(n, (bool, Value)) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= 16:
            raise TraceError("pow: the exponent must be an integer constant in 0 .. 16")
        if n == 0:
            return self.tr.const(1.0)
        out = self
        for _ in range(int(n) - 1):                   # ((x * x) * x) * ...: left to right
            out = out * self
        return out

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        # a numpy SCALAR on the left of + - * / lands here: the same single operation as the Python operator
        op = {"add": "ADD", "subtract": "SUB", "multiply": "MUL", "true_divide": "DIV", "divide": "DIV"}.get(ufunc.__name__)
        if op and method == "__call__" and not kwargs and len(inputs) == 2 and all(isinstance(v, Value) or np.ndim(v) == 0 for v in inputs):
            return self.tr.apply(op, *[v if isinstance(v, Value) else float(v) for v in inputs])
        raise TraceError(f"numpy.{ufunc.__name__}: numpy functions cannot be traced; use this module's functions")

    __rpow__ = _refuse("rpow")
    __bool__ = _refuse("bool (an `if`, `and`, `or` or `not` on a traced value)")
    __lt__ = _refuse("lt (comparison)")
    __le__ = _refuse("le (comparison)")
    __gt__ = _refuse("gt (comparison)")
    __ge__ = _refuse("ge (comparison)")
    __eq__ = _refuse("eq (comparison)")
    __ne__ = _refuse("ne (comparison)")
    __hash__ = None
    __float__ = _refuse("float")
    __int__ = _refuse("int")
    __floordiv__ = _refuse("floordiv")
    __rfloordiv__ = _refuse("floordiv")
    __mod__ = _refuse("mod")
    __rmod__ = _refuse("mod")


def _call(op, *vs):
    """the operation on traced values; on plain numbers alone, the restated operation's value (the same fold)"""
    for v in vs:
        if isinstance(v, Value):
            return v.tr.apply(op, *vs)
    for v in vs:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TraceError(f"{op}: operand of type {type(v).__name__} is not a traced value or a real number")
    return _fold(op, [float(v) for v in vs])


def sin(a): return _call("SIN", a)
def cos(a): return _call("COS", a)
def fma(a, b, c): return _call("FMA", a, b, c)
def minimum(a, b): return _call("MIN", a, b)
def maximum(a, b): return _call("MAX", a, b)
def abs_(a): return _call("ABS", a)


def sqrt(a): raise TraceError("sqrt: not an operation of the plant program")
def exp(a): raise TraceError("exp: not an operation of the plant program")
def tanh(a): raise TraceError("tanh: not an operation of the plant program")
def where(*a): raise TraceError("where (select): not an operation of the plant program")


class NonlinearPlant:
    """The true plant x+ = program(x, u, d, q) and its LINEAR measurement y = C x + Dd d + h_offset (the reference's
    default get_measurement).  See the module's text for `f`.  Fields: nx, nu, nd, nq, ny, Ts and the program as
    arrays -- `consts` (n_consts,) float64, `ins` (n_ins, 5) int32 rows (op, dst, a, b, c), `out_slot` (nx,) int32,
    `n_slots`."""

    def __init__(self, f, nx, nu, nd=0, nq=0, Ts=None, C=None, Dd=None, h_offset=None):
        self.nx, self.nu, self.nd, self.nq = int(nx), int(nu), int(nd), int(nq)
        self.Ts = None if Ts is None else float(Ts)
        self.C = np.eye(self.nx) if C is None else np.asarray(C, float).reshape(-1, self.nx)
        self.ny = self.C.shape[0]
        self.Dd = np.zeros((self.ny, self.nd)) if Dd is None else np.asarray(Dd, float).reshape(self.ny, self.nd)
        self.h_offset = np.zeros(self.ny) if h_offset is None else np.asarray(h_offset, float).reshape(self.ny)
        tr = _Tracer()
        ins = [[tr.node(op, (a,)) for a in range(w)] for op, w in zip(_LOADS, (self.nx, self.nu, self.nd, self.nq))]
        out = f(*ins)
        try:
            out = list(out)
        except TypeError:
            raise TraceError("f: must return a sequence of nx expressions") from None
        if len(out) != self.nx:
            raise TraceError(f"f: must return nx = {self.nx} expressions, got {len(out)}")
        out = [tr.lift(v, "f (a returned expression)") for v in out]
        if self.Ts is not None:                       # x_a + Ts * f_a: separate multiply and add (model.jl:87)
            out = [ins[0][a] + self.Ts * out[a] for a in range(self.nx)]
        self._schedule(tr, [v.nid for v in out])

    def _schedule(self, tr, outs):
        """instructions in creation order (an operand is always created before its user), dead nodes dropped, slots
        reused once their last reader has run; the outputs stay live to the end"""
        live = set()
        stack = list(outs)
        while stack:
            n = stack.pop()
            if n in live:
                continue
            live.add(n)
            op, args = tr.nodes[n]
            if op not in _LOADS and op != "CONST":
                stack.extend(args)
        order = sorted(live)
        last = {n: len(order) for n in outs}
        for pos, n in enumerate(order):
            op, args = tr.nodes[n]
            if op not in _LOADS and op != "CONST":
                for a in args:
                    last[a] = max(last.get(a, -1), pos)
        consts, cindex, rows, slot_of, free, n_slots = [], {}, [], {}, [], 0
        for pos, n in enumerate(order):
            op, args = tr.nodes[n]
            if op == "CONST":
                if args[0] not in cindex:
                    cindex[args[0]] = len(consts)
                    consts.append(struct.unpack("<d", args[0])[0])
                operands = [cindex[args[0]]]
            elif op in _LOADS:
                operands = [args[0]]
            else:
                operands = [slot_of[a] for a in args]
                for a in set(args):                   # an operand read here for the last time frees its slot: the
                    if last[a] == pos:                # interpreter reads every operand before it writes dst
                        free.append(slot_of.pop(a))
            if free:
                dst = min(free)
                free.remove(dst)
            else:
                dst, n_slots = n_slots, n_slots + 1
            slot_of[n] = dst
            rows.append([OPS[op], dst] + operands + [0] * (3 - len(operands)))
        if len(rows) > MAX_INS:
            raise TraceError(f"n_ins: the program has {len(rows)} instructions, the cap is {MAX_INS}")
        if n_slots > MAX_SLOTS:
            raise TraceError(f"n_slots: the program needs {n_slots} slots, the cap is {MAX_SLOTS}")
        if len(consts) > MAX_CONSTS:
            raise TraceError(f"n_consts: the program has {len(consts)} constants, the cap is {MAX_CONSTS}")
        self.consts = np.array(consts, dtype=np.float64)
        self.ins = np.array(rows, dtype=np.int32).reshape(-1, 5)
        self.out_slot = np.array([slot_of[n] for n in outs], dtype=np.int32)
        self.n_slots = max(n_slots, 1)

    @classmethod
    def from_arrays(cls, nx, nu, nd, nq, n_slots, consts, ins, out_slot, C=None, Dd=None, h_offset=None):
        """A plant from a ready-made program (no tracing, no checking here: `lmpc_plant_program_check` judges it)."""
        self = cls.__new__(cls)
        self.nx, self.nu, self.nd, self.nq, self.Ts = int(nx), int(nu), int(nd), int(nq), None
        self.C = np.eye(self.nx) if C is None else np.asarray(C, float).reshape(-1, self.nx)
        self.ny = self.C.shape[0]
        self.Dd = np.zeros((self.ny, self.nd)) if Dd is None else np.asarray(Dd, float).reshape(self.ny, self.nd)
        self.h_offset = np.zeros(self.ny) if h_offset is None else np.asarray(h_offset, float).reshape(self.ny)
        self.consts = np.asarray(consts, np.float64).reshape(-1)
        self.ins = np.asarray(ins, np.int32).reshape(-1, 5)
        self.out_slot = np.asarray(out_slot, np.int32).reshape(-1)
        self.n_slots = int(n_slots)
        return self

    def check(self):
        """`lmpc_plant_program_check` (host only): raises LmpcError with the offending field's name first."""
        from ._cabi import check, lib
        p, keep = self.program()
        check(lib().lmpc_plant_program_check(ctypes.byref(p)))

    def measurement_rows(self):
        """MPC_MEASUREMENT_FUNCTION layout: rows [h_offset_j, C_j, Dd_j]."""
        return np.ascontiguousarray(np.hstack([self.h_offset[:, None], self.C, self.Dd]))

    def program(self):
        """(`lmpc_plant_program` struct, keep-alive list)"""
        from ._cabi import PlantProgram
        consts = np.ascontiguousarray(self.consts if self.consts.size else np.zeros(1))
        ins = np.ascontiguousarray(self.ins if self.ins.size else np.zeros((1, 5), np.int32))
        out = np.ascontiguousarray(self.out_slot)
        p = PlantProgram(self.nx, self.nu, self.nd, self.nq, self.n_slots, int(self.consts.size), int(self.ins.shape[0]),
                         consts.ctypes.data, ins.ctypes.data, out.ctypes.data)
        return p, [consts, ins, out]

    def eval_host(self, x, u=None, d=None, q=None):
        """`lmpc_plant_program_eval_host`: x (N, nx), u (N, nu), d (N, nd), q (nq,) shared or (N, nq) -> x+ (N, nx)."""
        from ._cabi import check, lib
        x = np.ascontiguousarray(np.asarray(x, float).reshape(-1, self.nx))
        N = x.shape[0]
        arr = lambda a, w: np.ascontiguousarray(np.zeros((N, w)) if a is None else np.asarray(a, float).reshape(N, w))
        u, d = arr(u, self.nu), arr(d, self.nd)
        q = np.zeros(self.nq) if q is None else np.ascontiguousarray(np.asarray(q, float))
        shared = q.ndim == 1
        q = np.ascontiguousarray(q.reshape((self.nq,) if shared else (N, self.nq)))
        out = np.empty((N, self.nx))
        p, keep = self.program()
        vp = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None
        check(lib().lmpc_plant_program_eval_host(ctypes.byref(p), N, vp(x), vp(u), vp(d), vp(q), int(shared), vp(out)))
        return out
