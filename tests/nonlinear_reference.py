"""TEST INFRASTRUCTURE: the nonlinear true plant restated on the host.

What tests/uncertain_reference.py is for `lmpc_simulate_scenario_uncertain_device`, this is for the plant program of
include/lmpc_hip.h (`lmpc_plant_program`) and `lmpc_simulate_scenario_nonlinear_device`:

    sincos / sin_ / cos_   the header's sine and cosine: Cody-Waite reduction with three constants, the two kernel
                           polynomials, the quadrant select -- every line one numpy operation or one glibc fma
    interpret              a program (any object with nx, nu, nd, nq, n_slots, consts, ins, out_slot) run one IEEE
                           operation at a time, across the scenarios
    Num / NumMath          numpy float64 behind the operators a plant function uses, `**` as left-to-right products:
                           a plant function evaluated DIRECTLY, without the tracer
    nonlinear_run          uncertain_reference.uncertain_run's loop with the plant step replaced by `interpret`
    cartpole, every_op ... the plant functions, the hand-made programs, the closed-loop cases and `check_conditions`

numpy and glibc's fma (through loop_reference.fma) only: nothing here imports the library or opens a device.
"""
import struct
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from oracle import ldp as oldp
from oracle import mpc2mpqp as omm

import scenario_reference as sr
import uncertain_reference as ur
from loop_reference import fma
from scenario_reference import _column, correct, measure, popcount, predict, run_trajectory, step_cost, step_violation, theta_block
from uncertain_reference import Box, draw

OPS = {"LOADX": 1, "LOADU": 2, "LOADD": 3, "LOADQ": 4, "CONST": 5, "ADD": 6, "SUB": 7, "MUL": 8, "DIV": 9, "NEG": 10,
       "ABS": 11, "FMA": 12, "MIN": 13, "MAX": 14, "SIN": 15, "COS": 16}
MAX_INS, MAX_SLOTS, MAX_CONSTS = 1024, 64, 256


def _b(h):
    return np.float64(struct.unpack("<d", struct.pack("<Q", h))[0])


TWO_OVER_PI = _b(0x3FE45F306DC9C883)
P1, P2, P3 = _b(0x3FF921FB54400000), _b(0x3DD0B4611A600000), _b(0x3BA3198A2E037073)
S1, S2, S3, S4, S5, S6 = (_b(h) for h in (0xBFC5555555555549, 0x3F8111111110F8A6, 0xBF2A01A019C161D5, 0x3EC71DE357B1FE7D,
                                          0xBE5AE5E68A2B9CEB, 0x3DE5D93A5ACFD57C))
C1, C2, C3, C4, C5, C6 = (_b(h) for h in (0x3FA555555555554C, 0xBF56C16C16C15177, 0x3EFA01A019CB1590, 0xBE927E4F809C52AD,
                                          0x3E21EE9EBDB4B1C4, 0xBDA8FAE9BE8838D4))


# ------------------------------------------------------------------ sine and cosine
def sincos(t):
    """sn, cs, m of the header's sequence, elementwise; m in {-2, -1, 0, 1, 2}"""
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        kd = np.rint(t * TWO_OVER_PI)
        nk = -kd
        r = fma(nk, P1, t)
        r = fma(nk, P2, r)
        r = fma(nk, P3, r)
        z = r * r
        ps = np.full(t.shape, S6)
        for c in (S5, S4, S3, S2, S1):
            ps = fma(ps, z, c)
        sn = fma(r * z, ps, r)
        pc = np.full(t.shape, C6)
        for c in (C5, C4, C3, C2, C1):
            pc = fma(pc, z, c)
        hz = 0.5 * z
        w = 1.0 - hz
        cs = w + fma(z * z, pc, (1.0 - w) - hz)
        m = kd - 4.0 * np.rint(0.25 * kd)
    return sn, cs, m


def sin_cos_(t):
    """(sin_(t), cos_(t)) from one evaluation of the sequence"""
    sn, cs, m = sincos(t)
    return (np.where(m == 0, sn, np.where(m == 1, cs, np.where(m == -1, -cs, -sn))),
            np.where(m == 0, cs, np.where(m == 1, -sn, np.where(m == -1, sn, -cs))))


def sin_(t):
    return sin_cos_(t)[0]


def cos_(t):
    return sin_cos_(t)[1]


def quadrant(t):
    """k & 3 of the reduction: 0 .. 3 (NaN for a non-finite t)"""
    m = sincos(t)[2]
    return np.where(m == -1, 3.0, np.abs(m))


# ------------------------------------------------------------------ the interpreter
def interpret(prog, x, u=None, d=None, q=None):
    """x+ (S, nx) of a program on x (S, nx), u (S, nu), d (S, nd), q (nq,) shared or (S, nq): one numpy operation per
    instruction, MIN / MAX as the header's selects"""
    x = np.asarray(x, np.float64).reshape(-1, prog.nx)
    S = x.shape[0]
    arr = lambda a, w: np.zeros((S, w)) if a is None else np.asarray(a, np.float64).reshape(S, w)
    u, d = arr(u, prog.nu), arr(d, prog.nd)
    q = np.zeros(prog.nq) if q is None else np.asarray(q, np.float64)
    q = np.broadcast_to(q, (S, prog.nq)) if q.ndim == 1 else q.reshape(S, prog.nq)
    slots = [None] * prog.n_slots
    name = {v: k for k, v in OPS.items()}
    with np.errstate(all="ignore"):
        for op, dst, a, b, c in np.asarray(prog.ins).reshape(-1, 5).tolist():
            o = name[op]
            if o == "LOADX": v = x[:, a].copy()
            elif o == "LOADU": v = u[:, a].copy()
            elif o == "LOADD": v = d[:, a].copy()
            elif o == "LOADQ": v = q[:, a].copy()
            elif o == "CONST": v = np.full(S, prog.consts[a], np.float64)
            elif o == "ADD": v = slots[a] + slots[b]
            elif o == "SUB": v = slots[a] - slots[b]
            elif o == "MUL": v = slots[a] * slots[b]
            elif o == "DIV": v = slots[a] / slots[b]
            elif o == "NEG": v = -slots[a]
            elif o == "ABS": v = np.abs(slots[a])
            elif o == "FMA": v = fma(slots[a], slots[b], slots[c])
            elif o == "MIN": v = np.where(slots[a] < slots[b], slots[a], slots[b])
            elif o == "MAX": v = np.where(slots[a] > slots[b], slots[a], slots[b])
            elif o == "SIN": v = sin_(slots[a])
            else: v = cos_(slots[a])
            slots[dst] = v
    return np.stack([slots[s] for s in np.asarray(prog.out_slot).tolist()], axis=1)


def same(a, b):
    """bit for bit, a NaN equal to any NaN (the sign and payload of a NaN result are not part of the contract)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint64) == b.view(np.uint64))))


# ------------------------------------------------------------------ a plant function evaluated directly
class Num:
    """a float64 vector over the scenarios behind the operators a plant function uses"""

    def __init__(self, v):
        self.v = np.asarray(v, np.float64)

    @staticmethod
    def of(o):
        return o.v if isinstance(o, Num) else np.float64(o)

    def _bin(self, o, f, swap=False):
        with np.errstate(all="ignore"):
            return Num(f(Num.of(o), self.v) if swap else f(self.v, Num.of(o)))

    def __add__(self, o): return self._bin(o, np.add)
    def __radd__(self, o): return self._bin(o, np.add, True)
    def __sub__(self, o): return self._bin(o, np.subtract)
    def __rsub__(self, o): return self._bin(o, np.subtract, True)
    def __mul__(self, o): return self._bin(o, np.multiply)
    def __rmul__(self, o): return self._bin(o, np.multiply, True)
    def __truediv__(self, o): return self._bin(o, np.divide)
    def __rtruediv__(self, o): return self._bin(o, np.divide, True)
    def __neg__(self): return Num(-self.v)
    def __abs__(self): return Num(np.abs(self.v))

    def __pow__(self, n):
        out = self
        for _ in range(int(n) - 1):
            out = out * self
        return out if n > 0 else Num(np.ones_like(self.v))


class NumMath:
    """the functions a plant function takes from its math namespace, on `Num`"""
    sin = staticmethod(lambda a: Num(sin_(a.v)))
    cos = staticmethod(lambda a: Num(cos_(a.v)))
    @staticmethod
    def fma(a, b, c):
        with np.errstate(all="ignore"):
            return Num(fma(*np.broadcast_arrays(Num.of(a), Num.of(b), Num.of(c))))

    minimum = staticmethod(lambda a, b: Num(np.where(Num.of(a) < Num.of(b), Num.of(a), Num.of(b))))
    maximum = staticmethod(lambda a, b: Num(np.where(Num.of(a) > Num.of(b), Num.of(a), Num.of(b))))
    abs_ = staticmethod(lambda a: Num(np.abs(a.v)))


def direct(f, x, u, d, q, Ts=None):
    """f evaluated on numpy float64, scenario-wise: x + Ts * f (separate multiply and add) or f itself"""
    x = np.asarray(x, np.float64)
    S = x.shape[0]
    q = np.asarray(q, np.float64)
    q = np.broadcast_to(q, (S, q.shape[-1])) if q.ndim == 1 else q
    cols = lambda a: [Num(a[:, j]) for j in range(a.shape[1])]
    out = f(cols(x), cols(np.asarray(u, np.float64)), cols(np.asarray(d, np.float64)), cols(q), NumMath)
    out = [np.broadcast_to(Num.of(o), (S,)) for o in out]
    if Ts is not None:
        out = [x[:, a] + np.float64(Ts) * out[a] for a in range(x.shape[1])]
    return np.stack(out, axis=1)


# ------------------------------------------------------------------ the plant functions (m: the math namespace)
def cartpole(x, u, d, q, m):
    """The cart-pole of the reference's invpend example (src/mpc_examples.jl:113-116), written anew: q = (M, m, l), damping
    10, g = 9.81, input scale 100.  States: cart position, velocity, pole angle, angular velocity."""
    M, mp, l = q[0], q[1], q[2]
    damp, g, scale = 10.0, 9.81, 100.0
    s, c = m.sin(x[2]), m.cos(x[2])
    Mm = M + mp
    force = scale * u[0] - damp * x[1] - mp * l * x[3] ** 2 * s
    return [x[1],
            (force + mp * g * s * c) / (M + mp * s ** 2),
            x[3],
            (g * s + force * c / Mm) / (l - mp * l * c ** 2 / Mm)]


CARTPOLE = dict(nx=4, nu=1, nd=0, nq=3, Ts=0.01)
CARTPOLE_Q = np.array([1.0, 1.0, 0.5])


def every_op(x, u, d, q, m):
    """every operation of the program once, each alone in an output: nx = 12, nu = nd = nq = 1"""
    return [x[0] + x[1], x[0] - x[1], x[0] * x[1], x[0] / x[1], -x[0], abs(x[0]), m.fma(x[0], x[1], x[2]),
            m.minimum(x[0], x[1]), m.maximum(x[0], x[1]), m.sin(x[0]), m.cos(x[0]),
            # the other inputs, a cube, and a constant on the LEFT of - and / (x[3] stays within [-2, 2])
            u[0] * d[0] + q[0] * x[3] ** 3 - 0.25 + (1.5 - x[3]) * (2.0 / (4.0 + x[3]))]


EVERY_OP = dict(nx=12, nu=1, nd=1, nq=1)


def linear_plant(rows, nx, nu, nd):
    """f_offset + F x + G u + Gd d as a plant function, in the row-sum order of dynamics_rows: from f_offset, the terms of
    F, G, Gd in index order, each one multiply and one add"""
    rows = np.asarray(rows, np.float64).reshape(nx, 1 + nx + nu + nd)

    def f(x, u, d, q, m=None):
        out = []
        for a in range(nx):
            acc = float(rows[a, 0])
            for j, v in enumerate(list(x) + list(u) + list(d)):
                acc = acc + float(rows[a, 1 + j]) * v
            out.append(acc)
        return out
    return f


def special_values():
    """inputs of every_op over +-0, +-inf, NaN, subnormals, ties of MIN / MAX and ordinary values: (x, u, d, q)"""
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, -1.0, 0.5 * np.pi, 3.0,
                     1e300, -1e300, 2.0 ** 20, 1e22])
    a, b = np.meshgrid(vals, vals, indexing="ij")
    S = a.size
    rng = np.random.default_rng(5)
    x = np.zeros((S, 12))
    x[:, 0], x[:, 1] = a.ravel(), b.ravel()
    x[:, 2] = rng.choice(vals, S)
    x[:, 3] = rng.uniform(-2, 2, S)
    return x, rng.choice(vals, (S, 1)), rng.choice(vals, (S, 1)), rng.choice(vals, (S, 1))


def program(nx, nu, nd, nq, n_slots, consts, ins, out_slot):
    return SimpleNamespace(nx=nx, nu=nu, nd=nd, nq=nq, n_slots=n_slots, consts=np.asarray(consts, np.float64),
                           ins=np.asarray(ins, np.int32).reshape(-1, 5), out_slot=np.asarray(out_slot, np.int32))


def slot_cap_program():
    """all 64 slots live at once: x_0 .. x_31 into slots 0 .. 31, x_i * x_(i+1 mod 32) into 32 .. 63, which are x+"""
    ins = [[OPS["LOADX"], i, i, 0, 0] for i in range(32)] + [[OPS["MUL"], 32 + i, i, (i + 1) % 32, 0] for i in range(32)]
    return program(32, 0, 0, 0, MAX_SLOTS, [], ins, range(32, 64))


def instruction_cap_program():
    """1024 instructions: two loads, then 511 times s0 <- sin_(s0 + s1)"""
    ins = [[OPS["LOADX"], 0, 0, 0, 0], [OPS["LOADX"], 1, 1, 0, 0]]
    for _ in range(511):
        ins += [[OPS["ADD"], 0, 0, 1, 0], [OPS["SIN"], 0, 0, 0, 0]]
    assert len(ins) == MAX_INS
    return program(2, 0, 0, 0, 2, [], ins, [0, 1])


SIZES = (1, 63, 64, 65, 257)


# ------------------------------------------------------------------ the loop
def nonlinear_run(ldp, dims, plant, prog, x0, T, q=None, r=None, d=None, p=None, noise=None, observer=None, previews=(0, 0, 0),
                  uprev0=None, warm=False, cost=None, settings=None, solve=None, process=None, measurement_noise=None,
                  Gw=None, seed=0, scenario_offset=0, step_offset=0, xhat0=None):
    """uncertain_reference.uncertain_run without a plant table and with x <- interpret(prog, x, u, d_k, q) in place of
    the plant's row sums; `plant` gives the (linear) measurement rows alone.  Same arguments, same namespace returned."""
    nx, nu, wr, nd, nup, wp = dims
    rH, dH, pH = previews
    x = np.array(x0, float).reshape(-1, nx)
    S = x.shape[0]
    ny = plant.C.shape[0]
    pmeas = np.hstack([plant.h_offset[:, None], plant.C, plant.Dd.reshape(ny, nd)])
    g = (np.arange(S, dtype=np.uint64) + np.uint64(scenario_offset))
    if observer is not None:
        odyn = np.asarray(observer[0], float).reshape(nx, 1 + nx + nu + nd)
        omeas = np.asarray(observer[1], float).reshape(ny, 1 + nx + nd)
        okt = np.asarray(observer[2], float).reshape(ny, nx)
    rt, dt, pt, vt = (None if a is None else run_trajectory(a, S, T) for a in (r, d, p, noise))
    et = None if (process is None or isinstance(process, Box)) else run_trajectory(process, S, T)
    mt = None if (measurement_noise is None or isinstance(measurement_noise, Box)) else run_trajectory(measurement_noise, S, T)
    assert not (vt is not None and measurement_noise is not None)
    if wr == 0:
        rt = None
    up0 = np.zeros(nup) if uprev0 is None else np.asarray(uprev0, float)
    uprev = up0[:, :nup].copy() if up0.ndim == 2 else np.tile(up0[:nup], (S, 1))
    xhat = x.copy() if xhat0 is None else np.array(xhat0, float).reshape(S, nx)
    if solve is None:
        solve = lambda th, wm: tuple(oldp.solve_batch(ldp, th, settings, warm=wm)[i] for i in (0, 1, 3))
    Gw = None if Gw is None else np.asarray(Gw, float).reshape(nx, -1)
    out = SimpleNamespace(xs=[x.copy()], us=[], xhats=[], yms=[], ys=[], ds=[], ws=[], thetas=[], flags=[], active=[])
    run, ulast, worst, act = np.zeros(S), np.zeros((S, nu)), np.zeros(S), None
    for k in range(T):
        kg = step_offset + k
        dk = np.zeros((S, nd)) if dt is None else _column(dt, k)
        if isinstance(measurement_noise, Box):
            vk = draw(seed, g, kg, 1, measurement_noise.lo, measurement_noise.hi)
        else:
            vk = _column(mt, k) if mt is not None else (None if vt is None else _column(vt, k))
        ym, y0 = measure(pmeas, x, dk, vk)
        xhat = correct(omeas, okt, xhat, ym, dk) if observer is not None else x.copy()
        theta = np.concatenate([xhat, theta_block(rt, wr, rH, k + 1 if rH else k, S) if wr else np.zeros((S, 0)),
                                theta_block(dt, nd, dH, k, S) if nd else np.zeros((S, 0)), uprev,
                                theta_block(pt, wp, pH, k, S) if wp else np.zeros((S, 0))], axis=1)
        u, flag, act = solve(theta, act if (warm and k > 0) else None)
        if cost is not None:
            run = run + step_cost(cost, x, u, ulast, None if rt is None else _column(rt, k))
            ulast = u
            v = step_violation(cost, x, u)
            worst = np.where(v > worst, v, worst)
        for key, val in (("us", u), ("xhats", xhat), ("yms", ym), ("ys", y0 if observer is not None else ym), ("ds", dk),
                         ("thetas", theta), ("flags", flag), ("active", act)):
            getattr(out, key).append(np.array(val))
        if observer is not None:
            xhat = predict(odyn, xhat, u, dk)             # the observer predicts with its own LINEAR model and sees no w
        x = interpret(prog, x, u, dk, q)
        if process is not None:
            e = draw(seed, g, kg, 0, process.lo, process.hi) if isinstance(process, Box) else _column(et, k)
            if Gw is None:
                w = e.copy()
                x = x + e
            else:
                w = np.zeros((S, nx))
                for a in range(nx):
                    for j in range(Gw.shape[1]):
                        t = Gw[a, j] * e[:, j]
                        x[:, a] = x[:, a] + t
                        w[:, a] = w[:, a] + t
            out.ws.append(w)
        uprev = u[:, :nup].copy()
        out.xs.append(x.copy())
    for key in ("xs", "us", "xhats", "yms", "ys", "ds", "thetas", "flags", "active"):
        setattr(out, key, np.array(getattr(out, key)))
    out.ws = np.array(out.ws) if process is not None else None
    out.flag_min = out.flags.min(axis=0).astype(np.int32)
    out.xhat_final, out.uprev_final = xhat, uprev
    out.active_sizes = popcount(out.active)
    out.cost = 0.5 * run if cost is not None else None
    out.violation = worst if cost is not None else None
    return out


# ------------------------------------------------------------------ the closed-loop cases
def controller(Np=10, Nc=5):
    """the pendulum controller of the GPU tests (oracle.mpc2mpqp.pendulum: the cart-pole linearised at the origin)"""
    return omm.pendulum(Np=Np, Nc=Nc)


def observer_arrays(prob):
    """a fixed-gain observer on the controller's model in the generated observer's layout: (MPC_PLANT_DYNAMICS,
    MPC_MEASUREMENT_FUNCTION, K_TRANSPOSE_OBSERVER)"""
    t = sr.plant_of(prob)
    K = np.array([[0.5, 0.0], [0.5, 0.0], [0.0, 0.5], [0.0, 0.5]])
    dyn = np.hstack([t.f_offset[:, None], t.F, t.G, t.Gd])
    meas = np.hstack([t.h_offset[:, None], t.C, t.Dd])
    return np.ascontiguousarray(dyn).reshape(-1), np.ascontiguousarray(meas).reshape(-1), np.ascontiguousarray(K.T).reshape(-1)


@dataclass
class Case:
    name: str
    S: int = 257
    T: int = 20
    q: str = "shared"                  # "shared": CARTPOLE_Q for everyone; "scenario": M, m, l drawn +-20 % per scenario
    process: bool = False              # drawn process noise through a Gw (nw = 2)
    meas: bool = False                 # drawn measurement noise, the observer on
    cost: bool = False
    warm: bool = False
    key: int = 0x9E3779B97F4A7C15
    scenario_offset: int = 0
    step_offset: int = 0


def case_data(case, pool=257):
    """deterministic in the case; the scenarios are the first S of a pool whose initial pole angles span [-3.3, 3.3] and
    whose other states shrink towards the middle of the pool (so that the first move is unsaturated there)"""
    prob = controller()
    rng = np.random.default_rng(9000)
    n = max(pool, case.S)
    angle = np.linspace(-3.3, 3.3, n)
    size = np.abs(np.linspace(-1.0, 1.0, n))
    x0 = np.stack([size * rng.uniform(-1, 1, n), size * rng.uniform(-1, 1, n), angle, size * rng.uniform(-1, 1, n)], axis=1)
    x0 = x0[rng.permutation(n)][:case.S]
    q = CARTPOLE_Q if case.q == "shared" else (CARTPOLE_Q[None, :] * rng.uniform(0.8, 1.2, (n, 3)))[:case.S]
    data = SimpleNamespace(prob=prob, x0=np.ascontiguousarray(x0), q=np.ascontiguousarray(q), process=None, Gw=None,
                           measurement_noise=None, observer=None, cost=None)
    if case.process:
        data.process = Box(np.array([-0.02, -0.05]), np.array([0.03, 0.05]))
        data.Gw = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [0.5, 1.0]])
    if case.meas:
        data.measurement_noise = Box(np.array([-0.01, -0.002]), np.array([0.01, 0.002]))
        data.observer = observer_arrays(prob)
    if case.cost:
        data.cost = dict(C=prob.C.copy(), Q=np.diag([1.44, 1.0]), R=np.array([[0.1]]), Rr=np.array([[1.0]]), S=None,
                         Ax=np.array([[1.0, 0, 0, 0], [0, 0, 1.0, 0]]), Au=np.zeros((2, 1)), lb=np.array([-0.5, -0.2]),
                         ub=np.array([0.5, 0.2]))
    return data


def run_kwargs(case, data):
    dims, previews = sr.dims_of(data.prob)
    return dict(dims=dims, plant=sr.plant_of(data.prob), x0=data.x0, T=case.T, q=data.q, observer=data.observer, previews=previews,
                uprev0=getattr(data.prob, "uprev0", None), warm=case.warm, cost=data.cost, process=data.process,
                measurement_noise=data.measurement_noise, Gw=data.Gw, seed=case.key, scenario_offset=case.scenario_offset,
                step_offset=case.step_offset)


def run_case(case, ldp, prog, data=None, settings=None, **override):
    data = case_data(case) if data is None else data
    kw = run_kwargs(case, data)
    kw.update(override)
    return nonlinear_run(ldp, prog=prog, settings=settings, **kw)


def linearised_run(case, ldp, data, settings=None):
    """the same case stepped by the controller's own F, G: what a loop that ignores the program would compute"""
    kw = run_kwargs(case, data)
    kw.pop("q")
    return ur.uncertain_run(ldp, settings=settings, **kw)


def saturated(us, umax=2.0):
    return np.abs(us) >= umax - 1e-9


def check_conditions(case, ref, lin, data):
    """What keeps a closed-loop case from passing emptily, asserted on the host reference's outputs alone: every flag
    >= 1; the reduction's k & 3 takes all four values over the angles visited (so both polynomials are selected for the
    sine and for the cosine); the first move is saturated for some scenarios and unsaturated for others; the
    trajectories differ from those of the linearised plant; drawn noise, where asked for, is non-zero."""
    assert ref.flags.min() >= 1, (case.name, int(ref.flags.min()))
    quads = set(np.unique(quadrant(ref.xs[:-1, :, 2])).astype(int).tolist())
    assert quads == {0, 1, 2, 3}, (case.name, "quadrants of the reduction", quads)
    first = saturated(ref.us[0, :, 0])
    assert first.any() and not first.all(), (case.name, "saturated first moves", int(first.sum()), first.size)
    differ = (ref.xs != lin.xs).any(axis=(0, 2))
    assert differ.mean() > 0.9, (case.name, "share of scenarios whose states differ from the linearised plant's", float(differ.mean()))
    assert not np.array_equal(ref.us, lin.us), (case.name, "the controls equal the linearised plant's")
    if case.process:
        assert ref.ws is not None and np.abs(ref.ws).max() > 0 and (ref.ws != 0).any(axis=(0, 1)).sum() >= 2, case.name
    if case.meas:
        quiet = measure(np.hstack([np.zeros((2, 1)), data.prob.C]), ref.xs[0], np.zeros((case.S, 0)), None)[0]
        assert not np.array_equal(ref.yms[0], quiet), (case.name, "the measurement noise never acted")
    if case.cost:
        # (the scenario in the middle of the pool starts at the origin and stays there: its cost is 0)
        assert (ref.cost > 0).sum() >= case.S - 1 and (ref.violation > 0).mean() > 0.2, case.name
    if case.warm:
        assert not np.array_equal(ref.active[1:], ref.active[:-1]), (case.name, "the working set never changes")


CLOSED_LOOP = [
    Case("plain"),
    Case("q-per-scenario", q="scenario"),
    Case("process-noise-gw", process=True),
    Case("measurement-noise-observer", meas=True),
    Case("cost-violation", cost=True),
    Case("warm", warm=True),
]
LOOP_SIZES = [Case(f"size-S{S}", S=S, T=3, q="scenario", process=True) for S in (1, 63, 64, 65)]
SPLIT = Case("split", S=130, T=8, q="scenario", process=True, meas=True, scenario_offset=5, step_offset=3)
HUNDRED = dict(x0=np.array([[5.0, 5.0, 0.0, 0.0], [-3.0, 2.0, 0.1, 0.0]]), T=100)
