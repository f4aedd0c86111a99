"""TEST INFRASTRUCTURE: the scenario loop under uncertainty, restated on the host.

What tests/scenario_reference.py is for `lmpc_simulate_scenario_device`, this is for
`lmpc_simulate_scenario_uncertain_device` (include/lmpc_hip.h).  The glue steps -- `measure`, `correct`, `predict`,
`theta_block`, `step_cost`, `step_violation` -- are imported from there; only what is new lives here:

    philox4x32_10      the counter-based generator (Salmon, Moraes, Dror, Shaw, SC'11) on uint64 arrays
    draw               component q of a source: min(hi_q, lo_q + u * (hi_q - lo_q)), u from a word pair
    uncertain_run      the loop: + v on ym (the place the descriptor's noise has), the scenario's own plant rows, then
                       x_a <- x_a + Gw_a0 e_0 + Gw_a1 e_1 + ... onto the finished row sum

Every sum is one numpy elementwise multiply and one elementwise add per term.  Nothing here imports the library or
opens a device.  Also here, shared by the CPU and the GPU tests: the cases and `check_conditions`.
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from oracle import ldp as oldp

import scenario_reference as sr
from scenario_reference import (_column, correct, measure, popcount, predict, run_trajectory, step_cost, step_violation,
                                theta_block)

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
SH32 = np.uint64(32)


# ------------------------------------------------------------------ the generator
def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or scalars) holding 32-bit words, key: two.  Returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & MASK for c in counter)
    k0, k1 = (np.asarray(k, np.uint64) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                         # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> SH32) ^ c1 ^ k0, p1 & MASK, (p0 >> SH32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def unit(a, b):
    """a word pair -> [0, 1): the 53 bits (a << 21) | (b >> 11) times 2^-53, exact"""
    bits = (np.asarray(a, np.uint64) << np.uint64(21)) | (np.asarray(b, np.uint64) >> np.uint64(11))
    return bits.astype(np.float64) * 2.0 ** -53


def units(seed, g, kglobal, stream, w):
    """u of components 0 .. w-1 for the global scenarios g (uint64 array) at global step kglobal: (len(g), w)"""
    g = np.asarray(g, np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    key = (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    out = np.empty((g.size, w))
    for j in range((w + 1) // 2):
        r = philox4x32_10((g & MASK, g >> SH32, np.full(g.size, kglobal, np.uint64),
                           np.full(g.size, (stream << 16) | j, np.uint64)), key)
        out[:, 2 * j] = unit(r[0], r[1])
        if 2 * j + 1 < w:
            out[:, 2 * j + 1] = unit(r[2], r[3])
    return out


def draw(seed, g, kglobal, stream, lo, hi):
    """(len(g), w) draws uniform in [lo, hi]: e_q = min(hi_q, lo_q + u * span_q) with span_q = hi_q - lo_q"""
    lo, hi = np.asarray(lo, float).reshape(-1), np.asarray(hi, float).reshape(-1)
    span = hi - lo
    u = units(seed, g, kglobal, stream, lo.size)
    return np.minimum(hi[None, :], lo[None, :] + u * span[None, :])


@dataclass
class Box:
    """a source drawn in [lo, hi]"""
    lo: np.ndarray
    hi: np.ndarray


# ------------------------------------------------------------------ the loop
def _rows(plant, nx, nd, ny):
    pdyn = np.hstack([plant.f_offset[:, None], plant.F, plant.G, plant.Gd.reshape(nx, nd)])
    pmeas = np.hstack([plant.h_offset[:, None], plant.C, plant.Dd.reshape(ny, nd)])
    return pdyn, pmeas


def uncertain_run(ldp, dims, plant, x0, T, r=None, d=None, p=None, noise=None, observer=None, previews=(0, 0, 0),
                  uprev0=None, warm=False, cost=None, settings=None, solve=None, process=None, measurement_noise=None,
                  Gw=None, seed=0, scenario_offset=0, step_offset=0, plants=None, plant_index=None, xhat0=None):
    """scenario_reference.reference_run's arguments, and: process / measurement_noise None, a `Box` (drawn) or an array
    (w, Tc) / (S, w, Tc) (supplied, column k at step k of THIS run, the last one held); Gw (nx, nw) or None; plants: a
    list of plant objects (the FIRST argument `plant` gives the shared measurement) or None; plant_index (S,) ints or
    None = (scenario_offset + i) mod len(plants); xhat0 (S, nx): the observer state a continued run carries (None: x0);
    uprev0 may be (S, nuprev).  Returns reference_run's namespace plus ws (T, S, nx), None without process noise."""
    nx, nu, wr, nd, nup, wp = dims
    rH, dH, pH = previews
    x = np.array(x0, float).reshape(-1, nx)
    S = x.shape[0]
    ny = plant.C.shape[0]
    pdyn, pmeas = _rows(plant, nx, nd, ny)
    g = (np.arange(S, dtype=np.uint64) + np.uint64(scenario_offset))
    if plants:
        idx = (g % np.uint64(len(plants))).astype(np.int64) if plant_index is None else \
            (np.asarray(plant_index).astype(np.uint32).astype(np.int64) % len(plants))
        table = np.array([_rows(q, nx, nd, ny)[0] for q in plants])
        pdyn = np.ascontiguousarray(np.moveaxis(table[idx], 0, -1))        # (nx, cols, S): entry [a, c] is a vector over S
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
    run, ulast, worst, vsteps, act = np.zeros(S), np.zeros((S, nu)), np.zeros(S), [], None
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
            vsteps.append(step_violation(cost, x, u))
            worst = np.where(vsteps[-1] > worst, vsteps[-1], worst)
        for key, val in (("us", u), ("xhats", xhat), ("yms", ym), ("ys", y0 if observer is not None else ym), ("ds", dk),
                         ("thetas", theta), ("flags", flag), ("active", act)):
            getattr(out, key).append(np.array(val))
        if observer is not None:
            xhat = predict(odyn, xhat, u, dk)             # the observer predicts with its own model and sees no w
        x = predict(pdyn, x, u, dk)
        if process is not None:
            e = draw(seed, g, kg, 0, process.lo, process.hi) if isinstance(process, Box) else _column(et, k)
            if Gw is None:
                w = e.copy()
                x = x + e
            else:
                w = np.zeros((S, nx))
                for a in range(nx):
                    for q in range(Gw.shape[1]):
                        t = Gw[a, q] * e[:, q]
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


# ------------------------------------------------------------------ the cases
@dataclass
class Case:
    name: str
    nx: int
    nu: int = 2
    ny: int = 3
    nd: int = 2
    seed: int = 0                      # of the problem family (scenario_reference.chain_problem)
    S: int = 300
    T: int = 6
    observer: bool = True
    warm: bool = False
    x0: float = 1.0
    cost: bool = False
    pool: int = 0                      # > 0: the scenarios are the first S of a pool of this many
    process: str = "draw"              # None, "draw", "block" (one per scenario), "shared"
    nw: int = 0                        # 0: Gw NULL (nw = nx); else Gw is nx x nw
    meas: str = "draw"                 # None, "draw", "block"
    noise: bool = False                # the descriptor's own noise block
    pbox: float = 0.2                  # the process box is [-pbox, pbox] (scaled per component)
    n_plants: int = 0                  # 0: the descriptor's plant; -1: one plant per scenario (S)
    index: bool = False                # an explicit plant_index with repeats
    pert: float = 0.3                  # relative perturbation of F and G over the ensemble
    scenario_offset: int = 0
    step_offset: int = 0
    key: int = 0x9E3779B97F4A7C15      # the generator's seed (both key words in use)

    @property
    def plants(self):
        return self.S if self.n_plants < 0 else self.n_plants


def case_data(case):
    """scenario_reference.case_data of the matching plain case, plus the sources, Gw and the ensemble; deterministic
    in the case; with `pool` cuts of one draw.  Supplied blocks are Gaussian, as a caller of example/observer.jl's
    kind would draw them."""
    base = sr.Case(case.name, case.nx, nu=case.nu, ny=case.ny, nd=case.nd, seed=case.seed, S=case.S, T=case.T,
                   observer=case.observer, noise=case.noise, warm=case.warm, x0=case.x0, cost=case.cost, pool=case.pool)
    data = sr.case_data(base)
    rng = np.random.default_rng(4000 + case.seed)
    n, S, T, nx, ny = max(case.pool, case.S), case.S, case.T, case.nx, case.ny
    nw = case.nw or nx
    scale = rng.uniform(0.5, 1.0, nw)
    box = Box(-case.pbox * scale, case.pbox * scale * rng.uniform(0.6, 1.0, nw))
    eblock = 0.5 * case.pbox * rng.standard_normal((n, nw, T))
    vblock = 0.02 * rng.standard_normal((n, ny, T))
    vbox = Box(-0.02 * rng.uniform(0.5, 1.0, ny), 0.02 * rng.uniform(0.5, 1.0, ny))
    data.Gw = rng.uniform(-1.0, 1.0, (nx, nw)) if case.nw else None
    data.process = {None: None, "draw": box, "block": eblock[:S], "shared": eblock[0]}[case.process]
    data.measurement_noise = {None: None, "draw": vbox, "block": vblock[:S]}[case.meas]
    data.plants, data.plant_index = None, None
    if case.plants:
        nominal = sr.plant_of(data.prob)
        data.plants = []
        for _ in range(case.plants):
            q = SimpleNamespace(**vars(nominal))
            q.F = nominal.F * (1.0 + case.pert * rng.uniform(-1.0, 1.0, nominal.F.shape))
            q.G = nominal.G * (1.0 + case.pert * rng.uniform(-1.0, 1.0, nominal.G.shape))
            q.f_offset = nominal.f_offset + 0.05 * rng.standard_normal(nx)
            data.plants.append(q)
        if case.index:
            data.plant_index = rng.integers(0, case.plants, n).astype(np.int32)[:S]
            data.plant_index[: min(S, 3)] = case.plants - 1              # repeats, and the table's last array
    return data


def run_kwargs(case, data):
    dims, previews = sr.dims_of(data.prob)
    obs = None if data.kf is None else data.kf.codegen_arrays()
    return dict(dims=dims, plant=sr.plant_of(data.prob), x0=data.x0, T=case.T, r=data.r, d=data.d, p=data.p, noise=data.noise,
                observer=obs, previews=previews, uprev0=getattr(data.prob, "uprev0", None), warm=case.warm, cost=data.cost,
                process=data.process, measurement_noise=data.measurement_noise, Gw=data.Gw, seed=case.key,
                scenario_offset=case.scenario_offset, step_offset=case.step_offset, plants=data.plants,
                plant_index=data.plant_index)


def run_case(case, ldp, data=None, settings=None, **override):
    data = case_data(case) if data is None else data
    kw = run_kwargs(case, data)
    kw.update(override)
    return uncertain_run(ldp, settings=settings, **kw)


def check_conditions(case, ref, ldp, data=None, settings=None):
    """What keeps a case from passing emptily, asserted on the reference's outputs alone: every flag >= 1; both solver
    outcomes on at least 5 % of the scenario-steps (a case of fewer than 40 scenario-steps is a cut of its pool, whose
    member the same sweep runs); with process noise at least 5 % of the scenario-steps whose final working set differs
    from the same case run noise-free; with an ensemble at least two plants whose scenarios' controls differ."""
    assert ref.flags.min() >= 1, (case.name, int(ref.flags.min()))
    big = case.S * case.T >= 40
    if big:
        share = float((ref.active_sizes > 0).mean())
        assert 0.05 <= share <= 0.95, (case.name, "share of scenario-steps with a non-empty working set", share)
    else:
        assert case.pool * case.T >= 40, case.name
    if case.process is not None:
        assert ref.ws is not None and np.abs(ref.ws).max() > 0
        if big and case.T > 1:
            quiet = run_case(case, ldp, data, settings, process=None, Gw=None)
            moved = float((ref.active != quiet.active).any(axis=-1).mean())
            assert moved >= 0.05, (case.name, "share of scenario-steps whose working set the process noise changed", moved)
    if case.meas is not None or case.noise:
        quiet = measure(_rows(sr.plant_of((data or case_data(case)).prob), case.nx, case.nd, case.ny)[1], ref.xs[0],
                        ref.ds[0], None)[0]
        assert not np.array_equal(ref.yms[0], quiet), (case.name, "the measurement noise never acted")
    if case.plants > 1 and big and case.T > 1:                # (the first step's controls do not know the plant)
        d = data or case_data(case)
        g = np.arange(case.S) + case.scenario_offset
        idx = g % case.plants if d.plant_index is None else d.plant_index % case.plants
        same = run_case(case, ldp, d, settings, plants=[d.plants[0]] * case.plants)
        differ = {int(q) for q in np.unique(idx) if not np.array_equal(ref.us[:, idx == q], same.us[:, idx == q])}
        assert len(differ) >= min(2, case.plants - 1), (case.name, "plants whose scenarios' controls differ", differ)
    if case.warm:
        assert case.T > 1 and not np.array_equal(ref.active[1:], ref.active[:-1]), (case.name, "warm start never differs")


X0 = {32: 3.0}                          # x0 range per nx where 1.0 does not give both solver outcomes
PBOX = {4: 0.6, 9: 0.6, 17: 0.6}        # process box per nx where 0.2 changes fewer than 5 % of the working sets (3.7 .. 4.9 %)

# one case per NX = 1 .. 8 and nx = 9, 17, 32: both sources drawn, the observer on for odd nx
STATES = [Case(f"nx{nx}", nx, seed=nx, observer=nx % 2 == 1, x0=X0.get(nx, 1.0), pbox=PBOX.get(nx, 0.2))
          for nx in (1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 32)]

DRAWS = [
    Case("gw-nw1", 4, seed=11, nw=1, pbox=0.4),
    Case("gw-nw2", 4, seed=12, nw=2),
    Case("gw-nw3", 5, seed=13, nw=3),
    Case("gw-nw5-nx12", 12, seed=14, nw=5),
    Case("gw-nw5-nx3", 3, seed=15, nw=5),
    Case("ny1", 3, ny=1, seed=16),
    Case("block-per-scenario", 4, seed=17, process="block", meas=None),
    Case("block-shared-gw", 4, seed=18, process="shared", nw=2, meas=None, pbox=0.4),
    Case("drawn-process-supplied-measurement", 5, seed=19, meas="block"),
    Case("supplied-process-drawn-measurement", 5, seed=20, process="block"),
    Case("descriptor-noise-drawn-process", 6, seed=21, meas=None, noise=True),
    Case("measurement-only", 3, seed=22, process=None),
]

ENSEMBLES = [
    Case("plants1", 4, seed=31, n_plants=1),
    Case("plants2", 4, seed=32, n_plants=2),
    Case("plants3-nd0", 5, nd=0, seed=33, n_plants=3),
    Case("plantsS", 3, seed=34, n_plants=-1, process=None, meas=None),
    Case("plants-index", 4, seed=35, n_plants=5, index=True),
    Case("plants3-offset", 4, seed=36, n_plants=3, scenario_offset=1000001),
    Case("plants4-nx12-nd0", 12, nd=0, seed=37, n_plants=4, index=True, pbox=0.6),
]

SIZES = [Case(f"size-S{S}-T{T}", 5, seed=55, S=S, T=T, pool=1000, n_plants=3) for T in (1, 2) for S in (1, 255, 256, 257, 1000)]

COST = [Case("cost-obs", 4, nu=3, ny=2, nd=1, seed=61, T=8, cost=True, x0=0.3),
        Case("cost-noobs", 4, nu=3, ny=2, nd=1, seed=61, T=8, cost=True, x0=0.3, observer=False)]
WARM = [Case("warm", 6, seed=62, warm=True, pbox=1.0), Case("cold", 6, seed=62, pbox=1.0)]
SHARD = Case("shard-1000", 4, seed=63, S=1000, T=3, n_plants=3, scenario_offset=7)
CONTINUE = Case("continue-T6", 5, seed=64, T=6, step_offset=11)
TWIN = Case("twin", 6, seed=65, S=70, T=7, nw=3, meas="block", n_plants=2, index=True)
RERUN = [Case(f"rerun-S{S}", 4, nu=3, ny=2, nd=1, seed=61, S=S, T=4, cost=True, pool=2000, n_plants=2) for S in (200, 2000, 50)]
PLAIN = Case("everything-off", 5, seed=66, process=None, meas=None, noise=True, warm=True)
LIST = Case("simulation-list", 4, seed=67, n_plants=3, meas=None)

CASES = STATES + DRAWS + ENSEMBLES + SIZES + COST + WARM + [SHARD, CONTINUE, TWIN] + RERUN + [PLAIN, LIST]


# ------------------------------------------------------------------ the robust chapter's worst case
def robust_problem():
    """oracle.mpc2mpqp.x0_uncertainty_kat without its x0_uncertainty: the double integrator with Np = 25, |u| <= 0.2 and
    soft |y| <= 0.5 on k = 2 .. 25 (docs/src/manual/robust.md: the nominal controller of the chapter)"""
    from oracle import mpc2mpqp as omm
    p = omm.x0_uncertainty_kat()
    p.x0_uncertainty = None
    return p
