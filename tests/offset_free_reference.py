"""TEST INFRASTRUCTURE: the scenario loop with the reference's offset-free observer, restated on the host.

What tests/scenario_reference.py is for `lmpc_simulate_scenario_device`, this is for
`lmpc_simulate_scenario_offset_free_device` (include/lmpc_hip.h).  The glue steps -- `measure`, `correct`, `predict`,
`theta_block`, `step_cost`, `step_violation` -- are imported from there; only what is new lives here:

    build_observer     set_offset_free_observer!'s augmented filter (reference src/setup.jl:392-448) with the Riccati
                       gains of oracle.observer.kalman_filter
    d_block            the d block of theta: max(H, 1) columns [d column k + c, held at the last; dhat]
                       (get_control_disturbance, src/observer.jl:203-222; format_disturbance, src/utils.jl:155-205)
    reference_run      the loop (src/simulation.jl:37-116 with an OffsetFreeObserver as mpc.state_observer)

Dimensions: nx plant and controller state, ndm measured disturbances (rows of the scenario's d, columns of the plant's
Gd / Dd), ndo estimated ones, na = nx + ndo the observer's state, the controller's model.nd = ndm + ndo.

Nothing here imports the library or opens a device.  Also here, shared by the CPU and the GPU tests: the problem
family `case_data`, the cases, and `check_conditions`.
"""
import copy
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from oracle import ldp as oldp
from oracle import observer as oobs

from scenario_reference import (_column, chain_problem, correct, host_ldp, measure, plant_of, popcount, predict,
                                run_trajectory, step_cost, step_violation, theta_block)

METHODS = {"state": "state_disturbance", "state_disturbance": "state_disturbance", "velocity": "velocity",
           "output": "output_disturbance", "output_disturbance": "output_disturbance", "general": "general"}


# ------------------------------------------------------------------ the augmented filter
def build_observer(F, G, C, Gd=None, Dd=None, f_offset=None, h_offset=None, method="state_disturbance", Q=None, R=None,
                   K=None, Bd=None, Cd=None, Kx=None, Kd=None):
    """build_offset_free_observer (setup.jl:392-448), statement for statement; Gd / Dd are the MEASURED columns
    (model.Gd[:, 1:nd_measured]).  Returns the estimator's arrays, Bd, Cd and the dimensions."""
    method = METHODS[method]
    F = np.atleast_2d(np.asarray(F, float))
    nx = F.shape[0]
    G = np.asarray(G, float).reshape(nx, -1)
    C = np.atleast_2d(np.asarray(C, float))
    ny, nu = C.shape[0], G.shape[1]
    Gd = np.zeros((nx, 0)) if Gd is None else np.asarray(Gd, float).reshape(nx, -1)
    ndm = Gd.shape[1]
    Dd = np.zeros((ny, ndm)) if Dd is None else np.asarray(Dd, float).reshape(ny, ndm)
    f_offset = np.zeros(nx) if f_offset is None else np.asarray(f_offset, float).reshape(nx)
    h_offset = np.zeros(ny) if h_offset is None else np.asarray(h_offset, float).reshape(ny)
    if method in ("state_disturbance", "velocity"):
        if K is None:                                     # nominal_observer_gain, setup.jl:377-380
            K = oobs.kalman_filter(F, np.zeros((nx, ny)), C, Q=Q, R=R).K
        K = np.asarray(K, float).reshape(nx, ny)
        Bd, Cd, Kx, Kd = K, np.eye(ny) - C @ K, K, np.eye(ny)
    elif method == "output_disturbance":
        Bd, Cd = np.zeros((nx, ny)), np.eye(ny)
    Bd, Cd = np.asarray(Bd, float), np.asarray(Cd, float)
    ndo = Bd.shape[1]
    assert Bd.shape[0] == nx and Cd.shape == (ny, ndo)
    if np.linalg.matrix_rank(np.block([[F - np.eye(nx), Bd], [C, Cd]])) != nx + ndo:     # setup.jl:382-390
        raise ValueError("Offset-free disturbance model violates rank([F-I Bd; C Cd]) = nx + nd")
    Faug = np.block([[F, Bd], [np.zeros((ndo, nx)), np.eye(ndo)]])
    Gaug = np.vstack([G, np.zeros((ndo, nu))])
    Gdaug = np.vstack([Gd, np.zeros((ndo, ndm))])
    Caug = np.hstack([C, Cd])
    faug = np.concatenate([f_offset, np.zeros(ndo)])
    if Kx is not None or Kd is not None:
        Kx = np.zeros((nx, ny)) if Kx is None else np.asarray(Kx, float).reshape(nx, ny)
        Kd = np.zeros((ndo, ny)) if Kd is None else np.asarray(Kd, float).reshape(ndo, ny)
        Kaug = np.vstack([Kx, Kd])
    else:
        Kaug = oobs.kalman_filter(Faug, Gaug, Caug, Gd=Gdaug, Dd=Dd, f_offset=faug, h_offset=h_offset, Q=Q, R=R).K
    est = oobs.KalmanFilter(Faug, Gaug, Gdaug, faug, Caug, Dd, h_offset, Kaug)
    return SimpleNamespace(estimator=est, codegen_arrays=est.codegen_arrays, nx=nx, nu=nu, ny=ny, nd_measured=ndm,
                           nd_offsetfree=ndo, Bd=Bd, Cd=Cd, K=Kaug, method=method)


# ------------------------------------------------------------------ the d block of theta
def d_block(dt, dhat, ndm, H, k):
    """dt: the run's measured trajectory (S, ndm, T) or None (zeros; no rows with ndm == 0); dhat (S, ndo).
    max(H, 1) columns, column c = [dt column k + c (held at the last); dhat]."""
    S = dhat.shape[0]
    cols = []
    for c in range(max(H, 1)):
        cols.append(np.zeros((S, ndm)) if dt is None else _column(dt, k + c))
        cols.append(dhat)
    return np.concatenate(cols, axis=1)


# ------------------------------------------------------------------ the loop
def reference_run(ldp, dims, plant, observer, x0, T, r=None, d=None, p=None, noise=None, previews=(0, 0, 0), uprev0=None,
                  warm=False, cost=None, settings=None, xaug0=None, solve=None):
    """dims = (nx, nu, wr, ndm, nuprev, wp) as scenario_reference.reference_run's, with ndm the MEASURED disturbances;
    plant: the true plant (Gd / Dd of ndm columns); observer: build_observer's result.  xaug0 (S, na) or None = [x0; 0]
    (set_state!, observer.jl:74-90).  Returns scenario_reference's namespace plus dhats (T, S, ndo) and xaug_final."""
    nx, nu, wr, ndm, nup, wp = dims
    rH, dH, pH = previews
    ndo, ny = observer.nd_offsetfree, plant.C.shape[0]
    na = nx + ndo
    x = np.array(x0, float).reshape(-1, nx)
    S = x.shape[0]
    pdyn = np.hstack([plant.f_offset[:, None], plant.F, plant.G, plant.Gd.reshape(nx, ndm)])
    pmeas = np.hstack([plant.h_offset[:, None], plant.C, plant.Dd.reshape(ny, ndm)])
    oa = observer.codegen_arrays()
    odyn = np.asarray(oa[0], float).reshape(na, 1 + na + nu + ndm)
    omeas = np.asarray(oa[1], float).reshape(ny, 1 + na + ndm)
    okt = np.asarray(oa[2], float).reshape(ny, na)
    rt, dt, pt, vt = (None if a is None else run_trajectory(a, S, T) for a in (r, d, p, noise))
    if wr == 0:
        rt = None
    if ndm == 0:
        dt = None
    uprev = np.tile(np.zeros(nup) if uprev0 is None else np.asarray(uprev0, float)[:nup], (S, 1))
    xaug = np.hstack([x, np.zeros((S, ndo))]) if xaug0 is None else np.array(xaug0, float).reshape(S, na)
    if solve is None:
        solve = lambda th, wm: tuple(oldp.solve_batch(ldp, th, settings, warm=wm)[i] for i in (0, 1, 3))
    out = SimpleNamespace(xs=[x.copy()], us=[], xhats=[], dhats=[], yms=[], ys=[], ds=[], thetas=[], flags=[], active=[],
                          noise_acted=False)
    run, ulast, worst, vsteps, act = np.zeros(S), np.zeros((S, nu)), np.zeros(S), [], None
    for k in range(T):
        dk = np.zeros((S, ndm)) if dt is None else _column(dt, k)
        ym, y0 = measure(pmeas, x, dk, None if vt is None else _column(vt, k))
        if vt is not None and not np.array_equal(ym, measure(pmeas, x, dk, None)[0]):
            out.noise_acted = True
        xaug = correct(omeas, okt, xaug, ym, dk)
        xhat, dhat = xaug[:, :nx].copy(), xaug[:, nx:].copy()            # both AFTER the correction
        theta = np.concatenate([xhat, theta_block(rt, wr, rH, k + 1 if rH else k, S) if wr else np.zeros((S, 0)),
                                d_block(dt, dhat, ndm, dH, k), uprev,
                                theta_block(pt, wp, pH, k, S) if wp else np.zeros((S, 0))], axis=1)
        u, flag, act = solve(theta, act if (warm and k > 0) else None)
        if cost is not None:
            run = run + step_cost(cost, x, u, ulast, None if rt is None else _column(rt, k))
            ulast = u
            vsteps.append(step_violation(cost, x, u))
            worst = np.where(vsteps[-1] > worst, vsteps[-1], worst)
        for key, val in (("us", u), ("xhats", xhat), ("dhats", dhat), ("yms", ym), ("ys", y0), ("ds", dk), ("thetas", theta),
                         ("flags", flag), ("active", act)):
            getattr(out, key).append(np.array(val))
        xaug = predict(odyn, xaug, u, dk)
        x = predict(pdyn, x, u, dk)
        uprev = u[:, :nup].copy()
        out.xs.append(x.copy())
    for key in ("xs", "us", "xhats", "dhats", "yms", "ys", "ds", "thetas", "flags", "active"):
        setattr(out, key, np.array(getattr(out, key)))
    out.flag_min = out.flags.min(axis=0).astype(np.int32)
    out.xaug_final, out.uprev_final = xaug, uprev
    out.active_sizes = popcount(out.active)
    out.cost = 0.5 * run if cost is not None else None
    out.violation = worst if cost is not None else None
    return out


# ------------------------------------------------------------------ the problem family and the cases
@dataclass
class Case:
    name: str
    nx: int
    ny: int = 3
    ndm: int = 2
    method: str = "velocity"
    preview: bool = False              # disturbance preview: Np columns [d; dhat] in theta
    nu: int = 2
    Np: int = 5
    Nc: int = 3
    seed: int = 0
    S: int = 300
    T: int = 12
    noise: bool = True
    warm: bool = False
    x0: float = 1.0                    # x0 uniform in [-x0, x0]
    cost: bool = False
    pool: int = 0                      # > 0: the scenarios are the first S of a pool of this many
    xaug: bool = False                 # the caller keeps xaug (and starts it away from [x0; 0])

    @property
    def ndo(self):
        return self.ny                 # velocity: Bd = K, Cd = I - C K; output: Bd = 0, Cd = I -- ny channels either way


def case_data(case):
    """chain_problem's family: the nominal model (its offsets included) gives the observer; the controller is condensed
    on Gd = [Gd Bd], Dd = [Dd Cd]; the TRUE plant carries an unknown bias of 0.05 N(0, 1) on f_offset."""
    base, _ = chain_problem(case.nx, case.nu, case.ny, case.ndm, 0, case.Np, case.Nc, (False, case.preview, False),
                            seed=case.seed)
    nx, ny, ndm = case.nx, case.ny, case.ndm
    Gd = np.zeros((nx, 0)) if base.Gd is None else base.Gd
    Dd = np.zeros((ny, 0)) if base.Dd is None else base.Dd
    obs = build_observer(base.F, base.G, base.C, Gd=Gd, Dd=Dd, f_offset=base.f_offset, h_offset=base.h_offset,
                         method=case.method, Q=np.ones(nx if METHODS[case.method] == "velocity" else nx + ny),
                         R=1e-2 * np.ones(ny))
    ctrl = copy.deepcopy(base)
    ctrl.Gd, ctrl.Dd = np.hstack([Gd, obs.Bd]), np.hstack([Dd, obs.Cd])
    ctrl.disturbance_preview = case.preview
    rng = np.random.default_rng(177 + case.seed)
    true = plant_of(base)
    true.Gd, true.Dd = Gd, Dd
    true.f_offset = true.f_offset + 0.05 * rng.standard_normal(nx)
    n = max(case.pool, case.S)
    T, S = case.T, case.S
    x0 = rng.uniform(-case.x0, case.x0, (n, nx))[:S]
    r = rng.uniform(-0.5, 0.5, (n, ny, T))[:S]
    d = rng.uniform(-0.3, 0.3, (n, ndm, T))[:S] if ndm else None
    noise = 0.01 * rng.standard_normal((n, ny, T))[:S] if case.noise else None
    xaug0 = np.hstack([x0 + 0.05 * rng.standard_normal((n, nx))[:S], 0.02 * rng.standard_normal((n, ny))[:S]]) \
        if case.xaug else None
    cost = None
    if case.cost:
        nu = case.nu
        Q = rng.uniform(0.5, 2.0, (ny, ny)); Q = Q @ Q.T
        cost = dict(C=base.C.copy(), Q=Q, R=np.diag(rng.uniform(0.1, 1.0, nu)), Rr=rng.uniform(-0.5, 0.5, (nu, nu)),
                    S=rng.uniform(-0.3, 0.3, (nx, nu)), Ax=rng.standard_normal((4, nx)), Au=rng.standard_normal((4, nu)),
                    lb=-rng.uniform(0.3, 1.0, 4), ub=rng.uniform(0.3, 1.0, 4))
    return SimpleNamespace(base=base, prob=ctrl, plant=true, obs=obs, x0=x0, r=r, d=d, noise=noise, cost=cost, xaug0=xaug0)


def dims_of(case, prob):
    """(nx, nu, wr, ndm, nuprev, wp) and (rH, dH, pH) of reference_run for a case's controller"""
    nx, nr, _, nup, _ = prob.parameter_dims()
    return (nx, case.nu, case.ny if nr else 0, case.ndm, nup, 0), (0, case.Np if case.preview else 0, 0)


def run_case(case, ldp, data=None, settings=None):
    data = case_data(case) if data is None else data
    dims, previews = dims_of(case, data.prob)
    return reference_run(ldp, dims, data.plant, data.obs, data.x0, case.T, r=data.r, d=data.d, noise=data.noise,
                         previews=previews, warm=case.warm, cost=data.cost, settings=settings, xaug0=data.xaug0)


def check_conditions(case, ref, sim=None):
    """What keeps a case from passing emptily: every flag >= 1; both solver outcomes on 5 % .. 95 % of the
    scenario-steps (a case of fewer than 40 scenario-steps is a cut of its pool, whose member the same sweep runs);
    a disturbance estimate that is not zero; an estimate that is not the true state; noise and cost rows that acted."""
    assert ref.flags.min() >= 1, (case.name, int(ref.flags.min()))
    if sim is not None:
        assert sim.flag_min.min() >= 1
    if case.S * case.T >= 40:
        share = float((ref.active_sizes > 0).mean())
        assert 0.05 <= share <= 0.95, (case.name, "share of scenario-steps with a non-empty working set", share)
    else:
        assert case.pool * case.T >= 40, case.name
    assert np.abs(ref.dhats).max() > 0
    assert not np.array_equal(ref.xhats, ref.xs[:-1])
    if sim is not None:
        assert np.abs(sim.dhats).max() > 0 and not np.array_equal(sim.xhats, sim.xs)
    if case.noise:
        assert ref.noise_acted and not np.array_equal(ref.yms, ref.ys)
    if case.cost:
        assert ref.violation.max() > 0
    if case.warm:
        assert case.T > 1 and not np.array_equal(ref.active[1:], ref.active[:-1]), (case.name, "warm start never differs")


def _pairs():
    """one case per (nx, ndo) instantiation of the compile-time kernels, nx + ndo <= 8; ndm, the method, the preview and
    the warm start alternate over them"""
    out, i = [], 0
    for nx in range(1, 8):
        for ny in range(1, 9 - nx):
            # (an output-disturbance model needs rank [F - I 0; C I] = nx + ny: always there; ny > nx is fine as well)
            method = "output" if i % 3 == 2 else "velocity"
            out.append(Case(f"pair-nx{nx}-ndo{ny}-{method}", nx, ny=ny, ndm=(0, 2, 1)[i % 3], method=method,
                            preview=i % 4 == 1, warm=i % 2 == 1, seed=SEED.get((nx, ny), 100 + i), x0=X0_RANGE.get((nx, ny), 1.0)))
            i += 1
    return out


# x0 range per (nx, ndo) of the pairs where 1.0 gives fewer than 5 % non-empty working sets (0.00 .. 0.04 on the CPU)
X0_RANGE = {(1, 2): 3.0, (1, 3): 3.0, (1, 4): 3.0, (7, 1): 3.0}
SEED = {(1, 1): 1}                     # seed 100 never reaches the input bounds at nx = ny = 1 (share 0.00 at either range)

PAIRS = _pairs()

# the issue's table: shares checked on the CPU (tests/test_offset_free_host.py); nx + ndo = 8 | 9 is the gate between the
# compile-time and the run-time kernels, nx = 29 with ndo = 3 is na = 32
TABLE = [
    Case("t-nx1-vel", 1, ny=1, ndm=0, seed=1),
    Case("t-nx3-vel", 3, ny=3, ndm=2, seed=3),
    Case("t-nx5-out-gate8", 5, ny=3, ndm=2, method="output", seed=5),
    Case("t-nx6-vel-preview-ndm0-gate8", 6, ny=2, ndm=0, preview=True, seed=6),
    Case("t-nx6-vel-gate9", 6, ny=3, ndm=2, seed=6, warm=True),
    Case("t-nx8-out-preview-38", 8, ny=3, ndm=2, method="output", preview=True, seed=8),
    Case("t-nx17-vel", 17, ny=3, ndm=2, seed=17, warm=True),
    Case("t-nx2-preview-range3", 2, ny=1, ndm=1, preview=True, seed=2, x0=3.0),
    Case("t-nx29-na32-range3", 29, ny=3, ndm=1, seed=29, x0=3.0),
]

SIZES = [Case(f"size-nx{nx}-S{S}-T{T}", nx, ny=3, ndm=2, seed=50 + nx, S=S, T=T, pool=1000)
         for nx in (5, 12) for T in (1, 2) for S in (1, 255, 256, 257, 1000)]

COST = Case("cost-nx4", 4, ny=2, ndm=1, seed=61, T=8, cost=True)
XAUG = [Case("xaug-given-nx3", 3, ny=2, ndm=1, seed=62, xaug=True), Case("xaug-given-nx10", 10, ny=2, ndm=1, seed=63, xaug=True)]
RERUN = [Case(f"rerun-S{S}", 4, ny=2, ndm=1, seed=64, S=S, T=6, pool=2000) for S in (200, 2000, 50)]
TWIN = Case("twin-nx6", 6, ny=2, ndm=2, preview=True, seed=81, S=70, T=7)
NOISE_FREE = Case("no-noise-nx4", 4, ny=2, ndm=1, seed=65, noise=False, x0=2.0)

CASES = PAIRS + TABLE + SIZES + [COST] + XAUG + RERUN + [TWIN, NOISE_FREE]
