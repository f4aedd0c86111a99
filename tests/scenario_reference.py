"""TEST INFRASTRUCTURE: the scenario loop restated on the host, from the documents alone.

`reference_run` is the closed loop of the reference's `Simulation` (src/simulation.jl:37-116) for S scenarios at
once, in the order of operations that include/lmpc_hip.h states for `lmpc_simulate_scenario_device`:

    PRE    ym_j = h_j + sum_i C_ji x_i + sum_q Dd_jq d_q (+ v_j);  y_j the same sum from 0 without h and v when an
           observer runs (simulation.jl:95), y = ym otherwise;  xhat <- mpc_correct_state(xhat, ym, d_k)
           (oracle/observer.py::c_correct) or xhat = x;
           theta = [xhat; r-block; d-block; uprev; p-block]: r column k, or columns k+1 .. k+H with a preview, d and p
           column k, or k .. k+H-1 (simulation.jl:102-104); every trajectory is cut at the T columns of the run and its
           last column held (simulation.jl:69-88, get_preview's min(k + i, end));
    solve  oracle.ldp.solve_batch on the LDP it is given (warm = the previous step's final working set);
    POST   cost / violation of (x_k, u_k);  xhat <- mpc_predict_state(xhat, u, d_k) (c_predict);
           x <- f + F x + G u + Gd d_k by the same row sums;  uprev <- u.

Every sum is written as one numpy elementwise multiply and one elementwise add per term, in index order: numpy never
fuses the two, so each operation is one IEEE-754 binary64 operation and a kernel that keeps the stated order can be
asked to match bit for bit.  Nothing here imports the library or opens a device; the variational (`is_avi`) handle
has another oracle (oracle/avi.py) and can be plugged in through `solve=`, but no case here does: that handle is left
to the composed-loop test of tests/test_gpu_scenario.py.

Also here, because the CPU and the GPU tests share them: the problem family `chain_problem`, the list of cases
`CASES` that the GPU tests run, and `check_conditions`, which keeps a case from passing emptily.
"""
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

from oracle import ldp as oldp
from oracle import mpc2mpqp as omm
from oracle import observer as oobs


# ------------------------------------------------------------------ trajectories
def run_trajectory(a, S, T):
    """(w, Tc) shared or (S, w, Tc) per scenario -> (S, w, T): cut at T columns, the last one held."""
    a = np.asarray(a, float)
    if a.ndim == 2:
        a = np.broadcast_to(a, (S,) + a.shape)
    assert a.ndim == 3 and a.shape[0] == S, a.shape
    return a[..., np.minimum(np.arange(T), a.shape[-1] - 1)]


def _column(a, k):
    return a[..., min(max(k, 0), a.shape[-1] - 1)]


def theta_block(a, w, H, k0, S):
    """Columns k0 .. k0+H-1 (H > 0) or column k0 of a run trajectory, column after column; None -> zeros."""
    cols = max(H, 1)
    if a is None:
        return np.zeros((S, w * cols))
    return np.concatenate([_column(a, k0 + i) for i in range(cols)], axis=1)


# ------------------------------------------------------------------ glue steps, one IEEE operation at a time
def measure(meas, x, dk, vk):
    """rows [h_j, C_j, Dd_j] -> (ym, y0): ym from h_j, y0 the same products added to 0; noise last, into ym only."""
    S, nx = x.shape
    nd = dk.shape[1]
    ny = meas.shape[0]
    ym, y0 = np.empty((S, ny)), np.empty((S, ny))
    for j in range(ny):
        a, b = np.full(S, meas[j, 0]), np.zeros(S)
        for c in range(nx):
            t = meas[j, 1 + c] * x[:, c]
            a = a + t
            b = b + t
        for q in range(nd):
            t = meas[j, 1 + nx + q] * dk[:, q]
            a = a + t
            b = b + t
        if vk is not None:
            a = a + vk[:, j]
        ym[:, j], y0[:, j] = a, b
    return ym, y0


def correct(meas, kt, xh, ym, dk):
    """mpc_correct_state (oracle/observer.py::c_correct) for every scenario; meas (ny, 1+nx+nd), kt (ny, nx)."""
    nx, nd = xh.shape[1], dk.shape[1]
    out = xh.copy()
    for j in range(meas.shape[0]):
        inno = ym[:, j] - meas[j, 0]
        for c in range(nx):
            inno = inno - meas[j, 1 + c] * xh[:, c]
        for q in range(nd):
            inno = inno - meas[j, 1 + nx + q] * dk[:, q]
        for c in range(nx):
            out[:, c] = out[:, c] + kt[j, c] * inno
    return out


def predict(dyn, x, u, dk):
    """mpc_predict_state (c_predict) for every scenario; dyn (nx, 1+nx+nu+nd): rows [f_i, F_i, G_i, Gd_i]."""
    S, nx = x.shape
    nu, nd = u.shape[1], dk.shape[1]
    out = np.empty((S, nx))
    for a in range(nx):
        acc = np.full(S, dyn[a, 0])
        for c in range(nx):
            acc = acc + dyn[a, 1 + c] * x[:, c]
        for l in range(nu):
            acc = acc + dyn[a, 1 + nx + l] * u[:, l]
        for q in range(nd):
            acc = acc + dyn[a, 1 + nx + nu + q] * dk[:, q]
        out[:, a] = acc
    return out


def _quad(M, a, b):
    """sum_j a_j * (sum_l M_jl b_l): inner and outer sums from 0 in index order."""
    s = np.zeros(a.shape[0])
    for j in range(M.shape[0]):
        t = np.zeros(a.shape[0])
        for l in range(M.shape[1]):
            t = t + M[j, l] * b[:, l]
        s = s + a[:, j] * t
    return s


def step_cost(cost, x, u, ulast, rk):
    """One step's term of evaluate_cost (utils.jl:403-409), not halved: e'Qe + u'Ru + du'Rr du + x'Su added to 0 in
    that order, e = C x - r_k.  Absent weights add nothing."""
    S = x.shape[0]
    c = np.zeros(S)
    C, Q = cost.get("C"), cost.get("Q")
    if C is not None and Q is not None:
        e = np.empty((S, C.shape[0]))
        for j in range(C.shape[0]):
            t = np.zeros(S)
            for a in range(x.shape[1]):
                t = t + C[j, a] * x[:, a]
            e[:, j] = t - (rk[:, j] if rk is not None else 0.0)
        c = c + _quad(Q, e, e)
    if cost.get("R") is not None:
        c = c + _quad(cost["R"], u, u)
    if cost.get("Rr") is not None:
        du = u - ulast
        c = c + _quad(cost["Rr"], du, du)
    if cost.get("S") is not None:
        c = c + _quad(cost["S"], x, u)
    return c


def step_violation(cost, x, u):
    """One step of constraint_violation (utils.jl:417-420): max over the rows of max(lb - v, v - ub, 0) with
    v = Ax x + Au u (Ax terms first, from 0, index order)."""
    S = x.shape[0]
    worst = np.zeros(S)
    lb = cost.get("lb")
    for j in range(0 if lb is None else len(lb)):
        v = np.zeros(S)
        if cost.get("Ax") is not None:
            for a in range(x.shape[1]):
                v = v + cost["Ax"][j, a] * x[:, a]
        if cost.get("Au") is not None:
            for l in range(u.shape[1]):
                v = v + cost["Au"][j, l] * u[:, l]
        lo, hi = lb[j] - v, v - cost["ub"][j]
        worst = np.where(lo > worst, lo, worst)
        worst = np.where(hi > worst, hi, worst)
    return worst


def stored_cost(cost, xs, us, rs=None):
    """evaluate_cost on stored step-major trajectories xs (>= T, S, nx), us (T, S, nu), rs (S, w, T) or None: the
    steps' terms added to 0 in the order k = 0, 1, ..., du against u_{-1} = 0, the half last."""
    T, S, nu = us.shape
    run, ulast = np.zeros(S), np.zeros((S, nu))
    for k in range(T):
        run = run + step_cost(cost, xs[k], us[k], ulast, None if rs is None else _column(rs, k))
        ulast = us[k]
    return 0.5 * run


def stored_violation(cost, xs, us):
    """constraint_violation per step (T, S) and its maximum over the steps (S,)."""
    steps = np.array([step_violation(cost, xs[k], us[k]) for k in range(us.shape[0])])
    worst = np.zeros(us.shape[1])
    for k in range(us.shape[0]):
        worst = np.where(steps[k] > worst, steps[k], worst)
    return steps, worst


def popcount(act):
    return np.unpackbits(np.ascontiguousarray(act).view(np.uint8), axis=-1).sum(axis=-1)


# ------------------------------------------------------------------ the loop
def reference_run(ldp, dims, plant, x0, T, r=None, d=None, p=None, noise=None, observer=None, previews=(0, 0, 0),
                  uprev0=None, warm=False, cost=None, settings=None, solve=None):
    """dims = (nx, nu, wr, nd, nuprev, wp): wr / wp the widths of ONE column of the r / p block of theta (0 = no such
    block).  plant: an object with F, G, Gd, f_offset, C, Dd, h_offset (the true plant).  x0 (S, nx).  r, d, p, noise:
    (w, Tc) shared or (S, w, Tc) per scenario or None.  observer: (MPC_PLANT_DYNAMICS, MPC_MEASUREMENT_FUNCTION,
    K_TRANSPOSE_OBSERVER) flat, or None.  previews = (rH, dH, pH): Np or 0.  cost: dict with any of C, Q, R, Rr, S,
    Ax, Au, lb, ub.  solve(theta, warm_words) -> (u, flags, active words) replaces the LDP oracle.

    Returns a namespace: xs (T+1, S, nx), us, xhats, yms, ys, ds, thetas (T, S, .), flags, active (T, S, words),
    active_sizes (T, S), noise_acted (ym differs from the noise-free measurement), flag_min, cost, violation (S,), violation_steps (T, S)."""
    nx, nu, wr, nd, nup, wp = dims
    rH, dH, pH = previews
    x = np.array(x0, float).reshape(-1, nx)
    S = x.shape[0]
    ny = plant.C.shape[0]
    pdyn = np.hstack([plant.f_offset[:, None], plant.F, plant.G, plant.Gd.reshape(nx, nd)])
    pmeas = np.hstack([plant.h_offset[:, None], plant.C, plant.Dd.reshape(ny, nd)])
    if observer is not None:
        odyn = np.asarray(observer[0], float).reshape(nx, 1 + nx + nu + nd)
        omeas = np.asarray(observer[1], float).reshape(ny, 1 + nx + nd)
        okt = np.asarray(observer[2], float).reshape(ny, nx)
    rt, dt, pt, vt = (None if a is None else run_trajectory(a, S, T) for a in (r, d, p, noise))
    if wr == 0:
        rt = None                                         # no reference in theta: the loop's cost sees zeros
    uprev = np.tile(np.zeros(nup) if uprev0 is None else np.asarray(uprev0, float)[:nup], (S, 1))
    xhat = x.copy()                                       # set_state!(mpc, x0), simulation.jl:92
    if solve is None:
        solve = lambda th, wm: tuple(oldp.solve_batch(ldp, th, settings, warm=wm)[i] for i in (0, 1, 3))
    out = SimpleNamespace(xs=[x.copy()], us=[], xhats=[], yms=[], ys=[], ds=[], thetas=[], flags=[], active=[],
                          noise_acted=False)
    run, ulast, worst, vsteps, act = np.zeros(S), np.zeros((S, nu)), np.zeros(S), [], None
    for k in range(T):
        dk = np.zeros((S, nd)) if dt is None else _column(dt, k)
        ym, y0 = measure(pmeas, x, dk, None if vt is None else _column(vt, k))
        if vt is not None and not np.array_equal(ym, measure(pmeas, x, dk, None)[0]):
            out.noise_acted = True
        if observer is not None:
            xhat = correct(omeas, okt, xhat, ym, dk)
        else:
            xhat = x.copy()
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
            xhat = predict(odyn, xhat, u, dk)
        x = predict(pdyn, x, u, dk)
        uprev = u[:, :nup].copy()
        out.xs.append(x.copy())
    for key in ("xs", "us", "xhats", "yms", "ys", "ds", "thetas", "flags", "active"):
        setattr(out, key, np.array(getattr(out, key)))
    out.flag_min = out.flags.min(axis=0).astype(np.int32)
    out.xhat_final, out.uprev_final = xhat, uprev          # the observer's state after the last predict, the last u
    out.active_sizes = popcount(out.active)
    out.cost = 0.5 * run if cost is not None else None
    out.violation = worst if cost is not None else None
    out.violation_steps = np.array(vsteps) if cost is not None else None
    return out


# ------------------------------------------------------------------ the problem family
def chain_problem(nx, nu, ny, nd, np_=0, Np=5, Nc=3, previews=(False, False, False), soft=False, seed=0, rr=True,
                  ubound=0.3):
    """A random stable plant of the given sizes as an oracle MPCProblem with a Kalman filter for it: F scaled to
    spectral radius 0.9, random G, C, Gd, Dd and offsets, |u| <= ubound, Rr > 0 (theta carries uprev) unless rr is
    False, an affine input cost Eu p with np_ > 0 (the condensing then allows no f_offset), optionally one soft bound on
    the first output.  Returns (problem, observer)."""
    rng = np.random.default_rng(1000 + seed)
    F = rng.standard_normal((nx, nx))
    F *= 0.9 / np.abs(np.linalg.eigvals(F)).max()
    G = rng.standard_normal((nx, nu))
    C = rng.standard_normal((ny, nx))
    Gd = 0.3 * rng.standard_normal((nx, nd)) if nd else None
    Dd = 0.3 * rng.standard_normal((ny, nd)) if nd else None
    prob = omm.make_mpc(F, G, C, Np=Np, Nc=Nc, Q=np.ones(ny), R=0.1 * np.ones(nu), Rr=0.05 * np.ones(nu) if rr else None,
                        umin=-ubound * np.ones(nu), umax=ubound * np.ones(nu), Gd=Gd, Dd=Dd)
    prob.h_offset = 0.1 * rng.standard_normal(ny)
    prob.f_offset = 0.05 * rng.standard_normal(nx) if np_ == 0 else np.zeros(nx)
    prob.reference_preview, prob.disturbance_preview, prob.parameter_preview = (bool(v) for v in previews)
    if np_:
        prob.Eu = 0.2 * rng.standard_normal((nu, np_))
    if soft:
        prob.add_constraint(Ax=C[:1], lb=[-0.4], ub=[0.4], ks=range(2, Np + 1), soft=True)
    kf = oobs.kalman_filter(F, G, C, Gd=Gd, Dd=Dd, f_offset=prob.f_offset, h_offset=prob.h_offset,
                            Q=np.ones(nx), R=1e-2 * np.ones(ny))
    return prob, kf


def plant_of(prob):
    """The true plant of a problem as plain arrays (what reference_run reads)."""
    nx, ny, nd = prob.nx, prob.ny, prob.nd
    z = lambda a, shape: np.zeros(shape) if a is None else np.asarray(a, float).reshape(shape)
    return SimpleNamespace(F=prob.F, G=prob.G, C=prob.C, Gd=z(prob.Gd, (nx, nd)), Dd=z(prob.Dd, (ny, nd)),
                           f_offset=z(prob.f_offset, (nx,)), h_offset=z(prob.h_offset, (ny,)))


def dims_of(prob):
    """(nx, nu, wr, nd, nuprev, wp) of reference_run and the preview lengths (rH, dH, pH) of a problem."""
    nx, nr, ndw, nup, npw = prob.parameter_dims()
    dims = (nx, prob.nu, prob.ny if nr else 0, prob.nd, nup, prob.np_base())
    previews = (prob.Np if (prob.reference_preview and nr) else 0, prob.Np if (prob.disturbance_preview and prob.nd) else 0,
                prob.Np if (prob.parameter_preview and prob.np_base()) else 0)
    return dims, previews


def host_ldp(prob):
    """The problem condensed and transformed on the host (oracle.mpc2mpqp + oracle.ldp.qp2ldp), nout = nu."""
    q = omm.mpc2mpqp(prob)
    return oldp.qp2ldp(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, nout=prob.nu, K=prob.K)


# ------------------------------------------------------------------ the cases of the GPU tests
@dataclass
class Case:
    name: str
    nx: int
    nu: int = 2
    ny: int = 3
    nd: int = 2
    np_: int = 0
    Np: int = 5
    Nc: int = 3
    previews: tuple = (False, False, False)
    soft: bool = False
    seed: int = 0
    S: int = 300
    T: int = 12
    observer: bool = True
    noise: bool = True
    warm: bool = False
    x0: float = 1.0                    # x0 uniform in [-x0, x0]
    lengths: tuple = (None, None, None)   # columns of r, d, p (None = T)
    shared: tuple = (False, False, False)    # r, d, p: one trajectory for all scenarios (stride 0)
    cost: bool = False
    pool: int = 0                      # > 0: the scenarios are the first S of a pool of this many
    extra: dict = field(default_factory=dict)


def case_data(case):
    """Everything a run of `case` needs: problem, observer, x0, trajectories, cost.  Deterministic in the case; with
    `pool` the first S scenarios of the pool's draw, so that the members of a size sweep are cuts of one another."""
    prob, kf = chain_problem(case.nx, case.nu, case.ny, case.nd, case.np_, case.Np, case.Nc, case.previews, case.soft,
                             case.seed)
    rng = np.random.default_rng(77 + case.seed)
    n = max(case.pool, case.S)
    T, S = case.T, case.S
    x0 = rng.uniform(-case.x0, case.x0, (n, case.nx))[:S]
    lens = [T if l is None else l for l in case.lengths]

    def traj(w, cols, shared, lo, hi):
        a = rng.uniform(lo, hi, (n, w, max(cols, 1)))
        return None if w == 0 else (a[0] if shared else a[:S])

    r = traj(case.ny, lens[0], case.shared[0], -0.5, 0.5)
    d = traj(case.nd, lens[1], case.shared[1], -0.3, 0.3)
    p = traj(case.np_, lens[2], case.shared[2], -1.0, 1.0)
    noise = 0.01 * rng.standard_normal((n, case.ny, T))[:S] if case.noise else None
    cost = None
    if case.cost:
        nx, nu, ny = case.nx, case.nu, case.ny
        Q = rng.uniform(0.5, 2.0, (ny, ny)); Q = Q @ Q.T
        cost = dict(C=prob.C.copy(), Q=Q, R=np.diag(rng.uniform(0.1, 1.0, nu)), Rr=rng.uniform(-0.5, 0.5, (nu, nu)),
                    S=rng.uniform(-0.3, 0.3, (nx, nu)), Ax=rng.standard_normal((4, nx)), Au=rng.standard_normal((4, nu)),
                    lb=-rng.uniform(0.3, 1.0, 4), ub=rng.uniform(0.3, 1.0, 4))
    return SimpleNamespace(prob=prob, kf=kf if case.observer else None, x0=x0, r=r, d=d, p=p, noise=noise, cost=cost)


def run_case(case, ldp, data=None, settings=None):
    """reference_run of a case on the LDP it is given."""
    data = case_data(case) if data is None else data
    dims, previews = dims_of(data.prob)
    obs = None if data.kf is None else data.kf.codegen_arrays()
    return reference_run(ldp, dims, plant_of(data.prob), data.x0, case.T, r=data.r, d=data.d, p=data.p, noise=data.noise,
                         observer=obs, previews=previews, uprev0=getattr(data.prob, "uprev0", None), warm=case.warm,
                         cost=data.cost, settings=settings)


def check_conditions(case, ref, sim=None):
    """What keeps a case from passing emptily, from the reference's run (and, given `sim`, again from the GPU's
    arrays): every scenario solved; both solver outcomes -- empty and non-empty final working set -- on at least 5 %
    of the scenario-steps each; the observer, the noise, the soft row, the cost rows and the warm start really acted.

    5 % of the scenario-steps is less than one step below 20 of them, and S = 1 with T = 1 cannot hold both
    outcomes at all: a case with fewer than 40 scenario-steps is a cut of its pool (`pool`), and the share is asked of
    the pool's member, which the same sweep runs."""
    assert ref.flag_min.min() >= 1, (case.name, int(ref.flag_min.min()))
    if sim is not None:
        assert sim.flag_min.min() >= 1
    if case.S * case.T >= 40:
        share = float((ref.active_sizes > 0).mean())
        assert 0.05 <= share <= 0.95, (case.name, "share of scenario-steps with a non-empty working set", share)
    else:
        assert case.pool * case.T >= 40, case.name
    if case.observer:
        assert np.abs(ref.xhats - ref.xs[:-1]).max() > 0
        if sim is not None:
            assert np.abs(sim.xhats - sim.xs).max() > 0
    if case.noise:                                        # (without an observer ys IS yms, simulation.jl:95)
        assert ref.noise_acted
        if case.observer:
            assert not np.array_equal(ref.yms, ref.ys)
            if sim is not None:
                assert not np.array_equal(sim.yms, sim.ys)
    if case.soft:
        assert (ref.flags == 2).any(), (case.name, "no scenario-step ends on the soft row")
    if case.cost:
        assert ref.violation.max() > 0
        if sim is not None:
            assert sim.violation.max() > 0
    if case.warm:
        assert case.T > 1 and not np.array_equal(ref.active[1:], ref.active[:-1]), (case.name, "warm start never differs")


def _sweep():
    out = []
    for nx in (1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 32):
        for observer in (False, True):
            for warm in (False, True):
                out.append(Case(f"nx{nx}-{'obs' if observer else 'noobs'}-{'warm' if warm else 'cold'}", nx, seed=nx,
                                observer=observer, warm=warm, x0=X0_RANGE.get(nx, 1.0)))
    return out


X0_RANGE = {32: 3.0}       # x0 range per nx of the sweep where 1.0 does not give both solver outcomes

SWEEP = _sweep()

# r, d and p previews at once with nuprev = nu: nth = nx + Np (ny + nd + np) + nu
PREVIEWS = [
    # nth = 4 + 5 * 4 + 2 = 26: 16 < nth <= 32; r shorter than the run, d one shared trajectory, no observer
    Case("previews-nth26", 4, ny=2, nd=1, np_=1, Np=5, previews=(True, True, True), seed=41, T=10, observer=False,
         lengths=(6, 4, None), shared=(False, True, False), warm=True),
    # nth = 6 + 8 * 7 + 2 = 64: the wide record; p shorter than the run and shared, soft output row
    Case("previews-nth64", 6, ny=3, nd=2, np_=2, Np=8, Nc=3, previews=(True, True, True), seed=42, T=10, soft=True,
         lengths=(7, None, 5), shared=(False, False, True)),
]

SIZES = [Case(f"size-nx{nx}-S{S}-T{T}", nx, seed=50 + nx, S=S, T=T, pool=1000)
         for nx in (5, 12) for T in (1, 2) for S in (1, 255, 256, 257, 1000)]

# cost inside the loop: observer and Rr together (the two-part scratch), nu = 3, C / Q with ny = 2, S, nc = 4
COST = Case("cost-nx4-nu3", 4, nu=3, ny=2, nd=1, seed=61, T=8, soft=True, cost=True, x0=0.3)
RERUN = [Case(f"rerun-S{S}", 4, nu=3, ny=2, nd=1, seed=61, S=S, T=6, cost=True, pool=2000) for S in (200, 2000, 50)]
SCORING = [Case("scoring-nx32-nu8", 32, nu=8, ny=2, nd=1, seed=71, S=300, T=6, cost=True, x0=3.0),
           Case("scoring-nx3", 3, nu=2, ny=2, nd=1, seed=72, S=300, T=6, cost=True, x0=1.0)]
TWIN = Case("twin-nx6", 6, seed=81, S=70, T=7)

CASES = SWEEP + PREVIEWS + SIZES + [COST] + RERUN + SCORING + [TWIN]
