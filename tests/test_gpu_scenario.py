"""The scenario loop on the GPU (lmpc_simulate_scenario_device): bit for bit against the composition of the entry
points that existed before it AND against the host reference loop of tests/scenario_reference.py (numpy + the CPU
oracle on the handle's own pack, no call into the library) at every state-size instantiation of the glue kernels,
the reference's own closed-loop assertions through `Simulation`, the cost and constraint-violation scoring, and the
independence of scenarios."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


def _mpc(lmpc, p):
    from oracle import mpc2mpqp as omm
    q = omm.mpc2mpqp(p)
    nx, nr, nd, nup, npp = p.parameter_dims()
    mq = lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, is_symmetric=q.is_symmetric)
    mpc = lmpc.MPC(mq, nx=nx, nu=p.nu, nr=nr, nd=nd, nuprev=nup, np_=npp, K=p.K, Np=p.Np,
                   reference_preview=p.reference_preview, disturbance_preview=p.disturbance_preview,
                   parameter_preview=p.parameter_preview)
    if getattr(p, "uprev0", None) is not None:
        mpc.uprev = np.asarray(p.uprev0, float).copy()
    return mpc


def _plant(lmpc, p):
    return lmpc.Plant(p.F, p.G, Gd=p.Gd, f_offset=p.f_offset, C=p.C, Dd=p.Dd, h_offset=p.h_offset)


def _col(a, k):
    """column k (held at the last) of a (w, Tc) or (S, w, Tc) array"""
    return a[..., min(k, a.shape[-1] - 1)]


def _measure(plant, x, dk, vk, offset=True):
    """ym_j = h_j + sum_i C_ji x_i + sum_q Dd_jq d_q (+ v_j): plain float64 elementwise steps in that order (numpy
    never fuses a multiply into an add)"""
    S = x.shape[0]
    out = np.empty((S, plant.ny))
    for j in range(plant.ny):
        acc = np.full(S, plant.h_offset[j]) if offset else np.zeros(S)
        for i in range(plant.nx):
            acc = acc + plant.C[j, i] * x[:, i]
        for q in range(plant.nd):
            acc = acc + plant.Dd[j, q] * dk[:, q]
        if vk is not None:
            acc = acc + vk[:, j]
        out[:, j] = acc
    return out


def _composed(lmpc, mpc, plant, obs, x0, T, r=None, d=None, p=None, noise=None, warm=False):
    """The loop a caller had to stitch together before: correct_state -> form_parameter_device -> solve_device ->
    predict_state (observer) -> the plant step as predict_state on a SECOND handle of the same QP whose observer
    arrays are the plant's.  Returns xs (T+1,S,nx), us, xhats, yms, ys, flag_min."""
    import torch
    model = mpc.control_model()
    q = mpc.mpQP
    twin = lmpc.BatchedQP.from_mpqp(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, nout=mpc.nu,
                                    K=mpc.K if np.any(mpc.K) else None, nx=mpc.nx, settings=mpc.settings,
                                    is_avi=not q.is_symmetric)
    twin.set_observer(plant.dynamics_rows(), np.zeros((1, 1 + plant.nx + plant.nd)), np.zeros((1, plant.nx)),
                      plant.nx, plant.nu, plant.nd, 1)
    if obs is not None:
        model.set_observer(*obs, plant.nx, plant.nu, plant.nd, plant.ny)
    dev = torch.device("cuda", model.device)
    S = x0.shape[0]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x, xhat = t(x0.copy()), t(x0.copy())
    Np = mpc.Np
    rH = Np if (mpc.reference_preview and mpc.nr > 0) else 0
    dH = Np if (mpc.disturbance_preview and mpc.nd > 0) else 0
    pH = Np if (mpc.parameter_preview and mpc.np > 0) else 0
    rr = r
    if r is not None and rH:                  # preview of r starts one column later (simulation.jl:102)
        rr = r[..., np.minimum(np.arange(r.shape[-1]) + 1, r.shape[-1] - 1)]
    if r is None and mpc.nr > 0:
        rr = np.zeros((mpc.ny, 1))
    dd = d if d is not None else (np.zeros((plant.nd, 1)) if plant.nd else None)
    pp = p if p is not None else (np.zeros((mpc.np_base, 1)) if mpc.np else None)
    rt, dt, pt = t(rr), t(dd), t(pp)
    uprev = t(np.tile(mpc.uprev[:mpc.nuprev], (S, 1))) if mpc.nuprev else None
    act = torch.zeros((S, model.words), dtype=torch.int64, device=dev)
    xs, us, xhats, yms, ys, fmin = [x0.copy()], [], [], [], [], None
    for k in range(T):
        dk = np.zeros((S, plant.nd))
        if d is not None:
            dk = np.ascontiguousarray(np.broadcast_to(_col(d, k), (S, plant.nd)))
        vk = None if noise is None else np.broadcast_to(_col(noise, k), (S, plant.ny))
        xk = x.cpu().numpy()
        ym = _measure(plant, xk, dk, vk)
        yms.append(ym)
        ys.append(_measure(plant, xk, dk, None, offset=False) if obs is not None else ym)
        dkt = t(dk) if plant.nd else None
        if obs is not None:
            model.correct_state(xhat, t(ym), dkt)
        else:
            xhat = x.clone()
        xhats.append(xhat.cpu().numpy())
        theta = model.form_parameter_device(xhat, r=rt, d=dt, uprev=uprev, p=pt, r_preview=rH, d_preview=dH,
                                            p_preview=pH, k0=k)
        u, flag = model.solve_device(theta, active=act if warm else None, warm=act if (warm and k > 0) else None)
        if obs is not None:
            model.predict_state(xhat, u, dkt)
        twin.predict_state(x, u, dkt)
        if mpc.nuprev:
            uprev = u[:, :mpc.nuprev].clone()
        f = flag.cpu().numpy()
        fmin = f if fmin is None else np.minimum(fmin, f)
        us.append(u.cpu().numpy())
        xs.append(x.cpu().numpy())
    twin.close()
    return np.array(xs), np.array(us), np.array(xhats), np.array(yms), np.array(ys), fmin


def _both(lmpc, prob, x0, T, obs=None, warm=False, **traj):
    mpc = _mpc(lmpc, prob)
    plant = _plant(lmpc, prob)
    sim = lmpc.Simulation(mpc, lmpc.Scenario(x0, N=T, **traj), plant, observer=obs, warm=warm)
    ref = _composed(lmpc, mpc, plant, obs, x0, T, warm=warm, **traj)
    if not mpc.control_model().is_avi:                    # the host reference loop as well (its oracle is the LDP one)
        _assert_identical(sim, _host_reference(mpc, prob, x0, T, obs, warm, **traj), T)
    return sim, ref, mpc


def _oracle_settings(mpc):
    from oracle import ldp as oldp
    s = oldp.default_settings()
    for name in ("primal_tol", "dual_tol", "zero_tol", "progress_tol", "fval_bound", "rho_soft", "cycle_tol", "iter_limit"):
        setattr(s, name, getattr(mpc.settings, name))
    return s


def _host_reference(mpc, prob, x0, T, obs=None, warm=False, **traj):
    """reference_run on the handle's own pack, in the tuple _assert_identical reads"""
    import scenario_reference as sr
    from conftest import oracle_ldp_from
    dims, previews = sr.dims_of(prob)
    ref = sr.reference_run(oracle_ldp_from(mpc.control_model().ldp()), dims, sr.plant_of(prob), x0, T, observer=obs,
                           previews=previews, uprev0=getattr(prob, "uprev0", None), warm=warm,
                           settings=_oracle_settings(mpc), **traj)
    return ref.xs, ref.us, ref.xhats, ref.yms, ref.ys, ref.flag_min


def _assert_identical(sim, ref, T):
    xs, us, xhats, yms, ys, fmin = ref
    step = lambda a: a.transpose(1, 2, 0)                 # (T, S, w) -> (S, w, T)
    assert np.array_equal(sim.us, step(us)), np.abs(sim.us - step(us)).max()
    assert np.array_equal(sim.xs, step(xs[:T])) and np.array_equal(sim.x_final, xs[T])
    assert np.array_equal(sim.xhats, step(xhats))
    assert np.array_equal(sim.yms, step(yms)) and np.array_equal(sim.ys, step(ys))
    assert np.array_equal(sim.flag_min, fmin) and fmin.min() >= 1


def _dist_preview_sim(preview):
    """runtests.jl:384-409 "Disturbance Preview Simulation": double integrator, Gd = [0; 1], C = [1 0], Np = Nc = 5,
    |u| <= 0.5, Q = 10, R = 0.1"""
    from oracle import mpc2mpqp as omm
    p = omm.make_mpc([[1, 1], [0, 1]], [[0], [1]], [[1.0, 0.0]], Np=5, Nc=5, Q=[10.0], R=[0.1], umin=[-0.5], umax=[0.5],
                     Gd=[[0], [1]])
    p.disturbance_preview = preview
    return p


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("preview", [True, False])
def test_disturbance_preview_equals_the_composed_loop(lmpc, preview, warm):
    rng = np.random.default_rng(11)
    S, T = 300, 20
    x0 = rng.uniform(-0.5, 0.5, (S, 2))
    d = rng.uniform(-0.3, 0.3, (S, 1, 14))                # shorter than the run: held at the last column
    sim, ref, _ = _both(lmpc, _dist_preview_sim(preview), x0, T, warm=warm, d=d)
    _assert_identical(sim, ref, T)
    assert np.array_equal(sim.ds, d[..., np.minimum(np.arange(T), 13)])


@pytest.mark.parametrize("warm", [False, True])
def test_observer_with_disturbance_and_noise_equals_the_composed_loop(lmpc, warm):
    from oracle import mpc2mpqp as omm
    from oracle import observer as oobs
    p = omm.observer_disturbance_kat()
    kf = oobs.kalman_filter(p.F, p.G, p.C, Gd=p.Gd, Dd=p.Dd, Q=[1.0, 1], R=[1e-2])
    rng = np.random.default_rng(12)
    S, T = 256, 30
    x0 = np.tile([1.0, 0.0], (S, 1)) + rng.uniform(-0.1, 0.1, (S, 2))
    d = 1.0 + rng.uniform(-0.2, 0.2, (S, 2, T))
    noise = 0.01 * rng.standard_normal((S, 1, T))
    sim, ref, _ = _both(lmpc, p, x0, T, obs=kf.codegen_arrays(), warm=warm, d=d, noise=noise, r=np.zeros((1, 1)))
    _assert_identical(sim, ref, T)
    assert np.abs(sim.xhats - sim.xs).max() > 0           # the controller really saw the estimate


@pytest.mark.parametrize("warm", [False, True])
def test_parameter_preview_equals_the_composed_loop(lmpc, warm):
    from oracle import mpc2mpqp as omm
    rng = np.random.default_rng(13)
    S, T = 200, 25
    pt = rng.uniform(-0.5, 1.5, (S, 1, T))
    sim, ref, _ = _both(lmpc, omm.parameter_preview_kat(), rng.uniform(-1, 1, (S, 1)), T, warm=warm, p=pt)
    _assert_identical(sim, ref, T)


@pytest.mark.parametrize("warm", [False, True])
def test_offsets_equal_the_composed_loop(lmpc, warm):
    from oracle import mpc2mpqp as omm
    rng = np.random.default_rng(14)
    S, T = 200, 50
    sim, ref, _ = _both(lmpc, omm.offset_kat(), rng.uniform(-1, 1, (S, 1)), T, warm=warm, r=np.array([[1.5]]))
    _assert_identical(sim, ref, T)


def _soft_row_problem():
    from oracle import mpc2mpqp as omm
    p = omm.preview_sim_kat(True)
    p.Gd = np.array([[0.0], [1.0]])
    p.Dd = np.zeros((2, 1))
    return p


@pytest.mark.parametrize("warm", [False, True])
def test_soft_row_problem_equals_the_composed_loop(lmpc, warm):
    rng = np.random.default_rng(15)
    S, T = 300, 30
    r = np.zeros((S, 2, T))
    r[:, 0, 10:] = rng.uniform(0.5, 1.5, (S, 1))          # a step in r1 at k = 10, above the soft bound for some
    d = rng.uniform(-0.2, 0.2, (S, 1, T))
    sim, ref, mpc = _both(lmpc, _soft_row_problem(), rng.uniform(-0.4, 0.4, (S, 2)), T, warm=warm, r=r, d=d)
    _assert_identical(sim, ref, T)
    print("kernel:", mpc.control_model().kernel_name, " scenarios with a soft-optimal step:", int((sim.flag_min == 1).sum()))


def test_variational_handle_equals_the_composed_loop(lmpc):
    # an is_avi handle (game-theoretic MPC, runtests.jl:1337-1358): the loop's solve is the handle's own
    from oracle import mpc2mpqp as omm
    rng = np.random.default_rng(16)
    S, T = 128, 20
    p = omm.game_kat()
    x0 = np.tile([10.0, 10.0], (S, 1)) + rng.uniform(-1, 1, (S, 2))
    sim, ref, mpc = _both(lmpc, p, x0, T, r=np.array([[10.0], [0.0]]))
    assert mpc.control_model().is_avi
    _assert_identical(sim, ref, T)


# ------------------------------------------------------------------ the reference's own assertions
def test_reference_assertions_disturbance_preview(lmpc):
    # runtests.jl:393-408
    d = np.hstack([np.zeros((1, 8)), np.ones((1, 12))])
    sims = {}
    for preview in (True, False):
        p = _dist_preview_sim(preview)
        sims[preview] = lmpc.Simulation(_mpc(lmpc, p), lmpc.Scenario([0.0, 0.0], N=20, d=d), _plant(lmpc, p))
        assert sims[preview].flag_min >= 1
    a, b = sims[True], sims[False]
    print("norm(us_preview - us_no_preview) =", np.linalg.norm(a.us - b.us),
          " norm(ys_preview)/norm(ys_no_preview) =", np.linalg.norm(a.ys) / np.linalg.norm(b.ys))
    assert np.linalg.norm(a.us - b.us) > 1e-2
    assert np.linalg.norm(a.ys) / np.linalg.norm(b.ys) < 0.9


def test_reference_assertion_observer_disturbance(lmpc):
    # runtests.jl:951-962 with zero noise: |mean(ys[end-20:end])| < 1e-2
    from oracle import mpc2mpqp as omm
    from oracle import observer as oobs
    p = omm.observer_disturbance_kat()
    kf = oobs.kalman_filter(p.F, p.G, p.C, Gd=p.Gd, Dd=p.Dd, Q=[1.0, 1], R=[1e-2])
    sim = lmpc.Simulation(_mpc(lmpc, p), lmpc.Scenario([1.0, 0.0], N=100, d=np.ones((2, 1)), r=np.zeros((1, 1))),
                          _plant(lmpc, p), observer=kf)
    print("mean(ys[end-20:end]) =", np.mean(sim.ys[0, -21:]))
    assert sim.flag_min >= 1 and abs(np.mean(sim.ys[0, -21:])) < 1e-2


def test_reference_assertion_set_offset(lmpc):
    # runtests.jl:1320-1327: us[end] = 10.5, ys[end] = 1.5
    from oracle import mpc2mpqp as omm
    p = omm.offset_kat()
    sim = lmpc.Simulation(_mpc(lmpc, p), lmpc.Scenario([0.0], N=50, r=np.array([[1.5]])), _plant(lmpc, p))
    print("us[end] - 10.5 =", sim.us[0, -1] - 10.5, " ys[end] - 1.5 =", sim.ys[0, -1] - 1.5)
    assert sim.flag_min >= 1
    assert abs(sim.us[0, -1] - 10.5) < 1e-7 and abs(sim.ys[0, -1] - 1.5) < 1e-7


def test_parameter_trajectory_closed_form(lmpc):
    # parameter_preview_kat: Q = 0, so the moves decouple and every applied control is clip(2 p_k, 0, 2) for the p
    # column of its step (runtests.jl:1270-1304 is the same problem); asserted at the solver's primal_tol.
    # runtests.jl:1188-1190 (cost_p < cost_no_p on a problem with a terminal cost) is left out: the oracle's
    # condensing restates no terminal-cost variant of that problem.
    from oracle import mpc2mpqp as omm
    rng = np.random.default_rng(17)
    S, T = 64, 30
    pt = rng.uniform(-0.5, 1.5, (S, 1, 12))
    p = omm.parameter_preview_kat()
    mpc = _mpc(lmpc, p)
    sim = lmpc.Simulation(mpc, lmpc.Scenario(rng.uniform(-1, 1, (S, 1)), N=T, p=pt), _plant(lmpc, p))
    want = np.clip(2.0 * pt[..., np.minimum(np.arange(T), 11)], 0.0, 2.0)
    print("max |u - clip(2p, 0, 2)| =", np.abs(sim.us - want).max())
    assert sim.flag_min.min() >= 1
    assert np.abs(sim.us - want).max() <= mpc.settings.primal_tol


# ------------------------------------------------------------------ cost and constraint violation
def test_pinned_values_of_the_reference(lmpc):
    # runtests.jl:1591-1599
    c = lmpc.evaluate_cost(None, C=[[1.0]], Q=[[2.0]], R=[[3.0]], Rr=[[4.0]], S=[[5.0]], xs=np.array([[1.0, 2.0]]),
                           us=np.array([[0.0, 1.0]]), rs=np.array([[0.0, 1.0]]))
    assert c == pytest.approx(10.5, rel=1e-15)
    Ax, Au = [[1.0, 0.0]], [[1.0]]
    assert lmpc.constraint_violation(Ax, Au, [-1.0], [1.0], [0.8, 0.0], [0.5]) == pytest.approx(0.3)
    v = lmpc.constraint_violation(Ax, Au, [-1.0], [1.0], np.array([[0.8, 0.2], [0.0, 0.0]]), np.array([[0.5, 0.0]]))
    assert v == pytest.approx([0.3, 0.0])
    with pytest.raises(AssertionError):
        lmpc.constraint_violation(Ax, Au, [-1.0], [1.0], np.array([[0.8, 0.0]]).T, np.array([[0.5, 0.0, 0.1]]))


def _numpy_cost(xs, us, rs, C, Q, R, Rr, S):
    """utils.jl:397-411 in float64, plus K (scalar multiply-adds) and the sum of the terms' absolute values"""
    nu, T = us.shape
    dus = np.diff(np.hstack([np.zeros((nu, 1)), us]), axis=1)
    cost, absum, K = 0.0, 0.0, 0
    absq = lambda a, M, b: np.abs(a) @ np.abs(M) @ np.abs(b)
    for i in range(T):
        err = C @ xs[:, i] - rs[:, i]
        cost += err @ Q @ err + us[:, i] @ R @ us[:, i] + dus[:, i] @ Rr @ dus[:, i] + xs[:, i] @ S @ us[:, i]
        aerr = np.abs(C) @ np.abs(xs[:, i]) + np.abs(rs[:, i])
        absum += absq(aerr, Q, aerr) + absq(us[:, i], R, us[:, i]) + absq(dus[:, i], Rr, dus[:, i]) + absq(xs[:, i], S, us[:, i])
        K += C.size + C.shape[0] + 2 * Q.size + 2 * R.size + 2 * Rr.size + nu + 2 * S.size + 8
    return 0.5 * cost, 0.5 * absum, K


def test_running_cost_and_violation_equal_the_stored_run(lmpc):
    import torch
    rng = np.random.default_rng(18)
    S, T = 300, 30
    p = _soft_row_problem()
    mpc, plant = _mpc(lmpc, p), _plant(lmpc, p)
    r = np.zeros((S, 2, T)); r[:, 0, 10:] = rng.uniform(0.5, 1.5, (S, 1))
    d = rng.uniform(-0.2, 0.2, (S, 1, T))
    Q, R, Rr, Sx = np.array([[2.0, 0.3], [0.3, 1.0]]), np.array([[0.1]]), np.array([[0.7]]), np.array([[0.2], [-0.4]])
    Ax, Au = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]), np.array([[0.0], [0.0], [1.0]])
    lb, ub = np.array([-1.0, -0.5, -1.5]), np.array([1.0, 0.5, 1.5])
    cost = lmpc.BatchedQP.sim_cost(2, 1, C=plant.C, Q=Q, R=R, Rr=Rr, S=Sx, Ax=Ax, Au=Au, lb=lb, ub=ub)
    sim = lmpc.Simulation(mpc, lmpc.Scenario(rng.uniform(-0.4, 0.4, (S, 2)), N=T, r=r, d=d), plant, cost=cost)
    assert sim.flag_min.min() >= 1 and sim.violation.max() > 0
    # stand-alone on the stored trajectories: identical
    alone = lmpc.evaluate_cost(sim, Q=Q, R=R, Rr=Rr, S=Sx)
    assert np.array_equal(alone, sim.cost)
    steps = lmpc.constraint_violation(Ax, Au, lb, ub, sim.xs, sim.us, model=sim.model)
    assert steps.shape == (S, T) and np.array_equal(steps.max(axis=1), sim.violation)
    dev = torch.device("cuda", sim.model.device)
    X = torch.from_numpy(np.ascontiguousarray(sim.xs.transpose(2, 0, 1))).to(dev)
    U = torch.from_numpy(np.ascontiguousarray(sim.us.transpose(2, 0, 1))).to(dev)
    worst = sim.model.constraint_violation_device(X, U, cost)
    torch.cuda.synchronize()
    assert np.array_equal(worst.cpu().numpy(), sim.violation)
    # numpy float64 of the same formulas within the summation bound 4 K eps S
    worst_rel = 0.0
    for s in range(S):
        ref, absum, K = _numpy_cost(sim.xs[s], sim.us[s], sim.rs[s], plant.C, Q, R, Rr, Sx)
        bound = 4 * K * EPS * absum
        worst_rel = max(worst_rel, abs(sim.cost[s] - ref) / bound)
        assert abs(sim.cost[s] - ref) <= bound, (s, sim.cost[s], ref, bound)
        v = Ax @ sim.xs[s] + Au @ sim.us[s]
        vref = np.maximum(np.maximum(lb[:, None] - v, v - ub[:, None]), 0.0).max(axis=0)
        vb = 4 * 3 * EPS * (np.abs(Ax) @ np.abs(sim.xs[s]) + np.abs(Au) @ np.abs(sim.us[s]) + 1.5).max()
        assert np.abs(steps[s] - vref).max() <= vb
    print("largest |cost - numpy| / bound =", worst_rel)


# ------------------------------------------------------------------ independence of scenarios
def test_scenarios_are_independent(lmpc):
    from oracle import mpc2mpqp as omm
    from oracle import observer as oobs
    p = omm.observer_disturbance_kat()
    kf = oobs.kalman_filter(p.F, p.G, p.C, Gd=p.Gd, Dd=p.Dd, Q=[1.0, 1], R=[1e-2])
    mpc, plant = _mpc(lmpc, p), _plant(lmpc, p)
    rng = np.random.default_rng(19)
    S, T = 301, 25
    x0 = rng.uniform(-1, 1, (S, 2))
    d = 1.0 + rng.uniform(-0.2, 0.2, (S, 2, T))
    noise = 0.01 * rng.standard_normal((S, 1, T))
    run = lambda sl, dd, nn: lmpc.Simulation(mpc, lmpc.Scenario(x0[sl], N=T, d=dd, noise=nn, r=np.zeros((1, 1))), plant,
                                             observer=kf, warm=True)
    whole = run(slice(None), d, noise)
    h = 140
    for sl in (slice(0, h), slice(h, S)):
        part = run(sl, d[sl], noise[sl])
        for k in ("xs", "us", "xhats", "yms", "ys", "flag_min"):
            assert np.array_equal(getattr(part, k), getattr(whole, k)[sl]), k
    # one shared trajectory (stride 0) against the same trajectory repeated per scenario
    shared = run(slice(None), d[7], noise[7])
    tiled = run(slice(None), np.tile(d[7], (S, 1, 1)), np.tile(noise[7], (S, 1, 1)))
    for k in ("xs", "us", "xhats", "yms", "ys", "flag_min"):
        assert np.array_equal(getattr(shared, k), getattr(tiled, k)), k


def test_host_pointer_twin_gives_the_same_run(lmpc):
    # lmpc_simulate_scenario: every device array of the descriptor as a host array, synchronous
    import ctypes
    from linearmpc_jl_amd._cabi import Block, check
    from oracle import mpc2mpqp as omm
    p = omm.offset_kat()
    mpc, plant = _mpc(lmpc, p), _plant(lmpc, p)
    rng = np.random.default_rng(20)
    S, T = 50, 20
    x0 = rng.uniform(-1, 1, (S, 1))
    r = np.ascontiguousarray(rng.uniform(1.0, 2.0, (S, 7, 1)))            # per scenario: (S, Tc, w) column after column
    sim = lmpc.Simulation(mpc, lmpc.Scenario(x0, N=T, r=np.swapaxes(r, 1, 2)), plant)
    model = mpc.control_model()
    desc, keep = model.scenario_descriptor(plant.dynamics_rows(), 1, 0, plant.measurement_rows(), 1,
                                           r=Block(r.ctypes.data, 7, 1, 7, 0, 0), nuprev=1)
    x, up = x0.copy(), np.tile(mpc.uprev[:1], (S, 1))
    U, X, Y = np.empty((T, S, 1)), np.empty((T + 1, S, 1)), np.empty((T, S, 1))
    fm = np.empty(S, np.int32)
    desc.Y_traj = Y.ctypes.data
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    check(lmpc.lib().lmpc_simulate_scenario(model._h, S, T, ctypes.byref(desc), vp(x), None, vp(up), vp(U), vp(X), vp(fm)),
          model._h)
    assert np.array_equal(U.transpose(1, 2, 0), sim.us) and np.array_equal(X[:T].transpose(1, 2, 0), sim.xs)
    assert np.array_equal(Y.transpose(1, 2, 0), sim.ys) and np.array_equal(fm, sim.flag_min)
    assert np.array_equal(x, sim.x_final) and np.array_equal(up[:, 0], sim.us[:, 0, -1])


# ------------------------------------------------------------------ the host reference loop, bit for bit
# tests/scenario_reference.py restates the loop in numpy + the CPU oracle; the cases (scenario_reference.CASES) and the
# conditions that keep them from passing emptily are checked on the host first (tests/test_scenario_host.py).
def _cases(group):
    import scenario_reference as sr
    return [pytest.param(c, id=c.name) for c in group(sr)]


def _gpu_and_reference(lmpc, case, mpc=None):
    import scenario_reference as sr
    from conftest import oracle_ldp_from
    data = sr.case_data(case)
    mpc = _mpc(lmpc, data.prob) if mpc is None else mpc
    cost = None if data.cost is None else lmpc.BatchedQP.sim_cost(case.nx, case.nu, **data.cost)
    traj = {k: getattr(data, k) for k in ("r", "d", "p", "noise") if getattr(data, k) is not None}
    sim = lmpc.Simulation(mpc, lmpc.Scenario(data.x0, N=case.T, **traj), _plant(lmpc, data.prob), observer=data.kf,
                          warm=case.warm, cost=cost)
    ref = sr.run_case(case, oracle_ldp_from(mpc.control_model().ldp()), data, settings=_oracle_settings(mpc))
    return sim, ref, data, mpc


def _assert_bitwise(case, sim, ref):
    """np.array_equal on every output, no scenario or step left out.  Walks the steps in causal order first (PRE
    outputs, then u, then the POST state) so that a failure names the first array and step that differ."""
    T = case.T
    for k in range(T):
        nxt = sim.xs[..., k + 1] if k + 1 < T else sim.x_final
        for name, got, want in (("xs", sim.xs[..., k], ref.xs[k]), ("ds", sim.ds[..., k], ref.ds[k]),
                                ("yms", sim.yms[..., k], ref.yms[k]), ("ys", sim.ys[..., k], ref.ys[k]),
                                ("xhats", sim.xhats[..., k], ref.xhats[k]), ("us", sim.us[..., k], ref.us[k]),
                                ("x after the step", nxt, ref.xs[k + 1])):
            if not np.array_equal(got, want):
                bad = np.flatnonzero((got != want).any(axis=1))
                raise AssertionError(f"{case.name}: first difference in {name} at step {k}: {bad.size} of {len(got)} scenarios "
                                     f"(first {bad[:5]}), max |diff| = {np.abs(got - want).max():.3e}")
    step = lambda a: a.transpose(1, 2, 0)
    assert np.array_equal(sim.xs, step(ref.xs[:T])) and np.array_equal(sim.x_final, ref.xs[T])
    assert np.array_equal(sim.us, step(ref.us)) and np.array_equal(sim.xhats, step(ref.xhats))
    assert np.array_equal(sim.yms, step(ref.yms)) and np.array_equal(sim.ys, step(ref.ys))
    assert np.array_equal(sim.ds, step(ref.ds))
    assert np.array_equal(sim.flag_min, ref.flag_min)
    if case.cost:
        assert np.array_equal(sim.cost, ref.cost), np.abs(sim.cost - ref.cost).max()
        assert np.array_equal(sim.violation, ref.violation)


def _run_and_compare(lmpc, case, mpc=None):
    import scenario_reference as sr
    sim, ref, data, mpc = _gpu_and_reference(lmpc, case, mpc)
    _assert_bitwise(case, sim, ref)
    sr.check_conditions(case, ref, sim)
    return sim, ref, data, mpc


@pytest.mark.parametrize("case", _cases(lambda sr: sr.SWEEP))
def test_every_state_size_equals_the_host_reference(lmpc, case):
    # scenario_pre_kernel<NX> / scenario_post_kernel<NX, false>: NX = 1 .. 8 unrolled, 9 / 17 / 32 the generic form;
    # nu = 2, ny = 3, nd = 2, uprev in theta, noise, S = 300 (a ragged second workgroup)
    _, _, _, mpc = _run_and_compare(lmpc, case)
    if case.nx == 32:
        assert mpc.control_model().nth >= 34


@pytest.mark.parametrize("case", _cases(lambda sr: sr.PREVIEWS))
def test_all_previews_at_once_equal_the_host_reference(lmpc, case):
    # r, d and p previews with nuprev = nu: a record of 26 and one of 64 doubles; short (held) and shared trajectories
    _, _, data, mpc = _run_and_compare(lmpc, case)
    nth = mpc.control_model().nth
    assert (16 < nth <= 32) if case.name.endswith("26") else nth >= 60
    assert data.r.shape[-1] < case.T and any(a.ndim == 2 for a in (data.r, data.d, data.p))


@pytest.mark.parametrize("case", _cases(lambda sr: sr.SIZES))
def test_batch_and_run_sizes_equal_the_host_reference(lmpc, case):
    # S = 1, 255, 256, 257, 1000 (one lane, a workgroup less one, exactly one, one more, a ragged fourth) and
    # T = 1 (first and last in one POST launch), 2
    _run_and_compare(lmpc, case)


def _direct_run(lmpc, mpc, case, data, keep_xhat):
    """model.simulate_scenario as Simulation calls it, optionally with the caller's own xhat buffer"""
    import torch
    from linearmpc_jl_amd.simulation import scenario_blocks
    model = mpc.control_model()
    plant = _plant(lmpc, data.prob)
    dev = torch.device("cuda", model.device)
    traj = {k: getattr(data, k) for k in ("r", "d", "p", "noise") if getattr(data, k) is not None}
    specs = scenario_blocks(mpc, lmpc.Scenario(data.x0, N=case.T, **traj))
    up = lambda sp: None if sp["data"] is None else torch.from_numpy(np.swapaxes(sp["data"], -1, -2).copy()).to(dev)
    model.set_observer(*data.kf.codegen_arrays(), plant.nx, plant.nu, plant.nd, plant.ny)
    x = torch.from_numpy(data.x0.copy()).to(dev)
    xhat = x.clone() if keep_xhat else None
    uprev = torch.from_numpy(np.tile(np.asarray(mpc.uprev, float)[:mpc.nuprev], (case.S, 1))).to(dev)
    cost = lmpc.BatchedQP.sim_cost(case.nx, case.nu, **data.cost)
    out = model.simulate_scenario(
        x, case.T, plant.dynamics_rows(), plant.measurement_rows(), nd=plant.nd, ny=plant.ny, r=up(specs["r"]),
        d=up(specs["d"]), p=up(specs["p"]), noise=up(specs["noise"]), r_preview=specs["r"]["H"], d_preview=specs["d"]["H"],
        p_preview=specs["p"]["H"], r_width=specs["r"]["w"], d_width=specs["d"]["w"], p_width=specs["p"]["w"], xhat=xhat,
        uprev=uprev, use_observer=True, warm=case.warm, cost=cost, want=("U", "X", "Y", "Ym", "Xhat", "D"), want_cost=True,
        want_violation=True)
    torch.cuda.synchronize(dev)
    model.check()
    return {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


def test_cost_inside_the_loop_with_observer_and_rr(lmpc):
    # COST = true with an observer and Rr together: the per-run scratch is [xhat | ulast]; then the same run with the
    # caller keeping xhat, scratch = [ulast] alone -- the same numbers
    import scenario_reference as sr
    case = sr.COST
    sim, ref, data, mpc = _run_and_compare(lmpc, case)
    assert data.cost["Rr"] is not None and data.cost["Ax"].shape == (4, case.nx) and case.nu == 3
    for keep in (False, True):
        out = _direct_run(lmpc, mpc, case, data, keep_xhat=keep)
        for key, want in (("U", ref.us), ("X", ref.xs), ("Y", ref.ys), ("Ym", ref.yms), ("Xhat", ref.xhats), ("D", ref.ds),
                          ("x", ref.xs[-1]), ("flag_min", ref.flag_min), ("cost", ref.cost), ("violation", ref.violation),
                          ("uprev", ref.uprev_final)):
            assert np.array_equal(out[key], want), (keep, key)
        if keep:
            assert np.array_equal(out["xhat"], ref.xhat_final)


def test_one_handle_several_runs(lmpc):
    # S = 200, then 2000 (the scratch and the outputs of the first run regrow), then 50 (what the larger run left
    # in cost / viol / ulast / flag_min must not be read): each run equals the reference
    import scenario_reference as sr
    mpc, model = None, None
    for case in sr.RERUN:
        _, _, _, mpc = _run_and_compare(lmpc, case, mpc)
        assert model is None or mpc.control_model() is model
        model = mpc.control_model()


@pytest.mark.parametrize("case", _cases(lambda sr: sr.SCORING))
def test_stand_alone_scoring_equals_the_host_reference(lmpc, case):
    # scenario_cost_kernel / scenario_violation_kernel on stored trajectories at nx = 32, nu = 8 and at nx = 3:
    # bitwise the reference's cost / violation / per-step violation, and the in-loop values
    import torch
    import scenario_reference as sr
    sim, ref, data, mpc = _run_and_compare(lmpc, case)
    model = mpc.control_model()
    dev = torch.device("cuda", model.device)
    X = torch.from_numpy(np.ascontiguousarray(sim.xs.transpose(2, 0, 1))).to(dev)
    U = torch.from_numpy(np.ascontiguousarray(sim.us.transpose(2, 0, 1))).to(dev)
    rs = sr.run_trajectory(data.r, case.S, case.T)
    k = data.cost
    weights = lmpc.BatchedQP.sim_cost(case.nx, case.nu, C=k["C"], Q=k["Q"], R=k["R"], Rr=k["Rr"], S=k["S"])
    rows = lmpc.BatchedQP.sim_cost(case.nx, case.nu, Ax=k["Ax"], Au=k["Au"], lb=k["lb"], ub=k["ub"])
    cost = model.evaluate_cost_device(X, U, weights, torch.from_numpy(np.ascontiguousarray(rs)).to(dev))
    worst = model.constraint_violation_device(X, U, rows)
    steps = model.constraint_violation_device(X, U, rows, per_step=True)
    torch.cuda.synchronize(dev)
    model.check()
    cost, worst, steps = cost.cpu().numpy(), worst.cpu().numpy(), steps.cpu().numpy()
    assert np.array_equal(cost, ref.cost) and np.array_equal(cost, sim.cost)
    assert np.array_equal(worst, ref.violation) and np.array_equal(worst, sim.violation)
    assert steps.shape == (case.T, case.S) and np.array_equal(steps, ref.violation_steps)
    # the package's own wrappers on the same trajectories
    assert np.array_equal(lmpc.evaluate_cost(sim, C=k["C"], Q=k["Q"], R=k["R"], Rr=k["Rr"], S=k["S"]), ref.cost)
    assert np.array_equal(lmpc.constraint_violation(k["Ax"], k["Au"], k["lb"], k["ub"], sim.xs, sim.us, model=model),
                          ref.violation_steps.T)


def test_host_pointer_twin_equals_the_host_reference(lmpc):
    # lmpc_simulate_scenario at nx = 6 with the observer, d and noise: host arrays in and out
    import ctypes
    import scenario_reference as sr
    from conftest import oracle_ldp_from
    from linearmpc_jl_amd._cabi import Block, check
    case = sr.TWIN
    data = sr.case_data(case)
    mpc, plant = _mpc(lmpc, data.prob), _plant(lmpc, data.prob)
    model = mpc.control_model()
    S, T, nx, nu, ny, nd = case.S, case.T, case.nx, case.nu, case.ny, case.nd
    model.set_observer(*data.kf.codegen_arrays(), nx, nu, nd, ny)
    lay = lambda a: np.ascontiguousarray(np.swapaxes(a, 1, 2))             # (S, w, T) -> (S, T, w): column after column
    r, d, v = lay(data.r), lay(data.d), lay(data.noise)
    blk = lambda a, w: Block(a.ctypes.data, w * T, w, T, 0, 0)
    desc, keep = model.scenario_descriptor(plant.dynamics_rows(), nx, nd, plant.measurement_rows(), ny, r=blk(r, ny),
                                           d=blk(d, nd), noise=blk(v, ny), nuprev=nu, use_observer=True)
    x, up = data.x0.copy(), np.zeros((S, nu))
    U, X, fm = np.empty((T, S, nu)), np.empty((T + 1, S, nx)), np.empty(S, np.int32)
    Y, Ym, Xh, D = np.empty((T, S, ny)), np.empty((T, S, ny)), np.empty((T, S, nx)), np.empty((T, S, nd))
    desc.Y_traj, desc.Ym_traj, desc.Xhat_traj, desc.D_traj = (a.ctypes.data for a in (Y, Ym, Xh, D))
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    check(lmpc.lib().lmpc_simulate_scenario(model._h, S, T, ctypes.byref(desc), vp(x), None, vp(up), vp(U), vp(X), vp(fm)),
          model._h)
    ref = sr.run_case(case, oracle_ldp_from(model.ldp()), data, settings=_oracle_settings(mpc))
    sr.check_conditions(case, ref)
    for name, got, want in (("X", X, ref.xs), ("U", U, ref.us), ("Y", Y, ref.ys), ("Ym", Ym, ref.yms), ("Xhat", Xh, ref.xhats),
                            ("D", D, ref.ds), ("x", x, ref.xs[-1]), ("uprev", up, ref.uprev_final), ("flag_min", fm, ref.flag_min)):
        assert np.array_equal(got, want), name
