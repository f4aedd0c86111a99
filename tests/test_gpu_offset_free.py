"""The scenario loop with the offset-free observer on the GPU (lmpc_simulate_scenario_offset_free_device): bit for bit
against the host reference loop of tests/offset_free_reference.py (numpy + the CPU oracle on the handle's own pack) at
every (nx, ndo) instantiation of the glue kernels, at the gate between the compile-time and the run-time kernels and at
na = 32; and, without a preview, against the composition of the single-step entry points that existed before it
(lmpc_correct_state_device -> lmpc_compute_control_observer_device -> lmpc_predict_state_device, and
lmpc_predict_state_device on a plant twin).  The cases and the conditions that keep them from passing emptily are
checked on the host first (tests/test_offset_free_host.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


def _mpc(lmpc, p):
    from oracle import mpc2mpqp as omm
    q = omm.mpc2mpqp(p)
    nx, nr, nd, nup, npp = p.parameter_dims()
    mq = lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, is_symmetric=q.is_symmetric)
    return lmpc.MPC(mq, nx=nx, nu=p.nu, nr=nr, nd=nd, nuprev=nup, np_=npp, K=p.K, Np=p.Np,
                    reference_preview=p.reference_preview, disturbance_preview=p.disturbance_preview,
                    parameter_preview=p.parameter_preview)


def _plant(lmpc, data):
    t = data.plant
    return lmpc.Plant(t.F, t.G, Gd=t.Gd, f_offset=t.f_offset, C=t.C, Dd=t.Dd, h_offset=t.h_offset)


def _observer(lmpc, case, data):
    import offset_free_reference as ofr
    b, o = data.base, data.obs
    gains = dict(K=o.Bd) if ofr.METHODS[case.method] in ("velocity", "state_disturbance") else dict(Kaug=o.K)
    return lmpc.offset_free_observer(b.F, b.G, b.C, Gd=data.plant.Gd, Dd=data.plant.Dd, f_offset=b.f_offset,
                                     h_offset=b.h_offset, method=case.method, **gains)


def _oracle_settings(mpc):
    from oracle import ldp as oldp
    s = oldp.default_settings()
    for name in ("primal_tol", "dual_tol", "zero_tol", "progress_tol", "fval_bound", "rho_soft", "cycle_tol", "iter_limit"):
        setattr(s, name, getattr(mpc.settings, name))
    return s


def _direct_run(lmpc, mpc, case, data, xaug0):
    """model.simulate_scenario_offset_free with the caller keeping xaug (started at xaug0): every array as numpy"""
    import torch
    model = mpc.control_model()
    plant, obs = _plant(lmpc, data), _observer(lmpc, case, data)
    dev = torch.device("cuda", model.device)
    model.set_observer(*obs.codegen_arrays(), case.nx + case.ndo, case.nu, case.ndm, case.ny)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x, xaug = t(data.x0.copy()), t(xaug0.copy())
    cost = None if data.cost is None else lmpc.BatchedQP.sim_cost(case.nx, case.nu, **data.cost)
    out = model.simulate_scenario_offset_free(
        x, case.T, plant.dynamics_rows(), plant.measurement_rows(), case.ndo, nd=case.ndm, ny=case.ny, r=t(data.r),
        d=t(data.d), noise=t(data.noise), d_preview=case.Np if case.preview else 0, xaug=xaug, warm=case.warm, cost=cost,
        want=("U", "X", "Y", "Ym", "Xhat", "Dhat") + (("D",) if case.ndm else ()), want_cost=cost is not None,
        want_violation=cost is not None)
    torch.cuda.synchronize(dev)
    model.check()
    return {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


def _assert_direct(case, out, ref):
    pairs = [("X", ref.xs), ("U", ref.us), ("Y", ref.ys), ("Ym", ref.yms), ("Xhat", ref.xhats), ("Dhat", ref.dhats),
             ("x", ref.xs[-1]), ("xaug", ref.xaug_final), ("uprev", ref.uprev_final), ("flag_min", ref.flag_min)]
    if case.ndm:
        pairs.append(("D", ref.ds))
    if case.cost:
        pairs += [("cost", ref.cost), ("violation", ref.violation)]
    for key, want in pairs:
        assert np.array_equal(out[key], want), (case.name, key, float(np.abs(out[key] - want).max()))


def _assert_bitwise(case, sim, ref):
    """np.array_equal on every output of a Simulation, no scenario or step left out; the steps in causal order first
    so that a failure names the first array and step that differ"""
    T = case.T
    for k in range(T):
        nxt = sim.xs[..., k + 1] if k + 1 < T else sim.x_final
        for name, got, want in (("xs", sim.xs[..., k], ref.xs[k]), ("ds", sim.ds[..., k], ref.ds[k]),
                                ("yms", sim.yms[..., k], ref.yms[k]), ("ys", sim.ys[..., k], ref.ys[k]),
                                ("xhats", sim.xhats[..., k], ref.xhats[k]), ("dhats", sim.dhats[..., k], ref.dhats[k]),
                                ("us", sim.us[..., k], ref.us[k]), ("x after the step", nxt, ref.xs[k + 1])):
            if not np.array_equal(got, want):
                bad = np.flatnonzero((got != want).any(axis=1))
                raise AssertionError(f"{case.name}: first difference in {name} at step {k}: {bad.size} of {len(got)} scenarios "
                                     f"(first {bad[:5]}), max |diff| = {np.abs(got - want).max():.3e}")
    step = lambda a: a.transpose(1, 2, 0)
    assert np.array_equal(sim.xs, step(ref.xs[:T])) and np.array_equal(sim.x_final, ref.xs[T])
    assert np.array_equal(sim.us, step(ref.us)) and np.array_equal(sim.xhats, step(ref.xhats))
    assert np.array_equal(sim.dhats, step(ref.dhats)) and sim.dhats.shape == (case.S, case.ndo, T)
    assert np.array_equal(sim.yms, step(ref.yms)) and np.array_equal(sim.ys, step(ref.ys))
    assert np.array_equal(sim.ds, step(ref.ds)) and np.array_equal(sim.flag_min, ref.flag_min)
    if case.cost:
        assert np.array_equal(sim.cost, ref.cost) and np.array_equal(sim.violation, ref.violation)


def _composed(lmpc, mpc, case, data, xaug0):
    """The loop a caller had to stitch together: correct_state (augmented filter) -> compute_control_observer_device ->
    predict_state, and the plant step as predict_state on a SECOND handle of the same QP whose observer arrays are the
    true plant's.  No preview.  Returns xs (T+1, S, nx), us, xhats, dhats, xaug_final, flag_min."""
    import torch
    import scenario_reference as sr
    model = mpc.control_model()
    q = mpc.mpQP
    plant, obs = _plant(lmpc, data), _observer(lmpc, case, data)
    nx, nu, ny, ndm, ndo = case.nx, case.nu, case.ny, case.ndm, case.ndo
    twin = lmpc.BatchedQP.from_mpqp(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, nout=nu, nx=nx, settings=mpc.settings)
    twin.set_observer(plant.dynamics_rows(), np.zeros((1, 1 + nx + ndm)), np.zeros((1, nx)), nx, nu, ndm, 1)
    model.set_observer(*obs.codegen_arrays(), nx + ndo, nu, ndm, ny)
    model.set_parameter_layout(nx, nr=ny, nd=ndm + ndo, nuprev=nu)
    dev = torch.device("cuda", model.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S, T = case.S, case.T
    x, xaug, control = t(data.x0.copy()), t(xaug0.copy()), torch.zeros((S, nu), dtype=torch.float64, device=dev)
    pmeas = plant.measurement_rows()
    rt, dt = sr.run_trajectory(data.r, S, T), None if data.d is None else sr.run_trajectory(data.d, S, T)
    vt = None if data.noise is None else sr.run_trajectory(data.noise, S, T)
    xs, us, xhats, dhats, fmin = [data.x0.copy()], [], [], [], None
    for k in range(T):
        dk = np.zeros((S, ndm)) if dt is None else np.ascontiguousarray(dt[..., k])
        ym, _ = sr.measure(pmeas, x.cpu().numpy(), dk, None if vt is None else vt[..., k])
        dkt = t(dk) if ndm else None
        model.correct_state(xaug, t(ym), dkt)
        xa = xaug.cpu().numpy()
        xhats.append(xa[:, :nx].copy()); dhats.append(xa[:, nx:].copy())
        flag = model.compute_control_observer_device(control, xaug, n_measured=ndm, reference=t(rt[..., k]),
                                                     measured_disturbance=dkt, warm=case.warm)
        model.predict_state(xaug, control, dkt)
        twin.predict_state(x, control, dkt)
        f = flag.cpu().numpy()
        fmin = f if fmin is None else np.minimum(fmin, f)
        us.append(control.cpu().numpy().copy())
        xs.append(x.cpu().numpy())
    twin.close()
    return np.array(xs), np.array(us), np.array(xhats), np.array(dhats), xaug.cpu().numpy(), fmin


def _run_and_compare(lmpc, case, mpc=None, composed=True):
    """Simulation (xaug NULL: the handle's scratch, started at [x0; 0]) unless the case starts xaug elsewhere, the direct
    call with the caller's xaug, and the composed loop where there is no preview: all equal the host reference."""
    import offset_free_reference as ofr
    from conftest import oracle_ldp_from
    data = ofr.case_data(case)
    mpc = _mpc(lmpc, data.prob) if mpc is None else mpc
    ref = ofr.run_case(case, oracle_ldp_from(mpc.control_model().ldp()), data, settings=_oracle_settings(mpc))
    sim = None
    if not case.xaug:
        cost = None if data.cost is None else lmpc.BatchedQP.sim_cost(case.nx, case.nu, **data.cost)
        traj = {k: getattr(data, k) for k in ("r", "d", "noise") if getattr(data, k) is not None}
        sim = lmpc.Simulation(mpc, lmpc.Scenario(data.x0, N=case.T, **traj), _plant(lmpc, data),
                              observer=_observer(lmpc, case, data), warm=case.warm, cost=cost)
        _assert_bitwise(case, sim, ref)
    xaug0 = data.xaug0 if case.xaug else np.hstack([data.x0, np.zeros((case.S, case.ndo))])
    out = _direct_run(lmpc, mpc, case, data, xaug0)
    _assert_direct(case, out, ref)
    ofr.check_conditions(case, ref, sim)
    if composed and not case.preview:
        xs, us, xhats, dhats, xaug_final, fmin = _composed(lmpc, mpc, case, data, xaug0)
        for name, got, want in (("xs", xs, out["X"]), ("us", us, out["U"]), ("xhats", xhats, out["Xhat"]),
                                ("dhats", dhats, out["Dhat"]), ("xaug", xaug_final, out["xaug"]), ("flag_min", fmin, out["flag_min"])):
            assert np.array_equal(got, want), (case.name, "composed loop", name)
    return sim, ref, data, mpc


def _cases(group):
    import offset_free_reference as ofr
    return [pytest.param(c, id=c.name) for c in group(ofr)]


@pytest.mark.parametrize("case", _cases(lambda ofr: ofr.PAIRS))
def test_every_instantiation_equals_the_host_reference(lmpc, case):
    # offset_free_pre_kernel<NX, NDO> / offset_free_post_kernel<NX, NDO, false> for every NX + NDO <= 8: ndm = 0, 1, 2,
    # velocity and output models, preview on and off, warm and cold, noise, S = 300 (a ragged second workgroup)
    _run_and_compare(lmpc, case)


@pytest.mark.parametrize("case", _cases(lambda ofr: ofr.TABLE + [ofr.NOISE_FREE]))
def test_gate_and_run_time_sizes_equal_the_host_reference(lmpc, case):
    # na = 8 (the last compile-time pair) | 9 (the first run-time size), 20, 32; records of 5 .. 38 doubles
    _, ref, _, mpc = _run_and_compare(lmpc, case)
    assert mpc.control_model().nth == ref.thetas.shape[-1]


@pytest.mark.parametrize("case", _cases(lambda ofr: ofr.SIZES))
def test_batch_and_run_sizes_equal_the_host_reference(lmpc, case):
    # S = 1, 255, 256, 257, 1000 and T = 1 (first and last in one POST launch), 2; nx = 5 (na = 8) and 12 (na = 15)
    _run_and_compare(lmpc, case, composed=case.S in (1, 257))


def test_cost_inside_the_loop(lmpc):
    # offset_free_post_kernel<4, 2, true>: cost and violation on the TRUE state, scratch = [xaug | ulast]
    import offset_free_reference as ofr
    _, ref, data, _ = _run_and_compare(lmpc, ofr.COST)
    assert data.cost["Rr"] is not None and ref.cost.min() > 0


@pytest.mark.parametrize("case", _cases(lambda ofr: ofr.XAUG))
def test_caller_kept_xaug_away_from_the_default_start(lmpc, case):
    _run_and_compare(lmpc, case)


def test_one_handle_several_runs_then_a_plain_solve(lmpc):
    # S = 200, then 2000 (the scratch regrows), then 50; afterwards the handle solves as a fresh one does
    import torch
    import offset_free_reference as ofr
    mpc = None
    for case in ofr.RERUN:
        _, ref, _, mpc = _run_and_compare(lmpc, case, mpc, composed=False)
    model, q = mpc.control_model(), mpc.mpQP
    fresh = lmpc.BatchedQP.from_mpqp(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, nout=mpc.nu, nx=mpc.nx,
                                     settings=mpc.settings)
    theta = np.ascontiguousarray(ref.thetas.reshape(-1, ref.thetas.shape[-1]))
    a, b = model.solve(theta), fresh.solve(theta)
    fresh.close()
    for got, want in zip(a, b):
        assert np.array_equal(np.asarray(got), np.asarray(want))
    assert np.array_equal(np.asarray(a[0]), ref.us.reshape(-1, mpc.nu))


def test_host_pointer_twin_equals_the_host_reference(lmpc):
    # lmpc_simulate_scenario_offset_free at nx = 6, ndo = 2 with a preview: host arrays in and out, xaug NULL and given
    import offset_free_reference as ofr
    from conftest import oracle_ldp_from
    from linearmpc_jl_amd._cabi import Block, OffsetFree, check
    case = ofr.TWIN
    data = ofr.case_data(case)
    mpc, plant = _mpc(lmpc, data.prob), _plant(lmpc, data)
    model = mpc.control_model()
    S, T, nx, nu, ny, ndm, ndo = case.S, case.T, case.nx, case.nu, case.ny, case.ndm, case.ndo
    model.set_observer(*_observer(lmpc, case, data).codegen_arrays(), nx + ndo, nu, ndm, ny)
    ref = ofr.run_case(case, oracle_ldp_from(model.ldp()), data, settings=_oracle_settings(mpc))
    ofr.check_conditions(case, ref)
    lay = lambda a: np.ascontiguousarray(np.swapaxes(a, 1, 2))             # (S, w, T) -> (S, T, w): column after column
    r, d, v = lay(data.r), lay(data.d), lay(data.noise)
    blk = lambda a, w, H=0: Block(a.ctypes.data, w * T, w, T, 0, H)
    for keep in (False, True):
        desc, hold = model.scenario_descriptor(plant.dynamics_rows(), nx, ndm, plant.measurement_rows(), ny, r=blk(r, ny),
                                               d=blk(d, ndm, case.Np), noise=blk(v, ny), nuprev=nu, use_observer=True)
        x, up = data.x0.copy(), np.zeros((S, nu))
        xaug = np.hstack([data.x0, np.zeros((S, ndo))]) if keep else None
        U, X, fm = np.empty((T, S, nu)), np.empty((T + 1, S, nx)), np.empty(S, np.int32)
        Y, Ym, Xh, D = np.empty((T, S, ny)), np.empty((T, S, ny)), np.empty((T, S, nx)), np.empty((T, S, ndm))
        Dh = np.empty((T, S, ndo))
        desc.Y_traj, desc.Ym_traj, desc.Xhat_traj, desc.D_traj = (a.ctypes.data for a in (Y, Ym, Xh, D))
        of = OffsetFree(ndo, Dh.ctypes.data)
        vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
        check(lmpc.lib().lmpc_simulate_scenario_offset_free(model._h, S, T, ctypes.byref(desc), ctypes.byref(of), vp(x),
                                                            vp(xaug), vp(up), vp(U), vp(X), vp(fm)), model._h)
        for name, got, want in (("X", X, ref.xs), ("U", U, ref.us), ("Y", Y, ref.ys), ("Ym", Ym, ref.yms), ("Xhat", Xh, ref.xhats),
                                ("D", D, ref.ds), ("Dhat", Dh, ref.dhats), ("x", x, ref.xs[-1]), ("uprev", up, ref.uprev_final),
                                ("flag_min", fm, ref.flag_min)):
            assert np.array_equal(got, want), (keep, name)
        if keep:
            assert np.array_equal(xaug, ref.xaug_final)


def test_refusals_come_before_the_device(lmpc):
    # na = 33, a missing observer, xaug on a handle without an observer, the explicit loop: LMPC_ERR_BADARG with the field first
    import torch
    import offset_free_reference as ofr
    case = ofr.TABLE[1]
    data = ofr.case_data(case)
    mpc, plant = _mpc(lmpc, data.prob), _plant(lmpc, data)
    model = mpc.control_model()
    dev = torch.device("cuda", model.device)
    x = torch.from_numpy(data.x0.copy()).to(dev)
    kw = dict(nd=case.ndm, ny=case.ny, r_width=case.ny)
    with pytest.raises(lmpc.LmpcError, match="xaug: given without an observer"):
        model.simulate_scenario_offset_free(x, 2, plant.dynamics_rows(), plant.measurement_rows(), case.ndo,
                                            xaug=torch.zeros((case.S, case.nx + case.ndo), dtype=torch.float64, device=dev), **kw)
    with pytest.raises(lmpc.LmpcError, match="use_observer: lmpc_set_observer has not been called"):
        model.simulate_scenario_offset_free(x, 2, plant.dynamics_rows(), plant.measurement_rows(), case.ndo, **kw)
    obs = _observer(lmpc, case, data)
    model.set_observer(*obs.codegen_arrays(), case.nx + case.ndo, case.nu, case.ndm, case.ny)
    with pytest.raises(lmpc.LmpcError, match="n_offset_free: nx \\+ n_offset_free <= 32, got 3 \\+ 30"):
        model.simulate_scenario_offset_free(x, 2, plant.dynamics_rows(), plant.measurement_rows(), 30, **kw)
    with pytest.raises(lmpc.LmpcError, match="n_offset_free: the observer was set with n_state = 6"):
        model.simulate_scenario_offset_free(x, 2, plant.dynamics_rows(), plant.measurement_rows(), 2, **kw)
    assert np.array_equal(x.cpu().numpy(), data.x0)
    with pytest.raises(ValueError, match="disturbances"):                  # a plant that carries the estimated columns too
        lmpc.Simulation(mpc, lmpc.Scenario(data.x0, N=2), lmpc.Plant(data.prob.F, data.prob.G, Gd=data.prob.Gd, C=data.prob.C,
                                                                    Dd=data.prob.Dd), observer=obs)


def test_simulation_reproduces_the_reference_assertions(lmpc):
    # runtests.jl:989-1011 through lmpc.Simulation: nominal loop off by > 5e-2, offset-free loop within 1e-3 of r = 0.5
    import offset_free_reference as ofr
    from oracle import mpc2mpqp as omm
    mk = lambda Gd=None: omm.make_mpc([[1, 0.1], [0, 1]], [[0.005], [0.1]], [[1.0, 0.0]], Np=20, Q=[1.0], R=[0.0], Rr=[0.1],
                                      umin=[-1.0], umax=[1.0], Gd=Gd)
    nominal = mk()
    true = lmpc.Plant(nominal.F, nominal.G, f_offset=[0.01, 0.0], C=nominal.C)
    sc = lmpc.Scenario(np.zeros(2), N=100, r=np.array([[0.5]]))
    sim_nominal = lmpc.Simulation(_mpc(lmpc, nominal), sc, true)
    assert abs(sim_nominal.xs[0, -1] - 0.5) > 5e-2
    ref = ofr.build_observer(nominal.F, nominal.G, nominal.C, method="velocity", Q=[1e-3, 1e-3], R=[1e-4])
    obs = lmpc.offset_free_observer(nominal.F, nominal.G, nominal.C, method="velocity", K=ref.Bd)
    tracked = mk(Gd=obs.Bd)
    tracked.Dd = obs.Cd
    sim = lmpc.Simulation(_mpc(lmpc, tracked), sc, true, observer=obs)
    assert sim.dhats.shape == (1, 100) and sim.xs.shape == (2, 100)
    assert abs(sim.xs[0, -1] - 0.5) < 1e-3 and sim.flag_min.min() >= 1
