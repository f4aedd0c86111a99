"""The scenario loop with an explicit controller on the GPU (lmpc_explicit_simulate_scenario_device through
`Simulation(ExplicitMPC, ...)`): the run-ahead form (mode 1) bit for bit against the host reference of
tests/explicit_scenario_reference.py (numpy restatement of the controller's table + the CPU oracle on the handle's own
pack; the library's evaluation is never called) AND against the lock-step form (mode 0), at every instantiation of
explicit_run_kernel that the library dispatches; batch and run sizes; cost across fallback rounds; all-miss and
all-hit controllers; one controller reused; the host-pointer twin.  The cases and the conditions that keep them from
passing emptily are checked on the host first (tests/test_explicit_scenario_host.py) and again here from the GPU's
own `regions`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OUTPUTS = ("xs", "x_final", "us", "xhats", "yms", "ys", "ds", "flag_min", "regions")


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


def _plant(lmpc, p):
    return lmpc.Plant(p.F, p.G, Gd=p.Gd, f_offset=p.f_offset, C=p.C, Dd=p.Dd, h_offset=p.h_offset)


def _oracle_settings(mpc):
    from oracle import ldp as oldp
    s = oldp.default_settings()
    for name in ("primal_tol", "dual_tol", "zero_tol", "progress_tol", "fval_bound", "rho_soft", "cycle_tol", "iter_limit"):
        setattr(s, name, getattr(mpc.settings, name))
    return s


_BUILT = {}


def _controller(lmpc, case, fresh=False):
    """(ExplicitMPC trained on the GPU over the case's box, its table, the oracle's LDP of the handle's pack); one
    build per problem and training recipe for the whole module"""
    import explicit_scenario_reference as er
    from conftest import oracle_ldp_from
    key = (er.problem_key(case), case.max_regions, case.nsamples, case.scale, case.kind)
    if fresh or key not in _BUILT:
        data = er.case_data(case)
        mpc = _mpc(lmpc, data.prob)
        opts = dict(max_regions=case.max_regions, soft_band=er.BAND)
        if case.kind == "miss":
            opts["box"] = er.training_box(case, data)
        empc = lmpc.ExplicitMPC(mpc, er.training_box(case, data), nsamples=case.nsamples, seed=900 + case.base.seed, **opts)
        built = (empc, er.Table(empc.controller.blob()), oracle_ldp_from(mpc.control_model().ldp()))
        if fresh:
            return built
        _BUILT[key] = built
    return _BUILT[key]


def _simulate(lmpc, case, empc, mode, data=None):
    import explicit_scenario_reference as er
    data = er.case_data(case) if data is None else data
    b = case.base
    cost = None if data.cost is None else lmpc.BatchedQP.sim_cost(b.nx, b.nu, **data.cost)
    traj = {k: getattr(data, k) for k in ("r", "d", "p", "noise") if getattr(data, k) is not None}
    return lmpc.Simulation(empc, lmpc.Scenario(data.x0, N=b.T, **traj), _plant(lmpc, data.prob), observer=data.kf, cost=cost,
                           mode=mode)


def _reference(case, empc, tab, ldp, data=None):
    import explicit_scenario_reference as er
    st = empc.mpc.settings
    return er.run_explicit_case(case, tab, ldp, data, settings=_oracle_settings(empc.mpc), primal_tol=st.primal_tol,
                                rho_soft=st.rho_soft)


def _assert_bitwise(case, sim, ref, what):
    """np.array_equal on every output; the steps in causal order first, so that a failure names the first array and
    step that differ"""
    T = case.base.T
    for k in range(T):
        nxt = sim.xs[..., k + 1] if k + 1 < T else sim.x_final
        for name, got, want in (("xs", sim.xs[..., k], ref.xs[k]), ("ds", sim.ds[..., k], ref.ds[k]),
                                ("yms", sim.yms[..., k], ref.yms[k]), ("ys", sim.ys[..., k], ref.ys[k]),
                                ("xhats", sim.xhats[..., k], ref.xhats[k]), ("regions", sim.regions[:, k, None], ref.regions[k][:, None]),
                                ("us", sim.us[..., k], ref.us[k]), ("x after the step", nxt, ref.xs[k + 1])):
            if not np.array_equal(got, want):
                bad = np.flatnonzero((got != want).any(axis=1))
                raise AssertionError(f"{case.name} ({what}): first difference in {name} at step {k}: {bad.size} of {len(got)} "
                                     f"scenarios (first {bad[:5]})")
    assert np.array_equal(sim.flag_min, ref.flag_min), what
    if case.base.cost:
        assert np.array_equal(sim.cost, ref.cost), (what, np.abs(sim.cost - ref.cost).max())
        assert np.array_equal(sim.violation, ref.violation), what


def _assert_same_run(a, b, cost):
    for k in OUTPUTS + (("cost", "violation") if cost else ()):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def _run_and_compare(lmpc, case, built=None):
    import explicit_scenario_reference as er
    empc, tab, ldp = _controller(lmpc, case) if built is None else built
    data = er.case_data(case)
    ahead = _simulate(lmpc, case, empc, 1, data)
    lock = _simulate(lmpc, case, empc, 0, data)
    ref = _reference(case, empc, tab, ldp, data)
    _assert_bitwise(case, ahead, ref, "run-ahead against the host reference")
    _assert_same_run(ahead, lock, case.base.cost)
    er.check_explicit_conditions(case, ref, ahead.regions.T, ahead.stats)
    assert lock.stats["rounds"] == case.base.T and lock.stats["fallback_steps"] == ahead.stats["fallback_steps"]
    assert 1 <= ahead.stats["rounds"] <= case.base.T + 1
    # a scenario that misses in m steps needs m + 1 launches
    assert ahead.stats["rounds"] == 1 + int((ahead.regions < 0).sum(axis=1).max())
    return ahead, lock, ref, empc


def _cases(group):
    import explicit_scenario_reference as er
    return [pytest.param(c, id=c.name) for c in group(er)]


@pytest.mark.parametrize("case", _cases(lambda er: er.INSTANCES))
def test_every_instantiation_equals_the_host_reference_and_lock_step(lmpc, case):
    # explicit_run_kernel<NXT, NT>: NXT = 1 .. 8 and 0 (nx = 9), NT = 8, 16, 32; S = 300 (a ragged second workgroup),
    # T = 12, observer on and off, noise on
    import explicit_scenario_reference as er
    ahead, _, _, empc = _run_and_compare(lmpc, case)
    assert er.expected_class(case, empc.controller.nth)[1] == case.nt
    print(case.name, "nth", empc.controller.nth, ahead.stats)


@pytest.mark.parametrize("case", _cases(lambda er: er.SIZES))
def test_batch_and_run_sizes(lmpc, case):
    # S = 1, 63, 64, 65 (a wavefront less one, exactly one, one more), 255, 256, 257 and T = 1 (first and last step in
    # one), 2
    _run_and_compare(lmpc, case)


@pytest.mark.parametrize("case", _cases(lambda er: er.COST))
def test_cost_and_violation_across_fallback_rounds(lmpc, case):
    # Rr: the previous control of the du term is carried from a round into the next one
    import explicit_scenario_reference as er
    ahead, lock, ref, _ = _run_and_compare(lmpc, case)
    assert er.case_data(case).cost["Rr"] is not None and ahead.violation.max() > 0
    assert (ahead.regions < 0).any(axis=1).sum() > 0
    alone = lmpc.evaluate_cost(ahead, **{k: v for k, v in er.case_data(case).cost.items() if k in ("Q", "R", "Rr", "S")})
    assert np.array_equal(alone, ahead.cost)


def test_a_controller_that_never_locates_equals_the_implicit_loop(lmpc):
    # trained on a box disjoint from everything the loop visits (the regions carry the box's rows): every step falls
    # back, T rounds of the handle's own solve, so the run is the implicit Simulation's on the same handle, bit for bit
    import explicit_scenario_reference as er
    case = er.ALL_MISS
    ahead, lock, ref, empc = _run_and_compare(lmpc, case)
    T, S = case.base.T, case.base.S
    assert (ahead.regions == -1).all()
    assert ahead.stats == dict(rounds=T + 1, fallback_steps=S * T, located_steps=0, largest_batch=S)
    data = er.case_data(case)
    traj = {k: getattr(data, k) for k in ("r", "d", "noise")}
    implicit = lmpc.Simulation(empc.mpc, lmpc.Scenario(data.x0, N=T, **traj), _plant(lmpc, data.prob), observer=data.kf, warm=False)
    for k in ("xs", "x_final", "us", "xhats", "yms", "ys", "ds", "flag_min"):
        assert np.array_equal(getattr(ahead, k), getattr(implicit, k)), k


def test_a_controller_that_always_locates_needs_one_launch(lmpc):
    import explicit_scenario_reference as er
    case = er.ALL_HIT
    ahead, lock, ref, _ = _run_and_compare(lmpc, case)
    T, S = case.base.T, case.base.S
    assert (ahead.regions >= 0).all()
    assert ahead.stats == dict(rounds=1, fallback_steps=0, located_steps=S * T, largest_batch=0)


def test_one_controller_several_runs_then_the_older_entry_points(lmpc):
    # S = 200, 700, 50 on one controller (the scratch regrows, then what the larger run left must not be read), then
    # evaluate_device and a plain solve_device on the same handle: each equal to a fresh controller / handle
    import torch
    import explicit_scenario_reference as er
    built = _controller(lmpc, er.RERUN[0])
    for case in er.RERUN:
        _run_and_compare(lmpc, case, built)
    empc = built[0]
    fresh = _controller(lmpc, er.RERUN[0], fresh=True)[0]
    assert fresh.controller is not empc.controller and np.array_equal(fresh.controller.blob(), empc.controller.blob())
    data = er.case_data(er.RERUN[1])
    lb, ub = er.training_box(er.RERUN[1], data)
    th = lb + (ub - lb) * 1.5 * np.random.default_rng(3).random((1000, lb.size))
    for ctl in (empc, fresh):
        dev = torch.device("cuda", ctl.mpc.control_model().device)
        t = torch.from_numpy(th).to(dev)
        x, f, r = ctl.controller.evaluate_device(t)
        xs, fs = ctl.mpc.control_model().solve_device(t)
        torch.cuda.synchronize(dev)
        ctl.result = tuple(a.cpu().numpy() for a in (x, f, r, xs, fs))
    for a, b in zip(empc.result, fresh.result):
        assert np.array_equal(a, b)
    assert (empc.result[2] < 0).any() and (empc.result[2] >= 0).any()


@pytest.mark.parametrize("mode", [1, 0])
def test_host_pointer_twin(lmpc, mode):
    # lmpc_explicit_simulate_scenario: host arrays in and out, synchronous
    import ctypes
    import explicit_scenario_reference as er
    from linearmpc_jl_amd._cabi import Block
    from linearmpc_jl_amd.explicit import _bind
    case = er.TWIN
    b = case.base
    empc, tab, ldp = _controller(lmpc, case)
    data = er.case_data(case)
    plant = _plant(lmpc, data.prob)
    model = empc.mpc.control_model()
    S, T, nx, nu, ny, nd = b.S, b.T, b.nx, b.nu, b.ny, b.nd
    model.set_observer(*data.kf.codegen_arrays(), nx, nu, nd, ny)
    lay = lambda a: np.ascontiguousarray(np.swapaxes(a, 1, 2))             # (S, w, T) -> (S, T, w): column after column
    r, d, v = lay(data.r), lay(data.d), lay(data.noise)
    blk = lambda a, w: Block(a.ctypes.data, w * T, w, T, 0, 0)
    desc, keep = model.scenario_descriptor(plant.dynamics_rows(), nx, nd, plant.measurement_rows(), ny, r=blk(r, ny),
                                           d=blk(d, nd), noise=blk(v, ny), nuprev=nu, use_observer=True)
    x, up = data.x0.copy(), np.zeros((S, nu))
    U, X, fm = np.empty((T, S, nu)), np.empty((T + 1, S, nx)), np.empty(S, np.int32)
    Y, Ym, Xh, D = np.empty((T, S, ny)), np.empty((T, S, ny)), np.empty((T, S, nx)), np.empty((T, S, nd))
    reg, stats = np.empty((T, S), np.int32), np.zeros(4, np.int64)
    desc.Y_traj, desc.Ym_traj, desc.Xhat_traj, desc.D_traj = (a.ctypes.data for a in (Y, Ym, Xh, D))
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = _bind().lmpc_explicit_simulate_scenario(empc.controller._e, S, T, ctypes.byref(desc), vp(x), None, vp(up), vp(U), vp(X),
                                                 vp(fm), vp(reg), mode, vp(stats))
    empc.controller._check(rc)
    ref = _reference(case, empc, tab, ldp, data)
    er.check_explicit_conditions(case, ref, reg)
    for name, got, want in (("X", X, ref.xs), ("U", U, ref.us), ("Y", Y, ref.ys), ("Ym", Ym, ref.yms), ("Xhat", Xh, ref.xhats),
                            ("D", D, ref.ds), ("x", x, ref.xs[-1]), ("uprev", up, ref.uprev_final), ("flag_min", fm, ref.flag_min),
                            ("regions", reg, ref.regions)):
        assert np.array_equal(got, want), name
    assert stats[1] == (reg < 0).sum() and stats[2] == (reg >= 0).sum()
