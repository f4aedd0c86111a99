"""The scenario loop under uncertainty on the GPU (lmpc_simulate_scenario_uncertain_device): bit for bit against the host
reference loop of tests/uncertain_reference.py (numpy + the CPU oracle on the handle's own pack) at every state-size
instantiation of the glue kernels, every shape of the draw, plant ensembles, batch sizes around the workgroup, sharded
and continued runs, and -- with every source off -- against lmpc_simulate_scenario_device on the same handle.  The cases
and the conditions that keep them from passing emptily are checked on the host first (tests/test_uncertain_host.py)."""
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


def _plant(lmpc, t):
    return lmpc.Plant(t.F, t.G, Gd=t.Gd, f_offset=t.f_offset, C=t.C, Dd=t.Dd, h_offset=t.h_offset)


def _oracle_settings(mpc):
    from oracle import ldp as oldp
    s = oldp.default_settings()
    for name in ("primal_tol", "dual_tol", "zero_tol", "progress_tol", "fval_bound", "rho_soft", "cycle_tol", "iter_limit"):
        setattr(s, name, getattr(mpc.settings, name))
    return s


def _source(lmpc, a, dev, sl=slice(None), cols=slice(None)):
    """a reference-side source (None, Box or array) as the package takes it"""
    import torch
    import uncertain_reference as ur
    if a is None:
        return None
    if isinstance(a, ur.Box):
        return lmpc.Uniform(a.lo, a.hi)
    a = a[..., cols] if a.ndim == 2 else a[sl][..., cols]
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _direct(lmpc, mpc, case, data, sl=slice(None), cols=slice(None), T=None, state=None, plain=False, **over):
    """model.simulate_scenario_uncertain on the scenarios `sl` and the trajectory columns `cols` of a case: every array
    as numpy.  state = (x, xhat, uprev) tensors of a run that is continued; plain: lmpc_simulate_scenario_device itself."""
    import torch
    import scenario_reference as sr
    model = mpc.control_model()
    nominal = sr.plant_of(data.prob)
    plant = _plant(lmpc, nominal)
    dev = torch.device("cuda", model.device)
    if data.kf is not None:
        model.set_observer(*data.kf.codegen_arrays(), case.nx, case.nu, case.nd, case.ny)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a if a.ndim == 2 else a[sl])[..., cols].copy()).to(dev)
    x, xhat, uprev = (torch.from_numpy(np.ascontiguousarray(data.x0[sl])).to(dev), None, None) if state is None else state
    cost = None if data.cost is None else lmpc.BatchedQP.sim_cost(case.nx, case.nu, **data.cost)
    T = case.T if T is None else T
    kw = dict(nd=case.nd, ny=case.ny, r=t(data.r), d=t(data.d), noise=t(data.noise), xhat=xhat, uprev=uprev,
              use_observer=data.kf is not None, warm=case.warm, cost=cost, want_cost=cost is not None,
              want_violation=cost is not None)
    want = ("U", "X", "Y", "Ym", "Xhat") + (("D",) if case.nd else ())
    if plain:
        out = model.simulate_scenario(x, T, plant.dynamics_rows(), plant.measurement_rows(), want=want, **kw)
    else:
        un = dict(process=_source(lmpc, data.process, dev, sl, cols), measurement_noise=_source(lmpc, data.measurement_noise, dev, sl, cols),
                  Gw=data.Gw, seed=case.key, scenario_offset=case.scenario_offset, step_offset=case.step_offset,
                  plants=None if data.plants is None else np.stack([_plant(lmpc, q).dynamics_rows() for q in data.plants]),
                  plant_index=None if data.plant_index is None else torch.from_numpy(data.plant_index[sl].copy()).to(dev))
        un.update(over)
        out = model.simulate_scenario_uncertain(x, T, plant.dynamics_rows(), plant.measurement_rows(),
                                                want=want + (("W",) if un["process"] is not None else ()), **un, **kw)
    torch.cuda.synchronize(dev)
    model.check()
    res = {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}
    res["_state"] = (out["x"], out["xhat"], out["uprev"])
    return res


def _pairs(case, ref):
    pairs = [("X", ref.xs), ("U", ref.us), ("Y", ref.ys), ("Ym", ref.yms), ("Xhat", ref.xhats), ("x", ref.xs[-1]),
             ("uprev", ref.uprev_final), ("flag_min", ref.flag_min)]
    if case.nd:
        pairs.append(("D", ref.ds))
    if ref.ws is not None:
        pairs.append(("W", ref.ws))
    if case.cost:
        pairs += [("cost", ref.cost), ("violation", ref.violation)]
    return pairs


def _assert_equal(case, out, ref):
    """np.array_equal on every output; the steps in causal order first so that a failure names the first array and step"""
    for k in range(ref.us.shape[0]):
        for name, got, want in (("Ym", out["Ym"][k], ref.yms[k]), ("Xhat", out["Xhat"][k], ref.xhats[k]), ("U", out["U"][k], ref.us[k]),
                                ("X after the step", out["X"][k + 1], ref.xs[k + 1])):
            if not np.array_equal(got, want):
                bad = np.flatnonzero((got != want).any(axis=1))
                raise AssertionError(f"{case.name}: first difference in {name} at step {k}: {bad.size} of {len(got)} scenarios "
                                     f"(first {bad[:5]}), max |diff| = {np.abs(got - want).max():.3e}")
    for key, want in _pairs(case, ref):
        assert np.array_equal(out[key], want), (case.name, key, float(np.abs(out[key] - want).max()))


def _reference(mpc, case, data, **over):
    import uncertain_reference as ur
    from conftest import oracle_ldp_from
    return ur.run_case(case, oracle_ldp_from(mpc.control_model().ldp()), data, settings=_oracle_settings(mpc), **over)


def _run_and_compare(lmpc, case, mpc=None):
    import uncertain_reference as ur
    data = ur.case_data(case)
    mpc = _mpc(lmpc, data.prob) if mpc is None else mpc
    ref = _reference(mpc, case, data)
    out = _direct(lmpc, mpc, case, data)
    _assert_equal(case, out, ref)
    return out, ref, data, mpc


def _cases(group):
    import uncertain_reference as ur
    return [pytest.param(c, id=c.name) for c in group(ur)]


@pytest.mark.parametrize("case", _cases(lambda ur: ur.STATES))
def test_every_state_size_equals_the_host_reference(lmpc, case):
    # uncertain_pre_kernel<NX> / uncertain_post_kernel<NX, false> for NX = 1 .. 8 and the run-time kernels at nx = 9, 17,
    # 32: process and measurement noise both drawn, the observer on for odd nx, S = 300 (a ragged second workgroup)
    _run_and_compare(lmpc, case)


@pytest.mark.parametrize("case", _cases(lambda ur: ur.DRAWS))
def test_shapes_of_the_draw(lmpc, case):
    # nw = nx without Gw; nw = 1, 2, 3, 5 through a Gw (an odd count uses half a block); ny = 1, 3; supplied blocks per
    # scenario and shared; drawn with supplied and the reverse; the descriptor's noise with drawn process noise
    _run_and_compare(lmpc, case)


@pytest.mark.parametrize("case", _cases(lambda ur: ur.ENSEMBLES))
def test_plant_ensembles(lmpc, case):
    # n_plants = 1, 2, 3, S with the default index, an explicit index with repeats, a scenario_offset under the modulo,
    # nd = 0 and 2 (the stride of a plant's rows)
    _run_and_compare(lmpc, case)


@pytest.mark.parametrize("case", _cases(lambda ur: ur.SIZES))
def test_batch_and_run_sizes(lmpc, case):
    # S = 1, 255, 256, 257, 1000 with T = 1 (first and last step in one POST launch) and 2
    _run_and_compare(lmpc, case)


@pytest.mark.parametrize("case", _cases(lambda ur: ur.COST + ur.WARM))
def test_cost_and_warm_start_paths(lmpc, case):
    # uncertain_post_kernel<4, true> with and without the observer (scratch = [xhat | ulast]); warm and cold solves
    out, ref, _, _ = _run_and_compare(lmpc, case)
    if case.cost:
        assert ref.cost.min() > 0 and ref.violation.max() > 0


def test_sharded_run_equals_the_whole(lmpc):
    # 1000 scenarios = two calls of 500 with scenario_offset: the draws and the default plant index follow the GLOBAL index
    import uncertain_reference as ur
    case = ur.SHARD
    whole, ref, data, mpc = _run_and_compare(lmpc, case)
    for lo in (0, 500):
        part = _direct(lmpc, mpc, case, data, sl=slice(lo, lo + 500), scenario_offset=case.scenario_offset + lo)
        for key in ("X", "U", "Xhat", "Ym", "W", "flag_min"):
            want = whole[key][lo:lo + 500] if key == "flag_min" else whole[key][:, lo:lo + 500]
            assert np.array_equal(part[key], want), (lo, key)
    local = _direct(lmpc, mpc, case, data, sl=slice(500, 1000))
    assert not np.array_equal(local["W"], whole["W"][:, 500:])


def test_continued_run_equals_the_whole(lmpc):
    # T = 6 = two calls of 3, the second with step_offset + 3, the carried x / xhat / uprev and the shifted trajectories
    import torch
    import uncertain_reference as ur
    case = ur.CONTINUE
    whole, ref, data, mpc = _run_and_compare(lmpc, case)
    dev = torch.device("cuda", mpc.control_model().device)
    x = torch.from_numpy(data.x0.copy()).to(dev)
    state = (x, x.clone(), torch.zeros((case.S, case.nu), dtype=torch.float64, device=dev))
    first = _direct(lmpc, mpc, case, data, T=3, state=state)
    second = _direct(lmpc, mpc, case, data, cols=slice(3, None), T=3, state=first["_state"], step_offset=case.step_offset + 3)
    for key in ("U", "Xhat", "Ym", "Y", "W"):
        assert np.array_equal(np.concatenate([first[key], second[key]]), whole[key]), key
    assert np.array_equal(np.concatenate([first["X"], second["X"][1:]]), whole["X"])
    assert np.array_equal(second["x"], ref.xs[-1]) and np.array_equal(second["xhat"], ref.xhat_final)


def test_same_seed_repeats_and_another_seed_differs(lmpc):
    import uncertain_reference as ur
    case = ur.STATES[3]
    first, ref, data, mpc = _run_and_compare(lmpc, case)
    again = _direct(lmpc, mpc, case, data)
    other = _direct(lmpc, mpc, case, data, seed=case.key + 1)
    for key in ("X", "U", "W", "Ym"):
        assert np.array_equal(again[key], first[key]), key
        assert not np.array_equal(other[key], first[key]), key
    assert np.array_equal(other["W"], _reference(mpc, case, data, seed=case.key + 1).ws)


def test_everything_off_is_the_plain_loop_bit_for_bit(lmpc):
    # no source, no plant table: lmpc_simulate_scenario_device on the same handle, output for output
    import uncertain_reference as ur
    case = ur.PLAIN
    out, ref, data, mpc = _run_and_compare(lmpc, case)
    plain = _direct(lmpc, mpc, case, data, plain=True)
    assert "W" not in out
    for key in ("X", "U", "Y", "Ym", "Xhat", "D", "x", "uprev", "flag_min"):
        assert np.array_equal(out[key], plain[key]), key


def test_one_handle_several_runs_then_a_plain_solve(lmpc):
    # S = 200, then 2000 (the scratch and the constants regrow), then 50; afterwards the handle solves as a fresh one does
    import uncertain_reference as ur
    mpc = None
    for case in ur.RERUN:
        _, ref, _, mpc = _run_and_compare(lmpc, case, mpc)
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
    # lmpc_simulate_scenario_uncertain: host arrays in and out -- a drawn process source through Gw, a supplied
    # measurement block, the plant table with a HOST index, W_traj
    import scenario_reference as sr
    import uncertain_reference as ur
    from linearmpc_jl_amd._cabi import Block, Uncertainty, check
    case = ur.TWIN
    data = ur.case_data(case)
    mpc = _mpc(lmpc, data.prob)
    plant = _plant(lmpc, sr.plant_of(data.prob))
    model = mpc.control_model()
    S, T, nx, nu, ny, nd = case.S, case.T, case.nx, case.nu, case.ny, case.nd
    model.set_observer(*data.kf.codegen_arrays(), nx, nu, nd, ny)
    ref = _reference(mpc, case, data)
    lay = lambda a: np.ascontiguousarray(np.swapaxes(a, 1, 2))             # (S, w, T) -> (S, T, w): column after column
    r, d, v = lay(data.r), lay(data.d), lay(data.measurement_noise)
    blk = lambda a, w: Block(a.ctypes.data, w * T, w, T, 0, 0)
    desc, hold = model.scenario_descriptor(plant.dynamics_rows(), nx, nd, plant.measurement_rows(), ny, r=blk(r, ny),
                                           d=blk(d, nd), nuprev=nu, use_observer=True)
    x, up = data.x0.copy(), np.zeros((S, nu))
    U, X, fm = np.empty((T, S, nu)), np.empty((T + 1, S, nx)), np.empty(S, np.int32)
    Y, Ym, Xh, D, W = (np.empty((T, S, w)) for w in (ny, ny, nx, nd, nx))
    desc.Y_traj, desc.Ym_traj, desc.Xhat_traj, desc.D_traj = (a.ctypes.data for a in (Y, Ym, Xh, D))
    lo, hi = np.ascontiguousarray(data.process.lo), np.ascontiguousarray(data.process.hi)
    Gw = np.ascontiguousarray(data.Gw)
    table = np.ascontiguousarray(np.stack([_plant(lmpc, q).dynamics_rows() for q in data.plants]))
    index = np.ascontiguousarray(data.plant_index)
    un = Uncertainty()
    un.process.w, un.process.lo, un.process.hi, un.Gw = case.nw, lo.ctypes.data, hi.ctypes.data, Gw.ctypes.data
    un.measurement.w, un.measurement.src = ny, blk(v, ny)
    un.seed, un.scenario_offset, un.step_offset = case.key, case.scenario_offset, case.step_offset
    un.n_plants, un.plants, un.plant_index, un.W_traj = len(data.plants), table.ctypes.data, index.ctypes.data, W.ctypes.data
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    check(lmpc.lib().lmpc_simulate_scenario_uncertain(model._h, S, T, ctypes.byref(desc), ctypes.byref(un), vp(x), None, vp(up),
                                                      vp(U), vp(X), vp(fm)), model._h)
    for name, got, want in (("X", X, ref.xs), ("U", U, ref.us), ("Y", Y, ref.ys), ("Ym", Ym, ref.yms), ("Xhat", Xh, ref.xhats),
                            ("D", D, ref.ds), ("W", W, ref.ws), ("x", x, ref.xs[-1]), ("uprev", up, ref.uprev_final),
                            ("flag_min", fm, ref.flag_min)):
        assert np.array_equal(got, want), name


def test_simulation_with_a_list_of_plants_and_a_uniform(lmpc):
    import scenario_reference as sr
    import uncertain_reference as ur
    case = ur.LIST
    data = ur.case_data(case)
    mpc = _mpc(lmpc, data.prob)
    ref = _reference(mpc, case, data)
    sc = lmpc.Scenario(data.x0, N=case.T, r=data.r, d=data.d, process_noise=lmpc.Uniform(data.process.lo, data.process.hi))
    sim = lmpc.Simulation(mpc, sc, [_plant(lmpc, q) for q in data.plants], observer=data.kf.codegen_arrays(), seed=case.key)
    step = lambda a: a.transpose(1, 2, 0)
    assert sim.ws.shape == (case.S, case.nx, case.T)
    for name, got, want in (("xs", sim.xs, step(ref.xs[:-1])), ("us", sim.us, step(ref.us)), ("xhats", sim.xhats, step(ref.xhats)),
                            ("yms", sim.yms, step(ref.yms)), ("ys", sim.ys, step(ref.ys)), ("ds", sim.ds, step(ref.ds)),
                            ("ws", sim.ws, step(ref.ws)), ("x_final", sim.x_final, ref.xs[-1]), ("flag_min", sim.flag_min, ref.flag_min)):
        assert np.array_equal(got, want), name
    # the new arguments are refused where the loop is not extended; without them the existing path runs
    obs = lmpc.offset_free_observer(data.prob.F, data.prob.G, data.prob.C, Gd=data.prob.Gd, Dd=data.prob.Dd, method="velocity",
                                    K=np.zeros((case.nx, case.ny)))
    with pytest.raises(ValueError, match="not available"):
        lmpc.Simulation(mpc, sc, _plant(lmpc, data.plants[0]), observer=obs)
    with pytest.raises(ValueError, match="agree in nx"):
        lmpc.Simulation(mpc, lmpc.Scenario(data.x0, N=2), [_plant(lmpc, data.plants[0]), lmpc.Plant(np.eye(2), np.ones((2, 1)))])
    plain = lmpc.Simulation(mpc, lmpc.Scenario(data.x0, N=case.T, r=data.r, d=data.d), _plant(lmpc, sr.plant_of(data.prob)),
                            observer=data.kf.codegen_arrays())
    assert not hasattr(plain, "ws") and np.array_equal(plain.us[..., 0], ref.us[0])


def test_robust_worst_case_through_simulation(lmpc):
    # docs/src/manual/robust.md:17,78: the nominal controller keeps y <= 0.5 without w and breaks it under w = +0.005
    import scenario_reference as sr
    import uncertain_reference as ur
    p = ur.robust_problem()
    mpc = _mpc(lmpc, p)
    dims, previews = sr.dims_of(p)
    from conftest import oracle_ldp_from
    ldp = oracle_ldp_from(mpc.control_model().ldp())
    r = np.array([[0.5]])
    ref = ur.uncertain_run(ldp, dims, sr.plant_of(p), np.zeros((1, 2)), 100, r=r, previews=previews, settings=_oracle_settings(mpc),
                           process=ur.Box(np.full(2, 0.005), np.full(2, 0.005)))
    plant = _plant(lmpc, sr.plant_of(p))
    sim = lmpc.Simulation(mpc, lmpc.Scenario(np.zeros(2), N=100, r=r, process_noise=lmpc.Uniform([0.005, 0.005], [0.005, 0.005])), plant)
    assert sim.ys.max() > 0.55 and sim.flag_min.min() >= 1
    assert np.array_equal(sim.ys, ref.ys[:, 0].T) and np.array_equal(sim.us, ref.us[:, 0].T) and np.array_equal(sim.xs, ref.xs[:-1, 0].T)
    assert np.array_equal(sim.ws, np.full((2, 100), 0.005))
    quiet = lmpc.Simulation(mpc, lmpc.Scenario(np.zeros(2), N=100, r=r), plant)
    assert quiet.ys.max() < 0.5 + 1e-9
