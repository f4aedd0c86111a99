"""The nonlinear true plant on the GPU: lmpc_plant_program_eval_device against the CPU interpreter and the host
restatement, and lmpc_simulate_scenario_nonlinear_device -- bit for bit against lmpc_simulate_scenario_uncertain_device
for a plant program that writes the linear row sums (a check that needs nothing of the new reference), and against the
host reference loop of tests/nonlinear_reference.py for the cart-pole in closed loop with the pendulum controller
(Np = 10, Nc = 5).  The cases and the conditions that keep them from passing emptily are checked on the host first
(tests/test_nonlinear_host.py)."""
import numpy as np
import pytest

from test_gpu_uncertain import _mpc, _oracle_settings, _plant, _source

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


@pytest.fixture(scope="module")
def cartpole(lmpc):
    import nonlinear_reference as nr
    dims = {k: v for k, v in nr.CARTPOLE.items() if k != "Ts"}
    return lmpc.NonlinearPlant(lambda x, u, d, q: nr.cartpole(x, u, d, q, lmpc), Ts=nr.CARTPOLE["Ts"], C=nr.controller().C, **dims)


@pytest.fixture(scope="module")
def pendulum(lmpc):
    """the controller, its oracle-side LDP and settings: shared by the closed-loop tests"""
    import nonlinear_reference as nr
    from conftest import oracle_ldp_from
    mpc = _mpc(lmpc, nr.controller())
    return mpc, oracle_ldp_from(mpc.control_model().ldp()), _oracle_settings(mpc)


def _dev(model):
    import torch
    return torch.device("cuda", model.device)


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ 1. one plant step
def _eval_device(lmpc, model, plant, x, u=None, d=None, q=None):
    import torch
    dev = _dev(model)
    out = model.plant_program_eval_device(plant, _t(x, dev), _t(u, dev) if plant.nu else None, _t(d, dev) if plant.nd else None,
                                          params=_t(q, dev))
    torch.cuda.synchronize(dev)
    model.check()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def model(pendulum):
    return pendulum[0].control_model()


def test_eval_device_every_operation_over_special_values(lmpc, model):
    import nonlinear_reference as nr
    plant = lmpc.NonlinearPlant(lambda x, u, d, q: nr.every_op(x, u, d, q, lmpc), **nr.EVERY_OP)
    x, u, d, q = nr.special_values()
    got = _eval_device(lmpc, model, plant, x, u, d, q)
    assert nr.same(got, plant.eval_host(x, u, d, q)), "device against the CPU interpreter"
    assert nr.same(got, nr.interpret(plant, x, u, d, q)), "device against the host restatement"


@pytest.mark.parametrize("which", ["slots", "instructions"])
def test_eval_device_at_the_caps(lmpc, model, which):
    import nonlinear_reference as nr
    p = nr.slot_cap_program() if which == "slots" else nr.instruction_cap_program()
    plant = lmpc.NonlinearPlant.from_arrays(p.nx, p.nu, p.nd, p.nq, p.n_slots, p.consts, p.ins, p.out_slot)
    x = np.random.default_rng(8).uniform(-2, 2, (65, p.nx))
    got = _eval_device(lmpc, model, plant, x)
    assert np.array_equal(got, plant.eval_host(x)) and np.array_equal(got, nr.interpret(p, x))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_eval_device_cartpole_q_shared_and_per_scenario(lmpc, model, cartpole, N):
    import nonlinear_reference as nr
    rng = np.random.default_rng(N)
    x, u, q = rng.uniform(-3, 3, (N, 4)), rng.uniform(-2, 2, (N, 1)), rng.uniform(0.5, 1.5, (N, 3))
    x[:, 2] = np.linspace(-7.0, 7.0, N)
    for qq in (q, q[0].copy()):
        got = _eval_device(lmpc, model, cartpole, x, u, None, qq)
        assert np.array_equal(got, cartpole.eval_host(x, u, None, qq)) and np.array_equal(got, nr.interpret(cartpole, x, u, None, qq))


def test_eval_device_refuses_a_bad_program_before_the_gpu(lmpc, model):
    import nonlinear_reference as nr
    import torch
    O = nr.OPS
    bad = lmpc.NonlinearPlant.from_arrays(1, 0, 0, 0, 2, [], [[O["LOADX"], 0, 0, 0, 0], [O["ADD"], 1, 0, 5, 0]], [1])
    with pytest.raises(lmpc.LmpcError, match=r"lmpc_plant_program_eval_device: ins\[1\]\.b"):
        model.plant_program_eval_device(bad, torch.zeros((4, 1), dtype=torch.float64, device=_dev(model)))


# ------------------------------------------------------------------ 2. linear cross-check against the uncertain loop
def _sparse_rows(rows, nx):
    """dense rows for nx <= 9; for larger nx F keeps its diagonal and superdiagonal, so that the program stays under the
    instruction and constant caps"""
    rows = rows.copy()
    if nx > 9:
        F = rows[:, 1:1 + nx]
        rows[:, 1:1 + nx] = np.triu(F) - np.triu(F, 2)
    return rows


def _linear_program(lmpc, rows, nx, nu, nd):
    """f_offset + F x + G u + Gd d in the row-sum order of dynamics_rows; a term whose coefficient is exactly 0 is left out
    (it would add +-0 to a sum that is not zero here: no bit changes)"""
    def f(x, u, d, q):
        out = []
        for a in range(nx):
            acc = float(rows[a, 0])
            for j, v in enumerate(list(x) + list(u) + list(d)):
                if rows[a, 1 + j] != 0.0:
                    acc = acc + float(rows[a, 1 + j]) * v
            out.append(acc)
        return out
    return f


@pytest.mark.parametrize("quiet", [False, True], ids=["noise-observer", "quiet"])
@pytest.mark.parametrize("nx", [1, 4, 9, 32])
def test_linear_program_equals_the_uncertain_loop(lmpc, nx, quiet):
    # nonlinear_post_kernel<1>, <4> and the run-time instantiation at nx = 9, 32; process noise drawn for nx <= 9, through a
    # Gw for nx = 32; measurement noise drawn; the observer on for odd nx.  quiet: every source and the observer off.
    import torch
    import scenario_reference as sr
    import uncertain_reference as ur
    case = next(c for c in ur.STATES if c.nx == nx)
    if nx == 32:
        case = ur.Case("nx32-gw", 32, seed=32, observer=False, x0=ur.X0[32], nw=3)
    data = ur.case_data(case)
    mpc = _mpc(lmpc, data.prob)
    model = mpc.control_model()
    dev = _dev(model)
    nominal = sr.plant_of(data.prob)
    lin = _plant(lmpc, nominal)
    rows = _sparse_rows(lin.dynamics_rows(), nx)
    plant = lmpc.NonlinearPlant(_linear_program(lmpc, rows, nx, case.nu, case.nd), nx, case.nu, case.nd, C=nominal.C, Dd=nominal.Dd,
                                h_offset=nominal.h_offset)
    obs = data.kf is not None and not quiet
    if obs:
        model.set_observer(*data.kf.codegen_arrays(), nx, case.nu, case.nd, case.ny)
    want = ("U", "X", "Y", "Ym", "Xhat", "D") + (() if quiet else ("W",))
    outs = []
    for which in ("uncertain", "nonlinear"):
        x = _t(data.x0, dev)
        kw = dict(r=_t(data.r, dev), d=_t(data.d, dev), use_observer=obs, want=want, nd=case.nd, ny=case.ny,
                  process=None if quiet else _source(lmpc, data.process, dev), Gw=None if quiet else data.Gw,
                  measurement_noise=None if quiet else _source(lmpc, data.measurement_noise, dev), seed=case.key)
        if which == "uncertain":
            out = model.simulate_scenario_uncertain(x, case.T, rows, lin.measurement_rows(), **kw)
        else:
            out = model.simulate_scenario_nonlinear(x, case.T, plant, **kw)
        torch.cuda.synchronize(dev)
        model.check()
        outs.append({k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)})
    a, b = outs
    assert set(a) == set(b) and {"X", "U", "x", "uprev", "flag_min"} <= set(a) and (quiet or "W" in a) and (not obs or "Xhat" in a)
    for key in sorted(a):
        assert np.array_equal(a[key], b[key]), (case.name, key, float(np.abs(a[key] - b[key]).max()))
    assert np.abs(a["U"]).max() > 0 and not np.array_equal(a["X"][1], a["X"][0]) and (quiet or np.abs(a["W"]).max() > 0)


# ------------------------------------------------------------------ 3. the cart-pole in closed loop
def _direct(lmpc, mpc, plant, case, data, sl=slice(None), T=None, state=None, **over):
    """model.simulate_scenario_nonlinear on the scenarios `sl` of a case: every array as numpy.  state = (x, xhat, uprev)
    tensors of a run that is continued."""
    import torch
    model = mpc.control_model()
    dev = _dev(model)
    if data.observer is not None:
        model.set_observer(*data.observer, 4, 1, 0, 2)
    x, xhat, uprev = (_t(data.x0[sl], dev), None, None) if state is None else state
    cost = None if data.cost is None else lmpc.BatchedQP.sim_cost(4, 1, **data.cost)
    q = data.q if data.q.ndim == 1 else data.q[sl]
    un = dict(params=q, process=_source(lmpc, data.process, dev), measurement_noise=_source(lmpc, data.measurement_noise, dev),
              Gw=data.Gw, seed=case.key, scenario_offset=case.scenario_offset, step_offset=case.step_offset)
    un.update(over)
    out = model.simulate_scenario_nonlinear(
        x, case.T if T is None else T, plant, r_width=2, xhat=xhat, uprev=uprev, use_observer=data.observer is not None,
        warm=case.warm, cost=cost, want_cost=cost is not None, want_violation=cost is not None,
        want=("U", "X", "Y", "Ym", "Xhat") + (("W",) if data.process is not None else ()), **un)
    torch.cuda.synchronize(dev)
    model.check()
    res = {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}
    res["_state"] = (out["x"], out["xhat"], out["uprev"])
    return res


def _assert_equal(case, out, ref):
    """np.array_equal on every output; the steps in causal order first so that a failure names the first array and step"""
    for k in range(ref.us.shape[0]):
        for name, got, want in (("Ym", out["Ym"][k], ref.yms[k]), ("Xhat", out["Xhat"][k], ref.xhats[k]), ("U", out["U"][k], ref.us[k]),
                                ("X after the step", out["X"][k + 1], ref.xs[k + 1])):
            if not np.array_equal(got, want):
                bad = np.flatnonzero((got != want).any(axis=1))
                raise AssertionError(f"{case.name}: first difference in {name} at step {k}: {bad.size} of {len(got)} scenarios "
                                     f"(first {bad[:5]}), max |diff| = {np.abs(got - want).max():.3e}")
    pairs = [("X", ref.xs), ("U", ref.us), ("Y", ref.ys), ("Ym", ref.yms), ("Xhat", ref.xhats), ("x", ref.xs[-1]),
             ("uprev", ref.uprev_final), ("flag_min", ref.flag_min)]
    pairs += [("W", ref.ws)] if ref.ws is not None else []
    pairs += [("cost", ref.cost), ("violation", ref.violation)] if ref.cost is not None else []
    for key, want in pairs:
        assert np.array_equal(out[key], want), (case.name, key, float(np.abs(out[key] - want).max()))


def _run_and_compare(lmpc, pendulum, plant, case):
    import nonlinear_reference as nr
    mpc, ldp, settings = pendulum
    data = nr.case_data(case)
    ref = nr.run_case(case, ldp, plant, data, settings=settings)
    out = _direct(lmpc, mpc, plant, case, data)
    _assert_equal(case, out, ref)
    return out, ref, data


def _cases(group):
    import nonlinear_reference as nr
    return [pytest.param(c, id=c.name) for c in group(nr)]


@pytest.mark.parametrize("case", _cases(lambda nr: nr.CLOSED_LOOP))
def test_cartpole_closed_loop_equals_the_host_reference(lmpc, pendulum, cartpole, case):
    # 257 scenarios (four full workgroups and one lane), 20 steps, initial pole angles over [-3.3, 3.3]: plain; q per
    # scenario; drawn process noise through Gw; measurement noise and the observer; cost and violation; warm
    out, ref, data = _run_and_compare(lmpc, pendulum, cartpole, case)
    import nonlinear_reference as nr
    assert set(np.unique(nr.quadrant(out["X"][:-1, :, 2])).astype(int)) == {0, 1, 2, 3}


@pytest.mark.parametrize("case", _cases(lambda nr: nr.LOOP_SIZES))
def test_batch_sizes_around_the_workgroup(lmpc, pendulum, cartpole, case):
    # N = 1, 63, 64, 65 (the POST kernel's workgroup is one wavefront); q per scenario, process noise through Gw
    _run_and_compare(lmpc, pendulum, cartpole, case)


# ------------------------------------------------------------------ 4. split runs
def test_runs_split_by_scenarios_and_by_time_equal_the_whole(lmpc, pendulum, cartpole):
    import torch
    import nonlinear_reference as nr
    case = nr.SPLIT
    whole, ref, data = _run_and_compare(lmpc, pendulum, cartpole, case)
    mpc = pendulum[0]
    half = case.S // 2
    for lo in (0, half):
        part = _direct(lmpc, mpc, cartpole, case, data, sl=slice(lo, lo + half), scenario_offset=case.scenario_offset + lo)
        for key in ("X", "U", "Xhat", "Ym", "W", "flag_min"):
            want = whole[key][lo:lo + half] if key == "flag_min" else whole[key][:, lo:lo + half]
            assert np.array_equal(part[key], want), (lo, key)
    local = _direct(lmpc, mpc, cartpole, case, data, sl=slice(half, 2 * half))
    assert not np.array_equal(local["W"], whole["W"][:, half:])
    dev = _dev(mpc.control_model())
    x = _t(data.x0, dev)
    state = (x, x.clone(), torch.zeros((case.S, 1), dtype=torch.float64, device=dev))
    T1 = case.T // 2
    first = _direct(lmpc, mpc, cartpole, case, data, T=T1, state=state)
    second = _direct(lmpc, mpc, cartpole, case, data, T=case.T - T1, state=first["_state"], step_offset=case.step_offset + T1)
    for key in ("U", "Xhat", "Ym", "Y", "W"):
        assert np.array_equal(np.concatenate([first[key], second[key]]), whole[key]), key
    assert np.array_equal(np.concatenate([first["X"], second["X"][1:]]), whole["X"])
    assert np.array_equal(second["x"], ref.xs[-1]) and np.array_equal(second["xhat"], ref.xhat_final)
    assert np.array_equal(np.minimum(first["flag_min"], second["flag_min"]), whole["flag_min"])


# ------------------------------------------------------------------ 5. the reference's hundred steps
def test_hundred_steps_cold_and_warm(lmpc, cartpole):
    """test/runtests.jl:85-117 on the device: the example's controller (Np = 50, Nc = 5), the cart-pole from [5, 5, 0, 0]
    (and a second start), 100 steps: cold and warm each equal the host reference, and |u_cold - u_warm| < 1e-9 (the host
    check held: measured 0.0 on the host reference)."""
    import nonlinear_reference as nr
    import scenario_reference as sr
    from conftest import oracle_ldp_from
    prob = nr.controller(Np=50, Nc=5)
    mpc = _mpc(lmpc, prob)
    ldp, settings = oracle_ldp_from(mpc.control_model().ldp()), _oracle_settings(mpc)
    dims, previews = sr.dims_of(prob)
    data = nr.case_data(nr.Case("hundred", S=2))
    data.x0 = nr.HUNDRED["x0"].copy()
    us = {}
    for warm in (False, True):
        case = nr.Case("hundred-warm" if warm else "hundred-cold", S=2, T=nr.HUNDRED["T"], warm=warm)
        ref = nr.nonlinear_run(ldp, dims, sr.plant_of(prob), cartpole, data.x0, case.T, q=data.q, previews=previews, warm=warm,
                               settings=settings)
        out = _direct(lmpc, mpc, cartpole, case, data)
        _assert_equal(case, out, ref)
        us[warm] = out["U"]
    diff = float(np.abs(us[False] - us[True]).max())
    print("max |u_cold - u_warm| over 100 steps on the device:", diff)
    assert diff < 1e-9, diff


# ------------------------------------------------------------------ 6. call sequences on one handle
def test_nonlinear_then_uncertain_then_nonlinear_then_a_plain_solve(lmpc, pendulum, cartpole):
    import torch
    import nonlinear_reference as nr
    import scenario_reference as sr
    mpc, ldp, settings = pendulum
    model = mpc.control_model()
    dev = _dev(model)
    case = nr.CLOSED_LOOP[2]                                # drawn process noise through Gw
    first, ref, data = _run_and_compare(lmpc, pendulum, cartpole, case)
    lin = _plant(lmpc, sr.plant_of(data.prob))
    want = nr.linearised_run(case, ldp, data, settings=settings)
    out = model.simulate_scenario_uncertain(_t(data.x0, dev), case.T, lin.dynamics_rows(), lin.measurement_rows(), ny=2, r_width=2,
                                            process=_source(lmpc, data.process, dev), Gw=data.Gw, seed=case.key, want=("U", "X", "W"))
    torch.cuda.synchronize(dev)
    model.check()
    for key, w in (("X", want.xs), ("U", want.us), ("W", want.ws)):
        assert np.array_equal(out[key].cpu().numpy(), w), key
    again = _direct(lmpc, mpc, cartpole, case, data)
    for key in ("X", "U", "W", "Ym", "flag_min"):
        assert np.array_equal(again[key], first[key]), key
    q = mpc.mpQP
    fresh = lmpc.BatchedQP.from_mpqp(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, nout=mpc.nu, nx=mpc.nx, settings=mpc.settings)
    theta = np.ascontiguousarray(ref.thetas.reshape(-1, ref.thetas.shape[-1]))
    a, b = model.solve(theta), fresh.solve(theta)
    fresh.close()
    for got, w in zip(a, b):
        assert np.array_equal(np.asarray(got), np.asarray(w))
    assert np.array_equal(np.asarray(a[0]), ref.us.reshape(-1, mpc.nu))


def test_host_pointer_twin_equals_the_host_reference(lmpc, pendulum, cartpole):
    # lmpc_simulate_scenario_nonlinear: host arrays in and out -- q per scenario (HOST), a drawn process source through Gw,
    # W_traj; s->plant NULL
    import ctypes
    import nonlinear_reference as nr
    from linearmpc_jl_amd._cabi import Block, Uncertainty, check
    mpc, ldp, settings = pendulum
    case = nr.Case("twin", S=65, T=4, q="scenario", process=True)
    data = nr.case_data(case)
    ref = nr.run_case(case, ldp, cartpole, data, settings=settings)
    model = mpc.control_model()
    S, T = case.S, case.T
    desc, hold = model.scenario_descriptor(np.zeros(1), 4, 0, cartpole.measurement_rows(), 2, r=Block(None, 0, 2, 1, 0, 0), nuprev=1)
    desc.plant = None
    x, up, q = data.x0.copy(), np.zeros((S, 1)), np.ascontiguousarray(data.q)
    U, X, fm = np.empty((T, S, 1)), np.empty((T + 1, S, 4)), np.empty(S, np.int32)
    Ym, W = np.empty((T, S, 2)), np.empty((T, S, 4))
    desc.Ym_traj = Ym.ctypes.data
    lo, hi, Gw = (np.ascontiguousarray(a) for a in (data.process.lo, data.process.hi, data.Gw))
    un = Uncertainty()
    un.process.w, un.process.lo, un.process.hi, un.Gw = 2, lo.ctypes.data, hi.ctypes.data, Gw.ctypes.data
    un.seed, un.W_traj = case.key, W.ctypes.data
    p, keep = cartpole.program()
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    check(lmpc.lib().lmpc_simulate_scenario_nonlinear(model._h, S, T, ctypes.byref(desc), ctypes.byref(un), ctypes.byref(p), vp(q), 0,
                                                      vp(x), None, vp(up), vp(U), vp(X), vp(fm)), model._h)
    for name, got, want in (("X", X, ref.xs), ("U", U, ref.us), ("Ym", Ym, ref.yms), ("W", W, ref.ws), ("x", x, ref.xs[-1]),
                            ("uprev", up, ref.uprev_final), ("flag_min", fm, ref.flag_min)):
        assert np.array_equal(got, want), name
    # a plant table is refused, with the field named first; so is a program of another width
    un.n_plants, un.plants = 1, Gw.ctypes.data
    with pytest.raises(lmpc.LmpcError, match="lmpc_simulate_scenario_nonlinear: n_plants:"):
        check(lmpc.lib().lmpc_simulate_scenario_nonlinear(model._h, S, T, ctypes.byref(desc), ctypes.byref(un), ctypes.byref(p), vp(q), 0,
                                                          vp(x), None, vp(up), vp(U), vp(X), vp(fm)), model._h)
    un.n_plants, un.plants = 0, None
    desc.nd = 1
    with pytest.raises(lmpc.LmpcError, match="lmpc_simulate_scenario_nonlinear: "):
        check(lmpc.lib().lmpc_simulate_scenario_nonlinear(model._h, S, T, ctypes.byref(desc), ctypes.byref(un), ctypes.byref(p), vp(q), 0,
                                                          vp(x), None, vp(up), vp(U), vp(X), vp(fm)), model._h)


# ------------------------------------------------------------------ 7. Simulation
def test_simulation_with_a_nonlinear_plant(lmpc, pendulum, cartpole):
    import nonlinear_reference as nr
    import scenario_reference as sr
    mpc, ldp, settings = pendulum
    case = nr.Case("simulation", S=70, T=6, q="scenario", process=True, meas=True)
    data = nr.case_data(case)
    ref = nr.run_case(case, ldp, cartpole, data, settings=settings)
    direct = _direct(lmpc, mpc, cartpole, case, data)
    sc = lmpc.Scenario(data.x0, N=case.T, process_noise=lmpc.Uniform(data.process.lo, data.process.hi),
                       measurement_noise=lmpc.Uniform(data.measurement_noise.lo, data.measurement_noise.hi))
    sim = lmpc.Simulation(mpc, sc, cartpole, params=data.q, observer=data.observer, Gw=data.Gw, seed=case.key)
    step = lambda a: a.transpose(1, 2, 0)
    for name, got, key in (("xs", sim.xs, "X"), ("us", sim.us, "U"), ("xhats", sim.xhats, "Xhat"), ("yms", sim.yms, "Ym"),
                           ("ys", sim.ys, "Y"), ("ws", sim.ws, "W")):
        want = direct[key][:case.T]
        assert np.array_equal(got, step(want)), name
    assert np.array_equal(sim.x_final, direct["x"]) and np.array_equal(sim.flag_min, direct["flag_min"])
    assert np.array_equal(sim.us, step(ref.us)) and np.array_equal(sim.x_final, ref.xs[-1])
    with pytest.raises(ValueError, match="list of plants"):
        lmpc.Simulation(mpc, sc, [cartpole, cartpole], params=data.q)
    empc = lmpc.ExplicitMPC.__new__(lmpc.ExplicitMPC)
    with pytest.raises(ValueError, match="explicit controller"):
        lmpc.Simulation(empc, sc, cartpole, params=data.q)
    t = sr.plant_of(data.prob)
    off = lmpc.OffsetFreeObserver.__new__(lmpc.OffsetFreeObserver)
    with pytest.raises(ValueError, match="offset-free observer"):
        lmpc.Simulation(mpc, sc, cartpole, params=data.q, observer=off)
    lin = _plant(lmpc, t)
    with pytest.raises(ValueError, match="params needs"):
        lmpc.Simulation(mpc, lmpc.Scenario(data.x0, N=2), lin, params=data.q)
