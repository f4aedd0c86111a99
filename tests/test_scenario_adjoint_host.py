"""Scenario loop adjoint on the host (lmpc_scenario_vjp_host): no GPU.  Tapes come from the scenario loop's host
reference (scenario_reference.run_case); the host twin is held bit for bit to the numpy restatement of the sweep
(scenario_adjoint_reference.py), and the sweep itself to the truth twice: the tangent run propagated in extended
precision through the per-step Jacobians of lmpc_solve_jacobian_host, and central differences of the reference loop."""
import copy

import numpy as np
import pytest

import scenario_adjoint_reference as sar
import scenario_reference as sr
import sens_cases as sc

SIZES = [c for c in sr.SIZES if c.S in (1, 257)]
CASES = sr.SWEEP + sr.PREVIEWS + [sr.COST] + SIZES
SOFT = {"previews-nth64", "cost-nx4-nu3"}
TRUTH = [c for c in sr.SWEEP if c.nx in (1, 4, 9, 17, 32)] + sr.PREVIEWS + [sr.COST]

# Bounds of the two truth measures: the next power of two at or above 8 x the worst value measured with the reference
# over the cases of TRUTH (DESIGN.md 3.7c has the table), apart for the cases with SOFT rows, whose K form loses digits
# at rho_soft = 1e-6.
BOUND_TANGENT = {False: 2.0 ** -48, True: 2.0 ** -29}        # measured 2.38e-16 / 1.82e-10
BOUND_DIFFERENCE = {False: 2.0 ** -28, True: 2.0 ** -11}     # measured 3.30e-10 / 5.53e-5 (usable scenarios: >= 99.67 %)
USABLE = 0.9                                                 # share of a case's scenarios whose tape is unchanged at +-h


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


_CACHE = {}


def _setup(lmpc, case):
    """Problem, tape and the reference's sweep of a case (computed once)."""
    if case.name in _CACHE:
        return _CACHE[case.name]
    data = sr.case_data(case)
    L = sr.host_ldp(data.prob)
    pack = sc.pack_of(L)
    ref = sr.run_case(case, L, data)
    dims, previews = sr.dims_of(data.prob)
    nx, nu, wr, nd, nup, wp = dims
    plant = sr.plant_of(data.prob)
    ny = plant.C.shape[0]
    dyn, meas = sar.plant_rows(plant, nx, nu, nd)
    blocks = sar.case_blocks(case, data, dims, previews)
    obs = None if data.kf is None else data.kf.codegen_arrays()
    Xb, Ub = sar.cotangents(case, nx, nu)
    S = lmpc.default_settings()
    d = dict(data=data, L=L, pack=pack, ref=ref, dims5=(nx, nu, nd, ny, nup), dims=dims, previews=previews, dyn=dyn, meas=meas,
             blocks=blocks, obs=obs, Xb=Xb, Ub=Ub, S=S, cache=sar.sens_ref.derived(pack),
             sim=dict(nx=nx, nu=nu, nd=nd, ny=ny, plant=dyn, measurement=meas, nuprev=nup, use_observer=obs is not None, **blocks))
    d["adj"] = _reference(d, ref.active, ref.flags)
    _CACHE[case.name] = d
    return d


def _reference(d, active, flags, Xb="case", Ub="case", xhat_given=False):
    return sar.adjoint(d["pack"], d["dims5"], d["dyn"], d["meas"], active, flags, d["Xb"] if isinstance(Xb, str) else Xb,
                       d["Ub"] if isinstance(Ub, str) else Ub, d["blocks"], d["obs"], xhat_given, d["S"].rho_soft,
                       d["S"].zero_tol, d["cache"])


def _host(lmpc, d, active, flags, Xb="case", Ub="case", xhat_given=False):
    return lmpc.scenario_vjp_host(d["pack"], d["sim"], active, flags, d["Xb"] if isinstance(Xb, str) else Xb,
                                  d["Ub"] if isinstance(Ub, str) else Ub, observer=d["obs"], xhat_given=xhat_given)


def _twin(lmpc, d):
    """The host twin's sweep of the case's tape with the case's cotangents, as a namespace (computed once): what the
    truth measures and the conditions are taken on, so that they hold the library's export and not the reference alone."""
    if "twin" not in d:
        from types import SimpleNamespace
        d["twin"] = SimpleNamespace(**_host(lmpc, d, d["ref"].active, d["ref"].flags))
    return d["twin"]


def _assert_equal(adj, got):
    for k in ("x0bar", "xhat0bar", "uprev0bar", "rbar", "dbar", "pbar", "status_min"):
        a, b = getattr(adj, k), got[k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_host_twin_equals_the_reference_bit_for_bit(lmpc, case):
    d = _setup(lmpc, case)
    ref = d["ref"]
    _assert_equal(d["adj"], _host(lmpc, d, ref.active, ref.flags))
    assert (d["adj"].status_min == 1).all()
    if case.S * case.T >= 40:
        sar.check_conditions(d["blocks"], d["adj"], ref.active_sizes, case.T, need_clamp=any(l is not None for l in case.lengths),
                             need_big=case.name in SOFT)


@pytest.mark.parametrize("case", [sr.SWEEP[4 * 3 + 3], sr.SWEEP[4 * 8 + 0], sr.PREVIEWS[1]], ids=lambda c: c.name)
def test_failed_steps_give_zero_and_say_so(lmpc, case):
    # exit flags set to -1 on chosen scenario-steps: theta-bar of the step is zero, its control a constant, status_min 0
    d = _setup(lmpc, case)
    ref = d["ref"]
    flags = ref.flags.copy()
    rng = np.random.default_rng(5)
    hit = rng.random(flags.shape) < 0.1
    hit[:, 0] = False                                   # scenario 0 stays whole ...
    hit[-1, 1], hit[0, 2] = True, True                  # ... the last and the first step fail somewhere
    flags[hit] = -1
    adj = _reference(d, ref.active, flags)
    _assert_equal(adj, _host(lmpc, d, ref.active, flags))
    assert np.array_equal(adj.status_min == 0, hit.any(axis=0)) and set(np.unique(adj.status_min)) == {0, 1}
    for k in range(case.T):
        assert (adj.thbars[k][hit[k]] == 0).all() and (adj.thbars[k][~hit[k]] != 0).any()
    assert not np.array_equal(adj.x0bar[hit.any(axis=0)], d["adj"].x0bar[hit.any(axis=0)])
    assert np.array_equal(adj.x0bar[~hit.any(axis=0)], d["adj"].x0bar[~hit.any(axis=0)])


def test_cotangents_may_be_absent_and_xhat_given(lmpc):
    case = sr.SWEEP[4 * 3 + 2]                           # nx4, observer, cold
    d = _setup(lmpc, case)
    ref = d["ref"]
    for Xb, Ub in ((None, "case"), ("case", None), (None, None)):
        adj = _reference(d, ref.active, ref.flags, Xb, Ub)
        _assert_equal(adj, _host(lmpc, d, ref.active, ref.flags, Xb, Ub))
    assert (adj.x0bar == 0).all()
    own = _reference(d, ref.active, ref.flags, xhat_given=True)
    _assert_equal(own, _host(lmpc, d, ref.active, ref.flags, xhat_given=True))
    assert np.array_equal(own.x0bar + own.xhat0bar, d["adj"].x0bar) and (own.xhat0bar != 0).any()


def test_an_observer_that_is_not_the_plant(lmpc):
    # the cases' filters are built from the true plant (C-hat = C, Dd-hat = Dd, ...): with every observer array perturbed
    # the twin must still read each where the contract says
    case = sr.SWEEP[4 * 3 + 2]
    d = _setup(lmpc, case)
    ref = d["ref"]
    rng = np.random.default_rng(41)
    other = tuple(np.asarray(a, float) * (1.0 + 0.2 * rng.standard_normal(np.shape(a))) for a in d["obs"])
    d2 = dict(d, obs=other)
    adj = _reference(d2, ref.active, ref.flags)
    _assert_equal(adj, _host(lmpc, d2, ref.active, ref.flags))
    assert not np.array_equal(adj.x0bar, d["adj"].x0bar) and not np.array_equal(adj.dbar, d["adj"].dbar)


def test_conditions_reject_batches_that_miss_them(lmpc):
    d = _setup(lmpc, sr.PREVIEWS[1])
    ref, case = d["ref"], sr.PREVIEWS[1]
    sar.check_conditions(d["blocks"], _twin(lmpc, d), ref.active_sizes, case.T, need_clamp=True, need_big=True)
    with pytest.raises(AssertionError, match="zero gradient column"):       # no cotangent on the controls or the states
        sar.check_conditions(d["blocks"], _reference(d, ref.active, ref.flags, None, None), ref.active_sizes, case.T)
    with pytest.raises(AssertionError, match="no clamped column"):
        full = {k: None if b is None else (b[0], case.T, b[2]) for k, b in d["blocks"].items()}
        sar.check_conditions(full, _twin(lmpc, d), ref.active_sizes, case.T, need_clamp=True)
    with pytest.raises(AssertionError, match="lane capacity"):
        sar.check_conditions(d["blocks"], _twin(lmpc, d), np.minimum(ref.active_sizes, 8), case.T, need_big=True)
    assert ref.active_sizes.max() >= 10 and _setup(lmpc, sr.COST)["ref"].active_sizes.max() >= 10


# ------------------------------------------------------------------ the truth
def _direction(d, case, rng, scale=1.0):
    """A direction in (x0, r, d, p) shaped like the case's inputs (a shared trajectory gets one direction)."""
    data = d["data"]
    out = dict(x0=scale * rng.standard_normal(data.x0.shape))
    for k in ("r", "d", "p"):
        a = getattr(data, k)
        out[k] = None if (a is None or d["blocks"][k] is None) else scale * rng.standard_normal(a.shape)
    return out


def _inner_terms(d, case, adj, dr):
    """The terms of <adjoint, direction> per scenario, (S, terms): their sum is the inner product, the sum of their
    magnitudes the size it is measured against."""
    S, T = case.S, case.T
    terms = [adj.x0bar * dr["x0"]]
    for k in ("r", "d", "p"):
        bar = getattr(adj, k + "bar")
        if bar is None or dr[k] is None:
            continue
        Tc = bar.shape[0]
        a = np.broadcast_to(dr[k], (S,) + dr[k].shape[-2:])[..., :Tc]       # (S, w, Tc)
        terms.append((bar.transpose(1, 2, 0) * a).reshape(S, -1))
    return np.concatenate(terms, axis=1).astype(np.longdouble)


def _tangent_run(lmpc, d, case, dr):
    """<Xbar, dX> + <Ubar, dU> per scenario of the tangent run along dr, in np.longdouble, through the per-step
    Jacobians of the solve (lmpc_solve_jacobian_host on the tape); with the magnitudes of its terms."""
    ld = np.longdouble
    nx, nu, nd, ny, nup = d["dims5"]
    _, _, wr, _, _, wp = d["dims"]
    rH, dH, pH = d["previews"]
    ref, S, T = d["ref"], case.S, case.T
    dyn, meas = d["dyn"].astype(ld), d["meas"].astype(ld)
    F, G, Gd = dyn[:, 1:1 + nx], dyn[:, 1 + nx:1 + nx + nu], dyn[:, 1 + nx + nu:]
    C, Dd = meas[:, 1:1 + nx], meas[:, 1 + nx:]
    obs = d["obs"] is not None
    if obs:
        od = np.asarray(d["obs"][0], ld).reshape(nx, -1)
        om = np.asarray(d["obs"][1], ld).reshape(ny, -1)
        kt = np.asarray(d["obs"][2], ld).reshape(ny, nx)
        Fh, Gh, Gdh, Ch, Ddh = od[:, 1:1 + nx], od[:, 1 + nx:1 + nx + nu], od[:, 1 + nx + nu:], om[:, 1:1 + nx], om[:, 1 + nx:]
    tr = {k: None if dr[k] is None else sr.run_trajectory(dr[k], S, T).astype(ld) for k in ("r", "d", "p")}
    blk = lambda k, w, H, k0: sr.theta_block(tr[k], w, H, k0, S).astype(ld) if w else np.zeros((S, 0), ld)
    dx = dr["x0"].astype(ld)
    dxh, dup = dx.copy(), np.zeros((S, nup), ld)
    total, size = np.zeros(S, ld), np.zeros(S, ld)
    Xb, Ub = d["Xb"].astype(ld), d["Ub"].astype(ld)

    def take(bar, val):
        nonlocal total, size
        total = total + (bar * val).sum(axis=1)
        size = size + np.abs(bar * val).sum(axis=1)

    for k in range(T):
        take(Xb[k], dx)
        dk = sr._column(tr["d"], k) if tr["d"] is not None else np.zeros((S, nd), ld)
        if obs:
            inno = dx @ C.T + dk @ Dd.T - dxh @ Ch.T - dk @ Ddh.T
            dxc = dxh + inno @ kt
        else:
            dxc = dx
        dth = np.concatenate([dxc, blk("r", wr, rH, k + 1 if rH else k), blk("d", nd, dH, k), dup, blk("p", wp, pH, k)], axis=1)
        J, _ = lmpc.sens_host(d["pack"], ref.active[k], ref.flags[k])
        du = np.einsum("sut,st->su", J.astype(ld), dth)
        take(Ub[k], du)
        if obs:
            dxh = dxc @ Fh.T + du @ Gh.T + dk @ Gdh.T
        dx = dx @ F.T + du @ G.T + dk @ Gd.T
        dup = du[:, :nup]
    take(Xb[T], dx)
    return total, size


def measure_tangent(lmpc, case):
    d = _setup(lmpc, case)
    dr = _direction(d, case, np.random.default_rng(300 + case.seed))
    terms = _inner_terms(d, case, _twin(lmpc, d), dr)
    total, size = _tangent_run(lmpc, d, case, dr)
    return float((np.abs(terms.sum(axis=1) - total) / (np.abs(terms).sum(axis=1) + size)).max())


def measure_difference(lmpc, case, h=1e-6):
    """Central differences of reference_run along h x a standard normal direction in x0, r, d, p, on the scenarios whose
    tape is the same at -h, 0 and +h: (worst error relative to the size of the terms, share of usable scenarios)."""
    d = _setup(lmpc, case)
    dr = _direction(d, case, np.random.default_rng(400 + case.seed))
    ref, data = d["ref"], d["data"]
    runs = []
    for sgn in (1.0, -1.0):
        pert = copy.copy(data)
        pert.x0 = data.x0 + sgn * h * dr["x0"]
        for k in ("r", "d", "p"):
            if dr[k] is not None:
                setattr(pert, k, getattr(data, k) + sgn * h * dr[k])
        runs.append(sr.run_case(case, d["L"], pert))
    same = np.ones(case.S, bool)
    for run in runs:
        same &= (run.active == ref.active).all(axis=(0, 2)) & (run.flags == ref.flags).all(axis=0)
    J = lambda run: (d["Xb"] * run.xs).sum(axis=(0, 2)) + (d["Ub"] * run.us).sum(axis=(0, 2))
    fd = (J(runs[0]) - J(runs[1])) / (2.0 * h)
    terms = _inner_terms(d, case, _twin(lmpc, d), dr)
    err = np.abs(terms.sum(axis=1).astype(float) - fd) / np.abs(terms).sum(axis=1).astype(float)
    return float(err[same].max()), float(same.mean())


@pytest.mark.parametrize("case", TRUTH, ids=lambda c: c.name)
def test_truth_tangent_run_in_extended_precision(lmpc, case):
    err = measure_tangent(lmpc, case)
    print(f"tangent {case.name}: {err:.3e}")
    assert err <= BOUND_TANGENT[case.name in SOFT], err


@pytest.mark.parametrize("case", TRUTH, ids=lambda c: c.name)
def test_truth_central_differences_of_the_reference_loop(lmpc, case):
    err, usable = measure_difference(lmpc, case)
    print(f"difference {case.name}: {err:.3e}, usable {usable:.4f}")
    assert usable >= USABLE, usable
    assert err <= BOUND_DIFFERENCE[case.name in SOFT], err


# ------------------------------------------------------------------ refusals, exports
def test_refusals_and_exports(lmpc):
    from linearmpc_jl_amd._cabi import LmpcError
    L = lmpc.lib()
    for name in ("lmpc_simulate_scenario_taped_device", "lmpc_simulate_scenario_taped", "lmpc_scenario_vjp_device",
                 "lmpc_scenario_vjp", "lmpc_scenario_vjp_host", "lmpc_scenario_adjoint_launch_info"):
        assert hasattr(L, name) and name in lmpc.SYMBOLS, name
    assert L.lmpc_abi_version() == 2
    case = sr.SWEEP[4 * 3]
    d = _setup(lmpc, case)
    ref = d["ref"]
    call = lambda pack=d["pack"], sim=d["sim"], **kw: lmpc.scenario_vjp_host(pack, sim, ref.active, ref.flags, d["Xb"], d["Ub"],
                                                                             observer=d["obs"], **kw)
    with pytest.raises(LmpcError, match="BINARY") as e:
        sense = np.array(d["pack"]["sense"]).copy()
        sense[0] |= 16
        call(dict(d["pack"], sense=sense))
    assert e.value.code == -103
    with pytest.raises(LmpcError, match="variational") as e:
        call(is_avi=True)
    assert e.value.code == -103
    with pytest.raises(LmpcError, match="proximal") as e:
        S = lmpc.default_settings()
        S.eps_prox = 1e-3
        call(settings=S)
    assert e.value.code == -103
    with pytest.raises(LmpcError, match="nth") as e:           # block widths that do not add up
        call(sim=dict(d["sim"], nuprev=0))
    assert e.value.code == -100
    with pytest.raises(LmpcError, match="use_observer") as e:
        lmpc.scenario_vjp_host(d["pack"], dict(d["sim"], use_observer=True), ref.active, ref.flags, d["Xb"], d["Ub"], observer=None)
    assert e.value.code == -100
    nth0 = dict(d["pack"], nth=0, Dth=np.zeros((d["pack"]["m"], 0)), Xth=np.zeros((d["pack"]["nout"], 0)))
    with pytest.raises(LmpcError, match="no parameter") as e:
        call(nth0)
    assert e.value.code == -100


def test_reference_imports_nothing_of_the_library():
    import ast
    tree = ast.parse(open(sar.__file__).read())
    names = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            names.append(node.module or "")
    assert names and all(n.split(".")[0] in ("types", "numpy", "sens_reference", "loop_reference") for n in names), names
