"""Host side of the scenario loop with an explicit controller (no GPU): the numpy restatement of the controller
(tests/explicit_scenario_reference.py) against lmpc_explicit_locate_host, the conditions that keep the cases of
tests/test_gpu_explicit_scenario.py from passing emptily, computed from the reference run alone on controllers built
on the host (lmpc_explicit_build_ldp from an oracle-solved sample of the same box), and the refusals of
lmpc_explicit_scenario_check / lmpc_explicit_simulate_scenario*."""
import ctypes

import numpy as np
import pytest

import explicit_scenario_reference as er
import scenario_reference as sr
from oracle import ldp as oldp


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


_BUILT = {}


def _host_controller(lmpc, case):
    """(controller, its table, the host LDP, the case's data); one build per problem and training recipe"""
    key = (er.problem_key(case), case.max_regions, case.nsamples, case.scale, case.kind)
    data = er.case_data(case)
    if key not in _BUILT:
        L = sr.host_ldp(data.prob)
        pk = dict(M=L.M, du=L.du0, dl=L.dl0, Dth=L.Dth, Rout=L.Rout, x0=L.x0, Xth=L.Xth, sense=L.sense, ms=L.ms)
        th = er.training_sample(case, data)
        _, ef, _, act = oldp.solve_batch(L, th)
        opts = dict(max_regions=case.max_regions, soft_band=er.BAND)
        if case.kind == "miss":
            opts["box"] = er.training_box(case, data)
        ec = lmpc.explicit.ExplicitController.build_ldp(pk, th, act, ef, **opts)
        _BUILT[key] = (ec, er.Table(ec.blob()), L)
    return _BUILT[key] + (data,)


# ------------------------------------------------------------------ the restatement against locate_host
def _points(case, data, n, rng):
    """theta points of the training box blown up by 1.5: inside regions, in none, and (soft problems) in the band"""
    lb, ub = er.training_box(case, data)
    mid, half = 0.5 * (lb + ub), 0.75 * (ub - lb)
    return mid + half * rng.uniform(-1, 1, (n, lb.size))


@pytest.mark.parametrize("case", [er.NT16[3], er.COST[0], er.NT32[1]], ids=lambda c: c.name)
def test_numpy_controller_equals_locate_host(lmpc, case):
    # hard-row problems (nth 12 and 29) and the soft-row problem: region, flag and x, np.array_equal, 2400 points
    ec, tab, L, data = _host_controller(lmpc, case)
    rng = np.random.default_rng(5)
    th = _points(case, data, 2400, rng)
    if case.base.soft:
        # points inside the band: for regions with soft multipliers, walk a located point along a ray until the soft
        # slack crosses primal_tol, then bisect onto the band
        x0, f0, r0, _ = ec.locate_host(th)
        lo, hi = th[f0 == 1], th[f0 == 2]
        if len(lo) and len(hi):
            n = min(len(lo), len(hi), 200)
            a, b = lo[:n].copy(), hi[:n].copy()
            for _ in range(60):
                mid = 0.5 * (a + b)
                fm = ec.locate_host(mid)[1]
                a[fm == 1], b[fm != 1] = mid[fm == 1], mid[fm != 1]
            th = np.vstack([th, a, b, 0.5 * (a + b)])
    x, f, r, _ = ec.locate_host(th)
    xn, fn, rn = er.locate(tab, th, 1e-6, 1e-6)
    assert np.array_equal(rn, r), int((rn != r).sum())
    assert np.array_equal(fn, f)
    loc = r >= 0
    assert np.array_equal(xn[loc], x[loc])
    assert 0.02 < (~loc).mean() < 0.98, "points in regions and points in none"
    if case.base.soft:
        assert (f == 2).any() and (f == 1).any()
        # the compared set holds points that a region holds and only the band rule sends to the implicit path
        in_band = (r < 0) & (er.locate(tab, th, 1e-6, 1e-6, band=-1.0)[2] >= 0)
        assert in_band.any(), "no point inside the soft band"
        print("points inside the soft band:", int(in_band.sum()))
        print("points located:", int(loc.sum()), "unlocated:", int((~loc).sum()), "flag 2:", int((f == 2).sum()))


def test_numpy_controller_covers_the_soft_band(lmpc):
    # a point whose soft slack lies inside the band is unlocated although a region holds it: built by widening the band
    case = er.COST[0]
    ec, tab, L, data = _host_controller(lmpc, case)
    th = _points(case, data, 2400, np.random.default_rng(6))
    _, f_narrow, r_narrow = er.locate(tab, th, 1e-6, 1e-6, band=er.BAND)
    _, f_wide, r_wide = er.locate(tab, th, 1e-6, 1e-6, band=0.999999)
    assert ((r_narrow >= 0) & (r_wide < 0)).any(), "no point between the two bands"
    assert np.array_equal(r_wide[r_wide >= 0], r_narrow[r_wide >= 0])


# ------------------------------------------------------------------ the cases' conditions
@pytest.mark.parametrize("case", er.ECASES, ids=lambda c: c.name)
def test_gpu_cases_do_not_pass_emptily(lmpc, case):
    ec, tab, L, data = _host_controller(lmpc, case)
    ref = er.run_explicit_case(case, tab, L, data)
    er.check_explicit_conditions(case, ref)
    dims, previews = sr.dims_of(data.prob)
    nth = L.nth
    assert er.expected_class(case, nth)[1] == case.nt, (case.name, nth)
    if case.base.S * case.base.T >= 40:
        print(case.name, "nth", nth, "regions", tab.nregions, "fallback share %.3f" % float((ref.regions < 0).mean()))


def test_case_list_covers_every_instantiation():
    got = set()
    for c in er.INSTANCES:
        data = er.case_data(c)
        got.add(er.expected_class(c, sr.host_ldp(data.prob).nth))
    want = {(nx, nt) for nx in range(1, 8) for nt in (8, 16, 32)} | {(nx, nt) for nx in (8, 0) for nt in (16, 32)}
    assert got == want, (sorted(want - got), sorted(got - want))
    assert {c.base.observer for c in er.INSTANCES if c.nt == 8} == {True, False}
    assert {c.base.S for c in er.SIZES} == {1, 63, 64, 65, 255, 256, 257} and {c.base.T for c in er.SIZES} == {1, 2}
    assert all(c.base.S == 300 and c.base.T == 12 for c in er.INSTANCES)
    assert {c.base.observer for c in er.COST} == {True, False} and all(c.base.cost for c in er.COST)


def test_reference_imports_nothing_of_the_library():
    import ast
    tree = ast.parse(open(er.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert not names & {"linearmpc_jl_amd", "torch", "ctypes"}, names


# ------------------------------------------------------------------ refusals
def _desc(lmpc, nx=2, nu=1, nd=1, ny=1, r=(1, 0), d=(1, 0), p=(0, 0), nuprev=1, **kw):
    from linearmpc_jl_amd._cabi import Block, ScenarioSim
    buf = np.zeros(64)
    s = ScenarioSim()
    s.nx, s.nu, s.nd, s.ny = nx, nu, nd, ny
    s.plant, s.measurement = buf.ctypes.data, buf.ctypes.data
    s.r, s.d, s.p = (Block(None, 0, w, 1, 0, H) for w, H in (r, d, p))
    s.noise = Block(None, 0, 0, 1, 0, 0)
    s.nuprev = nuprev
    for k, v in kw.items():
        setattr(s, k, v)
    s._keep = buf
    return s


def _check(lmpc, s, nth=5, nout=1, obs=None, mode=1):
    from linearmpc_jl_amd._cabi import Observer, last_error
    o = None if obs is None else ctypes.byref(Observer(*obs, None, None, None))
    rc = lmpc.lib().lmpc_explicit_scenario_check(nth, nout, o, ctypes.byref(s) if s is not None else None, mode)
    return rc, last_error(None)


def test_symbols_are_exported_and_bound(lmpc):
    from linearmpc_jl_amd.explicit import _bind
    L = _bind()                                  # the lmpc_explicit_* entry points are bound there, on first use
    assert L is lmpc.lib()
    for name in ("lmpc_explicit_scenario_check", "lmpc_explicit_simulate_scenario_device", "lmpc_explicit_simulate_scenario"):
        assert name in lmpc.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.lmpc_abi_version() == 2


def test_a_well_formed_descriptor_passes(lmpc):
    for mode in (0, 1):
        rc, msg = _check(lmpc, _desc(lmpc), mode=mode)
        assert rc == 1, msg
    rc, msg = _check(lmpc, _desc(lmpc, use_observer=1), obs=(2, 1, 1, 1))
    assert rc == 1, msg


@pytest.mark.parametrize("field,kwargs,call", [
    ("warm", dict(warm=1), {}),
    ("mode", {}, dict(mode=2)),
    ("mode", {}, dict(mode=-1)),
    ("nth", dict(nx=30, r=(1, 0), d=(1, 0), nuprev=1), dict(nth=33)),
    # ... and what lmpc_scenario_check refuses, through the same entry point
    ("nx", dict(nx=33), {}),
    ("nu", dict(nu=2), {}),
    ("d.w", dict(d=(2, 0)), dict(nth=6)),
    ("r.H", dict(r=(1, -1)), {}),
    ("noise.H", dict(), dict(noise_H=3)),
    ("nuprev", dict(nuprev=2), dict(nth=6)),
    ("use_observer", dict(use_observer=1), {}),
    ("nx", dict(use_observer=1), dict(obs=(3, 1, 1, 1))),
    ("nth", dict(), dict(nth=7)),
])
def test_every_refusal_names_its_field(lmpc, field, kwargs, call):
    from linearmpc_jl_amd._cabi import Block
    s = _desc(lmpc, **kwargs)
    call = dict(call)
    if "noise_H" in call:
        s.noise = Block(None, 0, 1, 1, 0, call.pop("noise_H"))
    rc, msg = _check(lmpc, s, **call)
    assert rc == -100, (rc, msg)
    assert msg.startswith("lmpc_explicit_scenario_check: " + field + ":"), msg


def test_null_descriptor_and_outputs_are_refused(lmpc):
    buf = np.zeros(8)
    rc, msg = _check(lmpc, None)
    assert rc == -100 and msg.startswith("lmpc_explicit_scenario_check: s:")
    s = _desc(lmpc); s.cost_out = buf.ctypes.data
    rc, msg = _check(lmpc, s)
    assert rc == -100 and msg.startswith("lmpc_explicit_scenario_check: cost_out:")


def test_a_controller_without_a_handle_is_refused_before_the_gpu(lmpc):
    # lmpc_explicit_build_ldp leaves no handle: both entry points refuse, with the text in the controller's error slot
    from linearmpc_jl_amd.explicit import _bind
    case = er.NT16[3]
    ec, tab, L, data = _host_controller(lmpc, case)
    s = _desc(lmpc)
    x = np.zeros((4, 2))
    Lb = _bind()
    vp = ctypes.c_void_p
    rc = Lb.lmpc_explicit_simulate_scenario(ec._e, 4, 3, ctypes.byref(s), vp(x.ctypes.data), None, None, None, None, None,
                                            None, 1, None)
    msg = (Lb.lmpc_explicit_last_error(ec._e) or b"").decode()
    assert rc == -100 and msg.startswith("lmpc_explicit_simulate_scenario: e:"), (rc, msg)
    rc = Lb.lmpc_explicit_simulate_scenario_device(ec._e, 4, 3, ctypes.byref(s), vp(x.ctypes.data), None, None, None, None,
                                                   None, None, 1, None, None)
    msg = (Lb.lmpc_explicit_last_error(ec._e) or b"").decode()
    assert rc == -100 and msg.startswith("lmpc_explicit_simulate_scenario_device: e:"), (rc, msg)


def test_simulation_refuses_warm_and_an_unbuilt_tree(lmpc):
    # decided in Python before any handle is made
    mpc = object.__new__(lmpc.mpc.ExplicitMPC)
    mpc.controller, mpc.mpc, mpc.uprev = None, None, np.zeros(1)
    with pytest.raises(RuntimeError, match="binary search tree"):
        lmpc.Simulation(mpc, lmpc.Scenario([0.0], N=2), None)
    mpc.controller = object()
    with pytest.raises(ValueError, match="warm"):
        lmpc.Simulation(mpc, lmpc.Scenario([0.0], N=2), None, warm=True)
