"""Host side of the scenario loop (no GPU): the refusals of lmpc_scenario_check -- the check lmpc_simulate_scenario*
runs first, exposed so that it can be asked without a device --, the exported symbols, and the Python-side
formatting of trajectories into lmpc_block descriptors."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


def _desc(lmpc, nx=2, nu=1, nd=1, ny=1, r=(1, 0), d=(1, 0), p=(0, 0), noise=(0, 0), nuprev=0, use_observer=0):
    """A well-formed descriptor for a handle with nth = 4, nout = 1: theta = [x(2); r(1); d(1)]."""
    from linearmpc_jl_amd._cabi import Block, ScenarioSim
    keep = np.zeros(64)
    s = ScenarioSim()
    s.nx, s.nu, s.nd, s.ny = nx, nu, nd, ny
    s.plant = keep.ctypes.data
    s.measurement = keep.ctypes.data
    for name, (w, H) in (("r", r), ("d", d), ("p", p), ("noise", noise)):
        setattr(s, name, Block(None, 0, w, 1, 0, H))
    s.nuprev, s.use_observer, s.warm = nuprev, use_observer, 0
    s._keep = keep
    return s


def _check(lmpc, s, nth=4, nout=1, obs=None):
    from linearmpc_jl_amd._cabi import Observer, last_error
    o = None if obs is None else ctypes.byref(Observer(*obs, None, None, None))
    rc = lmpc.lib().lmpc_scenario_check(nth, nout, o, ctypes.byref(s) if s is not None else None)
    return rc, last_error(None)


def test_symbols_are_exported_and_bound(lmpc):
    L = lmpc.lib()
    for name in ("lmpc_scenario_check", "lmpc_simulate_scenario_device", "lmpc_simulate_scenario",
                 "lmpc_evaluate_cost_device", "lmpc_constraint_violation_device"):
        assert name in lmpc.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.lmpc_abi_version() == 2
    for name in ("Plant", "Scenario", "Simulation", "evaluate_cost", "constraint_violation"):
        assert hasattr(lmpc, name) and name in lmpc.__all__
    assert hasattr(lmpc.BatchedQP, "simulate_scenario")


def test_descriptor_layout_matches_the_header(lmpc, tmp_path):
    # sizeof / offsets of the two structs as a C compiler lays them out against the ctypes mirrors
    import os, shutil, subprocess
    from conftest import ROOT
    from linearmpc_jl_amd._cabi import ScenarioSim, SimCost
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lmpc_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(lmpc_scenario_sim), offsetof(lmpc_scenario_sim, r), '
                   'offsetof(lmpc_scenario_sim, noise), offsetof(lmpc_scenario_sim, nuprev), offsetof(lmpc_scenario_sim, Y_traj), '
                   'offsetof(lmpc_scenario_sim, cost), sizeof(lmpc_sim_cost), offsetof(lmpc_sim_cost, Ax));\nreturn 0; }\n')
    exe = tmp_path / "lay"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(ScenarioSim), ScenarioSim.r.offset, ScenarioSim.noise.offset, ScenarioSim.nuprev.offset,
                   ScenarioSim.Y_traj.offset, ScenarioSim.cost.offset, ctypes.sizeof(SimCost), SimCost.Ax.offset]


def test_a_well_formed_descriptor_passes(lmpc):
    rc, _ = _check(lmpc, _desc(lmpc))
    assert rc == 1
    rc, _ = _check(lmpc, _desc(lmpc, use_observer=1), obs=(2, 1, 1, 1))
    assert rc == 1
    # previews: widths count H columns
    rc, _ = _check(lmpc, _desc(lmpc, r=(1, 5), d=(1, 5), p=(2, 3), nuprev=1), nth=2 + 5 + 5 + 1 + 6)
    assert rc == 1


@pytest.mark.parametrize("field,kwargs,obs", [
    ("nx", dict(nx=33), None),
    ("nx", dict(nx=0), None),
    ("nu", dict(nu=2), None),
    ("nd", dict(nd=33, d=(33, 0)), None),
    ("ny", dict(ny=-1), None),
    ("r.w", dict(r=(-1, 0)), None),
    ("d.w", dict(d=(-2, 0)), None),
    ("p.w", dict(p=(-1, 0)), None),
    ("noise.w", dict(noise=(-1, 0)), None),
    ("r.H", dict(r=(1, -1)), None),
    ("d.H", dict(d=(1, -3)), None),
    ("p.H", dict(p=(1, -1)), None),
    ("d.w", dict(d=(2, 0)), None),                     # disagrees with nd = 1
    ("noise.w", dict(noise=(2, 0)), None),             # disagrees with ny = 1
    ("noise.H", dict(noise=(1, 4)), None),
    ("nuprev", dict(nuprev=2), None),
    ("nuprev", dict(nuprev=-1), None),
    ("use_observer", dict(use_observer=1), None),      # lmpc_set_observer never called
    ("nx", dict(use_observer=1), (3, 1, 1, 1)),
    ("nu", dict(use_observer=1), (2, 2, 1, 1)),
    ("nd", dict(use_observer=1), (2, 1, 0, 1)),
    ("ny", dict(use_observer=1), (2, 1, 1, 2)),
    ("nth", dict(r=(1, 2)), None),                     # 2 + 2 + 1 = 5 != 4
    ("nth", dict(nuprev=1), None),
    ("nth", dict(p=(1, 0)), None),
])
def test_every_refusal_names_its_field(lmpc, field, kwargs, obs):
    rc, msg = _check(lmpc, _desc(lmpc, **kwargs), obs=obs)
    assert rc == -100, (rc, msg)
    assert msg.startswith("lmpc_scenario_check: " + field + ":"), msg


def test_refusals_of_outputs_and_cost(lmpc):
    from linearmpc_jl_amd._cabi import SimCost
    buf = np.zeros(8)
    rc, msg = _check(lmpc, None)
    assert rc == -100 and "s:" in msg
    s = _desc(lmpc); s.plant = None
    rc, msg = _check(lmpc, s)
    assert rc == -100 and msg.startswith("lmpc_scenario_check: plant:")
    s = _desc(lmpc); s.measurement = None
    rc, msg = _check(lmpc, s)
    assert rc == -100 and msg.startswith("lmpc_scenario_check: measurement:")
    s = _desc(lmpc); s.cost_out = buf.ctypes.data
    rc, msg = _check(lmpc, s)
    assert rc == -100 and msg.startswith("lmpc_scenario_check: cost_out:")
    s = _desc(lmpc, ny=0); s.Y_traj = buf.ctypes.data
    rc, msg = _check(lmpc, s)
    assert rc == -100 and msg.startswith("lmpc_scenario_check: Y_traj:")
    s = _desc(lmpc, nd=0, d=(0, 0), p=(1, 0)); s.D_traj = buf.ctypes.data
    rc, msg = _check(lmpc, s)
    assert rc == -100 and msg.startswith("lmpc_scenario_check: D_traj:")
    c = SimCost(2, 0, buf.ctypes.data, buf.ctypes.data, None, None, None, None, None, None, None)
    s = _desc(lmpc); s.cost = ctypes.pointer(c)                     # C has 2 rows, r one
    rc, msg = _check(lmpc, s)
    assert rc == -100 and msg.startswith("lmpc_scenario_check: cost.ny:")
    c = SimCost(1, 2, None, None, None, None, None, buf.ctypes.data, None, None, None)
    s = _desc(lmpc); s.cost = ctypes.pointer(c)
    rc, msg = _check(lmpc, s)
    assert rc == -100 and msg.startswith("lmpc_scenario_check: cost.lb:")


def test_scenario_holds_short_trajectories_at_the_last_column(lmpc):
    r = np.array([[0.0, 0.5, 1.0]])
    sc = lmpc.Scenario([0.0, 0.0], N=6, r=r)
    assert sc.single and sc.n_scen == 1
    assert np.array_equal(sc.trajectory("r"), [[0, 0.5, 1, 1, 1, 1]])              # simulation.jl:71-72
    assert np.array_equal(sc.trajectory("d", 2), np.zeros((2, 6)))                # nothing given: zeros
    long = np.arange(10.0)[None]
    assert np.array_equal(lmpc.Scenario([0.0], N=4, d=long).trajectory("d"), [[0, 1, 2, 3]])
    per = np.arange(2 * 1 * 3, dtype=float).reshape(2, 1, 3)
    sc2 = lmpc.Scenario(np.zeros((2, 2)), N=5, d=per)
    assert not sc2.single and sc2.trajectory("d").shape == (2, 1, 5)
    assert np.array_equal(sc2.trajectory("d")[1, 0], [3, 4, 5, 5, 5])
    with pytest.raises(ValueError):
        lmpc.Scenario(np.zeros((2, 2)), N=5, d=np.zeros((3, 1, 4)))


def test_shapes_map_to_the_right_block(lmpc):
    w, T, S = 2, 7, 3
    shared = np.arange(w * T, dtype=float).reshape(w, T)
    per = np.arange(S * w * T, dtype=float).reshape(S, w, T)
    sc = lmpc.Scenario(np.zeros((S, 2)), N=10, r=shared, d=per)
    b = sc.block_spec("r", H=4)
    assert (b["stride"], b["w"], b["T"], b["H"]) == (0, w, T, 4)
    assert b["data"].shape == (T, w) and np.array_equal(b["data"][3], shared[:, 3])       # column after column
    b = sc.block_spec("d")
    assert (b["stride"], b["w"], b["T"], b["H"]) == (w * T, w, T, 0)
    assert b["data"].shape == (S, T, w) and b["data"].flags.c_contiguous and np.array_equal(b["data"][2, 5], per[2, :, 5])
    b = sc.block_spec("p", H=0, w=3)
    assert b["data"] is None and (b["stride"], b["w"], b["T"]) == (0, 3, 1)
    # a trajectory longer than the run is cut at N columns (the reference's rs / ds have N columns)
    assert lmpc.Scenario(np.zeros(2), N=4, r=shared).block_spec("r")["T"] == 4


def test_preview_follows_the_mpc_flags(lmpc):
    from linearmpc_jl_amd.simulation import scenario_blocks
    g = load_golden("dist_preview_kat")
    q = lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"])
    d = np.hstack([np.zeros((1, 8)), np.ones((1, 12))])
    sc = lmpc.Scenario(np.zeros((5, 2)), N=20, d=d)
    on = lmpc.MPC(q, nx=2, nu=1, nr=1, nd=4, Np=4, disturbance_preview=True)
    sp = scenario_blocks(on, sc)
    assert (sp["d"]["w"], sp["d"]["H"], sp["d"]["stride"]) == (1, 4, 0)
    assert (sp["r"]["w"], sp["r"]["H"]) == (1, 0) and sp["r"]["data"] is None     # no r given: zeros of width ny
    assert sp["p"]["w"] == 0 and sp["noise"]["w"] == 0
    off = lmpc.MPC(q, nx=2, nu=1, nr=1, nd=1, Np=4)
    sp = scenario_blocks(off, sc)
    assert (sp["d"]["w"], sp["d"]["H"]) == (1, 0)
    rp = lmpc.MPC(q, nx=2, nu=1, nr=4, nd=1, Np=4, reference_preview=True)
    sp = scenario_blocks(rp, lmpc.Scenario(np.zeros(2), N=20, r=np.ones((1, 3)), d=d))
    assert (sp["r"]["w"], sp["r"]["H"], sp["r"]["T"]) == (1, 4, 3)
    pp = lmpc.MPC(q, nx=2, nu=1, nr=1, np_=3, Np=3, parameter_preview=True)
    sp = scenario_blocks(pp, lmpc.Scenario(np.zeros((5, 2)), N=20, p=np.ones((5, 1, 9))))
    assert (sp["p"]["w"], sp["p"]["H"], sp["p"]["stride"]) == (1, 3, 9)
    with pytest.raises(ValueError):
        scenario_blocks(on, lmpc.Scenario(np.zeros(2), N=20, d=np.ones((2, 5))))         # two rows, model.nd = 1
    with pytest.raises(ValueError):
        scenario_blocks(lmpc.MPC(q, nx=2, nu=1, nr=1, nd=1, Np=4, reference_preview=True, reference_condensation=True,
                                 traj2setpoint=np.ones((1, 4))), sc)


def test_plant_rows_follow_the_generated_layout(lmpc):
    p = lmpc.Plant([[1, 1], [0, 1.0]], [[0], [1.0]], Gd=[[0.5], [1.0]], f_offset=[0.1, 0.2], C=[[1.0, 0]], Dd=[[0.3]],
                   h_offset=[0.7])
    assert (p.nx, p.nu, p.nd, p.ny) == (2, 1, 1, 1)
    assert np.array_equal(p.dynamics_rows(), [[0.1, 1, 1, 0, 0.5], [0.2, 0, 1, 1, 1.0]])
    assert np.array_equal(p.measurement_rows(), [[0.7, 1, 0, 0.3]])


# ------------------------------------------------------------------ the host reference loop (tests/scenario_reference.py)
# The GPU tests demand bit equality with `reference_run`; here the reference is pinned first, with the LDP of
# oracle.ldp.qp2ldp: the reference project's closed-loop assertions, the older CPU loop, an exact evaluation of the
# glue, and the conditions that keep each GPU case from passing emptily.
EPS = 2.0 ** -53


def _host_run(prob, x0, T, observer=None, **traj):
    import scenario_reference as sr
    dims, previews = sr.dims_of(prob)
    obs = None if observer is None else observer.codegen_arrays()
    return sr.reference_run(sr.host_ldp(prob), dims, sr.plant_of(prob), np.atleast_2d(np.asarray(x0, float)), T,
                            observer=obs, previews=previews, uprev0=getattr(prob, "uprev0", None), **traj)


def test_reference_loop_imports_nothing_of_the_library():
    import ast
    import scenario_reference as sr
    tree = ast.parse(open(sr.__file__).read())
    names = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            names.append(node.module or "")
    assert names and all(n.split(".")[0] in ("dataclasses", "types", "numpy", "oracle") for n in names), names
    assert "import_module" not in open(sr.__file__).read() and "__import__" not in open(sr.__file__).read()


def test_reference_loop_disturbance_preview_assertions():
    # runtests.jl:393-408: the preview changes the controls and lowers the output's norm
    from oracle import mpc2mpqp as omm
    d = np.hstack([np.zeros((1, 8)), np.ones((1, 12))])
    runs = {}
    for preview in (True, False):
        p = omm.make_mpc([[1, 1], [0, 1]], [[0], [1]], [[1.0, 0.0]], Np=5, Nc=5, Q=[10.0], R=[0.1], umin=[-0.5], umax=[0.5],
                         Gd=[[0], [1]])
        p.disturbance_preview = preview
        runs[preview] = _host_run(p, [0.0, 0.0], 20, d=d)
        assert runs[preview].flag_min.min() >= 1
    a, b = runs[True], runs[False]
    assert np.linalg.norm(a.us - b.us) > 1e-2
    assert np.linalg.norm(a.ys) / np.linalg.norm(b.ys) < 0.9
    assert np.array_equal(a.ds[:, 0, 0], d[0])


def test_reference_loop_observer_disturbance_assertion():
    # runtests.jl:951-962 with zero noise: |mean(ys[end-20:end])| < 1e-2
    from oracle import mpc2mpqp as omm
    from oracle import observer as oobs
    p = omm.observer_disturbance_kat()
    kf = oobs.kalman_filter(p.F, p.G, p.C, Gd=p.Gd, Dd=p.Dd, Q=[1.0, 1], R=[1e-2])
    run = _host_run(p, [1.0, 0.0], 100, observer=kf, d=np.ones((2, 1)), r=np.zeros((1, 1)))
    assert run.flag_min.min() >= 1 and abs(np.mean(run.ys[-21:, 0, 0])) < 1e-2


def test_reference_loop_set_offset_assertion():
    # runtests.jl:1320-1327: us[end] = 10.5, ys[end] = 1.5
    from oracle import mpc2mpqp as omm
    run = _host_run(omm.offset_kat(), [0.0], 50, r=np.array([[1.5]]))
    assert run.flag_min.min() >= 1
    assert abs(run.us[-1, 0, 0] - 10.5) < 1e-7 and abs(run.ys[-1, 0, 0] - 1.5) < 1e-7


def test_reference_loop_parameter_closed_form():
    # parameter_preview_kat: Q = 0, every applied control is clip(2 p_k, 0, 2) (runtests.jl:1270-1304)
    from oracle import ldp as oldp
    from oracle import mpc2mpqp as omm
    rng = np.random.default_rng(17)
    S, T = 64, 30
    pt = rng.uniform(-0.5, 1.5, (S, 1, 12))
    run = _host_run(omm.parameter_preview_kat(), rng.uniform(-1, 1, (S, 1)), T, p=pt)
    want = np.clip(2.0 * pt[..., np.minimum(np.arange(T), 11)], 0.0, 2.0)
    assert run.flag_min.min() >= 1
    assert np.abs(run.us[:, :, 0].T - want[:, 0]).max() <= oldp.default_settings().primal_tol


def test_reference_loop_preview_columns_and_hold():
    # theta's blocks, read back: r columns k+1 .. k+H, d and p columns k .. k+H-1, cut at the run, last column held
    import scenario_reference as sr
    case = sr.PREVIEWS[0]
    data = sr.case_data(case)
    ref = sr.run_case(case, sr.host_ldp(data.prob), data)
    nx, nu, ny, nd, H, T = case.nx, case.nu, case.ny, case.nd, case.Np, case.T
    col = lambda a, j: (a if a.ndim == 3 else a[None])[..., min(j, a.shape[-1] - 1, T - 1)]
    for k in (0, 3, T - 1):
        th = ref.thetas[k]
        for i in range(H):
            assert np.array_equal(th[:, nx + i * ny:nx + (i + 1) * ny], np.broadcast_to(col(data.r, k + 1 + i), (case.S, ny)))
            o = nx + H * ny
            assert np.array_equal(th[:, o + i * nd:o + (i + 1) * nd], np.broadcast_to(col(data.d, k + i), (case.S, nd)))
            o = nx + H * (ny + nd) + nu
            assert np.array_equal(th[:, o + i:o + i + 1], np.broadcast_to(col(data.p, k + i), (case.S, 1)))
        if k:
            assert np.array_equal(th[:, nx + H * (ny + nd):nx + H * (ny + nd) + nu], ref.us[k - 1])


def test_reference_loop_agrees_with_the_older_cpu_loop():
    """No d, offsets, observer or preview: the loop is oracle.ldp.simulate's, whose plant step fuses its multiply-adds,
    so the two agree to rounding only.  The bound is derived, not tuned.  Bounds wide enough that no row is ever
    active (asserted), so that u = x0 + Xth theta exactly and the error recursion is linear:
        a row sum of K terms evaluated twice differs by at most 2 * 4 K eps sum|terms|      (K = the row's length)
        |du_k|     <= |Xth_x| e_k + |Xth_u| |du_{k-1}| + 8 (nth + 1) eps (|x0| + |Xth| |theta_k|)
        e_{k+1}    <= |F| e_k + |G| |du_k| + 8 (nx + nu) eps (|F| |x_k| + |G| |u_k|),     e_0 = 0."""
    import scenario_reference as sr
    from oracle import ldp as oldp
    prob, _ = sr.chain_problem(4, 2, 2, 0, seed=5, ubound=1e3)
    prob.f_offset, prob.h_offset = np.zeros(4), np.zeros(2)
    L = sr.host_ldp(prob)
    rng = np.random.default_rng(3)
    S, T = 50, 25
    x0 = rng.uniform(-1, 1, (S, 4))
    r = rng.uniform(-0.5, 0.5, (S, 2))
    dims, previews = sr.dims_of(prob)
    assert dims == (4, 2, 2, 0, 2, 0) and previews == (0, 0, 0)
    ref = sr.reference_run(L, dims, sr.plant_of(prob), x0, T, r=r[:, :, None])
    old = oldp.simulate(L, x0, T, prob.F, prob.G, r=r, warm=False)
    assert ref.active_sizes.max() == 0 and ref.flag_min.min() >= 1 and old["flag_min"].min() >= 1
    aF, aG, aX = np.abs(prob.F), np.abs(prob.G), np.abs(L.Xth)
    e, du = np.zeros((S, 4)), np.zeros((S, 2))
    worst = 0.0
    for k in range(T):
        assert np.all(np.abs(ref.xs[k] - old["X"][k]) <= e), k
        du = e @ aX[:, :4].T + du @ aX[:, 6:8].T + 8 * (L.nth + 1) * EPS * (np.abs(L.x0) + np.abs(ref.thetas[k]) @ aX.T)
        assert np.all(np.abs(ref.us[k] - old["U"][k]) <= du), k
        e = e @ aF.T + du @ aG.T + 8 * (4 + 2) * EPS * (np.abs(ref.xs[k]) @ aF.T + np.abs(ref.us[k]) @ aG.T)
        worst = max(worst, float((np.abs(ref.xs[k + 1] - old["X"][k + 1]) / e).max()))
    assert np.all(np.abs(ref.xs[T] - old["X"][T]) <= e)
    print("largest |x - x_old| / bound =", worst)


def test_reference_glue_step_against_exact_arithmetic():
    """Measurement, correct, predict and plant step at nx = 7, ny = 3, nd = 2, nu = 2 evaluated exactly
    (fractions.Fraction on the binary64 inputs) against the float64 step, within 4 K eps sum|terms| with K the
    number of terms of the row; correct's second stage adds the first stage's bound through |K'|."""
    from fractions import Fraction as Fr
    import scenario_reference as sr
    nx, ny, nd, nu, S = 7, 3, 2, 2, 5
    prob, kf = sr.chain_problem(nx, nu, ny, nd, seed=9)
    pl = sr.plant_of(prob)
    rng = np.random.default_rng(4)
    x, xh = rng.uniform(-2, 2, (S, nx)), rng.uniform(-2, 2, (S, nx))
    u, dk, v = rng.uniform(-0.3, 0.3, (S, nu)), rng.uniform(-0.3, 0.3, (S, nd)), 0.01 * rng.standard_normal((S, ny))
    meas = np.hstack([pl.h_offset[:, None], pl.C, pl.Dd])
    dyn = np.hstack([pl.f_offset[:, None], pl.F, pl.G, pl.Gd])
    odyn, omeas, okt = kf.codegen_arrays()
    omeas, okt = omeas.reshape(ny, -1), okt.reshape(ny, nx)
    ym, y0 = sr.measure(meas, x, dk, v)
    xc = sr.correct(omeas, okt, xh, ym, dk)
    xp = sr.predict(dyn, x, u, dk)
    assert np.array_equal(sr.predict(odyn.reshape(nx, -1), x, u, dk), xp)      # observer model = plant here
    F_ = lambda a: [Fr(float(t)) for t in a]
    worst = 0.0

    def close(got, terms):
        nonlocal worst
        exact = sum(terms, Fr(0))
        bound = 4 * len(terms) * EPS * float(sum(abs(t) for t in terms))
        err = abs(Fr(float(got)) - exact)
        worst = max(worst, float(err) / bound)
        assert err <= Fr(bound), (float(err), bound)
        return bound

    for s in range(S):
        xs_, xh_, u_, d_, v_ = F_(x[s]), F_(xh[s]), F_(u[s]), F_(dk[s]), F_(v[s])
        inno, inno_b = [], []
        for j in range(ny):
            row = F_(meas[j])
            terms = [row[0]] + [row[1 + c] * xs_[c] for c in range(nx)] + [row[1 + nx + q] * d_[q] for q in range(nd)]
            close(ym[s, j], terms + [v_[j]])
            close(y0[s, j], terms[1:])
            orow = F_(omeas[j])
            it = [Fr(float(ym[s, j])), -orow[0]] + [-orow[1 + c] * xh_[c] for c in range(nx)] + \
                 [-orow[1 + nx + q] * d_[q] for q in range(nd)]
            inno.append(sum(it, Fr(0)))
            inno_b.append(4 * len(it) * EPS * float(sum(abs(t) for t in it)))
        for c in range(nx):
            kt = F_(okt[:, c])
            terms = [xh_[c]] + [kt[j] * inno[j] for j in range(ny)]
            exact = sum(terms, Fr(0))
            bound = 4 * len(terms) * EPS * float(sum(abs(t) for t in terms)) + sum(abs(float(kt[j])) * inno_b[j] for j in range(ny))
            err = abs(Fr(float(xc[s, c])) - exact)
            worst = max(worst, float(err) / bound)
            assert err <= Fr(bound), (float(err), bound)
        for a in range(nx):
            row = F_(dyn[a])
            close(xp[s, a], [row[0]] + [row[1 + c] * xs_[c] for c in range(nx)] + [row[1 + nx + l] * u_[l] for l in range(nu)] +
                  [row[1 + nx + nu + q] * d_[q] for q in range(nd)])
    # the vectorised steps are the scalar loops of oracle/observer.py, bit for bit
    from oracle import observer as oobs
    for s in range(S):
        assert np.array_equal(oobs.c_predict(dyn.reshape(-1), x[s], u[s], dk[s], nx, nu, nd), xp[s])
        assert np.array_equal(oobs.c_correct(omeas.reshape(-1), okt.reshape(-1), xh[s], ym[s], dk[s], nx, ny, nd), xc[s])
    print("largest error / bound =", worst)


def test_reference_cost_and_violation_against_exact_arithmetic():
    # the pinned values of runtests.jl:1591-1599 and an exact evaluation of one scenario's cost
    from fractions import Fraction as Fr
    import scenario_reference as sr
    one = dict(C=np.array([[1.0]]), Q=np.array([[2.0]]), R=np.array([[3.0]]), Rr=np.array([[4.0]]), S=np.array([[5.0]]))
    c = sr.stored_cost(one, np.array([[[1.0]], [[2.0]]]), np.array([[[0.0]], [[1.0]]]), np.array([[[0.0, 1.0]]]))
    assert c[0] == 10.5
    rows = dict(Ax=np.array([[1.0, 0.0]]), Au=np.array([[1.0]]), lb=np.array([-1.0]), ub=np.array([1.0]))
    steps, worst = sr.stored_violation(rows, np.array([[[0.8, 0.0]], [[0.2, 0.0]]]), np.array([[[0.5]], [[0.0]]]))
    assert steps[:, 0] == pytest.approx([0.3, 0.0]) and worst[0] == steps[0, 0]
    case = sr.COST
    data = sr.case_data(case)
    ref = sr.run_case(case, sr.host_ldp(data.prob), data)
    assert np.array_equal(sr.stored_cost(data.cost, ref.xs, ref.us, sr.run_trajectory(data.r, case.S, case.T)), ref.cost)
    steps, worst = sr.stored_violation(data.cost, ref.xs, ref.us)
    assert np.array_equal(steps, ref.violation_steps) and np.array_equal(worst, ref.violation)
    M = lambda a: [[Fr(float(v)) for v in row] for row in np.atleast_2d(a)]
    k = data.cost
    C, Q, R, Rr, Sx = M(k["C"]), M(k["Q"]), M(k["R"]), M(k["Rr"]), M(k["S"])
    nx, nu, ny = case.nx, case.nu, case.ny
    rs = sr.run_trajectory(data.r, case.S, case.T)
    for s in (0, 7):
        tot, absum, ul = Fr(0), 0.0, [Fr(0)] * nu
        for t in range(case.T):
            x, u = [Fr(float(v)) for v in ref.xs[t, s]], [Fr(float(v)) for v in ref.us[t, s]]
            e = [sum(C[j][a] * x[a] for a in range(nx)) - Fr(float(rs[s, j, t])) for j in range(ny)]
            du = [u[l] - ul[l] for l in range(nu)]
            for A_, a_, b_ in ((Q, e, e), (R, u, u), (Rr, du, du), (Sx, x, u)):
                tot += sum(a_[j] * A_[j][l] * b_[l] for j in range(len(a_)) for l in range(len(b_)))
            ae = [float(sum(abs(C[j][a] * x[a]) for a in range(nx)) + abs(rs[s, j, t])) for j in range(ny)]
            f = lambda v: [abs(float(t_)) for t_ in v]
            adu = [abs(float(u[l])) + abs(float(ul[l])) for l in range(nu)]
            for A_, a_, b_ in ((Q, ae, ae), (R, f(u), f(u)), (Rr, adu, adu), (Sx, f(x), f(u))):
                absum += sum(a_[j] * abs(float(A_[j][l])) * b_[l] for j in range(len(a_)) for l in range(len(b_)))
            ul = u
        K = case.T * (ny * nx + ny + 2 * ny * ny + 6 * nu * nu + nu + 2 * nx * nu + 8)      # multiply-adds of one scenario
        bound = 4 * K * EPS * 0.5 * absum
        assert abs(Fr(float(ref.cost[s])) - tot / 2) <= Fr(bound), (float(abs(Fr(float(ref.cost[s])) - tot / 2)), bound)


def _case_ids():
    import scenario_reference as sr
    return [c.name for c in sr.CASES]


@pytest.mark.parametrize("name", _case_ids())
def test_gpu_cases_do_not_pass_emptily(name):
    # the conditions of every case the GPU tests run, from the reference alone (host LDP)
    import scenario_reference as sr
    case = {c.name: c for c in sr.CASES}[name]
    data = sr.case_data(case)
    ref = sr.run_case(case, sr.host_ldp(data.prob), data)
    sr.check_conditions(case, ref)
    assert ref.xs.shape == (case.T + 1, case.S, case.nx) and np.isfinite(ref.xs).all()


def test_gpu_case_list_covers_what_it_must():
    import scenario_reference as sr
    assert {c.nx for c in sr.SWEEP} == {1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 32}
    assert {(c.observer, c.warm) for c in sr.SWEEP if c.nx == 32} == {(a, b) for a in (False, True) for b in (False, True)}
    assert all(c.nu == 2 and c.ny == 3 and c.nd == 2 and c.noise and c.S == 300 for c in sr.SWEEP)
    assert {(c.nx, c.S, c.T) for c in sr.SIZES} == {(nx, S, T) for nx in (5, 12) for S in (1, 255, 256, 257, 1000) for T in (1, 2)}
    nth = [sr.host_ldp(sr.case_data(c).prob).nth for c in sr.PREVIEWS]
    assert 16 < nth[0] <= 32 < nth[1] and nth[1] >= 60
    assert sr.host_ldp(sr.case_data(sr.SWEEP[-1]).prob).nth >= 34
    assert [c.S for c in sr.RERUN] == [200, 2000, 50] and all(c.cost for c in sr.RERUN)
    assert (sr.SCORING[0].nx, sr.SCORING[0].nu, sr.SCORING[1].nx) == (32, 8, 3)
    assert sr.COST.nu == 3 and sr.COST.ny == 2 and sr.COST.observer and sr.COST.soft
