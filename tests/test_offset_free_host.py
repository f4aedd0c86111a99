"""Host side of the offset-free scenario loop (no GPU): the reference's own closed-loop assertions on the host
reference loop (tests/offset_free_reference.py), the d block of theta against a transcription of the reference's two
formatting functions, `lmpc.offset_free_observer` against the reference builder, the refusals of
lmpc_scenario_offset_free_check, and the conditions that keep the GPU cases from passing emptily."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


# ------------------------------------------------------------------ the reference's tests
def _double_integrator(Gd=None):
    from oracle import mpc2mpqp as omm
    return omm.make_mpc([[1, 0.1], [0, 1]], [[0.005], [0.1]], [[1.0, 0.0]], Np=20, Q=[1.0], R=[0.0], Rr=[0.1], umin=[-1.0],
                        umax=[1.0], Gd=Gd)


def test_reference_offset_free_observer_closed_loop():
    # runtests.jl:989-1011: the plant carries f_offset = [0.01, 0] the model does not know; r = 0.5, 100 steps from 0
    import offset_free_reference as ofr
    import scenario_reference as sr
    nominal = _double_integrator()
    true = sr.plant_of(nominal)
    true.f_offset = np.array([0.01, 0.0])
    x0, r = np.zeros((1, 2)), np.array([[0.5]])
    dims, previews = sr.dims_of(nominal)
    run = sr.reference_run(sr.host_ldp(nominal), dims, true, x0, 100, r=r, previews=previews)
    assert abs(run.xs[99, 0, 0] - 0.5) > 5e-2                          # sim_nominal.xs[1, end]

    obs = ofr.build_observer(nominal.F, nominal.G, nominal.C, method="velocity", Q=[1e-3, 1e-3], R=[1e-4])
    assert obs.method == "velocity" and obs.nd_offsetfree == 1 and obs.nd_measured == 0
    tracked = _double_integrator(Gd=obs.Bd)
    tracked.Dd = obs.Cd
    assert tracked.Gd.shape == (2, 1) and tracked.Dd.shape == (1, 1)  # size(tracked.model.Gd) == (2, 1)
    run = ofr.reference_run(sr.host_ldp(tracked), (2, 1, 1, 0, 1, 0), true, obs, x0, 100, r=r)
    assert run.dhats.shape == (100, 1, 1)                              # length(get_estimated_disturbance) == 1
    assert abs(run.xs[99, 0, 0] - 0.5) < 1e-3                          # sim_tracked.xs[1, end]
    assert run.flags.min() >= 1 and np.abs(run.dhats).max() > 0


def test_vector_and_matrix_disturbance_give_different_controls():
    # runtests.jl:566-602: one measured and one estimated disturbance under disturbance_preview; a constant d = 0.5
    # (the vector form, repeated over the horizon) against a zero preview matrix
    import offset_free_reference as ofr
    import scenario_reference as sr
    from oracle import ldp as oldp
    from oracle import mpc2mpqp as omm
    F, G, Gd, C = [[1.0, 1.0], [0.0, 1.0]], [[0.0], [1.0]], [[1.0], [0.0]], [[1.0, 0.0]]
    obs = ofr.build_observer(F, G, C, Gd=Gd, method="state_disturbance", Q=[1e-3, 1e-3], R=[1e-4])
    assert obs.nd_measured == 1 and obs.nd_offsetfree == 1
    p = omm.make_mpc(F, G, C, Np=4, Nc=4, Q=[1.0], R=[0.1], umin=[-0.5], umax=[0.5], Gd=np.hstack([np.array(Gd), obs.Bd]),
                     Dd=np.hstack([np.zeros((1, 1)), obs.Cd]))
    p.disturbance_preview = True
    assert p.nd == 2                                                    # mpc.model.nd == 2
    ldp = sr.host_ldp(p)
    x, dhat = np.zeros((1, 2)), np.zeros((1, 1))
    us = []
    for d in (np.full((1, 1, 1), 0.5), np.zeros((1, 1, 4))):
        theta = np.concatenate([x, np.zeros((1, 1)), ofr.d_block(d, dhat, 1, 4, 0)], axis=1)
        assert theta.shape[1] == ldp.nth
        us.append(oldp.solve_batch(ldp, theta)[0])
    assert us[0].shape == (1, 1) and np.linalg.norm(us[0] - us[1]) > 1e-6


# ------------------------------------------------------------------ the d block
def _format_disturbance(d, dhat, ndm, nd_base, preview, Np):
    """get_control_disturbance (observer.jl:203-222) then format_disturbance (utils.jl:155-205) for ONE scenario,
    branch for branch; d: None, a vector or an (ndm, cols) matrix"""
    if d is None:
        d = np.concatenate([np.zeros(ndm), dhat])
    elif d.size == ndm and d.ndim == 1:
        d = np.concatenate([d, dhat])
    elif d.ndim == 2 and d.shape[0] == ndm:
        d = d if dhat.size == 0 else np.vstack([d, np.tile(dhat[:, None], (1, d.shape[1]))])
    if nd_base == 0:
        return np.zeros(0)
    if preview:
        if d.ndim == 1:
            assert d.size == nd_base
            return np.tile(d[:, None], (1, Np)).T.reshape(-1)
        assert d.shape[0] == nd_base
        if d.shape[1] >= Np:
            return d[:, :Np].T.reshape(-1)
        ext = np.zeros((nd_base, Np))
        ext[:, :d.shape[1]] = d
        ext[:, d.shape[1]:] = d[:, -1:]
        return ext.T.reshape(-1)
    if d.ndim == 1:
        assert d.size == nd_base
        return d
    return d[:, 0]


def _get_preview(ds, k, Np):
    """simulation.jl:128-134 with a 0-based step k: get_preview(ds, k - 1, Np) of the 1-based loop"""
    return np.stack([ds[:, min(k + i, ds.shape[1] - 1)] for i in range(Np)], axis=1)


@pytest.mark.parametrize("ndm,ndo,preview,have_d", [
    (2, 3, False, True), (2, 3, True, True), (2, 1, False, False), (2, 1, True, False), (0, 2, True, False),
    (0, 2, False, False), (1, 1, True, True)])
def test_d_block_follows_the_reference_formatting(ndm, ndo, preview, have_d):
    import offset_free_reference as ofr
    import scenario_reference as sr
    rng = np.random.default_rng(5)
    S, T, Np = 4, 7, 5
    dhat = rng.standard_normal((S, ndo))
    d = rng.standard_normal((S, ndm, 4)) if have_d else None          # shorter than the run: held at the last column
    dt = None if d is None else sr.run_trajectory(d, S, T)
    for k in range(T):
        got = ofr.d_block(dt, dhat, ndm, Np if preview else 0, k)
        for s in range(S):
            if dt is None:                                             # simulation.jl:60,81: ds zeros, no preview of them
                dk = np.zeros(ndm)
            else:                                                      # :103
                dk = _get_preview(dt[s], k, Np) if preview else dt[s][:, k]
            want = _format_disturbance(dk, dhat[s], ndm, ndm + ndo, preview, Np)
            assert np.array_equal(got[s], want), (k, s)
    assert got.shape[1] == (ndm + ndo) * (Np if preview else 1)


# ------------------------------------------------------------------ lmpc.offset_free_observer
def _package_observer(lmpc, case, data):
    import offset_free_reference as ofr
    b, o = data.base, data.obs
    gains = dict(K=o.Bd) if ofr.METHODS[case.method] in ("velocity", "state_disturbance") else dict(Kaug=o.K)
    return lmpc.offset_free_observer(b.F, b.G, b.C, Gd=data.plant.Gd, Dd=data.plant.Dd, f_offset=b.f_offset,
                                     h_offset=b.h_offset, method=case.method, **gains)


@pytest.mark.parametrize("name", ["t-nx3-vel", "t-nx5-out-gate8", "t-nx6-vel-preview-ndm0-gate8", "t-nx1-vel"])
def test_package_observer_equals_the_reference_builder(lmpc, name):
    import offset_free_reference as ofr
    case = next(c for c in ofr.CASES if c.name == name)
    data = ofr.case_data(case)
    obs = _package_observer(lmpc, case, data)
    for got, want in zip(obs.codegen_arrays(), data.obs.codegen_arrays()):
        assert np.array_equal(got, want)
    assert (obs.nx, obs.nd_measured, obs.nd_offsetfree) == (case.nx, case.ndm, case.ndo)
    assert np.array_equal(obs.Bd, data.obs.Bd) and np.array_equal(obs.Cd, data.obs.Cd)
    assert obs.formulation == ofr.METHODS[case.method]


def test_package_observer_methods_and_refusals(lmpc):
    F, G, C = np.array([[1.0, 0.1], [0.0, 1.0]]), np.array([[0.005], [0.1]]), np.array([[1.0, 0.0]])
    K = np.array([[0.5], [0.2]])
    a = lmpc.offset_free_observer(F, G, C, method="state", K=K)
    b = lmpc.offset_free_observer(F, G, C, method="velocity", K=K)
    assert a.formulation == "state_disturbance" and b.formulation == "velocity"
    assert all(np.array_equal(x, y) for x, y in zip(a.codegen_arrays(), b.codegen_arrays()))
    assert np.array_equal(a.K, np.vstack([K, np.eye(1)])) and np.array_equal(a.Cd, np.eye(1) - C @ K)
    Fs = np.array([[0.9, 0.1], [0.0, 0.8]])                          # (an integrator has no output-disturbance model: rank)
    o = lmpc.offset_free_observer(Fs, G, C, method="output", Kx=K, Kd=[[0.3]])
    assert o.formulation == "output_disturbance" and np.array_equal(o.Bd, np.zeros((2, 1))) and np.array_equal(o.Cd, np.eye(1))
    g = lmpc.offset_free_observer(F, G, C, method="general", Bd=[[0.0], [1.0]], Cd=[[0.0]], Kaug=[[0.5], [0.2], [0.1]])
    assert g.nd_offsetfree == 1 and g.F.shape == (3, 3) and np.array_equal(g.F[:2, 2], [0.0, 1.0])
    with pytest.raises(ValueError, match="Unknown offset-free method"):
        lmpc.offset_free_observer(F, G, C, method="kalman", K=K)
    with pytest.raises(ValueError, match="needs the nominal observer gain K"):
        lmpc.offset_free_observer(F, G, C, method="velocity")
    with pytest.raises(ValueError, match="requires Bd"):
        lmpc.offset_free_observer(F, G, C, method="general", Cd=[[1.0]], Kaug=np.zeros((3, 1)))
    with pytest.raises(ValueError, match="Kx / Kd or Kaug"):
        lmpc.offset_free_observer(Fs, G, C, method="output")
    with pytest.raises(ValueError, match=r"rank\(\[F-I Bd; C Cd\]\)"):
        lmpc.offset_free_observer(F, G, C, method="output", Kx=K, Kd=[[0.3]])
    # setup.jl:382-390: an integrating plant with an input disturbance that the output cannot tell from the state
    with pytest.raises(ValueError, match=r"rank\(\[F-I Bd; C Cd\]\)"):
        lmpc.offset_free_observer(F, G, C, method="general", Bd=[[1.0, 0.0], [0.0, 1.0]], Cd=[[0.0, 0.0]], Kaug=np.zeros((4, 1)))
    import offset_free_reference as ofr
    with pytest.raises(ValueError, match="rank"):
        ofr.build_observer(F, G, C, method="general", Bd=[[1.0, 0.0], [0.0, 1.0]], Cd=[[0.0, 0.0]], Kx=np.zeros((2, 1)))


# ------------------------------------------------------------------ the refusals of the C check
def _desc(lmpc, nx=2, nu=1, nd=1, ny=1, r=(1, 0), d=(1, 0), p=(0, 0), noise=(0, 0), nuprev=0, use_observer=1):
    """A well-formed descriptor for a handle with nth = 2 + 1 + (1 + 1) = 5, nout = 1 and n_offset_free = 1"""
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


def _check(lmpc, s, ndo=1, nth=5, nout=1, obs=(3, 1, 1, 1), of="given"):
    from linearmpc_jl_amd._cabi import Observer, OffsetFree, last_error
    o = None if obs is None else ctypes.byref(Observer(*obs, None, None, None))
    f = None if of is None else ctypes.byref(OffsetFree(ndo, None))
    rc = lmpc.lib().lmpc_scenario_offset_free_check(nth, nout, o, ctypes.byref(s) if s is not None else None, f)
    return rc, last_error(None)


def test_symbols_are_exported_and_bound(lmpc):
    L = lmpc.lib()
    for name in ("lmpc_scenario_offset_free_check", "lmpc_simulate_scenario_offset_free_device",
                 "lmpc_simulate_scenario_offset_free"):
        assert name in lmpc.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.lmpc_abi_version() == 2
    assert hasattr(lmpc, "offset_free_observer") and "offset_free_observer" in lmpc.__all__
    assert hasattr(lmpc.BatchedQP, "simulate_scenario_offset_free")


def test_well_formed_descriptors_pass(lmpc):
    assert _check(lmpc, _desc(lmpc))[0] == 1
    # preview: 3 columns [d; dhat]; with and without a measured trajectory (d.w == 0), and with ndm == 0
    assert _check(lmpc, _desc(lmpc, d=(1, 3)), nth=2 + 1 + 2 * 3)[0] == 1
    assert _check(lmpc, _desc(lmpc, d=(0, 3)), nth=2 + 1 + 2 * 3)[0] == 1
    assert _check(lmpc, _desc(lmpc, nd=0, d=(0, 3)), ndo=2, nth=2 + 1 + 2 * 3, obs=(4, 1, 0, 1))[0] == 1
    assert _check(lmpc, _desc(lmpc, nx=29, d=(1, 0)), ndo=3, nth=29 + 1 + 4, obs=(32, 1, 1, 1))[0] == 1   # na = 32


@pytest.mark.parametrize("field,kwargs,extra", [
    ("of", {}, dict(of=None)),
    ("n_offset_free", {}, dict(ndo=0)),
    ("n_offset_free", {}, dict(ndo=-1)),
    ("n_offset_free", dict(nx=30), dict(ndo=3, nth=30 + 1 + 4, obs=(33, 1, 1, 1))),      # na = 33
    ("use_observer", dict(use_observer=0), {}),
    ("use_observer", {}, dict(obs=None)),                           # lmpc_set_observer never called
    ("n_offset_free", {}, dict(obs=(2, 1, 1, 1))),                  # the plain filter's n_state = nx
    ("n_offset_free", {}, dict(obs=(4, 1, 1, 1))),
    ("nu", {}, dict(obs=(3, 2, 1, 1))),
    ("nd", {}, dict(obs=(3, 1, 2, 1))),                             # the observer counts the estimated channel as measured
    ("ny", {}, dict(obs=(3, 1, 1, 2))),
    ("d.w", dict(d=(2, 0)), {}),                                    # the controller's width instead of the measured one
    ("nth", {}, dict(nth=4)),                                       # the plain loop's sum
    ("nth", dict(d=(1, 3)), dict(nth=2 + 1 + 3 + 1)),               # dhat in the first column only
    ("nth", dict(nuprev=1), {}),
    # everything lmpc_scenario_check refuses, through the same code
    ("nx", dict(nx=0), {}),
    ("nu", dict(nu=2), {}),
    ("nd", dict(nd=33, d=(33, 0)), {}),
    ("r.w", dict(r=(-1, 0)), {}),
    ("d.H", dict(d=(1, -3)), {}),
    ("noise.w", dict(noise=(2, 0)), {}),
    ("noise.H", dict(noise=(1, 4)), {}),
    ("nuprev", dict(nuprev=2), {}),
    ("ny", dict(ny=0, noise=(0, 0)), dict(obs=(3, 1, 1, 0))),
])
def test_every_refusal_names_its_field(lmpc, field, kwargs, extra):
    rc, msg = _check(lmpc, _desc(lmpc, **kwargs), **extra)
    assert rc == -100, (rc, msg)
    assert msg.startswith("lmpc_scenario_offset_free_check: " + field + ":"), msg


def test_refusal_texts(lmpc):
    msg = _check(lmpc, _desc(lmpc), nth=4)[1]
    assert "nx + width(r) + (nd + n_offset_free) * max(d.H, 1) + nuprev + width(p) = 5 must equal the handle's nth = 4" in msg
    msg = _check(lmpc, _desc(lmpc, nx=30), ndo=3, nth=35, obs=(33, 1, 1, 1))[1]
    assert "nx + n_offset_free <= 32, got 30 + 3" in msg
    msg = _check(lmpc, _desc(lmpc), obs=(2, 1, 1, 1))[1]
    assert "n_state = 2, the descriptor says nx + n_offset_free = 3" in msg
    assert _check(lmpc, None)[1].startswith("lmpc_scenario_offset_free_check: s:")
    # the plain check keeps its own texts: the same descriptor there asks for the plain sum and the plain n_state
    from linearmpc_jl_amd._cabi import Observer, last_error
    rc = lmpc.lib().lmpc_scenario_check(5, 1, ctypes.byref(Observer(3, 1, 1, 1, None, None, None)), ctypes.byref(_desc(lmpc)))
    assert rc == -100 and last_error(None).startswith("lmpc_scenario_check: nx: the observer was set with n_state = 3")


def test_offset_free_struct_layout_matches_the_header(lmpc, tmp_path):
    import os, shutil, subprocess
    from conftest import ROOT
    from linearmpc_jl_amd._cabi import OffsetFree
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lmpc_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu\\n", sizeof(lmpc_offset_free), offsetof(lmpc_offset_free, Dhat_traj));\nreturn 0; }\n')
    exe = tmp_path / "lay"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(OffsetFree), OffsetFree.Dhat_traj.offset]


# ------------------------------------------------------------------ the reference module and the cases
def test_reference_loop_imports_nothing_of_the_library():
    import ast
    import offset_free_reference as ofr
    tree = ast.parse(open(ofr.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names <= {"copy", "dataclasses", "types", "numpy", "oracle", "scenario_reference"}, names


def test_cases_cover_every_instantiation_and_the_gate():
    import offset_free_reference as ofr
    pairs = {(c.nx, c.ndo) for c in ofr.PAIRS}
    assert pairs == {(a, b) for a in range(1, 8) for b in range(1, 8) if a + b <= 8} and len(ofr.PAIRS) == 28
    na = {c.nx + c.ndo for c in ofr.CASES}
    assert {8, 9, 32} <= na and max(na) == 32
    assert {c.ndm for c in ofr.PAIRS} == {0, 1, 2} and {c.method for c in ofr.PAIRS} == {"velocity", "output"}
    assert any(c.preview and c.ndm == 0 for c in ofr.CASES) and any(c.preview and c.ndm > 0 for c in ofr.CASES)
    assert any(c.warm for c in ofr.PAIRS) and any(not c.warm for c in ofr.PAIRS)


def _all_cases():
    import offset_free_reference as ofr
    return [pytest.param(c, id=c.name) for c in ofr.CASES]


@pytest.mark.parametrize("case", _all_cases())
def test_case_conditions_on_the_host_reference(case):
    # every case the GPU tests run, on the CPU first: both solver outcomes on 5 % .. 95 % of the scenario-steps, every
    # flag >= 1, a disturbance estimate that moved, an estimate that is not the state
    import offset_free_reference as ofr
    import scenario_reference as sr
    data = ofr.case_data(case)
    ref = ofr.run_case(case, sr.host_ldp(data.prob), data)
    ofr.check_conditions(case, ref)
    nth = case.nx + case.ny + (case.ndm + case.ndo) * (case.Np if case.preview else 1) + case.nu
    assert ref.thetas.shape == (case.T, case.S, nth) and ref.dhats.shape == (case.T, case.S, case.ndo)
    if case.xaug:
        assert not np.array_equal(data.xaug0[:, case.nx:], np.zeros((case.S, case.ndo)))
