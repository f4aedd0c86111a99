"""The older loop and observer entry points on the GPU, bit for bit against tests/loop_reference.py (numpy, glibc's
fma and the CPU oracle on the handle's own pack; no call into the library): lmpc_predict_state / lmpc_correct_state at
every state-size instantiation, lmpc_simulate_ref_device, lmpc_simulate in every execution mode of the lane and the
wavefront path and at the gates between them, lmpc_simulate_f32, the NULL-able outputs of the C ABI, the generated
controller's parameter formation, and the state a loop leaves on its handle.  Every comparison is np.array_equal.

Left out: the error-return paths of the loops.  They are reached only when a HIP call fails inside a loop, and no test
provokes that; a loop's state lives on its own stack (LoopMode), so they leave nothing on the handle either."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT, oracle_ldp_from

pytestmark = pytest.mark.gpu

KEYS = ("U", "X", "x", "uprev", "flag_min")
LANE_MODES = ({}, {"sim_small": 0}, {"sim_blind": 0}, {"sim_blind": 5}, {"sim_async": 0}, {"sim_async": 0, "sim_fused": 0})
WAVE_MODES = [{"sim_keep_factor": k, "sim_fused": f, "sim_async": a} for k in (0, 1) for f in (0, 1) for a in (0, 2)]
SIZES = (1, 255, 256, 257, 1000)


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


def _ids(cases):
    return [pytest.param(c, id=c.name) for c in cases]


def _handle(lmpc, data, opts=None, settings=None, wave=False):
    qp = lmpc.BatchedQP.from_mpqp(*data.qp, nout=data.nout, settings=settings)
    if wave:
        qp.set_option("wave", 1)
        assert qp.kernel_name.endswith("wave")
    for k, v in (opts or {}).items():
        qp.set_option(k, v)
    return qp


def _same(got, want, what, keys=KEYS):
    for key in keys:
        if want[key] is None or (key == "uprev" and want[key].size == 0):
            assert got[key] is None or got[key].size == 0, (what, key)
            continue
        if not np.array_equal(got[key], want[key]):
            bad = np.argwhere(got[key] != want[key])
            raise AssertionError(f"{what}: {key} differs at {len(bad)} entries, first {bad[0]}, "
                                 f"max |diff| = {np.abs(got[key].astype(float) - want[key].astype(float)).max():.3e}")


def _solve_dev(qp, theta):
    """solve_device with every output: (x, exitflag, iterations, active) as numpy arrays"""
    import torch
    dev = torch.device("cuda", qp.device)
    th = torch.from_numpy(np.ascontiguousarray(theta)).to(dev)
    it = torch.empty(len(theta), dtype=torch.int32, device=dev)
    act = torch.zeros((len(theta), qp.words), dtype=torch.int64, device=dev)
    x, ef = qp.solve_device(th, iters=it, active=act)
    torch.cuda.synchronize(dev)
    qp.check()
    return tuple(a.cpu().numpy() for a in (x, ef, it, act))


def _probe_theta(case, data, n=300):
    """a batch for the plain solve after a loop: other problems than the loop's, another size than the loop's"""
    rng = np.random.default_rng(900 + case.seed)
    return rng.uniform(-case.x0, case.x0, (n, case.nx + data.nr + data.nup))


def _assert_plain_solve_as_fresh(qp, fresh, theta, what):
    for a, b, name in zip(_solve_dev(qp, theta), fresh, ("x", "exitflag", "iterations", "active")):
        assert np.array_equal(a, b), (what, "plain solve after the loop", name)


# ------------------------------------------------------------------ observer entry points
@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("nd", [0, 2])
@pytest.mark.parametrize("nx", [1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 32])
def test_observer_entry_points_equal_the_host_reference(lmpc, nx, nd, path):
    # predict_state_kernel<NXT> / correct_state_kernel<NXT>: NXT = 1 .. 8 unrolled, 9 / 17 / 32 the run-time form;
    # ny = 1, 3 and ny > nx; one lane, a workgroup less one, exactly one, one more, a ragged fourth; the disturbance
    # given and NULL; device tensors in place, and host arrays through the staging wrappers
    import torch
    import loop_reference as lr
    nu = 2
    data = lr.loop_data(lr.LAYOUT[0])
    qp = _handle(lmpc, data)
    dev = torch.device("cuda", qp.device)
    for ny in (1, 3, nx + 2):
        dyn, meas, kt, x, u, y, d = lr.observer_data(nx, nu, nd, ny, max(SIZES))
        qp.set_observer(dyn, meas, kt, nx, nu, nd, ny)
        for N in SIZES:
            for given in ((True, False) if nd else (False,)):
                dz = d[:N] if given else np.zeros((N, nd))
                want_p = lr.predict(dyn, x[:N], u[:N], dz)
                want_c = lr.correct(meas, kt, want_p, y[:N], dz)
                if path == "device":
                    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                    xs, dd = t(x[:N]), (t(d[:N]) if given else None)
                    qp.predict_state(xs, t(u[:N]), dd)
                    torch.cuda.synchronize(dev)
                    got_p = xs.cpu().numpy()
                    qp.correct_state(xs, t(y[:N]), dd)
                    torch.cuda.synchronize(dev)
                    got_c = xs.cpu().numpy()
                else:
                    xs = np.ascontiguousarray(x[:N].copy())
                    dd = np.ascontiguousarray(d[:N]) if given else None
                    qp.predict_state(xs, u[:N], dd)
                    got_p = xs.copy()
                    qp.correct_state(xs, y[:N], dd)
                    got_c = xs
                assert np.array_equal(got_p, want_p), (nx, nd, ny, N, given, "predict", np.abs(got_p - want_p).max())
                assert np.array_equal(got_c, want_c), (nx, nd, ny, N, given, "correct", np.abs(got_c - want_c).max())
                assert not np.array_equal(got_c, got_p)
    qp.close()


# ------------------------------------------------------------------ lmpc_simulate_ref_device
def _run_ref(lmpc, case, check=True):
    import loop_reference as lr
    data = lr.loop_data(case)
    qp = _handle(lmpc, data)
    H = case.Np if case.preview else 0
    out = qp.simulate_ref(data.x0, case.T, data.F, data.G, data.rtraj, preview=H, uprev=data.uprev, warm=case.warm)
    ref = lr.run_loop_case(case, oracle_ldp_from(qp.ldp()), data, entry="ref")
    _same(out, ref, case.name)
    if check:
        lr.check_loop_conditions(case, ref)
    return qp, data, out


def _ref_cases():
    import loop_reference as lr
    return _ids(lr.REF_CASES)


@pytest.mark.parametrize("case", _ref_cases())
def test_reference_trajectory_loop_equals_the_host_reference(lmpc, case):
    # plant_kernel<NXT> and the r-block of form_parameter_kernel inside the loop: every state size, preview on and off,
    # nuprev = nu and 0, cold and warm; r shorter than the run (held), longer than it, shared by all scenarios
    qp, data, _ = _run_ref(lmpc, case)
    other = _handle(lmpc, data)
    theta = _probe_theta_ref(case, qp)
    _assert_plain_solve_as_fresh(qp, _solve_dev(other, theta), theta, case.name)
    other.close()
    qp.close()


def _probe_theta_ref(case, qp, n=300):
    return np.random.default_rng(900 + case.seed).uniform(-case.x0, case.x0, (n, qp.nth))


# ------------------------------------------------------------------ lmpc_simulate, binary64
def _run_sim_modes(lmpc, case, modes, wave=False, one_handle=False):
    """`case` through lmpc_simulate in every mode: each run equals the host reference; after each run the handle solves
    a plain batch like a fresh handle"""
    import loop_reference as lr
    from oracle import ldp as oldp
    data = lr.loop_data(case)
    fresh = _handle(lmpc, data, wave=wave)
    L = oracle_ldp_from(fresh.ldp())
    ref = lr.run_loop_case(case, L, data)
    lr.check_loop_conditions(case, ref)
    kept = None
    theta = _probe_theta(case, data)
    plain = _solve_dev(fresh, theta)
    qp = None
    for opts in modes:
        if qp is None or not one_handle:
            qp = _handle(lmpc, data, wave=wave)
        for k, v in opts.items():
            qp.set_option(k, v)
        want = ref
        if wave and case.warm and opts.get("sim_keep_factor", 1) and case.T > 1:
            # the kept factorisation: the C oracle's warm == 2, which oracle/ldp.py exposes through its whole loop only
            if kept is None:
                kept = oldp.simulate(L, data.x0, case.T, data.F, data.G, r=data.r, uprev=data.uprev, warm=2)
            want = kept
        out = qp.simulate(data.x0, case.T, data.F, data.G, r=data.r, uprev=data.uprev, warm=case.warm)
        _same(out, want, (case.name, opts))
        _assert_plain_solve_as_fresh(qp, plain, theta, (case.name, opts))
        if not one_handle:
            qp.close()
    name = fresh.kernel_name
    fresh.close()
    if one_handle:
        qp.close()
    return data, ref, name


def _sim_cases(group):
    import loop_reference as lr
    return _ids(getattr(lr, group))


@pytest.mark.parametrize("case", _sim_cases("SIM_LANE"))
def test_closed_loop_lane_path_every_state_size_and_mode(lmpc, case):
    # nx = 1 .. 8: the scenario-asynchronous rounds, the fused lock-step loop, the plain loop (plant_theta_kernel);
    # nx = 9, 17, 32: beyond the rounds' gate (fused or plain)
    assert "lane" in _run_sim_modes(lmpc, case, LANE_MODES)[2]


@pytest.mark.parametrize("case", _sim_cases("SIM_WAVE"))
def test_closed_loop_wave_path_every_state_size_and_mode(lmpc, case):
    # "wave" 1 with "sim_keep_factor" 0 / 1, "sim_fused" 0 / 1, "sim_async" 0 / 2, on one handle whose options change
    _run_sim_modes(lmpc, case, WAVE_MODES, wave=True, one_handle=True)


def test_the_gate_constant_is_the_one_the_cases_assume():
    import loop_reference as lr
    found = []
    for path in glob.glob(os.path.join(ROOT, "linearmpc.jl_amd", "csrc", "*.hpp")):
        found += re.findall(r"constexpr\s+int\s+kMaxSimU\s*=\s*(\d+)\s*;", open(path).read())
    assert found == [str(lr.K_MAX_SIM_U)], found


@pytest.mark.parametrize("case", _sim_cases("GATES") + _sim_cases("LAYOUT"))
def test_closed_loop_gates_and_theta_layouts(lmpc, case):
    # nx 8 | 9 and nth 16 | 17 (the rounds' gate), nu = kMaxSimU | kMaxSimU + 1 (the fused loops' gate); nuprev 0,
    # 1 of 3, 3 of 3; no reference block
    assert "lane" in _run_sim_modes(lmpc, case, LANE_MODES)[2]


@pytest.mark.parametrize("case", _sim_cases("WAVE_GATES"))
def test_closed_loop_wave_path_input_count_gate(lmpc, case):
    # nu = kMaxSimU | kMaxSimU + 1 on a wavefront-path handle: the rounds and the fused plant step, or the plain loop
    _run_sim_modes(lmpc, case, WAVE_MODES, wave=True, one_handle=True)


@pytest.mark.parametrize("case", _sim_cases("SIM_SIZES"))
def test_closed_loop_batch_and_run_sizes(lmpc, case):
    _run_sim_modes(lmpc, case, ({}, {"sim_async": 0}, {"sim_async": 0, "sim_fused": 0}))


# ------------------------------------------------------------------ lmpc_simulate_f32
def _copy_settings(s):
    from oracle import ldp as oldp
    so = oldp.Settings()
    for f, _ in so._fields_:
        setattr(so, f, getattr(s, f, 0))
    return so


def _run_f32(lmpc, case, qp=None):
    import loop_reference as lr
    data = lr.loop_data(case)
    s32 = lmpc.default_settings_f32()
    qp = _handle(lmpc, data, settings=s32) if qp is None else qp
    x0, r = data.x0.astype(np.float32), data.r.astype(np.float32)
    up = None if data.uprev is None else data.uprev.astype(np.float32)
    out = qp.simulate_f32(x0, case.T, data.F, data.G, r=r, uprev=up, warm=case.warm)
    ref = lr.simulate_reference(oracle_ldp_from(qp.ldp()), x0, case.T, data.F, data.G, r=r, uprev=up, warm=case.warm,
                                dtype=np.float32, settings=_copy_settings(s32))
    assert out["U"].dtype == np.float32 and ref["U"].dtype == np.float32
    _same(out, ref, case.name)
    return qp, data, ref


@pytest.mark.parametrize("case", _sim_cases("SIM_F32"))
def test_closed_loop_binary32_equals_the_binary32_reference(lmpc, case):
    import loop_reference as lr
    qp, data, ref = _run_f32(lmpc, case)
    lr.check_loop_conditions(case, ref)
    qp.close()


# ------------------------------------------------------------------ C ABI: outputs that may be NULL
def test_c_abi_output_combinations(lmpc):
    import loop_reference as lr
    from linearmpc_jl_amd._cabi import check
    case = {c.name: c for c in lr.SIM_LANE}["sim-lane-nx5-warm"]
    data = lr.loop_data(case)
    S, T, nx, nu, nr, nup = case.S, case.T, case.nx, case.nu, data.nr, data.nup
    F, G, r = (np.ascontiguousarray(a, dtype=float) for a in (data.F, data.G, data.r))
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)

    def call(qp, absent, up0=None):
        x, up = data.x0.copy(), (np.zeros((S, nup)) if up0 is None else up0.copy())
        U, X, fm = np.full((T, S, nu), np.nan), np.full((T + 1, S, nx), np.nan), np.full(S, -99, np.int32)
        arg = {"uprev": up, "U": U, "X": X, "flag_min": fm}
        arg[absent] = None
        check(lmpc.lib().lmpc_simulate(qp._h, S, T, nx, nr, nup, vp(F), vp(G), vp(x), vp(r), vp(arg["uprev"]), vp(arg["U"]),
                                       vp(arg["X"]), vp(arg["flag_min"]), 1), qp._h)
        arg["x"] = x
        return arg, up

    first = _handle(lmpc, data)
    L = oracle_ldp_from(first.ldp())
    first.close()
    assert data.uprev is not None and data.uprev.any()
    ref = lr.run_loop_case(case, L, data)                                  # from the case's random uprev
    zero = lr.simulate_reference(L, data.x0, T, data.F, data.G, r=data.r, warm=True)        # from zeros
    assert not np.array_equal(ref["U"][0], zero["U"][0])
    for opts in LANE_MODES:
        for absent in (None, "U", "X", "flag_min", "uprev"):
            qp = _handle(lmpc, data, opts)
            # uprev NULL: the loop starts from zeros and copies nothing back; the other outputs are those of an explicit
            # array of zeros, and differ from those of the case's own uprev
            got, up = call(qp, absent, None if absent == "uprev" else data.uprev)
            _same(got, zero if absent == "uprev" else ref, (opts, absent), [k for k in KEYS if k != absent])
            if absent is None:
                assert np.array_equal(up, ref["uprev"])
                got0, up0 = call(qp, None)
                got0["uprev"] = up0
                _same(got0, zero, (opts, "zeros given"))
            qp.close()


# ------------------------------------------------------------------ the generated controller's parameter formation
@pytest.mark.parametrize("nr,nph", [(1, 4), (3, 5), (2, 0)])
def test_compute_control_parameter_formation(lmpc, nr, nph):
    # update_parameter_kernel: the five arrays present and absent, the condensation sum at nr = 1 and 3 (separate multiply
    # and add in q order), in place on the device and through both host stagings (mapped block, staging block); with
    # nph = 0 also the gather fused into the screening kernel ("cc_fused" 1, lane path only) against the kernel
    import torch
    import loop_reference as lr
    from oracle import ldp as oldp
    nx, nd, nup, npar, nu = 3, 2, 1, 2, 2
    nth = nx + nr + nd + nup + npar
    rng = np.random.default_rng(40 + nr)
    qpd = lr.random_qp(rng, 4, 6, nth, wscale=0.1)        # hard rows: the lane / screening path, where the gather is
    qpd[2][:] *= 1.3
    data = type("D", (), dict(qp=qpd, nout=nu))
    t2s = rng.standard_normal((nr, nr * nph)) / np.sqrt(nr * nph) if nph else None
    for N in (300, 3000):                                 # 300: the mapped block; 3000: the staging block
        arrays = dict(control=rng.uniform(-1, 1, (N, nu)), state=rng.uniform(-1.5, 1.5, (N, nx)),
                      reference=rng.uniform(-1, 1, (N, nr * max(nph, 1))), disturbance=rng.uniform(-1, 1, (N, nd)),
                      parameter=rng.uniform(-1, 1, (N, npar)))
        for fused in ((1, 0) if nph == 0 else (1,)):
            qp = _handle(lmpc, data, {"cc_fused": fused})
            assert "lane" in qp.kernel_name
            L = oracle_ldp_from(qp.ldp())
            qp.set_parameter_layout(nx, nr, nd, nup, npar, preview_horizon=nph, traj2setpoint=t2s)
            dev = torch.device("cuda", qp.device)
            for absent in (None, "control", "reference", "disturbance", "parameter"):
                kw = {k: (None if k == absent else v) for k, v in arrays.items()}
                theta = lr.update_parameter_reference(N, nu, nx, nr, nd, nup, npar, nph=nph, t2s=t2s, **kw)
                xo, efo, _, _ = oldp.solve_batch(L, theta)
                assert (efo >= 1).all() and 0.05 < (lr.popcount(oldp.solve_batch(L, theta)[3]) > 0).mean() < 0.95
                c0 = np.zeros((N, nu)) if kw["control"] is None else kw["control"]
                ch = np.ascontiguousarray(c0.copy())
                ef = qp.compute_control(ch, kw["state"], kw["reference"], kw["disturbance"], kw["parameter"])
                assert np.array_equal(ch, xo) and np.array_equal(ef, efo), (N, fused, absent, "host")
                t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                cd = t(c0.copy())
                efd = qp.compute_control_device(cd, t(kw["state"]), t(kw["reference"]), t(kw["disturbance"]), t(kw["parameter"]))
                torch.cuda.synchronize(dev)
                assert np.array_equal(cd.cpu().numpy(), xo) and np.array_equal(efd.cpu().numpy(), efo), (N, fused, absent, "device")
            # a plain solve after the controller call: as a fresh handle's
            th = rng.uniform(-1, 1, (257, nth))
            other = _handle(lmpc, data)
            _assert_plain_solve_as_fresh(qp, _solve_dev(other, th), th, (nr, nph, N, fused))
            other.close()
            qp.close()


@pytest.mark.parametrize("ndm", [0, 1, 3])
def test_compute_control_observer_split(lmpc, ndm):
    # split_observer_state_kernel with no, one and only measured disturbances, then the controller call
    import torch
    import loop_reference as lr
    from oracle import ldp as oldp
    nx, nr, nd, nup, nu, N = 3, 1, 3, 1, 2, 1000
    ndo = nd - ndm
    nth = nx + nr + nd + nup
    rng = np.random.default_rng(50 + ndm)
    data = type("D", (), dict(qp=lr.random_qp(rng, 4, 6, nth, wscale=0.1), nout=nu))
    obs, meas = rng.uniform(-1, 1, (N, nx + ndo)), rng.uniform(-1, 1, (N, ndm))
    ref, u0 = rng.uniform(-1, 1, (N, nr)), rng.uniform(-1, 1, (N, nu))
    for fused in (1, 0):
        qp = _handle(lmpc, data, {"cc_fused": fused})
        assert "lane" in qp.kernel_name
        qp.set_parameter_layout(nx, nr, nd, nup, 0)
        L = oracle_ldp_from(qp.ldp())
        dev = torch.device("cuda", qp.device)
        t = lambda a: None if a is None or a.shape[1] == 0 else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        for m in ((meas, None) if ndm else (None,)):
            st, di = lr.split_observer_reference(obs, m, nx, ndm, ndo)
            theta = lr.update_parameter_reference(N, nu, nx, nr, nd, nup, 0, control=u0, state=st, reference=ref, disturbance=di)
            xo, efo, _, acto = oldp.solve_batch(L, theta)
            assert (efo >= 1).all() and 0.05 < (lr.popcount(acto) > 0).mean() < 0.95
            c = torch.from_numpy(u0.copy()).to(dev)
            ef = qp.compute_control_observer_device(c, torch.from_numpy(obs).to(dev), ndm, t(ref), t(m))
            torch.cuda.synchronize(dev)
            assert np.array_equal(c.cpu().numpy(), xo) and np.array_equal(ef.cpu().numpy(), efo), (ndm, fused, m is None)
        qp.close()


# ------------------------------------------------------------------ what a loop leaves on its handle
def _rerun_cases():
    import loop_reference as lr
    by = {c.name: c for c in lr.SIM_CASES + lr.SIM_F32 + lr.REF_CASES}
    out = []
    for entry, name, modes in (("lane", "sim-lane-nx4-warm", LANE_MODES), ("lane", "sim-lane-nx9-warm", LANE_MODES[-2:]),
                               ("wave", "sim-wave-nx6-warm", WAVE_MODES), ("f32", "sim-f32-nx8-warm", ({},)),
                               ("ref", "ref-nx7-prev-warm", ({},))):
        for i, opts in enumerate(modes):
            out.append(pytest.param(entry, by[name], opts, id=f"{name}-mode{i}"))
    return out


@pytest.mark.parametrize("entry,case,opts", _rerun_cases())
def test_a_second_and_a_third_loop_on_one_handle(lmpc, entry, case, opts):
    # S = 100, then 40 (what the larger run left in the handle's buffers must not be read), then 700 (they regrow):
    # each run equals a fresh handle's run of the same size, which the sweeps above tie to the host reference
    import dataclasses
    import loop_reference as lr
    cases = [dataclasses.replace(case, S=S, pool=1000) for S in (100, 40, 700)]
    s32 = lmpc.default_settings_f32() if entry == "f32" else None

    def run(qp, c):
        d = lr.loop_data(c)
        if entry == "f32":
            return qp.simulate_f32(d.x0.astype(np.float32), c.T, d.F, d.G, r=d.r.astype(np.float32),
                                   uprev=None if d.uprev is None else d.uprev.astype(np.float32), warm=c.warm)
        if entry == "ref":
            return qp.simulate_ref(d.x0, c.T, d.F, d.G, d.rtraj, preview=c.Np if c.preview else 0, uprev=d.uprev, warm=c.warm)
        return qp.simulate(d.x0, c.T, d.F, d.G, r=d.r, uprev=d.uprev, warm=c.warm)

    data = lr.loop_data(cases[0])
    one = _handle(lmpc, data, opts, settings=s32, wave=entry == "wave")
    theta = _probe_theta(case, data) if entry != "ref" else _probe_theta_ref(case, one)
    if entry == "f32":
        theta = theta.astype(np.float32)
    for c in cases:
        assert np.array_equal(lr.loop_data(c).x0[:40], lr.loop_data(cases[1]).x0)          # cuts of one pool
        fresh = _handle(lmpc, data, opts, settings=s32, wave=entry == "wave")
        _same(run(one, c), run(fresh, c), (case.name, opts, c.S))
        fresh.close()
        fresh = _handle(lmpc, data, opts, settings=s32, wave=entry == "wave")
        _assert_plain_solve_as_fresh(one, _solve_dev(fresh, theta), theta, (case.name, opts, c.S))
        fresh.close()
    one.close()
