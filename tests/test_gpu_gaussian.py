"""Gaussian noise drawn on the GPU: lmpc_noise_draw_device against lmpc_noise_draw_host bit for bit (the agreement of the
two sides' square root and division), the uncertain and the nonlinear scenario loop with drawn Gaussian sources against
the host reference of tests/gaussian_reference.py at every state-size instantiation with and without the cost rows, the
same loops fed the device's own draws as supplied blocks, split runs, `Simulation` with `lmpc.Gaussian`, and a uniform
run before and after on one handle.  The cases' conditions are checked on the host (tests/test_gaussian_host.py)."""
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_nonlinear as tgn
import test_gpu_uncertain as tgu
from test_gpu_nonlinear import cartpole, pendulum  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


def _src(lmpc, a, dev, sl=slice(None), cols=slice(None)):
    """a reference-side source (None, Normal, Box or array) as the package takes it"""
    import gaussian_reference as gr
    if isinstance(a, gr.Normal):
        return lmpc.Gaussian(a.mean, a.std)
    return tgu._source(lmpc, a, dev, sl, cols)


def _direct(lmpc, mpc, case, data, sl=slice(None), cols=slice(None), **kw):
    """test_gpu_uncertain._direct on the base case with the sources of `data` (a Gaussian among them) put in"""
    import torch
    dev = torch.device("cuda", mpc.control_model().device)
    bare = SimpleNamespace(**{**vars(data), "process": None, "measurement_noise": None})
    kw.setdefault("process", _src(lmpc, data.process, dev, sl, cols))
    kw.setdefault("measurement_noise", _src(lmpc, data.measurement_noise, dev, sl, cols))
    return tgu._direct(lmpc, mpc, case.base, bare, sl=sl, cols=cols, **kw)


def _reference(mpc, case, data, **over):
    import gaussian_reference as gr
    from conftest import oracle_ldp_from
    return gr.gaussian_run(case, oracle_ldp_from(mpc.control_model().ldp()), data, settings=tgu._oracle_settings(mpc), **over)


def _run_and_compare(lmpc, case, mpc=None):
    import gaussian_reference as gr
    data = gr.case_data(case)
    mpc = tgu._mpc(lmpc, data.prob) if mpc is None else mpc
    ref = _reference(mpc, case, data)
    out = _direct(lmpc, mpc, case, data)
    tgu._assert_equal(case.base, out, ref)
    return out, ref, data, mpc


def _cases(group):
    import gaussian_reference as gr
    return [pytest.param(c, id=c.name) for c in group(gr)]


# ------------------------------------------------------------------ the draw
@pytest.mark.parametrize("dist", ["gauss", "uniform"])
def test_draw_device_equals_draw_host(lmpc, dist):
    # w = 1, 2, 3, 5; N = 1, 63, 64, 65, 257 with T = 3 (a ragged second workgroup at 257 * 3); both streams; a
    # scenario_offset above 2^32 with a step_offset; std = 0.  For "gauss" this is the agreement of the device's division
    # and square root with the host's on these arguments.
    import torch
    import gaussian_reference as gr
    import uncertain_reference as ur
    model = tgu._mpc(lmpc, ur.case_data(ur.STATES[1]).prob).control_model()
    for w in gr.DRAW_W:
        src = _src(lmpc, gr.draw_source(w, dist), None)
        for N in gr.DRAW_N:
            for so, ko in gr.DRAW_OFFSETS:
                for stream in (0, 1):
                    kw = dict(seed=gr.DRAW_SEED, stream=stream, scenario_offset=so, step_offset=ko)
                    got = model.noise_draw(src, N, gr.DRAW_T, **kw)
                    torch.cuda.synchronize()
                    want = lmpc.noise_draw(src, N, gr.DRAW_T, **kw)
                    assert tuple(got.shape) == want.shape == (N, w, gr.DRAW_T)
                    got = got.cpu().numpy()
                    assert np.array_equal(got, want), (dist, w, N, so, ko, stream, int((got != want).sum()), float(np.abs(got - want).max()))
    model.check()
    # a larger sample of pairs, where a square root that is not correctly rounded would show: 2 * 10^5 draws
    src = lmpc.Gaussian([0.0, 0.0], [1.0, 1.0]) if dist == "gauss" else lmpc.Uniform([-1.0, 0.0], [1.0, 3.0])
    got = model.noise_draw(src, 50000, 2, seed=11, stream=0)
    torch.cuda.synchronize()
    model.check()
    want = lmpc.noise_draw(src, 50000, 2, seed=11, stream=0)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (int((got != want).sum()), float(np.abs(got - want).max()))
    with pytest.raises(lmpc.LmpcError, match="lmpc_noise_draw_device: stream:"):
        model.noise_draw(src, 2, 2, stream=2)


# ------------------------------------------------------------------ the uncertain loop
@pytest.mark.parametrize("case", _cases(lambda gr: gr.STATES))
def test_every_state_size_with_and_without_cost_equals_the_host_reference(lmpc, case):
    # uncertain_pre_kernel<NX, true> and uncertain_post_kernel<NX, COST, true> for NX = 1 .. 8 and the run-time kernels
    # at nx = 9: both sources Gaussian, the observer on for odd nx, 65 scenarios (a ragged second wavefront) x 3 steps
    out, ref, _, _ = _run_and_compare(lmpc, case)
    if case.base.cost:
        assert "cost" in out and "violation" in out and ref.cost.min() > 0


@pytest.mark.parametrize("case", _cases(lambda gr: gr.SHAPES))
def test_shapes_and_mixtures_of_the_sources(lmpc, case):
    # nw = 1, 3 through a Gw (an odd count uses half a pair); ny = 1; Gaussian with uniform, with a supplied block, and
    # the reverses; process noise alone; a scenario_offset above 2^32 with a step_offset
    _run_and_compare(lmpc, case)


@pytest.mark.parametrize("name", ["gw-nw3", "nx9-cost"])
def test_drawn_gaussian_equals_the_device_draws_supplied_as_blocks(lmpc, name):
    # independent of the host reference: the loop's own draw against lmpc_noise_draw_device's output handed back as
    # per-scenario supplied blocks
    import gaussian_reference as gr
    case = next(c for c in gr.CASES if c.name == name)
    data = gr.case_data(case)
    mpc = tgu._mpc(lmpc, data.prob)
    model, b = mpc.control_model(), case.base
    drawn = _direct(lmpc, mpc, case, data)
    kw = dict(seed=b.key, scenario_offset=b.scenario_offset, step_offset=b.step_offset)
    e = model.noise_draw(lmpc.Gaussian(data.process.mean, data.process.std), b.S, b.T, stream=0, **kw)
    v = model.noise_draw(lmpc.Gaussian(data.measurement_noise.mean, data.measurement_noise.std), b.S, b.T, stream=1, **kw)
    fed = _direct(lmpc, mpc, case, data, process=e, measurement_noise=v)
    for key in ("X", "U", "Y", "Ym", "Xhat", "W", "x", "uprev", "flag_min") + (("cost", "violation") if b.cost else ()):
        assert np.array_equal(drawn[key], fed[key]), (name, key)
    assert np.abs(drawn["W"]).max() > 0


def test_split_runs_equal_the_whole(lmpc):
    # 130 scenarios = 2 x 65 with scenario_offset; 6 steps = 2 x 3 with step_offset, the carried state and the shifted
    # trajectories
    import torch
    import gaussian_reference as gr
    case = gr.SPLIT
    b = case.base
    whole, ref, data, mpc = _run_and_compare(lmpc, case)
    for lo in (0, 65):
        part = _direct(lmpc, mpc, case, data, sl=slice(lo, lo + 65), scenario_offset=b.scenario_offset + lo)
        for key in ("X", "U", "Xhat", "Ym", "W", "flag_min"):
            want = whole[key][lo:lo + 65] if key == "flag_min" else whole[key][:, lo:lo + 65]
            assert np.array_equal(part[key], want), (lo, key)
    dev = torch.device("cuda", mpc.control_model().device)
    x = torch.from_numpy(data.x0.copy()).to(dev)
    state = (x, x.clone(), torch.zeros((b.S, b.nu), dtype=torch.float64, device=dev))
    first = _direct(lmpc, mpc, case, data, T=3, state=state)
    second = _direct(lmpc, mpc, case, data, cols=slice(3, None), T=3, state=first["_state"], step_offset=b.step_offset + 3)
    for key in ("U", "Xhat", "Ym", "Y", "W"):
        assert np.array_equal(np.concatenate([first[key], second[key]]), whole[key]), key
    assert np.array_equal(np.concatenate([first["X"], second["X"][1:]]), whole["X"])
    assert np.array_equal(second["x"], ref.xs[-1]) and np.array_equal(second["xhat"], ref.xhat_final)


def test_uniform_and_quiet_runs_before_and_after_a_gaussian_one_on_one_handle(lmpc):
    # the instantiations without GAUSS go on serving every other run: a case with both sources uniform and the same case
    # with every source off, against their existing reference (uncertain_reference.run_case), before and after a
    # Gaussian run on the same handle
    from dataclasses import replace
    import gaussian_reference as gr
    import uncertain_reference as ur
    uniform = replace(ur.STATES[4], S=65, T=3)
    off = replace(uniform, name="nx5-off", process=None, meas=None)
    gauss = next(c for c in gr.STATES if c.base.nx == 5 and not c.base.cost)
    assert uniform.nx == 5 and uniform.seed == gauss.base.seed and uniform.observer == gauss.base.observer
    gdata = gr.case_data(gauss)
    mpc = tgu._mpc(lmpc, gdata.prob)
    for _ in range(2):
        for case in (uniform, off):
            data = ur.case_data(case)
            out = tgu._direct(lmpc, mpc, case, data)
            tgu._assert_equal(case, out, tgu._reference(mpc, case, data))
            assert ("W" in out) == (case.process is not None)
        tgu._assert_equal(gauss.base, _direct(lmpc, mpc, gauss, gdata), _reference(mpc, gauss, gdata))


# ------------------------------------------------------------------ the nonlinear loop
def test_cartpole_with_gaussian_process_and_measurement_noise(lmpc, pendulum, cartpole):
    # nonlinear_post_kernel<4, false, true> after uncertain_pre_kernel<4, true>: 65 scenarios x 20 steps, q per
    # scenario, the process noise through a Gw, the observer on, a scenario_offset and a step_offset
    import torch
    import gaussian_reference as gr
    mpc, ldp, settings = pendulum
    case, data = gr.NONLINEAR, gr.nonlinear_data()
    ref = gr.nonlinear_gaussian_run(case, ldp, cartpole, data, settings=settings)
    out = _nonlinear(lmpc, mpc, cartpole, case, data, torch.device("cuda", mpc.control_model().device))
    tgn._assert_equal(case, out, ref)
    assert np.abs(out["W"]).max() > 0


def _nonlinear(lmpc, mpc, plant, case, data, dev):
    """model.simulate_scenario_nonlinear with the Gaussian sources of `data`: every array as numpy"""
    import torch
    model = mpc.control_model()
    model.set_observer(*data.observer, 4, 1, 0, 2)
    out = model.simulate_scenario_nonlinear(
        tgn._t(data.x0, dev), case.T, plant, r_width=2, use_observer=True, warm=case.warm, params=data.q,
        process=_src(lmpc, data.process, dev), measurement_noise=_src(lmpc, data.measurement_noise, dev), Gw=data.Gw,
        seed=case.key, scenario_offset=case.scenario_offset, step_offset=case.step_offset, want=("U", "X", "Y", "Ym", "Xhat", "W"))
    torch.cuda.synchronize(dev)
    model.check()
    return {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


# ------------------------------------------------------------------ Simulation
def test_simulation_with_gaussian_sources(lmpc):
    import gaussian_reference as gr
    case = gr.SIMULATION
    b = case.base
    data = gr.case_data(case)
    mpc = tgu._mpc(lmpc, data.prob)
    ref = _reference(mpc, case, data)
    sc = lmpc.Scenario(data.x0, N=b.T, r=data.r, d=data.d, process_noise=lmpc.Gaussian(data.process.mean, data.process.std),
                       measurement_noise=lmpc.Gaussian(data.measurement_noise.mean, data.measurement_noise.std))
    import scenario_reference as sr
    sim = lmpc.Simulation(mpc, sc, tgu._plant(lmpc, sr.plant_of(data.prob)), observer=data.kf.codegen_arrays(), Gw=data.Gw, seed=b.key)
    step = lambda a: a.transpose(1, 2, 0)
    assert sim.ws.shape == (b.S, b.nx, b.T)
    for name, got, want in (("xs", sim.xs, step(ref.xs[:-1])), ("us", sim.us, step(ref.us)), ("xhats", sim.xhats, step(ref.xhats)),
                            ("yms", sim.yms, step(ref.yms)), ("ys", sim.ys, step(ref.ys)), ("ws", sim.ws, step(ref.ws)),
                            ("x_final", sim.x_final, ref.xs[-1]), ("flag_min", sim.flag_min, ref.flag_min)):
        assert np.array_equal(got, want), name
