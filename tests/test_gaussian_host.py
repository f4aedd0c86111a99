"""Host side of the Gaussian draw (no GPU): lmpc_noise_draw_host against the restatement of tests/gaussian_reference.py
bit for bit, sharded and continued draws, the uniform distribution through the same entry point, the accuracy of the
stated logarithm, the distribution of a million draws, every new refusal by its field, the struct layouts against a C
compiler and against the previous header's offsets, the Python argument checks, and the conditions that keep the
closed-loop GPU cases of tests/test_gpu_gaussian.py from passing emptily."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


def _obj(lmpc, src):
    import gaussian_reference as gr
    return lmpc.Gaussian(src.mean, src.std) if isinstance(src, gr.Normal) else lmpc.Uniform(src.lo, src.hi)


# ------------------------------------------------------------------ the draw
@pytest.mark.parametrize("w", [1, 2, 3, 5])
def test_draw_host_equals_the_restatement(lmpc, w):
    # N = 1, 63, 64, 65, 257, T = 3, both streams, a scenario_offset above 2^32 with a step_offset, std = 0 (w >= 3)
    import gaussian_reference as gr
    src = gr.draw_source(w, "gauss")
    assert (src.std[-1] == 0.0) == (w >= 3)
    for N in gr.DRAW_N:
        for so, ko in gr.DRAW_OFFSETS:
            for stream in (0, 1):
                got = lmpc.noise_draw(_obj(lmpc, src), N, gr.DRAW_T, seed=gr.DRAW_SEED, stream=stream, scenario_offset=so, step_offset=ko)
                want = gr.blocks(src, gr.DRAW_SEED, stream, so, N, ko, gr.DRAW_T)
                assert got.shape == (N, w, gr.DRAW_T)
                assert np.array_equal(got, want), (w, N, so, ko, stream, float(np.abs(got - want).max()))
                if w >= 3:
                    assert np.array_equal(got[:, -1], np.full((N, gr.DRAW_T), src.mean[-1]))
    a, b = (lmpc.noise_draw(_obj(lmpc, src), 65, 3, seed=gr.DRAW_SEED, stream=s) for s in (0, 1))
    assert (a[:, 0] != b[:, 0]).all()                                       # the streams differ
    assert gr.DRAW_OFFSETS[1][0] > 2 ** 32


def test_the_layout_is_the_supplied_block_and_odd_counts_use_half_a_pair(lmpc):
    import gaussian_reference as gr
    s5, s3 = gr.draw_source(5, "gauss"), gr.draw_source(5, "gauss")
    s3 = gr.Normal(s3.mean[:3], s3.std[:3])
    a = lmpc.noise_draw(_obj(lmpc, s5), 7, 4, seed=3)
    b = lmpc.noise_draw(_obj(lmpc, s3), 7, 4, seed=3)
    assert np.array_equal(a[:, :3], b)
    # the C side's buffer is (N, T, w): record (i, k) at (i * T + k) * w, i.e. stride w * T per scenario
    assert a.base is not None and a.base.shape == (7, 4, 5) and a.base.flags["C_CONTIGUOUS"]


def test_sharded_and_continued_draws_equal_the_unsplit_ones(lmpc):
    import gaussian_reference as gr
    for dist in ("gauss", "uniform"):
        src = _obj(lmpc, gr.draw_source(3, dist))
        kw = dict(seed=77, stream=1)
        whole = lmpc.noise_draw(src, 130, 6, scenario_offset=9, step_offset=4, **kw)
        for lo in (0, 65):
            part = lmpc.noise_draw(src, 65, 6, scenario_offset=9 + lo, step_offset=4, **kw)
            assert np.array_equal(part, whole[lo:lo + 65]), (dist, lo)
        for k0 in (0, 3):
            part = lmpc.noise_draw(src, 130, 3, scenario_offset=9, step_offset=4 + k0, **kw)
            assert np.array_equal(part, whole[..., k0:k0 + 3]), (dist, k0)
        assert not np.array_equal(lmpc.noise_draw(src, 65, 6, scenario_offset=9, step_offset=4, **kw), whole[65:])


@pytest.mark.parametrize("w", [1, 2, 3, 5])
def test_dist_zero_through_the_new_functions_is_the_uniform_restatement(lmpc, w):
    import gaussian_reference as gr
    import uncertain_reference as ur
    src = gr.draw_source(w, "uniform")
    for N in (1, 65, 257):
        for so, ko in gr.DRAW_OFFSETS:
            for stream in (0, 1):
                got = lmpc.noise_draw(_obj(lmpc, src), N, 3, seed=gr.DRAW_SEED, stream=stream, scenario_offset=so, step_offset=ko)
                g = np.arange(N, dtype=np.uint64) + np.uint64(so)
                for k in range(3):
                    assert np.array_equal(got[..., k], ur.draw(gr.DRAW_SEED, g, ko + k, stream, src.lo, src.hi)), (w, N, so, stream, k)


# ------------------------------------------------------------------ the stated logarithm
def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_the_logarithm_is_within_two_ulp_of_numpy():
    """Bound: 2 ulp -- each side's documented error is below 1 ulp (as for sin_ / cos_).  Measured maxima against numpy:
    1.0 ulp on each of the three sets."""
    import gaussian_reference as gr
    rng = np.random.default_rng(2026)
    sets = {"uniform": rng.integers(1, 2 ** 53, 10 ** 6, endpoint=True).astype(np.float64) * 2.0 ** -53,
            "below one": 1.0 - np.arange(0, 10 ** 4 + 1) * 2.0 ** -53,
            "smallest": np.arange(1, 10 ** 4 + 1) * 2.0 ** -53}
    worst = {}
    for name, t in sets.items():
        assert t.min() >= 2.0 ** -53 and t.max() <= 1.0
        got, want = gr.log_(t), np.log(t)
        assert (got <= 0).all()
        zero = want == 0
        assert np.array_equal(got[zero], want[zero])
        worst[name] = float(_ulps(got[~zero], want[~zero]).max())
    print("max ulp difference of log_ against numpy:", worst)
    assert max(worst.values()) <= 2.0, worst
    one = gr.log_(np.array([1.0]))
    assert one[0] == 0.0 and not np.signbit(one[0])
    assert gr.log_(np.array([2.0 ** -53]))[0] == -53 * np.log(2.0)


def test_distribution_of_a_million_draws(lmpc):
    # five standard errors at n = 10^6: mean 1e-3, variance sqrt(2) e-3, correlation 1e-3; Kolmogorov's 1.95 / sqrt(n)
    from math import erf, sqrt
    import gaussian_reference as gr
    z = lmpc.noise_draw(lmpc.Gaussian([0.0, 0.0], [1.0, 1.0]), 250000, 2, seed=20261019)       # 5 * 10^5 pairs
    z0, z1 = z[:, 0].reshape(-1), z[:, 1].reshape(-1)
    flat = np.concatenate([z0, z1])
    assert flat.size == 10 ** 6
    figures = dict(mean=float(flat.mean()), var=float(flat.var()), corr=float(np.corrcoef(z0, z1)[0, 1]), zmax=float(np.abs(flat).max()))
    s = np.sort(flat)
    cdf = 0.5 * (1.0 + np.vectorize(erf)(s / sqrt(2.0)))
    n = s.size
    figures["ks"] = float(max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(0, n) / n).max()))
    print("distribution of 10^6 draws:", figures)
    assert abs(figures["mean"]) < 0.005
    assert abs(figures["var"] - 1.0) < 0.0071
    assert abs(figures["corr"]) < 0.005
    assert figures["ks"] < 1.95e-3
    assert figures["zmax"] <= gr.Z_MAX
    # the largest |z| there is: u1 = 2^-53
    assert np.sqrt(-2.0 * gr.log_(np.array([2.0 ** -53])))[0] <= gr.Z_MAX
    # ... and a sample of the same draws is the restatement's
    want = gr.normals(20261019, np.arange(1000, dtype=np.uint64), 1, 0, 2)
    assert np.array_equal(z[:1000, :, 1], want)


# ------------------------------------------------------------------ the refusals
def _noise(w=2, dist=1, lo=(0.0, 0.0), hi=(1.0, 1.0), H=0):
    from linearmpc_jl_amd._cabi import Block, Noise
    n, keep = Noise(), []

    def vec(a):
        if a is None:
            return None
        keep.append(np.ascontiguousarray(np.asarray(a, float)))
        return keep[-1].ctypes.data

    n.w, n.dist, n.lo, n.hi = w, dist, vec(lo), vec(hi)
    n.src = Block(None, 0, w, 1, 0, H)
    n._keep = keep
    return n


def _draw_rc(lmpc, n, stream=0, N=2, step_offset=0, T=2, out=True):
    from linearmpc_jl_amd._cabi import last_error
    buf = np.zeros(64)
    rc = lmpc.lib().lmpc_noise_draw_host(None if n is None else ctypes.byref(n), 1, stream, 0, N, step_offset, T,
                                         ctypes.c_void_p(buf.ctypes.data) if out else None)
    return rc, last_error(None)


@pytest.mark.parametrize("field,noise,call", [
    ("noise", None, {}),
    ("noise.w", dict(w=-1), {}),
    ("noise.dist", dict(dist=2), {}),
    ("noise.dist", dict(dist=-1), {}),
    ("noise.lo", dict(lo=None), {}),
    ("noise.hi", dict(hi=None), {}),
    ("noise.lo", dict(lo=None, hi=None), {}),
    ("noise.lo", dict(lo=(0.0, float("nan"))), {}),
    ("noise.lo", dict(lo=(float("inf"), 0.0)), {}),
    ("noise.hi", dict(hi=(1.0, -1e-300)), {}),
    ("noise.hi", dict(hi=(float("inf"), 1.0)), {}),
    ("noise.hi", dict(hi=(1.0, float("nan"))), {}),
    ("noise.src.H", dict(H=2), {}),
    ("noise.lo", dict(dist=0, lo=None, hi=None), {}),                    # a supplied source draws nothing
    ("noise.lo", dict(dist=0, lo=(2.0, 0.0)), {}),                        # the uniform refusals, word for word
    ("stream", {}, dict(stream=2)),
    ("N", {}, dict(N=-1)),
    ("T", {}, dict(T=-1)),
    ("step_offset", {}, dict(step_offset=-1)),
    ("step_offset", {}, dict(step_offset=2 ** 31 - 2)),
    ("out", {}, dict(out=False)),
])
def test_every_refusal_of_the_draw_names_its_field(lmpc, field, noise, call):
    rc, msg = _draw_rc(lmpc, None if noise is None else _noise(**noise), **call)
    assert rc == -100, (rc, msg)
    assert msg.startswith("lmpc_noise_draw_host: " + field + ":"), msg


def test_well_formed_draws_pass(lmpc):
    assert _draw_rc(lmpc, _noise())[0] == 1
    assert _draw_rc(lmpc, _noise(hi=(0.0, 0.0)))[0] == 1                    # std == 0
    assert _draw_rc(lmpc, _noise(dist=0))[0] == 1
    assert _draw_rc(lmpc, _noise(), N=0, out=False)[0] == 1
    assert "lo > hi at component 0" in _draw_rc(lmpc, _noise(dist=0, lo=(2.0, 0.0)))[1]


@pytest.mark.parametrize("field,which,noise", [
    ("process.dist", "process", dict(dist=2)),
    ("measurement.dist", "measurement", dict(w=1, dist=7, lo=(0.0,), hi=(1.0,))),
    ("process.lo", "process", dict(lo=None)),
    ("process.hi", "process", dict(hi=None)),
    ("measurement.lo", "measurement", dict(w=1, lo=None, hi=(1.0,))),
    ("process.lo", "process", dict(lo=(float("nan"), 0.0))),
    ("process.hi", "process", dict(hi=(-1.0, 1.0))),
    ("measurement.hi", "measurement", dict(w=1, lo=(0.0,), hi=(float("inf"),))),
])
def test_the_loop_check_refuses_a_bad_gaussian_source_by_its_field(lmpc, field, which, noise):
    from linearmpc_jl_amd._cabi import Uncertainty, last_error
    from test_uncertain_host import _desc
    un = Uncertainty()
    n = _noise(**noise)
    setattr(un, which, n)
    rc = lmpc.lib().lmpc_scenario_uncertain_check(4, 1, None, ctypes.byref(_desc(lmpc)), ctypes.byref(un))
    msg = last_error(None)
    assert rc == -100 and msg.startswith("lmpc_scenario_uncertain_check: " + field + ":"), (rc, msg)


def test_the_loop_check_accepts_gaussian_sources_in_either_slot(lmpc):
    from linearmpc_jl_amd._cabi import Uncertainty
    from test_uncertain_host import _desc
    for pd, md in ((1, 1), (1, 0), (0, 1)):
        un = Uncertainty()
        un.process = _noise(dist=pd, lo=(-1.0, 0.0))
        un.measurement = _noise(w=1, dist=md, lo=(-0.5,), hi=(0.5,))
        keep = (un.process, un.measurement)
        assert lmpc.lib().lmpc_scenario_uncertain_check(4, 1, None, ctypes.byref(_desc(lmpc)), ctypes.byref(un)) == 1, (pd, md, keep)


# ------------------------------------------------------------------ the ABI
def test_symbols_are_exported_and_bound(lmpc):
    L = lmpc.lib()
    for name in ("lmpc_noise_draw_host", "lmpc_noise_draw_device"):
        assert name in lmpc.SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.lmpc_abi_version() == 2
    for name in ("Gaussian", "noise_draw"):
        assert hasattr(lmpc, name) and name in lmpc.__all__, name
    assert hasattr(lmpc.BatchedQP, "noise_draw") and hasattr(lmpc.BatchedQP, "noise_draw_host")


# sizeof(lmpc_noise), sizeof(lmpc_uncertainty) and the offsets of every field the header had before `dist` went into the
# padding behind lmpc_noise.w (LP64, from that header)
PREVIOUS_LAYOUT = {"sizeof(lmpc_noise)": 56, "sizeof(lmpc_uncertainty)": 168,
                   "lmpc_noise": dict(w=0, src=8, lo=40, hi=48),
                   "lmpc_uncertainty": dict(process=0, Gw=56, measurement=64, seed=120, scenario_offset=128, step_offset=136,
                                            n_plants=140, plants=144, plant_index=152, W_traj=160)}


def test_struct_layouts_match_the_header_and_no_offset_moved(lmpc, tmp_path):
    import os, shutil, subprocess
    from conftest import ROOT
    from linearmpc_jl_amd._cabi import Noise, Uncertainty
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    nf = [n for n, _ in Noise._fields_]
    uf = [n for n, _ in Uncertainty._fields_]
    body = 'printf("%zu %zu %d %d\\n", sizeof(lmpc_noise), sizeof(lmpc_uncertainty), LMPC_NOISE_UNIFORM, LMPC_NOISE_GAUSSIAN);\n'
    body += "".join(f'printf("%zu\\n", offsetof(lmpc_noise, {n}));\n' for n in nf)
    body += "".join(f'printf("%zu\\n", offsetof(lmpc_uncertainty, {n}));\n' for n in uf)
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lmpc_hip.h"\nint main(void) {\n' + body + 'return 0; }\n')
    exe = tmp_path / "lay"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(Noise), ctypes.sizeof(Uncertainty), 0, 1] + [getattr(Noise, n).offset for n in nf] + \
        [getattr(Uncertainty, n).offset for n in uf]
    assert got == want
    assert nf[:2] == ["w", "dist"] and Noise.dist.offset == 4 and Noise.dist.size == 4
    if ctypes.sizeof(ctypes.c_void_p) == 8:
        assert ctypes.sizeof(Noise) == PREVIOUS_LAYOUT["sizeof(lmpc_noise)"]
        assert ctypes.sizeof(Uncertainty) == PREVIOUS_LAYOUT["sizeof(lmpc_uncertainty)"]
        assert {n: getattr(Noise, n).offset for n in nf if n != "dist"} == PREVIOUS_LAYOUT["lmpc_noise"]
        assert {n: getattr(Uncertainty, n).offset for n in uf} == PREVIOUS_LAYOUT["lmpc_uncertainty"]


# ------------------------------------------------------------------ Python arguments
def test_gaussian_and_scenario_arguments(lmpc):
    g = lmpc.Gaussian([0.0, 1.0], [0.5, 0.0])
    assert g.mean.shape == (2,) and g.std.shape == (2,) and g.dist == 1
    assert np.array_equal(lmpc.Gaussian(0.0, [1.0, 2.0]).mean, [0.0, 0.0])
    assert np.array_equal(lmpc.Gaussian([1.0, 2.0, 3.0], 0.1).std, [0.1, 0.1, 0.1])
    for mean, std in (([0.0], [-1.0]), ([float("nan")], [1.0]), ([0.0], [float("inf")]), ([0.0, 1.0], [1.0, 2.0, 3.0]),
                      (np.zeros((2, 2)), np.ones((2, 2)))):
        with pytest.raises(ValueError):
            lmpc.Gaussian(mean, std)
    sc = lmpc.Scenario(np.zeros((3, 2)), N=4, process_noise=g, measurement_noise=lmpc.Gaussian(0.0, 0.01))
    assert sc.process_noise is g and isinstance(sc.measurement_noise, lmpc.Gaussian)
    sc = lmpc.Scenario(np.zeros((3, 2)), N=4, process_noise=lmpc.Uniform([0.0], [1.0]), measurement_noise=g)
    assert sc.measurement_noise is g
    with pytest.raises(ValueError, match="noise and measurement_noise"):
        lmpc.Scenario(np.zeros(2), N=4, noise=np.zeros((1, 4)), measurement_noise=g)
    with pytest.raises(lmpc.LmpcError, match="lmpc_noise_draw_host: stream:"):
        lmpc.noise_draw(g, 2, 2, stream=3)


# ------------------------------------------------------------------ the reference module and the cases
def test_reference_imports_nothing_of_the_library():
    import ast
    import gaussian_reference as gr
    tree = ast.parse(open(gr.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names <= {"dataclasses", "numpy", "loop_reference", "nonlinear_reference", "uncertain_reference"}, names


def test_cases_cover_the_table():
    import gaussian_reference as gr
    assert sorted({c.base.nx for c in gr.STATES}) == list(range(1, 10))
    assert {(c.base.nx, c.base.cost) for c in gr.STATES} == {(nx, cost) for nx in range(1, 10) for cost in (False, True)}
    assert all(c.process == "gauss" and c.meas == "gauss" and c.base.S == 65 and c.base.T == 3 for c in gr.STATES)
    assert {c.base.observer for c in gr.STATES} == {False, True}
    assert {c.base.nw for c in gr.SHAPES} >= {0, 1, 3} and {c.base.ny for c in gr.SHAPES + gr.STATES} >= {1, 3}
    assert {(c.process, c.meas) for c in gr.SHAPES} >= {("gauss", "uniform"), ("uniform", "gauss"), ("gauss", "block"), ("block", "gauss")}
    assert any(c.base.scenario_offset > 2 ** 32 and c.base.step_offset for c in gr.SHAPES)
    assert (gr.SPLIT.base.S, gr.SPLIT.base.T) == (130, 6)
    assert (gr.NONLINEAR.S, gr.NONLINEAR.T) == (65, 20) and gr.NONLINEAR.process and gr.NONLINEAR.meas
    assert len({c.name for c in gr.CASES}) == len(gr.CASES)


def _all_cases():
    import gaussian_reference as gr
    return [pytest.param(c, id=c.name) for c in gr.CASES]


@pytest.mark.parametrize("case", _all_cases())
def test_case_conditions_on_the_host_reference(case):
    import gaussian_reference as gr
    import scenario_reference as sr
    data = gr.case_data(case)
    ldp = sr.host_ldp(data.prob)
    ref = gr.gaussian_run(case, ldp, data)
    gr.check_conditions(case, ref, ldp, data)
    assert ref.xs.shape == (case.base.T + 1, case.base.S, case.base.nx)
    # a drawn source run through the loop equals its restated block run through the loop: by construction here; the
    # uniform slot of a mixed case is drawn by the loop itself and must equal ITS block as well
    if "uniform" in (case.process, case.meas):
        kw = gr.ur.run_kwargs(case.base, data)
        name, stream = ("process", 0) if case.process == "uniform" else ("measurement_noise", 1)
        blk = gr.blocks(kw[name], kw["seed"], stream, kw["scenario_offset"], case.base.S, kw["step_offset"], case.base.T)
        again = gr.gaussian_run(case, ldp, data, **{name: blk})
        assert np.array_equal(again.xs, ref.xs) and np.array_equal(again.us, ref.us)


def test_nonlinear_case_conditions_on_the_host_reference(lmpc):
    import gaussian_reference as gr
    import nonlinear_reference as nr
    import scenario_reference as sr
    case, data = gr.NONLINEAR, gr.nonlinear_data()
    ldp = sr.host_ldp(data.prob)
    dims = {k: v for k, v in nr.CARTPOLE.items() if k != "Ts"}
    plant = lmpc.NonlinearPlant(lambda x, u, d, q: nr.cartpole(x, u, d, q, lmpc), Ts=nr.CARTPOLE["Ts"], C=nr.controller().C, **dims)
    ref = gr.nonlinear_gaussian_run(case, ldp, plant, data)
    quiet = gr.nonlinear_gaussian_run(case, ldp, plant, data, process=None, Gw=None, measurement_noise=None)
    assert ref.flags.min() >= 1
    assert (ref.active_sizes == 0).any() and (ref.active_sizes > 0).any()
    assert (ref.ws != 0).any(axis=(0, 1)).sum() >= 2 and not np.array_equal(ref.yms[0], quiet.yms[0])
    assert not (np.array_equal(ref.active, quiet.active) and np.array_equal(ref.flags, quiet.flags))
