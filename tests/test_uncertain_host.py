"""Host side of the scenario loop under uncertainty (no GPU): the generator's known answers and the properties of a
draw, the host reference loop (tests/uncertain_reference.py) against the plain one, sharded and continued runs, the
robust chapter's worst case, the refusals of lmpc_scenario_uncertain_check, and the conditions that keep the GPU cases
from passing emptily."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


# ------------------------------------------------------------------ the generator
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    import uncertain_reference as ur
    got = tuple(int(v) for v in ur.philox4x32_10(counter, key))
    assert got == want, [hex(v) for v in got]


def test_first_unit_of_the_all_zero_block():
    import uncertain_reference as ur
    r = ur.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert float(ur.unit(r[0], r[1])) == float.fromhex("0x1.989fa35785a70p-2")
    assert float(ur.units(0, [0], 0, 0, 1)[0, 0]) == float.fromhex("0x1.989fa35785a70p-2")
    # the largest pair stays below 1, the smallest is 0: [0, 1)
    assert float(ur.unit(0xffffffff, 0xffffffff)) == 1.0 - 2.0 ** -53 and float(ur.unit(0, 0x7ff)) == 0.0


def test_draws_stay_in_the_box():
    import uncertain_reference as ur
    g = np.arange(20000, dtype=np.uint64)
    lo = np.array([-0.3, 0.005, 1.0, -1e-3, 0.1])
    # lo == hi (the constant), a span of 2^-40 at 1, a span of three ulps
    hi = np.array([0.7, 0.005, 1.0 + 2.0 ** -40, 1e-3, 0.1 + 3 * np.spacing(0.1)])
    for k in (0, 5):
        e = ur.draw(12345, g, k, 0, lo, hi)
        assert e.shape == (20000, 5) and (e >= lo).all() and (e <= hi).all()
        assert np.array_equal(e[:, 1], np.full(20000, 0.005))
        assert len(np.unique(e[:, 0])) > 19000
    # spans of a few ulps, a span far below |lo|, a span that hi - lo rounds UP (1 - 2^-53 + 3 * 2^-55 -> 1.0): with the
    # largest u = 1 - 2^-53 the sum lands on hi or below (a search over 2 * 10^7 random boxes found no sum beyond hi; the
    # min is what makes the bound hold whatever the rounding does)
    u = 1.0 - 2.0 ** -53
    lo = np.array([0.1, 1e6, -3 * 2.0 ** -55, 1.0, -1.0 / 3.0])
    hi = np.array([0.1 + 3 * np.spacing(0.1), 1e6 + 1e-9, 1.0 - 2.0 ** -53, 3.0, 1.0 / 3.0])
    e = np.minimum(hi, lo + u * (hi - lo))
    assert (e >= lo).all() and (e <= hi).all() and e[3] == 3.0
    e = ur.draw(7, g, 1, 1, lo, hi)
    assert (e >= lo).all() and (e <= hi).all()


def test_unit_statistics_components_and_streams():
    import uncertain_reference as ur
    g = np.arange(100000, dtype=np.uint64)
    u = ur.units(2024, g, 3, 0, 2)
    assert abs(u[:, 0].mean() - 0.5) < 0.005 and abs(u[:, 1].mean() - 0.5) < 0.005      # 5 sigma, sigma = 0.00091
    assert (u >= 0).all() and (u < 1).all()
    assert not np.array_equal(u[:, 0], u[:, 1]) and (u[:, 0] != u[:, 1]).mean() > 0.999    # components 2j and 2j + 1
    v = ur.units(2024, g, 3, 1, 2)
    assert (u != v).mean() > 0.999                                                         # streams 0 and 1
    assert (ur.units(2024, g, 4, 0, 2) != u).mean() > 0.999 and (ur.units(2025, g, 3, 0, 2) != u).mean() > 0.999
    # components 2 and 3 come from the block of pair index 1, component 2 of an odd count from half of it
    w5, w3 = ur.units(2024, g[:100], 3, 0, 5), ur.units(2024, g[:100], 3, 0, 3)
    assert np.array_equal(w5[:, :3], w3) and np.array_equal(w5[:, :2], u[:100])
    # the global scenario index beyond 2^32 reaches counter word 1
    big = ur.units(1, np.array([5, 5 + 2 ** 32], np.uint64), 0, 0, 1)
    assert big[0, 0] != big[1, 0]


# ------------------------------------------------------------------ the reference loop
def _setup(case):
    import scenario_reference as sr
    import uncertain_reference as ur
    data = ur.case_data(case)
    return data, sr.host_ldp(data.prob)


FIELDS = ("xs", "us", "xhats", "yms", "ys", "ds", "thetas", "flags", "active", "flag_min", "xhat_final", "uprev_final")


def test_every_source_off_equals_the_plain_reference():
    import scenario_reference as sr
    import uncertain_reference as ur
    for case in (ur.PLAIN, ur.COST[0]):
        data, ldp = _setup(case)
        kw = ur.run_kwargs(case, data)
        for k in ("process", "measurement_noise", "Gw", "seed", "scenario_offset", "step_offset", "plants", "plant_index"):
            kw.pop(k)
        a, b = ur.uncertain_run(ldp, **kw), sr.reference_run(ldp, **kw)
        for f in FIELDS + (("cost", "violation") if case.cost else ()):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (case.name, f)
        assert a.ws is None


def test_sharding_by_scenario_offset():
    import uncertain_reference as ur
    case = ur.SHARD
    data, ldp = _setup(case)
    whole = ur.run_case(case, ldp, data)
    kw = ur.run_kwargs(case, data)
    cut = lambda a, sl: a if (a is None or isinstance(a, ur.Box) or a.ndim == 2) else a[sl]
    for sl, off in ((slice(0, 500), 0), (slice(500, 1000), 500)):
        part = dict(kw)
        for k in ("r", "d", "p", "noise", "process", "measurement_noise"):
            part[k] = cut(kw[k], sl)
        part["x0"] = kw["x0"][sl]
        part["scenario_offset"] = case.scenario_offset + off
        half = ur.uncertain_run(ldp, **part)
        for f in ("xs", "us", "xhats", "yms", "ws"):
            assert np.array_equal(getattr(half, f), getattr(whole, f)[:, sl]), (off, f)
    # ... and the offset matters: the second half run as scenarios 0 .. 499 differs
    part["scenario_offset"] = case.scenario_offset
    assert not np.array_equal(ur.uncertain_run(ldp, **part).ws, whole.ws[:, 500:])


def test_continuation_by_step_offset():
    import uncertain_reference as ur
    case = ur.CONTINUE
    data, ldp = _setup(case)
    whole = ur.run_case(case, ldp, data)
    kw = ur.run_kwargs(case, data)
    kw["T"] = 3
    first = ur.uncertain_run(ldp, **kw)
    shift = lambda a: None if a is None else a[..., 3:]
    second = ur.uncertain_run(ldp, **{**kw, "x0": first.xs[-1], "xhat0": first.xhat_final, "uprev0": first.uprev_final,
                                      "r": shift(kw["r"]), "d": shift(kw["d"]), "step_offset": case.step_offset + 3})
    for f in ("us", "xhats", "yms", "ys", "ws"):
        assert np.array_equal(np.concatenate([getattr(first, f), getattr(second, f)]), getattr(whole, f)), f
    assert np.array_equal(np.concatenate([first.xs, second.xs[1:]]), whole.xs)
    again = ur.uncertain_run(ldp, **{**kw, "x0": first.xs[-1], "xhat0": first.xhat_final, "uprev0": first.uprev_final,
                                     "r": shift(kw["r"]), "d": shift(kw["d"])})
    assert not np.array_equal(again.ws, whole.ws[3:])         # without the offset the second part repeats the first's draws
    assert np.array_equal(again.ws, first.ws)


def test_robust_chapter_worst_case():
    # docs/src/manual/robust.md:17,78 / example/robust.jl:5,25 on the nominal controller: the soft bound y <= 0.5 holds
    # without w and is broken by the worst case w = +0.005 on both states (max y = 0.5601, final y = 0.5050)
    import scenario_reference as sr
    import uncertain_reference as ur
    p = ur.robust_problem()
    dims, previews = sr.dims_of(p)
    ldp = sr.host_ldp(p)
    kw = dict(dims=dims, plant=sr.plant_of(p), x0=np.zeros((1, 2)), T=100, r=np.array([[0.5]]), previews=previews)
    quiet = ur.uncertain_run(ldp, **kw)
    assert quiet.ys.max() < 0.5 + 1e-9 and quiet.flags.min() >= 1
    worst = ur.uncertain_run(ldp, process=ur.Box(np.full(2, 0.005), np.full(2, 0.005)), **kw)
    assert worst.ys.max() > 0.55 and worst.flags.min() >= 1
    assert np.array_equal(np.unique(worst.ws), [0.005])
    # the same loop in exact arithmetic, the plant's f_offset moved by w: the two figures to the four digits quoted (the
    # two loops round differently, and the solver's tolerances sit between a last-bit difference and y)
    off = sr.plant_of(p)
    off.f_offset = off.f_offset + 0.005
    moved = ur.uncertain_run(ldp, **{**kw, "plant": off})
    assert abs(moved.ys.max() - 0.5601) < 1e-4 and abs(moved.ys[-1, 0, 0] - 0.5050) < 1e-4
    assert abs(worst.ys.max() - 0.5601) < 1e-4 and abs(worst.ys[-1, 0, 0] - 0.5050) < 1e-4


# ------------------------------------------------------------------ the refusals of the C check
def _desc(lmpc, nx=2, nu=1, nd=1, ny=1, r=(1, 0), d=(1, 0), noise=(0, 0), nuprev=0, use_observer=0):
    """A well-formed descriptor for a handle with nth = 2 + 1 + 1 = 4, nout = 1"""
    from linearmpc_jl_amd._cabi import Block, ScenarioSim
    keep = np.zeros(64)
    s = ScenarioSim()
    s.nx, s.nu, s.nd, s.ny = nx, nu, nd, ny
    s.plant = keep.ctypes.data
    s.measurement = keep.ctypes.data
    for name, (w, H) in (("r", r), ("d", d), ("p", (0, 0)), ("noise", noise)):
        setattr(s, name, Block(None, 0, w, 1, 0, H))
    s.nuprev, s.use_observer, s.warm = nuprev, use_observer, 0
    s._keep = keep
    return s


def _un(pw=2, mw=1, plo=(-1.0, -1.0), phi=(1.0, 1.0), mlo=None, mhi=None, Gw=None, pH=0, mH=0, n_plants=0, plants=False,
        plant_index=False, W=False, step_offset=0):
    from linearmpc_jl_amd._cabi import Block, Uncertainty
    un, keep = Uncertainty(), []

    def vec(a):
        if a is None:
            return None
        keep.append(np.ascontiguousarray(np.asarray(a, float)))
        return keep[-1].ctypes.data

    un.process.w, un.process.lo, un.process.hi = pw, vec(plo), vec(phi)
    un.process.src = Block(None, 0, pw, 1, 0, pH)
    un.measurement.w, un.measurement.lo, un.measurement.hi = mw, vec(mlo), vec(mhi)
    un.measurement.src = Block(None, 0, mw, 1, 0, mH)
    un.Gw = vec(Gw)
    un.n_plants = n_plants
    un.plants = vec(np.zeros(64)) if plants else None
    un.plant_index = vec(np.zeros(8)) if plant_index else None     # (never read: the check needs no device)
    un.W_traj = vec(np.zeros(8)) if W else None
    un.step_offset = step_offset
    un._keep = keep
    return un


def _check(lmpc, s, un, nth=4, nout=1, obs=None):
    from linearmpc_jl_amd._cabi import Observer, last_error
    o = None if obs is None else ctypes.byref(Observer(*obs, None, None, None))
    rc = lmpc.lib().lmpc_scenario_uncertain_check(nth, nout, o, ctypes.byref(s) if s is not None else None,
                                                  ctypes.byref(un) if un is not None else None)
    return rc, last_error(None)


def test_symbols_are_exported_and_bound(lmpc):
    L = lmpc.lib()
    for name in ("lmpc_scenario_uncertain_check", "lmpc_simulate_scenario_uncertain_device", "lmpc_simulate_scenario_uncertain"):
        assert name in lmpc.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.lmpc_abi_version() == 2
    assert hasattr(lmpc, "Uniform") and "Uniform" in lmpc.__all__
    assert hasattr(lmpc.BatchedQP, "simulate_scenario_uncertain")


def test_well_formed_descriptors_pass(lmpc):
    assert _check(lmpc, _desc(lmpc), _un())[0] == 1
    assert _check(lmpc, _desc(lmpc), _un(pw=0, mw=0, plo=None, phi=None))[0] == 1            # every source absent
    assert _check(lmpc, _desc(lmpc), _un(pw=3, plo=(0,) * 3, phi=(1,) * 3, Gw=np.ones(6)))[0] == 1
    assert _check(lmpc, _desc(lmpc), _un(plo=(0.5, 0.5), phi=(0.5, 0.5), W=True))[0] == 1     # lo == hi
    assert _check(lmpc, _desc(lmpc), _un(plo=None, phi=None, mlo=(-1.0,), mhi=(1.0,)))[0] == 1
    assert _check(lmpc, _desc(lmpc), _un(n_plants=3, plants=True, plant_index=True))[0] == 1
    assert _check(lmpc, _desc(lmpc, noise=(1, 0)), _un(mw=0))[0] == 1                         # s->noise with process noise
    assert _check(lmpc, _desc(lmpc), _un(step_offset=2 ** 31 - 1))[0] == 1                    # (T is the call's)


@pytest.mark.parametrize("field,desc,un", [
    ("un", {}, None),
    ("process.w", {}, dict(pw=-1)),
    ("measurement.w", {}, dict(mw=-2)),
    ("process.w", {}, dict(pw=1, plo=(0.0,), phi=(1.0,))),                  # Gw NULL and nw not in {0, nx}
    ("process.w", {}, dict(pw=3, plo=None, phi=None)),
    ("measurement.w", {}, dict(mw=2)),                                      # not in {0, ny}
    ("measurement.w", dict(noise=(1, 0)), {}),                              # together with s->noise
    ("process.hi", {}, dict(phi=None)),
    ("process.lo", {}, dict(plo=None)),
    ("measurement.hi", {}, dict(mlo=(0.0,))),
    ("measurement.lo", {}, dict(mhi=(0.0,))),
    ("process.lo", {}, dict(plo=(0.0, 2.0))),                               # lo_1 > hi_1
    ("process.lo", {}, dict(plo=(float("nan"), 0.0))),
    ("process.hi", {}, dict(phi=(1.0, float("inf")))),
    ("measurement.lo", {}, dict(mlo=(float("-inf"),), mhi=(0.0,))),
    ("process.src.H", {}, dict(pH=3)),
    ("measurement.src.H", {}, dict(mH=1)),
    ("n_plants", {}, dict(n_plants=-1)),
    ("plants", {}, dict(n_plants=2)),
    ("plant_index", {}, dict(plant_index=True)),
    ("W_traj", {}, dict(pw=0, plo=None, phi=None, W=True)),
    ("step_offset", {}, dict(step_offset=-1)),
    # everything lmpc_scenario_check refuses, through the same code
    ("nx", dict(nx=0), {}),
    ("nu", dict(nu=2), {}),
    ("d.w", dict(d=(2, 0)), {}),
    ("noise.H", dict(noise=(1, 4)), dict(mw=0)),
    ("nth", dict(nuprev=1), {}),
    ("use_observer", dict(use_observer=1), {}),
])
def test_every_refusal_names_its_field(lmpc, field, desc, un):
    rc, msg = _check(lmpc, _desc(lmpc, **desc), None if un is None else _un(**un))
    assert rc == -100, (rc, msg)
    assert msg.startswith("lmpc_scenario_uncertain_check: " + field + ":"), msg


def test_null_descriptor_and_texts(lmpc):
    assert _check(lmpc, None, _un())[1].startswith("lmpc_scenario_uncertain_check: s:")
    assert "must be nx = 2 (or 0: none) without Gw, got 3" in _check(lmpc, _desc(lmpc), _un(pw=3, plo=None, phi=None))[1]
    assert "lo > hi at component 1" in _check(lmpc, _desc(lmpc), _un(plo=(0.0, 2.0)))[1]


def test_struct_layouts_match_the_header(lmpc, tmp_path):
    import os, shutil, subprocess
    from conftest import ROOT
    from linearmpc_jl_amd._cabi import Noise, Uncertainty
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    nf = [n for n, _ in Noise._fields_]
    uf = [n for n, _ in Uncertainty._fields_]
    body = 'printf("%zu %zu\\n", sizeof(lmpc_noise), sizeof(lmpc_uncertainty));\n'
    body += "".join(f'printf("%zu\\n", offsetof(lmpc_noise, {n}));\n' for n in nf)
    body += "".join(f'printf("%zu\\n", offsetof(lmpc_uncertainty, {n}));\n' for n in uf)
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lmpc_hip.h"\nint main(void) {\n' + body + 'return 0; }\n')
    exe = tmp_path / "lay"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(Noise), ctypes.sizeof(Uncertainty)] + [getattr(Noise, n).offset for n in nf] + \
        [getattr(Uncertainty, n).offset for n in uf]
    assert got == want


def test_scenario_and_simulation_arguments(lmpc):
    u = lmpc.Uniform([-1.0, 0.0], [1.0, 0.0])
    assert u.lo.shape == (2,)
    with pytest.raises(ValueError):
        lmpc.Uniform([0.0, 1.0], [1.0, 0.5])
    with pytest.raises(ValueError):
        lmpc.Uniform([0.0], [float("inf")])
    sc = lmpc.Scenario(np.zeros((3, 2)), N=4, process_noise=u, measurement_noise=np.zeros((3, 1, 4)))
    assert sc.process_noise is u and sc.measurement_noise.shape == (3, 1, 4) and sc.noise is None
    assert lmpc.Scenario(np.zeros(2), 5, None, None, None, np.zeros((1, 5))).noise.shape == (1, 5)   # positional noise
    with pytest.raises(ValueError, match="noise and measurement_noise"):
        lmpc.Scenario(np.zeros(2), N=4, noise=np.zeros((1, 4)), measurement_noise=u)
    with pytest.raises(ValueError, match="process_noise must have shape"):
        lmpc.Scenario(np.zeros((3, 2)), N=4, process_noise=np.zeros((2, 2, 4)))


# ------------------------------------------------------------------ the reference module and the cases
def test_reference_loop_imports_nothing_of_the_library():
    import ast
    import uncertain_reference as ur
    tree = ast.parse(open(ur.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names <= {"dataclasses", "types", "numpy", "oracle", "scenario_reference"}, names


def test_cases_cover_the_table():
    import uncertain_reference as ur
    assert [c.nx for c in ur.STATES] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 32]
    assert all(c.observer == (c.nx % 2 == 1) and c.process == "draw" and c.meas == "draw" for c in ur.STATES)
    assert {c.nw for c in ur.DRAWS} >= {0, 1, 2, 3, 5} and {c.ny for c in ur.DRAWS + ur.STATES} >= {1, 3}
    assert {c.process for c in ur.DRAWS} == {None, "draw", "block", "shared"}
    assert {(c.process, c.meas) for c in ur.DRAWS} >= {("draw", "block"), ("block", "draw")}
    assert any(c.noise and c.process == "draw" for c in ur.DRAWS)
    assert {c.plants for c in ur.ENSEMBLES} >= {1, 2, 3, 300} and any(c.index for c in ur.ENSEMBLES)
    assert any(c.scenario_offset and c.plants and not c.index for c in ur.ENSEMBLES)
    assert {c.nd for c in ur.ENSEMBLES} == {0, 2}
    assert {(c.S, c.T) for c in ur.SIZES} == {(S, T) for S in (1, 255, 256, 257, 1000) for T in (1, 2)}
    assert len({c.name for c in ur.CASES}) == len(ur.CASES)


def _all_cases():
    import uncertain_reference as ur
    return [pytest.param(c, id=c.name) for c in ur.CASES]


@pytest.mark.parametrize("case", _all_cases())
def test_case_conditions_on_the_host_reference(case):
    import uncertain_reference as ur
    data, ldp = _setup(case)
    ref = ur.run_case(case, ldp, data)
    ur.check_conditions(case, ref, ldp, data)
    assert ref.xs.shape == (case.T + 1, case.S, case.nx)
    if case.process is not None:
        assert ref.ws.shape == (case.T, case.S, case.nx)
