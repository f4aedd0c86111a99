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
