"""What a closed loop tells a launch never outlives the loop, and the probe of a fresh wavefront-kernel handle -- the one
launch that has to be a plain cold solve whatever runs around it -- leaves results, profiling and the loop alone.

1. The probe on a plain solve: a fresh handle with default options and profiling on solves 4 x kProbe points twice; its
   launch records show the probe once, in front of the first batch, and no event of it; the results are those of a handle
   that never probes and of the oracle.
2. The probe inside lmpc_simulate_device, cold and warm: the loop of a probing handle equals the loop of one that does
   not probe, and the handle then solves a plain batch like the oracle.
3. Every form in turn on one lane-kernel and one wavefront-kernel handle with profiling on: plain solve, lmpc_simulate in
   every execution mode, plain solve, the generated controller's call fused and not, a warm plain solve, a plain solve.
   The cold plain solves equal the first one bit for bit -- results, front-pass / wavefront / one-launch records (all
   words but `seq`), kernel name and the first-pass capacity lmpc_wave_stats reports -- and the oracle; the warm one
   equals the oracle's warm solve; every loop equals tests/loop_reference.py; lmpc_profile_read counts exactly the calls
   that bracket (the scenario-asynchronous loop records none).

Every comparison is np.array_equal: results never depend on how a batch is split into passes."""
import dataclasses
import glob
import os
import re

import numpy as np
import pytest

import loop_reference as lr
import test_gpu_loops as tgl
import test_gpu_wave as tw
import wave_cases as wc
from conftest import ROOT, oracle_ldp_from

pytestmark = pytest.mark.gpu

K_PROBE = 16384            # linearmpc.jl_amd/csrc: `constexpr int64_t kProbe` (test_the_probe_constant reads it from the source)
N_BIG = 4 * K_PROBE        # the smallest batch a fresh handle probes
N_REF = 300


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def test_the_probe_constant_is_the_one_the_tests_assume():
    found = []
    for path in glob.glob(os.path.join(ROOT, "linearmpc.jl_amd", "csrc", "*.hpp")):
        found += re.findall(r"constexpr\s+int64_t\s+kProbe\s*=\s*(\d+)\s*;", open(path).read())
    assert found == [str(K_PROBE)], found


def _fresh(lmpc, probe):
    """wave_cases.TWO_PASS (n = 48, m = 100, nth = 5, capacity 49: the smallest case the probe acts on) on a handle that
    keeps every default but, with probe false, "wave_probe" """
    case = wc.TWO_PASS
    H, f, f_theta, A, bu, bl, W, sense = wc.problem(case)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, senses=sense, nout=1, settings=tw._settings(lmpc, case))
    if not probe:
        qp.set_option("wave_probe", 0)
    assert qp.kernel_name.endswith("wave"), qp.kernel_name
    assert (qp.n, qp.m, qp.nth, qp.nout) == (case.n, case.m, case.nth, 1) and min(case.n + 1, 64) >= 40
    qp._oset = tw._oset(tw._settings(lmpc, case))
    return qp


def _big_theta():
    th = wc.two_pass_theta("mixed")
    return th, np.ascontiguousarray(np.tile(th, (-(-N_BIG // len(th)), 1))[:N_BIG])


def _oracle_mixed(qp):
    th = wc.two_pass_theta("mixed")
    return tw._cached((wc.TWO_PASS, "mixed"), lambda: tw._oracle(qp, wc.TWO_PASS, th))


def _last_seq(recs):
    return recs[-1]["seq"] if recs else 0


# ------------------------------------------------------------------ 1: the probe on a plain solve
def test_probe_in_front_of_a_plain_solve(lmpc):
    case = wc.TWO_PASS
    th400, th = _big_theta()
    a, b = _fresh(lmpc, True), _fresh(lmpc, False)
    a.profile(True)
    # first call: the probe's launches (kProbe points) ahead of the batch's own
    a1, recs1 = tw._solve(a, case, th)
    fronts1, rows1 = a.front_pass_info(), a.row_launch_info()
    print("first call:", recs1, fronts1, rows1)
    probe = [r for r in recs1 if r["nprob"] == K_PROBE]
    batch = [r for r in recs1 if r["nprob"] == N_BIG]
    assert probe and batch and recs1 == probe + batch, recs1
    assert all(r["pass"] == 0 and r["SIM"] == 0 for r in probe), probe
    assert [r["nprob"] for r in fronts1] == [K_PROBE, N_BIG], fronts1
    assert all(r["nprob"] == N_BIG for r in rows1), rows1
    # second call of the same batch: the lifetime counts grow by the batch's launches alone
    seq1 = tw._seq(a)
    a2, recs2 = tw._solve(a, case, th)
    fronts2, rows2 = a.front_pass_info(_last_seq(fronts1)), a.row_launch_info(_last_seq(rows1))
    print("second call:", recs2, fronts2, rows2)
    assert recs2 and all(r["nprob"] == N_BIG for r in recs2) and tw._seq(a) - seq1 == len(recs2) <= 2, recs2
    assert [r["nprob"] for r in fronts2] == [N_BIG], fronts2
    assert len(rows2) <= 1 and all(r["nprob"] == N_BIG for r in rows2), rows2
    # two bracketed calls: the probe records no events
    assert a.profile_read()[0] == 2
    # the handle that never probes
    b1, recsb = tw._solve(b, case, th)
    assert recsb and all(r["nprob"] == N_BIG for r in recsb), recsb
    assert [r["nprob"] for r in b.front_pass_info()] == [N_BIG]
    b2, _ = tw._solve(b, case, th)
    for got, what in ((a1, "A, first call"), (a2, "A, second call"), (b2, "B, second call")):
        tw._same(got, b1, N_BIG, what)
    ref = _oracle_mixed(b)
    for got, what in ((a1, "A, first call"), (b1, "B, first call")):
        tw._same(tuple(v[:N_REF] for v in got), ref, N_REF, what + ", the oracle")
    a.check()
    b.check()
    a.close()
    b.close()


# ------------------------------------------------------------------ 2: the probe inside a loop
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_probe_inside_a_closed_loop(lmpc, warm):
    case = wc.TWO_PASS
    th400, x0 = _big_theta()
    nx, T = case.nth, 2
    F, G = 0.5 * np.eye(nx), np.zeros((nx, 1))
    a, b = _fresh(lmpc, True), _fresh(lmpc, False)
    got_a = tw._simulate_device(lmpc, a, x0, T, F, G, warm)
    got_b = tw._simulate_device(lmpc, b, x0, T, F, G, warm)
    # (the probe's screening pass is the one front pass whose batch is kProbe points; the ring keeps the last four)
    fa, fb = a.front_pass_info(), b.front_pass_info()
    print("front passes:", fa, fb, "wavefront launches:", a.wave_launch_info(), b.wave_launch_info())
    assert any(r["nprob"] == K_PROBE for r in fa) and not any(r["nprob"] == K_PROBE for r in fb), (fa, fb)
    for key in ("U", "X", "flag_min", "x"):
        assert got_a[key].shape == got_b[key].shape and np.array_equal(got_a[key], got_b[key]), \
            (warm, key, np.argwhere(got_a[key] != got_b[key])[:4].tolist())
    assert np.array_equal(got_a["X"][0], x0) and not np.array_equal(got_a["X"][1], got_a["X"][2]) and got_a["U"].any()
    ref = _oracle_mixed(b)
    for qp, what in ((a, "A"), (b, "B")):
        got, recs = tw._solve(qp, case, th400[:N_REF])
        assert recs and all(r["SIM"] == 0 and r["nprob"] == N_REF for r in recs), (what, recs)
        tw._same(got, ref, N_REF, what + ": plain solve after the loop")
        qp.check()
        qp.close()


# ------------------------------------------------------------------ 3: every form in turn, profiling on
SIM_DEFAULTS = dict(sim_small=1, sim_blind=2, sim_async=1, sim_fused=1, sim_keep_factor=1)


def _strip(recs):
    return [{k: v for k, v in r.items() if k != "seq"} for r in recs]


def _plain(qp, theta, warm=None):
    """One plain device solve with every output: (results, what the call left in the launch records, handle state)"""
    import torch
    dev = torch.device("cuda", qp.device)
    f0, w0 = _last_seq(qp.front_pass_info()), tw._seq(qp)
    fast0 = (qp.fast_launch_info() or dict(seq=0))["seq"]
    th = torch.from_numpy(np.ascontiguousarray(theta)).to(dev)
    it = torch.empty(len(theta), dtype=torch.int32, device=dev)
    act = torch.zeros((len(theta), qp.words), dtype=torch.int64, device=dev)
    w = None if warm is None else torch.from_numpy(np.ascontiguousarray(warm).view(np.int64)).to(dev)
    x, ef = qp.solve_device(th, iters=it, active=act, warm=w)
    torch.cuda.synchronize(dev)
    qp.check()
    fast = qp.fast_launch_info() or dict(seq=0)
    recs = dict(front=_strip(qp.front_pass_info(f0)), wave=_strip(qp.wave_launch_info(w0)),
                fast=_strip([fast]) if fast["seq"] > fast0 else [], fast_launches=fast["seq"] - fast0)
    # (the first-pass capacity of a plain call, read with "wave_two_pass" 1: "wave_cap1" rows wherever two passes are
    # possible, whatever the working-set statistics have grown to -- and 0 if the question still saw a warm run-ahead loop)
    qp.set_option("wave_two_pass", 1)
    state = (qp.kernel_name, qp.wave_stats()["first_pass_rows"])
    qp.set_option("wave_two_pass", -1)
    x, ef, it, act = (t.cpu().numpy() for t in (x, ef, it, act))
    return (x, ef, it, act.view(np.uint64)), recs, state


def _forms_in_turn(lmpc, case, modes, wave):
    import torch
    from oracle import ldp as oldp
    data = lr.loop_data(case)
    qp = tgl._handle(lmpc, data, wave=wave)
    L = oracle_ldp_from(qp.ldp())
    ref = lr.run_loop_case(case, L, data)
    lr.check_loop_conditions(case, ref)
    kept = None
    theta = tgl._probe_theta(case, data, case.S)
    want = oldp.solve_batch(L, theta)
    assert (want[1] >= 1).all() and 0.05 < (lr.popcount(want[3]) > 0).mean() < 0.95
    names = ("x", "exitflag", "iterations", "active")
    qp.profile(True)
    brackets = 0

    def cold(what, first=None):
        got, recs, state = _plain(qp, theta)
        for g, r, name in zip(got, want, names):
            assert np.array_equal(g, r), (case.name, what, name, "against the oracle")
        assert len(recs["front"]) + recs["fast_launches"] == 1 and (len(recs["wave"]) >= 1) == wave, (what, recs)
        if first is not None:
            for g, r, name in zip(got, first[0], names):
                assert np.array_equal(g, r), (case.name, what, name, "against the first solve")
            assert recs == first[1], (case.name, what, "launch records", recs, first[1])
            assert state == first[2], (case.name, what, "kernel name / first-pass capacity", state, first[2])
        return got, recs, state

    # 1: a plain solve
    first = cold("1: plain solve")
    brackets += 1
    print(case.name, first[1], first[2])
    assert first[2][1] == (24 if wave else 0), first[2]       # (the wavefront case's capacity is 49: a first pass is possible)
    # 2: lmpc_simulate in every mode (the rounds record no events; a lock-step loop brackets each of its T solves)
    nth = case.nx + data.nr + data.nup
    for opts in modes:
        o = {**SIM_DEFAULTS, **opts}
        for k, v in o.items():
            qp.set_option(k, v)
        exp = ref
        if wave and case.warm and o["sim_keep_factor"] and case.T > 1:
            kept = oldp.simulate(L, data.x0, case.T, data.F, data.G, r=data.r, uprev=data.uprev, warm=2) if kept is None else kept
            exp = kept
        out = qp.simulate(data.x0, case.T, data.F, data.G, r=data.r, uprev=data.uprev, warm=case.warm)
        tgl._same(out, exp, (case.name, opts))
        # (mirrors `asyncLoop` of lmpc_simulate_device at these cases: nx <= 8, nth <= 16, nu <= kMaxSimU, a screening pass)
        assert case.nx <= 8 and nth <= 16 and case.nu <= lr.K_MAX_SIM_U
        rounds = o["sim_async"] == 2 if wave else bool(o["sim_async"] and o["sim_fused"])
        brackets += 0 if rounds else case.T
    for k, v in SIM_DEFAULTS.items():
        qp.set_option(k, v)
    # 3: a plain solve
    cold("3: plain solve after the loops", first)
    brackets += 1
    # 4: the generated controller's call, fused into the screening pass and not
    nx, nr, nup, nu = case.nx, data.nr, data.nup, case.nu
    qp.set_parameter_layout(nx, nr, 0, nup, 0)
    rng = np.random.default_rng(77 + case.seed)
    S = case.S
    state_, refr, u0 = theta[:, :nx], theta[:, nx:nx + nr], rng.uniform(-0.3, 0.3, (S, nu))
    th_cc = lr.update_parameter_reference(S, nu, nx, nr, 0, nup, 0, control=u0, state=state_, reference=refr)
    xo, efo, _, _ = oldp.solve_batch(L, th_cc)
    dev = torch.device("cuda", qp.device)
    t = lambda v: None if v.shape[1] == 0 else torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    for fused in (1, 0):
        qp.set_option("cc_fused", fused)
        c = torch.from_numpy(u0.copy()).to(dev)
        ef = qp.compute_control_device(c, t(state_), t(refr))
        torch.cuda.synchronize(dev)
        assert np.array_equal(c.cpu().numpy(), xo) and np.array_equal(ef.cpu().numpy(), efo), (case.name, "cc_fused", fused)
        brackets += 1
    qp.set_option("cc_fused", 1)
    # 5: a warm plain solve (from the neighbouring points' final sets): the oracle's warm solve
    masks = wc.warm_masks(want[1], want[3])
    got, _, _ = _plain(qp, theta, warm=masks)
    for g, r, name in zip(got, oldp.solve_batch(L, theta, warm=masks), names):
        assert np.array_equal(g, r), (case.name, "5: warm plain solve", name)
    brackets += 1
    # 6: a plain solve
    cold("6: plain solve at the end", first)
    brackets += 1
    assert qp.profile_read()[0] == brackets, (case.name, brackets)
    qp.check()
    qp.close()


def test_lane_handle_every_form_in_turn_with_profiling_on(lmpc):
    # 257 scenarios: a second tile of the screening pass
    case = dataclasses.replace({c.name: c for c in lr.SIM_LANE}["sim-lane-nx4-warm"], S=257, pool=1000)
    _forms_in_turn(lmpc, case, tgl.LANE_MODES, wave=False)


def test_wave_handle_every_form_in_turn_with_profiling_on(lmpc):
    case = {c.name: c for c in lr.SIM_WAVE}["sim-wave-nx4-warm"]
    assert case.S == 100
    _forms_in_turn(lmpc, case, tgl.WAVE_MODES, wave=True)
