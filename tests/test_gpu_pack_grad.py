"""Gradient with respect to the pack on the GPU (lmpc_solve_pack_vjp_device, BatchedQP.solve_pack_vjp*, solve_mpqp_autograd):
every case of pack_grad_cases.py, the launch record first, then the seven sums, thbar and status value for value
(np.array_equal) against the numpy restatement of the contract (pack_grad_reference.py) on guarded outputs -- every
batch size, each capacity of the lane kernel and the forced list pass, the smallest and the default slab -- and the chain
from the solver's own masks, outputs left out one at a time, call sequences on one handle and the autograd function."""
import numpy as np
import pytest

import pack_grad_cases as pc
import pack_grad_reference as pr
import sens_cases as sc

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _data(lmpc, case):
    """Handle, its pack, the case's batch on that pack and the reference's per-point results (once per case); the sums
    of a prefix are made on first use."""
    if case.name not in _CACHE:
        H, f, f_theta, A, bu, bl, W, sense = sc.problem(case)
        qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=case.nout, device=0)
        S = lmpc.default_settings()
        pack = qp.ldp()
        b = pc.build(case, pack)
        cache = pr.derived(pack)
        solved = pr.point_solve(pack, b["theta"], b["active"], b["exitflag"], b["xbar"], S.rho_soft, S.zero_tol, cache)
        _CACHE[case.name] = dict(case=case, qp=qp, pack=pack, batch=b, cache=cache, solved=solved, S=S, refs={})
    return _CACHE[case.name]


def _ref(d, N):
    if N not in d["refs"]:
        b = d["batch"]
        d["refs"][N] = pr.pack_vjp(d["pack"], b["theta"][:N], b["active"][:N], b["exitflag"][:N], b["xbar"][:N],
                                   solved=pr.prefix(d["solved"], N))
        if N == pc.N_COND:
            pc.check_conditions(d["case"], d["pack"], b, d["refs"][N])
    return d["refs"][N]


def _call(torch, d, N, option=0, force=False, slab=0, want=pc.NAMES, want_thbar=True):
    """One device call on the first N points with guarded outputs.  Asserts the launch record, the guards and that every
    entry was written; returns the results as numpy arrays."""
    qp, pack, b = d["qp"], d["pack"], d["batch"]
    G = sc.GUARD
    dev = torch.device("cuda", 0)
    shp = pc.shapes(pack)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    th, xb, ef = up(b["theta"][:N]), up(b["xbar"][:N]), up(b["exitflag"][:N])
    act = up(b["active"][:N].view(np.int64))
    bufs = {k: torch.full((int(np.prod(shp[k])) + 2 * G,), sc.SENT, dtype=torch.float64, device=dev) for k in want}
    outs = {k: v[G:len(v) - G].view(shp[k]) for k, v in bufs.items()}
    thbar = torch.full((N + 2 * G, pack["nth"]), sc.SENT, dtype=torch.float64, device=dev) if want_thbar else None
    status = torch.full((N + 2 * G,), sc.SENT_I, dtype=torch.int32, device=dev)
    qp.set_option("sens_cap", option)
    qp.set_option("sens_force_list", int(force))
    qp.set_option("pack_grad_slab", slab)
    seen = qp.pack_grad_launch_info()
    since = seen[-1]["seq"] if seen else 0
    qp.solve_pack_vjp_device(th, act, ef, xb, status=status[G:N + G], out=outs, want=want,
                             thbar=thbar[G:N + G] if want_thbar else None)
    torch.cuda.synchronize()
    qp.check()
    rec = qp.pack_grad_launch_info(since)
    assert len(rec) == 1 and rec[0]["seq"] == since + 1
    exp = pc.expected_record(pack, N, option, force, slab, torch.cuda.get_device_properties(0).multi_processor_count, bool(want))
    got = {k: rec[0][k] for k in exp}
    assert got == exp, (got, exp)
    assert rec[0]["scratch_kib"] > 0
    res = {}
    for k, v in bufs.items():
        a = v.cpu().numpy()
        assert (a[:G] == sc.SENT).all() and (a[len(a) - G:] == sc.SENT).all(), f"a guard of {k}-bar was written"
        assert not (a[G:len(a) - G] == sc.SENT).any(), f"an entry of {k}-bar was not written"
        res[k] = a[G:len(a) - G].reshape(shp[k])
    st = status.cpu().numpy()
    assert (st[:G] == sc.SENT_I).all() and (st[N + G:] == sc.SENT_I).all() and not (st[G:N + G] == sc.SENT_I).any()
    res["status"] = st[G:N + G]
    if want_thbar:
        t = thbar.cpu().numpy()
        assert (t[:G] == sc.SENT).all() and (t[N + G:] == sc.SENT).all() and not (t[G:N + G] == sc.SENT).any()
        res["thbar"] = t[G:N + G]
    return res


def _same(got, ref):
    for k in pc.NAMES + ("thbar", "status"):
        if k in got:
            assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_every_batch_size_and_slab_equals_the_reference(lmpc, torch, case):
    d = _data(lmpc, case)
    for N in pc.SIZES:
        _same(_call(torch, d, N), _ref(d, N))
    for N in (257, pc.N_COND):                                  # 2 and 10 slabs of 256 points, the last one partial
        _same(_call(torch, d, N, slab=pc.SLAB_MIN), _ref(d, N))


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_each_capacity_and_the_forced_list_pass(lmpc, torch, case):
    d = _data(lmpc, case)
    for option in sc.CAPS:
        for force in (False, True):
            _same(_call(torch, d, pc.N_COND, option, force, slab=pc.SLAB_MIN), _ref(d, pc.N_COND))
    _same(_call(torch, d, 65, 0, True), _ref(d, 65))


def test_the_table_reaches_both_gathers_and_both_capacities(lmpc):
    packs = [sc.host_pack(c) for c in pc.CASES]
    assert {pc.stages_m(p) for p in packs} == {True, False}, "M gathered from LDS in one case and from global memory in another"
    assert {sc.lane_cap(p) for p in packs} == set(sc.CAPS)
    assert pc.default_slab(packs[0]) > pc.SLAB_MIN


def test_thbar_and_status_equal_the_vjp_call(lmpc, torch):
    for name in ("own-n12-m76-nth17", "wave-mr1-n4-m40-nth7"):
        d = _data(lmpc, pc.BY_NAME[name])
        qp, b = d["qp"], d["batch"]
        dev = torch.device("cuda", 0)
        got = _call(torch, d, pc.N_COND, want=())
        act = torch.from_numpy(b["active"].view(np.int64)).to(dev)
        thbar, status = qp.solve_vjp_device(act, torch.from_numpy(b["exitflag"]).to(dev), torch.from_numpy(b["xbar"]).to(dev))
        torch.cuda.synchronize()
        assert np.array_equal(got["thbar"], thbar.cpu().numpy()) and np.array_equal(got["status"], status.cpu().numpy())
        assert set(got["status"].tolist()) >= {1, 0}


CHAIN = ("fast-n5-nth7", "wave-mr1-n4-m40-nth7", "wave-deep-n40-m90-nth6", "own-n12-m76-nth17")


@pytest.mark.parametrize("name", CHAIN)
def test_chain_from_the_solvers_own_masks(lmpc, torch, name):
    d = _data(lmpc, pc.BY_NAME[name])
    qp, b = d["qp"], d["batch"]
    dev = torch.device("cuda", 0)
    n0 = pc.N_COND - sc.N_SOLVER
    th = torch.from_numpy(b["theta"][n0:]).to(dev)
    act = torch.zeros((sc.N_SOLVER, qp.words), dtype=torch.int64, device=dev)
    for k, v in (("sens_cap", 0), ("sens_force_list", 0), ("pack_grad_slab", 0)):
        qp.set_option(k, v)
    x, ef = qp.solve_device(th, active=act)
    g = qp.solve_pack_vjp_device(th, act, ef, torch.from_numpy(b["xbar"][n0:]).to(dev), want_thbar=True)
    torch.cuda.synchronize()
    qp.check()
    assert np.array_equal(ef.cpu().numpy(), b["exitflag"][n0:])
    assert np.array_equal(act.cpu().numpy().view(np.uint64), b["active"][n0:])
    ref = pr.pack_vjp(d["pack"], b["theta"][n0:], b["active"][n0:], b["exitflag"][n0:], b["xbar"][n0:], d["S"].rho_soft,
                      d["S"].zero_tol, d["cache"])
    _same({k: v.cpu().numpy() for k, v in g.items()}, ref)


def test_outputs_left_out_one_at_a_time_and_the_host_pointer_call(lmpc, torch):
    d = _data(lmpc, pc.BY_NAME["own-n5-m80-nth17"])
    N = 257
    ref = _ref(d, N)
    for skip in pc.NAMES:
        _same(_call(torch, d, N, want=tuple(k for k in pc.NAMES if k != skip)), ref)
    _same(_call(torch, d, N, want_thbar=False), ref)
    b = d["batch"]
    got = d["qp"].solve_pack_vjp(b["theta"][:N], b["active"][:N], b["exitflag"][:N], b["xbar"][:N])
    _same(got, ref)
    got = d["qp"].solve_pack_vjp(b["theta"][:N], b["active"][:N], b["exitflag"][:N], b["xbar"][:N], want=("Dth", "x0"))
    assert set(got) == {"Dth", "x0", "thbar", "status"}
    _same(got, ref)


def test_call_sequences_on_one_handle(lmpc, torch):
    d = _data(lmpc, pc.BY_NAME["own-n5-m80-nth17"])
    qp, b = d["qp"], d["batch"]
    dev = torch.device("cuda", 0)
    n0 = pc.N_COND - sc.N_SOLVER
    th = torch.from_numpy(b["theta"][n0:]).to(dev)
    act = torch.from_numpy(b["active"][:65].view(np.int64)).to(dev)
    ef = torch.from_numpy(b["exitflag"][:65]).to(dev)
    xb = torch.from_numpy(b["xbar"][:65]).to(dev)
    qp.reserve(pc.N_COND)                                       # (what lmpc_reserve keeps outside the scratch is in the baseline)
    qp.release_scratch()
    base = lmpc.lib().lmpc_debug_live_blocks()
    thbar0, st0 = qp.solve_vjp_device(act, ef, xb)
    torch.cuda.synchronize()
    sens_seen = qp.sens_launch_info()
    _same(_call(torch, d, 65), _ref(d, 65))                     # pack gradient, plain solve, VJP, pack gradient at another N
    x0, ef0 = qp.solve_device(th)
    thbar1, st1 = qp.solve_vjp_device(act, ef, xb)
    torch.cuda.synchronize()
    assert torch.equal(thbar0, thbar1) and torch.equal(st0, st1)
    assert np.array_equal(ef0.cpu().numpy(), b["exitflag"][n0:])
    sens_now = qp.sens_launch_info()
    assert sens_now[-1]["seq"] == sens_seen[-1]["seq"] + 1 and sens_now[-2] == sens_seen[-1], \
        "the pack gradient left lmpc_sens_launch_info alone"
    _same(_call(torch, d, pc.N_COND, slab=pc.SLAB_MIN), _ref(d, pc.N_COND))
    assert qp.sens_launch_info() == sens_now
    # after lmpc_reserve with "pack_grad_reserve": nothing more is allocated by calls of that size or smaller
    qp.release_scratch()
    qp.set_option("pack_grad_reserve", 1)
    qp.set_option("pack_grad_slab", pc.SLAB_MIN)
    qp.reserve(pc.N_COND)
    grown = lmpc.lib().lmpc_debug_live_blocks()
    _same(_call(torch, d, pc.N_COND, slab=pc.SLAB_MIN), _ref(d, pc.N_COND))
    _same(_call(torch, d, 257, slab=pc.SLAB_MIN), _ref(d, 257))
    assert lmpc.lib().lmpc_debug_live_blocks() == grown > base
    qp.set_option("pack_grad_reserve", 0)
    qp.release_scratch()
    assert lmpc.lib().lmpc_debug_live_blocks() == base
    _same(_call(torch, d, 64), _ref(d, 64))                     # ... and everything comes back
    with pytest.raises(lmpc.LmpcError) as e:
        qp.set_option("pack_grad_slab", 7)
    assert e.value.code == -100


def test_solve_mpqp_autograd_equals_the_direct_calls(lmpc, torch):
    case = pc.BY_NAME["own-n12-m76-nth17"]
    d = _data(lmpc, case)
    qp, b = d["qp"], d["batch"]
    dev = torch.device("cuda", 0)
    n0 = pc.N_COND - sc.N_SOLVER
    H, f, f_theta, A, bu, bl, W, sense = sc.problem(case)
    data = [torch.tensor(np.asarray(a, float), dtype=torch.float64, requires_grad=True) for a in (H, f, f_theta, A, bu, bl, W)]
    theta = torch.from_numpy(b["theta"][n0:]).to(dev).requires_grad_(True)
    c = torch.from_numpy(b["xbar"][n0:]).to(dev)
    x, ef = lmpc.solve_mpqp_autograd(*data, theta, senses=sense, nout=case.nout)
    assert x.requires_grad and not ef.requires_grad and x.grad_fn.sens_status is None
    grads = torch.autograd.grad((x * c).sum(), data + [theta])
    torch.cuda.synchronize()
    assert np.array_equal(ef.cpu().numpy(), b["exitflag"][n0:])
    # the direct calls on the same handle data
    for k, v in (("sens_cap", 0), ("sens_force_list", 0), ("pack_grad_slab", 0)):
        qp.set_option(k, v)
    act = torch.from_numpy(b["active"][n0:].view(np.int64)).to(dev)
    g = qp.solve_pack_vjp_device(theta.detach(), act, ef, c, want_thbar=True)
    torch.cuda.synchronize()
    assert np.array_equal(x.grad_fn.sens_status.cpu().numpy(), g["status"].cpu().numpy())
    assert np.array_equal(grads[7].cpu().numpy(), g["thbar"].cpu().numpy())           # theta: bit for bit
    t = lmpc.transform_vjp(H, f, f_theta, A, bu, bl, W, {k: g[k].cpu().numpy() for k in pc.NAMES}, senses=sense, nout=case.nout)
    for q, name in enumerate(("H", "f", "f_theta", "A", "bu", "bl", "W")):
        assert np.array_equal(grads[q].numpy(), np.asarray(t[name]).reshape(grads[q].shape)), name
        assert np.any(grads[q].numpy() != 0), name
    # with nothing but theta requiring grad it equals solve_autograd
    th2 = torch.from_numpy(b["theta"][n0:]).to(dev).requires_grad_(True)
    x2, _ = lmpc.solve_mpqp_autograd(*[a.detach() for a in data], th2, senses=sense, nout=case.nout)
    x2.backward(c)
    rec = x2.grad_fn.qp.pack_grad_launch_info()[-1]                         # ... at the VJP's cost: stage 1 alone
    assert rec["tree_launches"] == 0 and rec["reduce_grid"] == 0 and rec["nprob"] == sc.N_SOLVER
    th3 = torch.from_numpy(b["theta"][n0:]).to(dev).requires_grad_(True)
    x3, _ = qp.solve_autograd(th3)
    x3.backward(c)
    torch.cuda.synchronize()
    assert torch.equal(x2.detach(), x3.detach()) and torch.equal(th2.grad, th3.grad)


def test_refusals_on_the_device(lmpc, torch):
    import wave_cases as wc
    H, f, f_theta, A, bu, bl, W, sense = wc.problem(wc.BNB_CASES[0])
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=1, device=0)
    dev = torch.device("cuda", 0)
    act = torch.zeros((4, qp.words), dtype=torch.int64, device=dev)
    ef = torch.ones(4, dtype=torch.int32, device=dev)
    with pytest.raises(lmpc.LmpcError) as e:
        qp.solve_pack_vjp_device(torch.ones((4, qp.nth), dtype=torch.float64, device=dev), act, ef,
                                 torch.ones((4, 1), dtype=torch.float64, device=dev))
    assert e.value.code == -103
    assert qp.pack_grad_launch_info() == []
    d = _data(lmpc, pc.BY_NAME["own-n5-m25-nth1"])
    with pytest.raises(ValueError):                                        # theta of another dtype
        a1 = torch.zeros((4, 1), dtype=torch.int64, device=dev)
        d["qp"].solve_pack_vjp_device(torch.ones((4, 1), dtype=torch.float32, device=dev), a1, ef,
                                      torch.ones((4, 5), dtype=torch.float64, device=dev))
