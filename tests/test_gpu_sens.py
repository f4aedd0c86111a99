"""Differentiable solve on the GPU (lmpc_solve_vjp_device / lmpc_solve_jacobian_device, BatchedQP.solve_autograd): every
case of sens_cases.py, the launch record first, then thbar / J / status bit for bit against the numpy restatement of the
contract (sens_reference.py) on guarded outputs -- plain, with the list pass forced, at each capacity of the lane
kernel -- and the chain from the solver's own masks, call sequences on one handle and the autograd function."""
import numpy as np
import pytest

import sens_cases as sc
import sens_reference as sr

pytestmark = pytest.mark.gpu

N_JAC = 257
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
    """Handle, its pack, the case's batch on that pack and the reference's results (once per case)."""
    if case.name not in _CACHE:
        H, f, f_theta, A, bu, bl, W, sense = sc.problem(case)
        qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=case.nout, device=0)
        S = lmpc.default_settings()
        pack = qp.ldp()
        b = sc.build(case, pack)
        cache = sr.derived(pack)
        v, sv = sr.sens(pack, b["active"], b["exitflag"], b["xbar"], S.rho_soft, S.zero_tol, cache)
        J, sj = sr.sens(pack, b["active"][:N_JAC], b["exitflag"][:N_JAC], None, S.rho_soft, S.zero_tol, cache)
        sc.check_conditions(case, pack, b, sv)
        _CACHE[case.name] = dict(qp=qp, pack=pack, batch=b, cache=cache, vjp=v, status=sv, jac=J, jstatus=sj, S=S)
    return _CACHE[case.name]


def _call(torch, d, N, jac, option=0, force=False):
    """One device call on the first N points with guarded outputs.  Asserts the launch record, the guards and that every
    row was written; returns (result, status) as numpy arrays."""
    qp, pack, b = d["qp"], d["pack"], d["batch"]
    G = sc.GUARD
    dev = torch.device("cuda", 0)
    per = pack["nout"] * pack["nth"] if jac else pack["nth"]
    act = torch.from_numpy(b["active"][:N].view(np.int64)).to(dev)
    ef = torch.from_numpy(b["exitflag"][:N]).to(dev)
    out = torch.full((N + 2 * G, per), sc.SENT, dtype=torch.float64, device=dev)
    status = torch.full((N + 2 * G,), sc.SENT_I, dtype=torch.int32, device=dev)
    qp.set_option("sens_cap", option)
    qp.set_option("sens_force_list", int(force))
    seen = qp.sens_launch_info()
    since = seen[-1]["seq"] if seen else 0
    if jac:
        qp.solve_jacobian_device(act, ef, J=out[G:N + G], status=status[G:N + G])
    else:
        qp.solve_vjp_device(act, ef, torch.from_numpy(b["xbar"][:N]).to(dev), thbar=out[G:N + G], status=status[G:N + G])
    torch.cuda.synchronize()
    qp.check()
    rec = qp.sens_launch_info(since)
    assert len(rec) == 1 and rec[0]["seq"] == since + 1
    want = sc.expected_record(pack, N, jac, option, force)
    got = {k: rec[0][k] for k in want}
    assert got == want, (got, want)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert rec[0]["wave_grid"] == (min(N, 4 * cus) if want["list_pass"] else 0)
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert (out[:G] == sc.SENT).all() and (out[N + G:] == sc.SENT).all(), "an output guard row was written"
    assert (status[:G] == sc.SENT_I).all() and (status[N + G:] == sc.SENT_I).all(), "a status guard was written"
    assert not (out[G:N + G] == sc.SENT).any() and not (status[G:N + G] == sc.SENT_I).any(), "an output row was not written"
    return out[G:N + G], status[G:N + G]


def _same(d, N, jac, out, status):
    if jac:
        assert np.array_equal(status, d["jstatus"][:N])
        assert np.array_equal(out.reshape(N, d["pack"]["nout"], d["pack"]["nth"]), d["jac"][:N])
    else:
        assert np.array_equal(status, d["status"][:N])
        assert np.array_equal(out, d["vjp"][:N])
    assert (out[status != 1] == 0).all()


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_every_batch_size_equals_the_reference(lmpc, torch, case):
    d = _data(lmpc, case)
    for N in sc.SIZES:
        _same(d, N, False, *_call(torch, d, N, False))
    for N in (1, 64, 65, N_JAC):
        _same(d, N, True, *_call(torch, d, N, True))


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_each_capacity_and_the_forced_list_pass(lmpc, torch, case):
    d = _data(lmpc, case)
    for option in sc.CAPS:
        for force in (False, True):
            _same(d, sc.N_COND, False, *_call(torch, d, sc.N_COND, False, option, force))
            _same(d, N_JAC, True, *_call(torch, d, N_JAC, True, option, force))
    _same(d, 65, False, *_call(torch, d, 65, False, 0, True))


def test_every_status_comes_back_from_the_device(lmpc, torch):
    d = _data(lmpc, sc.BY_NAME["own-n12-m76-nth17"])
    for force in (False, True):
        out, status = _call(torch, d, sc.N_COND, False, 0, force)
        assert set(status.tolist()) == {1, 0, -1, -7}
        assert np.array_equal(status, d["status"])
        kinds = d["batch"]["kind"]
        assert (status[kinds == "too-many"] == -7).all() and (status[kinds == "dependent"] == -1).all()
        assert (status[kinds == "dependent-wave"] == -1).all() and (status[kinds == "too-many-failed"] == 0).all()


CHAIN = ("fast-n5-nth7", "lane-box2-nth17", "wave-mr1-n4-m40-nth7", "wave-mr2-n3-m65-nth2", "wave-mr1-n12-m64-nth8",
         "wave-deep-n40-m90-nth6", "slow-slow-n6-m156-nth2", "own-n12-m76-nth17", "own-n65-m130-nth1")


@pytest.mark.parametrize("name", CHAIN)
def test_chain_from_the_solvers_own_masks(lmpc, torch, name):
    # solve_device -> solve_vjp_device without leaving the GPU: the solver's masks equal the oracle's, and the derivative on
    # them the reference's
    d = _data(lmpc, sc.BY_NAME[name])
    qp, b = d["qp"], d["batch"]
    dev = torch.device("cuda", 0)
    n0 = sc.N_COND - sc.N_SOLVER
    th = torch.from_numpy(b["theta"]).to(dev)
    act = torch.zeros((sc.N_SOLVER, qp.words), dtype=torch.int64, device=dev)
    qp.set_option("sens_cap", 0)
    qp.set_option("sens_force_list", 0)
    x, ef = qp.solve_device(th, active=act)
    thbar, status = qp.solve_vjp_device(act, ef, torch.from_numpy(b["xbar"][n0:]).to(dev))
    J, sj = qp.solve_jacobian_device(act, ef)
    torch.cuda.synchronize()
    qp.check()
    assert np.array_equal(ef.cpu().numpy(), b["exitflag"][n0:])
    assert np.array_equal(act.cpu().numpy().view(np.uint64), b["active"][n0:])
    assert np.array_equal(status.cpu().numpy(), d["status"][n0:]) and np.array_equal(thbar.cpu().numpy(), d["vjp"][n0:])
    Jr, sjr = sr.sens(d["pack"], b["active"][n0:], b["exitflag"][n0:], None, d["S"].rho_soft, d["S"].zero_tol, d["cache"])
    assert np.array_equal(sj.cpu().numpy(), sjr) and np.array_equal(J.cpu().numpy(), Jr)


def test_call_sequences_on_one_handle(lmpc, torch):
    case = sc.BY_NAME["own-n5-m80-nth17"]
    d = _data(lmpc, case)
    qp, b = d["qp"], d["batch"]
    dev = torch.device("cuda", 0)
    th = torch.from_numpy(b["theta"]).to(dev)
    n0 = sc.N_COND - sc.N_SOLVER
    x0, ef0 = qp.solve_device(th)
    torch.cuda.synchronize()
    _same(d, 65, False, *_call(torch, d, 65, False))            # solve, VJP, Jacobian, solve
    _same(d, 65, True, *_call(torch, d, 65, True))
    x1, ef1 = qp.solve_device(th)
    torch.cuda.synchronize()
    assert torch.equal(x0, x1) and torch.equal(ef0, ef1) and np.array_equal(ef1.cpu().numpy(), b["exitflag"][n0:])
    _same(d, sc.N_COND, False, *_call(torch, d, sc.N_COND, False))      # a batch larger than any before
    qp.release_scratch()                                                # the derived pack and the list go and come back
    _same(d, N_JAC, True, *_call(torch, d, N_JAC, True))
    blocks = lmpc.lib().lmpc_debug_live_blocks()
    qp.set_option("sens_reserve", 1)
    qp.reserve(sc.N_COND)
    _same(d, sc.N_COND, False, *_call(torch, d, sc.N_COND, False))      # after lmpc_reserve: nothing more is allocated
    grown = lmpc.lib().lmpc_debug_live_blocks()
    _same(d, 257, False, *_call(torch, d, 257, False))
    assert lmpc.lib().lmpc_debug_live_blocks() == grown >= blocks
    qp.set_option("sens_reserve", 0)
    # the host-pointer entry points
    v, s = qp.solve_vjp(b["active"][:N_JAC], b["exitflag"][:N_JAC], b["xbar"][:N_JAC])
    assert np.array_equal(v, d["vjp"][:N_JAC]) and np.array_equal(s, d["status"][:N_JAC])
    J, sj = qp.solve_jacobian(b["active"][:N_JAC], b["exitflag"][:N_JAC])
    assert np.array_equal(J, d["jac"]) and np.array_equal(sj, d["jstatus"])
    with pytest.raises(lmpc.LmpcError) as e:
        qp.set_option("sens_cap", 6)
    assert e.value.code == -100


@pytest.mark.parametrize("name", ("fast-n5-nth7", "own-n12-m76-nth17"))
def test_solve_autograd_gives_the_vjp_bit_for_bit(lmpc, torch, name):
    d = _data(lmpc, sc.BY_NAME[name])
    qp, b = d["qp"], d["batch"]
    dev = torch.device("cuda", 0)
    n0 = sc.N_COND - sc.N_SOLVER
    qp.set_option("sens_cap", 0)
    qp.set_option("sens_force_list", 0)
    c = torch.from_numpy(b["xbar"][n0:]).to(dev)
    grads = []
    for _ in range(2):                                          # a second backward on a fresh graph is identical
        theta = torch.from_numpy(b["theta"]).to(dev).requires_grad_(True)
        x, ef = qp.solve_autograd(theta)
        assert x.requires_grad and not ef.requires_grad and ef.dtype == torch.int32
        assert x.grad_fn.sens_status is None
        x.backward(c)
        torch.cuda.synchronize()
        assert np.array_equal(ef.cpu().numpy(), b["exitflag"][n0:])
        assert np.array_equal(x.grad_fn.sens_status.cpu().numpy(), d["status"][n0:])
        assert x.grad_fn.sens_status is qp.last_sens_status
        grads.append(theta.grad.cpu().numpy())
    assert np.array_equal(grads[0], d["vjp"][n0:]) and np.array_equal(grads[1], grads[0])
    # a loss through torch's own operations: d/dtheta sum(w * x) = the VJP of w
    theta = torch.from_numpy(b["theta"]).to(dev).requires_grad_(True)
    x, _ = qp.solve_autograd(theta)
    (x * c).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(theta.grad.cpu().numpy(), d["vjp"][n0:])
    # theta without requires_grad: the plain solve, no graph, no launch of the derivative
    seen = qp.sens_launch_info()
    x2, ef2 = qp.solve_autograd(torch.from_numpy(b["theta"]).to(dev))
    torch.cuda.synchronize()
    assert x2.grad_fn is None and not x2.requires_grad and torch.equal(x2, x.detach())
    assert qp.sens_launch_info() == seen
    qp.check()


def test_refusals_on_the_device(lmpc, torch):
    import wave_cases as wc
    H, f, f_theta, A, bu, bl, W, sense = wc.problem(wc.BNB_CASES[0])
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=1, device=0)
    dev = torch.device("cuda", 0)
    act = torch.zeros((4, qp.words), dtype=torch.int64, device=dev)
    ef = torch.ones(4, dtype=torch.int32, device=dev)
    with pytest.raises(lmpc.LmpcError) as e:
        qp.solve_vjp_device(act, ef, torch.ones((4, 1), dtype=torch.float64, device=dev))
    assert e.value.code == -103
    with pytest.raises(lmpc.LmpcError) as e:
        qp.solve_jacobian_device(act, ef)
    assert e.value.code == -103
    assert qp.sens_launch_info() == []
    d = _data(lmpc, sc.BY_NAME["own-n5-m25-nth1"])
    with pytest.raises(ValueError):                                        # masks of another word count
        a2 = torch.zeros((4, d["qp"].words + 1), dtype=torch.int64, device=dev)
        d["qp"].solve_vjp_device(a2, ef, torch.ones((4, 5), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):                                        # xbar of another dtype
        a1 = torch.zeros((4, 1), dtype=torch.int64, device=dev)
        d["qp"].solve_vjp_device(a1, ef, torch.ones((4, 5), dtype=torch.float32, device=dev))
