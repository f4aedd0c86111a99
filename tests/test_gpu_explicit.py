"""Explicit MPC on the GPU (lmpc_explicit_build / lmpc_explicit_eval_device): every point of a fresh sample against
the implicit path (qp.solve_device) -- same exit flags, same x where the located region is the solver's final active
set, within the solver's own stopping band elsewhere, fallback points bit for bit."""
import threading

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _qp(lmpc, name, nout=None):
    g = load_golden(name)
    return lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"],
                                    nout=g["H"].shape[0] if nout is None else nout)


def _parity(lmpc, qp, ec, th_np, same_tol=1e-8):
    import torch
    th = torch.from_numpy(th_np).to(f"cuda:{qp.device}")
    N = th.shape[0]
    xe, fe, re = ec.evaluate_device(th)
    act = torch.zeros((N, qp.words), dtype=torch.int64, device=th.device)
    xi, fi = qp.solve_device(th, active=act)
    torch.cuda.synchronize()
    xe, fe, re, xi, fi = (t.cpu().numpy() for t in (xe, fe, re, xi, fi))
    act = act.cpu().numpy().view(np.uint64)
    assert np.array_equal(fe, fi)                                                  # (a)
    loc = re >= 0
    assert np.array_equal(xe[~loc], xi[~loc])                                      # (d)
    masks = np.array([ec.region(k)["mask"] for k in range(ec.nregions)]).reshape(ec.nregions, -1)
    same = loc.copy()
    same[loc] = (masks[re[loc]] == act[loc]).all(1)
    d = np.abs(xe - xi)
    assert np.all(d[same] <= same_tol * (1 + np.abs(xi[same])))                     # (b)
    rnorm = np.linalg.norm(qp.ldp()["Rout"], axis=1)
    other = loc & ~same
    assert np.all(d[other] <= 10 * 1e-6 * rnorm + 1e-9 * (1 + np.abs(xi[other])))  # (c)
    return loc.mean(), re


def test_parity_pendulum_bench_range_and_wide_range(lmpc):
    import bench
    qp = _qp(lmpc, "pendulum", 1)
    for hard, want in ((False, 0.99), (True, 0.95)):
        ec = lmpc.explicit.ExplicitController.from_sample(qp, bench.make_theta("pendulum", 1_000_000, 21, hard))
        frac, _ = _parity(lmpc, qp, ec, bench.make_theta("pendulum", 1_000_000, 22, hard))
        assert frac >= want, (hard, frac)
        ec.close()


def test_parity_pendulum_N50_and_tree_independence(lmpc):
    import bench
    qp = _qp(lmpc, "pendulum_N50", 1)
    train = bench.make_theta("pendulum_N50", 200_000, 23)
    test = bench.make_theta("pendulum_N50", 200_000, 24)
    ec = lmpc.explicit.ExplicitController.from_sample(qp, train)
    frac, rd = _parity(lmpc, qp, ec, test)
    assert frac >= 0.95, frac
    flat = lmpc.explicit.ExplicitController.from_sample(qp, train, max_depth=0)
    frac0, rf = _parity(lmpc, qp, flat, test)
    import torch
    th = torch.from_numpy(test).cuda()
    xd, fd, _ = (t.cpu().numpy() for t in ec.evaluate_device(th))
    xf, ff, _ = (t.cpu().numpy() for t in flat.evaluate_device(th))
    assert np.array_equal(fd, ff)
    both = rd == rf
    assert np.array_equal(xd[both], xf[both])
    for i in np.flatnonzero((rd >= 0) & (rf >= 0) & (rd != rf)):                # shared facets only
        for r in (rd[i], rf[i]):
            reg = ec.region(int(r))
            assert np.all(reg["A"] @ test[i] <= reg["b"] + 1e-9 * (1 + np.abs(reg["b"])))
    misses = np.mean((rf >= 0) & (rd < 0))
    assert np.all(rd[rf < 0] < 0) and misses < 0.005, misses


def test_parity_soft_doc_half_infeasible(lmpc):
    # soft_doc's reduced systems reach condition 1e11 (more active rows than variables, rho_soft = 1e-6): the
    # implicit solver's own answer carries ~1e-7 relative rounding there, so (b) is asserted at 1e-5
    import bench
    qp = _qp(lmpc, "soft_doc", 1)
    ec = lmpc.explicit.ExplicitController.from_sample(qp, bench.make_theta("soft_doc", 200_000, 25))
    th = bench.make_theta("soft_doc", 200_000, 26)
    frac, _ = _parity(lmpc, qp, ec, th, same_tol=1e-5)
    assert 0.3 <= frac <= 0.6


def test_reference_anchor_explicit_mpc(lmpc):
    # runtests.jl:178-183: ExplicitMPC(invpend; range) + build_tree! -> compute_control([5,5,0,0]) = 1.7612519326
    g = load_golden("pendulum")
    mpc = lmpc.MPC(lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"]),
                   nx=4, nu=1, nr=2, nuprev=1)
    lb = np.array([-20.0] * 4 + [-20.0, 0.0] + [-2.0])
    ub = np.array([20.0] * 4 + [20.0, 0.0] + [2.0])
    empc = lmpc.ExplicitMPC(mpc, (lb, ub), nsamples=200_000, seed=1, extra_theta=mpc.form_parameter([5.0, 5, 0, 0]))
    u = empc.compute_control([5.0, 5, 0, 0])
    assert abs(u[0] - 1.7612519326) < 1e-6 and empc.last_region >= 0


def test_edge_cases(lmpc):
    import torch
    import bench
    rng = np.random.default_rng(31)
    # nth = 0: a constant law
    n = 4
    H = np.eye(n) * 2.0
    qp0 = lmpc.BatchedQP.from_mpqp(H, rng.standard_normal(n) * 3, np.zeros((n, 0)), np.zeros((0, n)), np.ones(n),
                                   -np.ones(n), np.zeros((n, 0)), np.zeros(n, np.int32))
    x0, f0, _, a0 = qp0.solve(np.zeros((8, 0)))
    ec0 = lmpc.explicit.ExplicitController.build(qp0, np.zeros((8, 0)), a0, f0)
    xe, fe, re = ec0.evaluate(np.zeros((5, 0)))
    assert np.all(re == 0) and np.all(fe == f0[0]) and np.abs(xe - x0[0]).max() <= 1e-12
    # N = 0 and N = 1
    qp = _qp(lmpc, "pendulum", 1)
    ec = lmpc.explicit.ExplicitController.from_sample(qp, bench.make_theta("pendulum", 100_000, 27))
    x, f, r = ec.evaluate_device(torch.zeros((0, 7), dtype=torch.float64, device="cuda:0"))
    assert x.shape == (0, 1)
    t1 = bench.make_theta("pendulum", 1, 28)
    xe, fe, re = ec.evaluate(t1)
    xi, fi, _, _ = qp.solve(t1)
    assert fe[0] == fi[0] and abs(xe[0, 0] - xi[0, 0]) <= 1e-8 * (1 + abs(xi[0, 0]))
    # a cap that drops most of mass_spring_3in's regions: flags still those of the implicit path
    q3 = _qp(lmpc, "mass_spring_3in", 3)
    ec3 = lmpc.explicit.ExplicitController.from_sample(q3, bench.make_theta("mass_spring_3in", 50_000, 29, "feasible"),
                                                       max_regions=50)
    info = ec3.info()
    assert info["regions"] == 50 and info["dropped_capacity"] > 1000
    frac, _ = _parity(lmpc, q3, ec3, bench.make_theta("mass_spring_3in", 50_000, 30, "feasible"))
    assert frac < 0.5


def test_two_controllers_on_two_handles_from_two_threads(lmpc):
    import bench
    import torch
    qa, qb = _qp(lmpc, "pendulum", 1), _qp(lmpc, "soft_doc", 1)
    ea = lmpc.explicit.ExplicitController.from_sample(qa, bench.make_theta("pendulum", 100_000, 31))
    eb = lmpc.explicit.ExplicitController.from_sample(qb, bench.make_theta("soft_doc", 100_000, 32))
    ta, tb = bench.make_theta("pendulum", 200_000, 33), bench.make_theta("soft_doc", 200_000, 34)
    ref = {"a": ea.evaluate(ta), "b": eb.evaluate(tb)}
    out, errs = {}, []

    def run(key, ec, th):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(3):
                    out[key] = ec.evaluate(th)
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=("a", ea, ta)), threading.Thread(target=run, args=("b", eb, tb))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for k in ("a", "b"):
        for u, v in zip(out[k], ref[k]):
            assert np.array_equal(u, v)
