"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle on the same
constant pack and the same seeded parameter points.

Bar (BASELINE.json north_star): |x_gpu - x_ref| <= 1e-10 per problem, identical exit flags and
identical final active sets.  Because the lane kernel and the oracle share one arithmetic contract
(explicit fma chains in index order) the observed difference is 0; the tolerance asserted is the
stated 1e-10.
"""
import os

import numpy as np
import pytest

from conftest import load_golden, oracle_ldp_from

pytestmark = pytest.mark.gpu
TOL = 1e-10
ROOT_DIR = __import__("os").path.abspath(__import__("os").path.join(__import__("os").path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _qp_from_golden(lmpc, g, nout=None):
    return lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"],
                                    g["senses"], nout=g["H"].shape[0] if nout is None else nout)


def _compare(qp, theta, warm=None, settings=None):
    from oracle import ldp as oldp
    L = oracle_ldp_from(qp.ldp())
    x, ef, it, act = qp.solve(theta, warm=warm)
    xo, efo, ito, acto = oldp.solve_batch(L, theta, settings, warm=warm)
    assert np.array_equal(ef, efo)
    assert np.array_equal(it, ito)
    assert np.array_equal(act, acto)
    err = np.abs(x - xo).max() if len(x) else 0.0
    assert err <= TOL, err
    return x, ef, it, act


def test_K1_through_c_abi(lmpc):
    # /root/reference/test/runtests.jl:62-66 -- same check the reference runs on its generated C (:78-81)
    g = load_golden("pendulum")
    mpc = lmpc.MPC(lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"]),
                   nx=4, nu=1, nr=2, nuprev=1)
    u = mpc.compute_control([5.0, 5, 0, 0])
    assert np.linalg.norm(u - 1.7612519326) < 1e-6
    U = mpc.compute_control_trajectory([5.0, 5, 0, 0], uprev=[0.0])
    assert np.abs(U - [1.76125193, 2.0, 1.69224018, 0.84197348, -0.16317228]).max() < 1e-6
    # solve_one == DAQP.solve shape
    x, flag = mpc.opt_model.solve_one(mpc.form_parameter([5.0, 5, 0, 0], uprev=[0.0]))
    assert flag == 1 and abs(x[0] - 1.7612519326) < 1e-6


@pytest.mark.parametrize("name", ["pendulum", "mass_spring", "mass_spring_3in", "preprocessing_kat"])
def test_golden_vectors(lmpc, name):
    g = load_golden(name)
    qp = _qp_from_golden(lmpc, g)
    x, ef, it, act = qp.solve(g["theta"])
    # The golden answers came from the numpy-transformed pack, the GPU uses the library's own
    # C++ transform: the two packs differ by rounding (<= 1e-13).  Every solvable problem must
    # agree in flag, iteration count, active set and (to 1e-10) solution; on infeasible problems
    # the path to the failure flag (-1 infeasible / -2 cycle) is rounding-sensitive, so only
    # "failed" is compared there.  Bit-level agreement on one shared pack is asserted in
    # test_gpu_vs_oracle_same_pack.
    ok = g["exitflag"] >= 1
    assert np.array_equal(ef >= 1, ok)
    assert np.array_equal(ef[ok], g["exitflag"][ok])
    assert np.array_equal(act[ok], g["active"][ok])
    assert np.array_equal(it[ok], g["iters"][ok])
    assert np.abs(x[ok] - g["X"][ok]).max() <= TOL


@pytest.mark.parametrize("name,nout", [("pendulum", 1), ("pendulum", 5), ("mass_spring", 1), ("mass_spring", 10)])
def test_gpu_vs_oracle_same_pack(lmpc, name, nout):
    g = load_golden(name)
    qp = _qp_from_golden(lmpc, g, nout)
    rng = np.random.default_rng(99)
    extra = rng.uniform(-6, 6, (3000, g["theta"].shape[1])) * (1.0 if name == "pendulum" else 0.5)
    if name == "pendulum":
        extra[:, 5] = 0.0
    _compare(qp, np.vstack([g["theta"], extra]))


@pytest.mark.parametrize("name", ["pendulum", "soft_doc", "prestab", "satellite20_preview"])
def test_ldp_setup_path_matches_mpqp_setup(lmpc, name):
    # generated-C style setup (lmpc_setup_ldp: the arrays LinearMPC.codegen writes, codegen.jl:183-189)
    # gives the same answers as the mpQP setup -- the reference checks the same pair, Julia path vs
    # generated C, on plain / preview / hybrid controllers (runtests.jl:78-81, :627-667, :836-858)
    g = load_golden(name)
    qp1 = _qp_from_golden(lmpc, g)
    pk = qp1.ldp()
    qp2 = lmpc.BatchedQP.from_ldp(pk["M"], pk["du"], pk["dl"], pk["Dth"], pk["Rout"], pk["x0"], pk["Xth"],
                                  pk["sense"], ms=pk["ms"])
    x1, ef1, _, a1 = qp1.solve(g["theta"])
    x2, ef2, _, a2 = qp2.solve(g["theta"])
    assert np.array_equal(x1, x2) and np.array_equal(ef1, ef2) and np.array_equal(a1, a2)


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 255, 257, 1000])
def test_ragged_batch_sizes(lmpc, N):
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    x, ef, it, act = _compare(qp, g["theta"][:N])
    assert x.shape == (N, 1)


def test_warm_start(lmpc):
    # K6 (/root/reference/test/runtests.jl:85-117): warm-started solves agree with cold ones
    for name in ("pendulum", "mass_spring"):
        g = load_golden(name)
        qp = _qp_from_golden(lmpc, g)
        ok = g["exitflag"] >= 1
        x, ef, it, act = _compare(qp, g["theta"][ok], warm=g["active"][ok])
        assert np.abs(x - g["X"][ok]).max() < 1e-9
        assert it.mean() < g["iters"][ok].mean()
    # a deliberately wrong / dependent warm set must still converge to the same answer
    g = load_golden("mass_spring")
    qp = _qp_from_golden(lmpc, g)
    ok = g["exitflag"] >= 1
    rng = np.random.default_rng(5)
    warm = rng.integers(0, 2**63, size=g["active"][ok].shape, dtype=np.uint64) & np.uint64((1 << 62) - 1)
    warm[:, 1] &= np.uint64((1 << 62) - 1)
    x, ef, it, act = _compare(qp, g["theta"][ok], warm=warm)
    good = ef >= 1
    assert good.mean() > 0.9
    assert np.abs(x[good] - g["X"][ok][good]).max() < 1e-6


def test_equality_immutable_and_one_sided_rows(lmpc):
    rng = np.random.default_rng(3)
    n, nth = 4, 3
    Hh = rng.standard_normal((n, n)); H = Hh @ Hh.T + n * np.eye(n)
    A = rng.standard_normal((3, n))
    bu = np.array([1.0, 1.0, 1e30, 1e30, 0.3, 1e30, 0.5])
    bl = np.array([-1.0, -1e30, -1e30, -1e30, 0.3, -1e30, -0.5])
    sense = np.array([0, 0, 4, 4, 5, 4, 0], np.int32)
    W = np.zeros((7, nth)); W[4] = [0.1, 0, 0]
    f_theta = rng.standard_normal((n, nth))
    qp = lmpc.BatchedQP.from_mpqp(H, np.zeros(n), f_theta, A, bu, bl, W, sense)
    theta = rng.uniform(-3, 3, (500, nth))
    x, ef, it, act = _compare(qp, theta)
    assert np.all(ef == 1)
    assert np.abs(x @ A[0] - (0.3 + 0.1 * theta[:, 0])).max() < 1e-9


def test_singular_and_infeasible_paths(lmpc):
    # duplicated / opposing general rows force the singular-direction branch; some theta are infeasible
    rng = np.random.default_rng(11)
    n, nth = 3, 2
    H = np.diag([1.0, 2.0, 3.0])
    a = np.array([1.0, 1.0, 0.0])
    A = np.vstack([a, 2 * a, -a, [0, 1.0, 1.0], [1.0, 0, -1.0], [1.0, 2.0, 1.0]])
    bu = np.array([1.0, 1.0, 1.0, 1.0, 2.2, 0.2, 1.0, 1.0, 3.0])
    bl = np.array([-1.0, -1.0, -1.0, 0.5, -9.0, -0.9, -1.0, -1.0, 2.0])
    W = np.zeros((9, nth)); W[3] = [1.0, 0]; W[5] = [0, 1.0]; W[8] = [0.5, 0.5]
    f_theta = rng.standard_normal((n, nth))
    qp = lmpc.BatchedQP.from_mpqp(H, np.zeros(n), f_theta, A, bu, bl, W, None)
    theta = rng.uniform(-2, 2, (4000, nth))
    x, ef, it, act = _compare(qp, theta)
    assert (ef == 1).any() and (ef == -1).any()


def test_iteration_limit_and_settings(lmpc):
    from oracle import ldp as oldp
    g = load_golden("mass_spring")
    s = lmpc.default_settings()
    s.iter_limit = 4
    so = oldp.default_settings(); so.iter_limit = 4
    qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"],
                                  settings=s)
    x, ef, it, act = _compare(qp, g["theta"], settings=so)
    assert (ef == -4).any() and it.max() == 4
    s.iter_limit = 10000; s.primal_tol = 1e-9
    so.iter_limit = 10000; so.primal_tol = 1e-9
    qp.set_settings(s)
    _compare(qp, g["theta"], settings=so)


def test_error_behaviour(lmpc):
    g = load_golden("pendulum")
    with pytest.raises(lmpc.LmpcError) as e:                      # DAQP.setup flag -5 (setup.jl:18-19)
        lmpc.BatchedQP.from_mpqp(-g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"])
    assert e.value.code == -5
    with pytest.raises(lmpc.LmpcError) as e:                      # DAQP.setup flag -1 (setup.jl:14-15)
        lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bl"], g["bu"], g["W"], g["senses"])
    assert e.value.code == -1
    mpc = lmpc.MPC(lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"]),
                   nx=4, nu=1, nr=2, nuprev=1)
    with pytest.raises(ValueError):
        mpc.compute_control([1.0, 2.0])
    gm = load_golden("mass_spring")
    mpcm = lmpc.MPC(lmpc.MPQP(gm["H"], gm["f"], gm["f_theta"], gm["A"], gm["bu"], gm["bl"], gm["W"], gm["senses"]),
                    nx=12, nu=1)
    bad = gm["theta"][np.flatnonzero(gm["exitflag"] == -1)[0]]
    with pytest.raises(AssertionError):                           # utils.jl:46 @assert exitflag >= 1
        mpcm.compute_control(bad)
    mpcm.compute_control(bad, check=False)


def test_device_resident_path_and_full_size_properties(lmpc):
    """BASELINE config 2 at full size (1e6 pendulum points, f64, inputs resident in HBM)."""
    import torch
    from oracle import ldp as oldp
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    rng = np.random.default_rng(1234)
    N = 1_000_000
    theta = np.hstack([rng.uniform([-5, -5, -.3, -2], [5, 5, .3, 2], (N, 4)), rng.uniform(-5, 5, (N, 1)),
                       np.zeros((N, 1)), rng.uniform(-2, 2, (N, 1))])
    th = torch.from_numpy(theta).cuda()
    it = torch.empty(N, dtype=torch.int32, device="cuda")
    act = torch.zeros((N, qp.words), dtype=torch.int64, device="cuda")
    x, ef = qp.solve_device(th, iters=it, active=act)
    torch.cuda.synchronize()
    x, ef, it, act = x.cpu().numpy(), ef.cpu().numpy(), it.cpu().numpy(), act.cpu().numpy().view(np.uint64)
    assert np.all(ef == 1)
    assert np.all(x <= 2 + 1e-6) and np.all(x >= -2 - 1e-6)                # first move obeys |u| <= 2
    # idempotence: same inputs, same bits
    x2, ef2 = qp.solve_device(th)
    torch.cuda.synchronize()
    assert np.array_equal(x2.cpu().numpy(), x)
    # permutation equivariance (problems are independent)
    perm = torch.from_numpy(rng.permutation(N)).cuda()
    x3, _ = qp.solve_device(th[perm].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(x3.cpu().numpy(), x[perm.cpu().numpy()])
    # inactive problems are affine in theta: x = x0 + Xth theta exactly
    pk = qp.ldp()
    free = np.flatnonzero(act[:, 0] == 0)
    lin = pk["x0"][0] + theta[free] @ pk["Xth"][0]
    assert np.abs(lin - x[free, 0]).max() < 1e-9
    # oracle on a 50k-problem sample of the same batch
    idx = rng.choice(N, 50_000, replace=False)
    xo, efo, ito, acto = oldp.solve_batch(oracle_ldp_from(pk), theta[idx])
    assert np.array_equal(efo, ef[idx]) and np.array_equal(ito, it[idx]) and np.array_equal(acto, act[idx])
    assert np.abs(xo - x[idx]).max() <= TOL


# ------------------------------------------------------------------ wavefront-per-QP kernel
def _random_qp(rng, n, mg, nth, nsoft=0, ms=None):
    ms = n if ms is None else ms
    Hh = rng.standard_normal((n, n))
    H = Hh @ Hh.T + n * np.eye(n)
    A = rng.standard_normal((mg, n))
    m = ms + mg
    bu = rng.uniform(0.5, 2.0, m)
    bl = -rng.uniform(0.5, 2.0, m)
    W = 0.3 * rng.standard_normal((m, nth))
    W[:ms] = 0.0
    f_theta = rng.standard_normal((n, nth))
    sense = np.zeros(m, np.int32)
    if nsoft:
        sense[ms + rng.choice(mg, nsoft, replace=False)] = 8
    return H, np.zeros(n), f_theta, A, bu, bl, W, sense


@pytest.mark.parametrize("name", ["pendulum", "mass_spring", "preprocessing_kat"])
def test_wave_kernel_matches_oracle_and_lane_kernel(lmpc, name):
    g = load_golden(name)
    qp = _qp_from_golden(lmpc, g)
    qp.set_option("wave", 0)              # (mass-spring's 63 general rows make the wavefront kernel the default)
    xl, efl, itl, actl = qp.solve(g["theta"])
    assert "lane" in qp.kernel_name
    qp.set_option("wave", 1)
    assert qp.kernel_name.endswith("wave")
    xw, efw, itw, actw = _compare(qp, g["theta"])
    assert np.array_equal(xw, xl) and np.array_equal(efw, efl) and np.array_equal(itw, itl)
    assert np.array_equal(actw, actl)
    ok = g["exitflag"] >= 1
    _compare(qp, g["theta"][ok], warm=g["active"][ok])


def test_wave_kernel_problem_queue(lmpc):
    # large batch: the wavefront kernel hands problems out through its shared counter in chunks of
    # several problems per ticket; results must not depend on who solved what (bit-identical to the
    # static split, to the lane kernel, and -- on a sample -- to the oracle)
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g)
    rng = np.random.default_rng(11)
    N = 600_001
    theta = np.hstack([rng.uniform(-20, 20, (N, 5)), np.zeros((N, 1)), rng.uniform(-2, 2, (N, 1))])
    xl, efl, itl, actl = qp.solve(theta)
    qp.set_option("wave", 1)
    xq, efq, itq, actq = qp.solve(theta)
    qp.set_option("wave_queue", 0)
    xs, efs, its, acts = qp.solve(theta)
    for a, b, c in ((xl, xq, xs), (efl, efq, efs), (itl, itq, its), (actl, actq, acts)):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    qp.set_option("wave_queue", 1)
    _compare(qp, theta[-5000:])


@pytest.mark.parametrize("name", ["mass_spring_3in", "soft_doc", "satellite20"])
def test_wave_kernel_layouts_and_staging_levels_agree(lmpc, name):
    # the factor's LDS layout (square / packed) and the staging level of the shared data are launch
    # choices: every combination must give the same bits
    g = load_golden(name)
    qp = _qp_from_golden(lmpc, g)
    ref = qp.solve(g["theta"])
    for packed in (0, 1):
        for level in (0, 1, 3):
            for nwv in (2, 8):
                qp.set_option("wave_packed", packed)
                qp.set_option("wave_level", level)
                qp.set_option("wave_nwv", nwv)
                out = qp.solve(g["theta"])
                for a, b in zip(ref, out):
                    assert np.array_equal(a, b), (packed, level, nwv)


def test_K8_soft_constraints_through_c_abi(lmpc):
    # /root/reference/docs/src/manual/simple.md:98-107: u = -1 at x = [0.5, 1], r = [0, 0]
    g = load_golden("soft_doc")
    mpc = lmpc.MPC(lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"]),
                   nx=2, nu=1, nr=2, nuprev=1)
    u = mpc.compute_control([0.5, 1.0], r=[0.0, 0.0])
    assert abs(u[0] + 1.0) < 1e-6
    assert mpc.opt_model.kernel_name.endswith("wave")
    x, ef, it, act = _compare(mpc.opt_model, g["theta"])
    assert (ef == 2).any() and (ef == 1).any() and (ef == -1).any()
    ok = g["exitflag"] >= 1
    assert np.array_equal(ef >= 1, ok)
    assert np.array_equal(act[ok], g["active"][ok])
    # golden X came from the numpy-transformed pack; with soft rows the KKT system carries the
    # 1/rho_soft = 1e6 penalty, so 1e-16 differences between the two packs grow to ~1e-5 in x on
    # the soft-optimal problems (same active set, same iteration count).  The bit-level check on
    # ONE pack is the _compare call above.
    assert np.abs(x[ok] - g["X"][ok]).max() <= 1e-3
    hard_only = ok & (g["exitflag"] == 1)
    assert np.abs(x[hard_only] - g["X"][hard_only]).max() <= 1e-6


@pytest.mark.parametrize("n,mg,nth,nsoft,seed", [(20, 30, 6, 0, 0), (30, 90, 8, 10, 1), (63, 100, 5, 0, 2),
                                                 (12, 200, 4, 40, 3), (3, 5, 2, 2, 4)])
def test_wave_kernel_random_problems(lmpc, n, mg, nth, nsoft, seed):
    rng = np.random.default_rng(seed)
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth, nsoft)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=min(n, 4))
    assert qp.kernel_name.endswith("wave")
    theta = rng.uniform(-2, 2, (600, nth))
    x, ef, it, act = _compare(qp, theta)
    assert (ef >= 1).mean() > 0.05
    _compare(qp, theta[:65], warm=act[:65])


@pytest.mark.parametrize("n,mg,nth,nsoft,seed", [(8, 300, 3, 0, 11), (20, 480, 5, 60, 12), (40, 984, 4, 100, 13),
                                                 (10, 500, 6, 200, 14),
                                                 (20, 150, 6, 0, 15), (70, 100, 5, 0, 16),       # 3 slots, one / two variable slots
                                                 (30, 270, 6, 30, 17), (80, 230, 4, 0, 18),      # 5 slots
                                                 (50, 330, 7, 0, 19), (100, 273, 7, 0, 20)])     # 6 slots (N = 125 of the benchmark class: m = 373)
def test_wave_kernel_many_rows(lmpc, n, mg, nth, nsoft, seed):
    # 128 < m <= 1024: the 3-, 5-, 6-, 8- and 16-slot instantiations (long prediction horizons with output bounds);
    # n + 1 + #soft may exceed the 64 lanes as long as the working sets themselves stay below
    rng = np.random.default_rng(seed)
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth, nsoft)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, 2 * bu, 2 * bl, 0.3 * W, sense, nout=min(n, 4))
    assert qp.kernel_name.endswith("wave") and qp.m == n + mg
    theta = rng.uniform(-2, 2, (300, nth))
    x, ef, it, act = _compare(qp, theta)
    assert (ef >= 1).mean() > 0.05 and (ef != -7).all()
    ok = ef >= 1
    _compare(qp, theta[ok][:65], warm=act[ok][:65])
    if nsoft == 0:                                       # binary32 on the same instantiations
        from oracle import ldp as oldp
        s32 = lmpc.default_settings_f32()
        qf = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, 2 * bu, 2 * bl, 0.3 * W, sense, nout=min(n, 4), settings=s32)
        th32 = theta.astype(np.float32)
        xf, eff, itf, actf = qf.solve_f32(th32)
        xo, efo, ito, acto = oldp.solve_batch(oracle_ldp_from(qf.ldp()), th32, _copy_settings(lmpc, s32), dtype=np.float32)
        assert np.array_equal(eff, efo) and np.array_equal(itf, ito) and np.array_equal(actf, acto)
        assert np.abs(xf - xo).max() <= 1e-6


def test_working_sets_beyond_the_64_lanes(lmpc):
    # soft rows never make a working set singular, so a problem with many of them can want more than 64 rows at
    # once -- more than the wavefront has lanes.  The wavefront kernel gives such a point up (its own flag -7, no
    # DAQP flag) and lists it; the one-problem-per-thread kernel behind it (lmpc_big_kernel.hpp, up to 256 rows)
    # re-solves it, so the caller gets exactly what the oracle gives -- cold, warm, binary32, and behind the
    # screening pass.  lmpc_set_option("big_path", 0) shows the flag.
    from oracle import ldp as oldp
    rng = np.random.default_rng(5)
    n, mg, nth = 6, 150, 2
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth, nsoft=mg)
    W[n:, 0] = np.abs(W[n:, 0]) + 0.5                    # theta_0 >> 0 pushes every soft row over its bound
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=2)
    theta = np.vstack([rng.uniform(-1, 1, (200, nth)),
                       np.hstack([rng.uniform(30, 60, (56, 1)), rng.uniform(-1, 1, (56, 1))])])
    L = oracle_ldp_from(qp.ldp())
    xo, efo, ito, acto = oldp.solve_batch(L, theta)
    nact = np.array([sum(bin(int(w)).count("1") for w in row) for row in acto])
    assert (nact > 64).sum() >= 20 and nact.max() <= 157
    qp.set_option("big_path", 0)
    x, ef, it, act = qp.solve(theta)
    over = ef == -7
    assert over.any() and (nact[over] >= 60).all()       # given up only where the working set is that large
    keep = ~over
    assert np.array_equal(ef[keep], efo[keep]) and np.array_equal(it[keep], ito[keep])
    assert np.array_equal(act[keep], acto[keep]) and np.abs(x[keep] - xo[keep]).max() <= TOL
    qp.set_option("big_path", 1)
    for scr in (0, 1):
        qp.set_option("screen_wave", scr)
        x, ef, it, act = qp.solve(theta)
        assert np.array_equal(ef, efo) and np.array_equal(it, ito) and np.array_equal(act, acto)
        assert (ef >= 1).all() and np.array_equal(x, xo)
    # warm start from the final working sets (the large ones included): the same masks come back
    xw, efw, itw, actw = qp.solve(theta, warm=act)
    xwo, efwo, itwo, actwo = oldp.solve_batch(L, theta, warm=acto)
    assert np.array_equal(efw, efwo) and np.array_equal(itw, itwo) and np.array_equal(actw, actwo)
    assert np.array_equal(xw, xwo)
    # more overflowing points than the slow path has threads (512): every thread walks several
    big = np.hstack([rng.uniform(30, 60, (1500, 1)), rng.uniform(-1, 1, (1500, 1))])
    xb, efb, itb, actb = qp.solve(big)
    xbo, efbo, itbo, actbo = oldp.solve_batch(L, big)
    assert np.array_equal(efb, efbo) and np.array_equal(itb, itbo) and np.array_equal(actb, actbo) and np.array_equal(xb, xbo)
    # binary32 on the same handle's scratch
    s32 = lmpc.default_settings_f32()
    qf = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=2, settings=s32)
    th32 = theta.astype(np.float32)
    xf, eff, itf, actf = qf.solve_f32(th32)
    xfo, effo, itfo, actfo = oldp.solve_batch(oracle_ldp_from(qf.ldp()), th32, _copy_settings(lmpc, s32), dtype=np.float32)
    assert np.array_equal(eff, effo) and np.array_equal(itf, itfo) and np.array_equal(actf, actfo)
    assert np.array_equal(xf, xfo)


# ------------------------------------------------------------------ closed-loop batch simulation
@pytest.mark.parametrize("warm", [False, True])
def test_closed_loop_simulation_matches_oracle(lmpc, warm):
    # reference src/simulation.jl:93-113 for N scenarios at once; K6 (test/runtests.jl:85-117)
    from oracle import ldp as oldp
    from oracle import mpc2mpqp as omm
    prob = omm.pendulum()
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    L = oracle_ldp_from(qp.ldp())
    rng = np.random.default_rng(8)
    N, T = 3000, 40
    x0 = rng.uniform([-5, -5, -.3, -2], [5, 5, .3, 2], (N, 4))
    x0[0] = [5.0, 5.0, 0.0, 0.0]
    r = np.stack([rng.uniform(-2, 2, N), np.zeros(N)], 1)
    r[0] = 0.0
    ref = oldp.simulate(L, x0, T, prob.F, prob.G, r=r, warm=warm)
    out = qp.simulate(x0, T, prob.F, prob.G, r=r, warm=warm)
    assert np.array_equal(out["flag_min"], ref["flag_min"]) and np.all(out["flag_min"] >= 1)
    # the plant step is specified operation by operation (fused multiply-adds from 0, F then G) and the oracle's loop
    # does exactly that: identical bits, not merely close ones (tests/loop_reference.py restates it a third time)
    for key in ("U", "X", "x", "uprev"):
        assert np.array_equal(out[key], ref[key]), (key, np.abs(out[key] - ref[key]).max())
    assert abs(out["U"][0, 0, 0] - 1.7612519326) < 1e-6


@pytest.mark.parametrize("warm", [False, True])
def test_closed_loop_execution_modes_agree_bit_for_bit(lmpc, warm):
    # scenario-asynchronous rounds (default), with and without un-asked rounds, the lock-step fused loop and
    # the unfused one run the same arithmetic per scenario and step: identical arrays, not merely close ones.
    # Sizes that are no multiple of a wavefront, a one-step loop, and a scenario that needs iterations at
    # every step of the transient (x0 far out) are in the set.
    from oracle import ldp as oldp
    from oracle import mpc2mpqp as omm
    prob = omm.pendulum()
    g = load_golden("pendulum")
    rng = np.random.default_rng(21)
    for N, T in ((1, 1), (37, 3), (700, 60)):
        x0 = rng.uniform([-8, -5, -.3, -2], [8, 5, .3, 2], (N, 4))
        r = np.stack([rng.uniform(-4, 4, N), np.zeros(N)], 1)
        outs = []
        for opts in ({}, {"sim_small": 0}, {"sim_blind": 0}, {"sim_blind": 5}, {"sim_async": 0},
                     {"sim_async": 0, "sim_fused": 0}):
            qp = _qp_from_golden(lmpc, g, 1)
            for k, v in opts.items():
                qp.set_option(k, v)
            outs.append(qp.simulate(x0, T, prob.F, prob.G, r=r, warm=warm))
        ref = oldp.simulate(oracle_ldp_from(qp.ldp()), x0, T, prob.F, prob.G, r=r, warm=warm)
        assert np.array_equal(outs[0]["flag_min"], ref["flag_min"])
        for key in ("U", "X", "x", "uprev"):
            assert np.array_equal(outs[0][key], ref[key]), (N, T, key, np.abs(outs[0][key] - ref[key]).max())
        for o in outs[1:]:
            for key in ("U", "X", "x", "uprev", "flag_min"):
                assert np.array_equal(o[key], outs[0][key]), (N, T, key)


def test_closed_loop_random_shapes_all_execution_modes(lmpc):
    # Random controllers on the lane-kernel path across the instantiations of the streaming kernel: one to four
    # inputs, nx below and above 4, nth below and above 8, with and without reference / previous-control blocks,
    # simple bounds only or general rows too.  Every execution order must reproduce the oracle's closed loop.
    from oracle import ldp as oldp
    rng = np.random.default_rng(77)
    shapes = [(2, 1, 0, 1, 3, 0), (4, 1, 2, 1, 4, 3), (3, 2, 1, 2, 4, 2), (6, 2, 1, 2, 5, 0), (5, 3, 0, 3, 6, 4),
              (8, 4, 2, 4, 6, 2), (4, 1, 0, 0, 2, 9), (7, 1, 3, 1, 3, 1)]
    for nx, nu, nr, nup, n, mg in shapes:
        nth = nx + nr + nup
        H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth)
        f_theta *= 0.6
        qp0 = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=nu)
        assert "lane" in qp0.kernel_name
        Fm = rng.standard_normal((nx, nx))
        Fm *= 0.9 / np.abs(np.linalg.eigvals(Fm)).max()
        Gm = 0.5 * rng.standard_normal((nx, nu))
        N, T = 333, 25
        x0 = rng.uniform(-2, 2, (N, nx))
        r = rng.uniform(-1, 1, (N, nr)) if nr else None
        L = oracle_ldp_from(qp0.ldp())
        for warm in (False, True):
            ref = oldp.simulate(L, x0, T, Fm, Gm, r=r, warm=warm)
            first = None
            for opts in ({}, {"sim_small": 0}, {"sim_async": 0}):
                qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=nu)
                for k, v in opts.items():
                    qp.set_option(k, v)
                out = qp.simulate(x0, T, Fm, Gm, r=r, warm=warm)
                assert np.array_equal(out["flag_min"], ref["flag_min"]), (nx, nu, nr, nup, opts)
                for key in ("U", "X", "x") + (("uprev",) if nup else ()):
                    assert np.array_equal(out[key], ref[key]), (nx, nu, nr, nup, opts, key, np.abs(out[key] - ref[key]).max())
                if first is None:
                    first = out
                    assert (out["U"] != 0).any()
                else:
                    for key in ("U", "X", "x", "flag_min"):
                        assert np.array_equal(out[key], first[key]), (nx, nu, nr, nup, opts, key)


def test_closed_loop_simulation_soft_problem_wave_kernel(lmpc):
    from oracle import ldp as oldp
    from oracle import mpc2mpqp as omm
    prob = omm.doc_simple_soft()
    g = load_golden("soft_doc")
    qp = _qp_from_golden(lmpc, g, 1)
    L = oracle_ldp_from(qp.ldp())
    rng = np.random.default_rng(9)
    N, T = 400, 10                       # docs/src/manual/simple.md:112-119: x0 = [0,0], r = [1,0], N = 10
    x0 = rng.uniform(0, 0.5, (N, 2)); x0[0] = 0.0
    r = np.tile([1.0, 0.0], (N, 1))
    for warm in (False, True):
        # (warm on the wavefront path: the factorisation is kept between two steps -- the oracle's warm == 2)
        ref = oldp.simulate(L, x0, T, prob.F, prob.G, r=r, warm=2 if warm else False)
        out = qp.simulate(x0, T, prob.F, prob.G, r=r, warm=warm)
        assert np.array_equal(out["flag_min"], ref["flag_min"])
        assert np.abs(out["U"] - ref["U"]).max() <= TOL and np.abs(out["X"] - ref["X"]).max() <= TOL


def test_region_discovery_on_gpu(lmpc):
    # config 4 of BASELINE.json on one GPU: sample the example's +-20 ParameterRange
    # (/root/reference/src/mpc_examples.jl:128-134), batched solve, distinct active sets
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g)
    lb = np.array([-20.0] * 4 + [-20.0, 0.0] + [-2.0])
    ub = np.array([20.0] * 4 + [20.0, 0.0] + [2.0])
    theta = lmpc.explicit.sample_range(lb, ub, 500000, seed=1)
    out = lmpc.explicit.discover_regions(qp.solve, theta)
    assert out["n_solved"] == 500000 and 44 <= len(out["masks"]) <= 243
    i = int(out["first_index"][3])
    Fz, gz = lmpc.explicit.affine_law(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], out["masks"][3])
    x, ef, _, act = qp.solve(theta[i][None])
    assert np.array_equal(act[0], out["masks"][3]) and np.abs(Fz @ theta[i] + gz - x[0]).max() < 1e-8


def test_sampled_complexity_certificate_on_gpu(lmpc):
    # the caller side of /root/reference/src/certify.jl: the reference certifies invpend over its
    # ParameterRange and gets a partition of more than 100 regions of equal working-set SEQUENCE
    # (runtests.jl:199-204); the sample's distinct (final active set, iteration count) pairs are unions of
    # such regions (about 50 on this range), its largest iteration count a lower bound of the certified one
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g)
    lb = np.array([-20.0] * 4 + [-20.0, 0.0] + [-2.0])
    ub = np.array([20.0] * 4 + [20.0, 0.0] + [2.0])
    theta = lmpc.explicit.sample_range(lb, ub, 300000, seed=2)
    out = lmpc.explicit.certify_sampled(qp.solve, theta)
    assert 40 <= out["n_cells"] <= 243 * 8 and out["exitflags"] == {1: 300000} and out["max_iterations"] >= 7
    x, ef, it, act = qp.solve(out["argmax_theta"][None])
    assert it[0] == out["max_iterations"] == len(out["iterations_hist"]) - 1


def test_K2_prestabilising_feedback_through_c_abi(lmpc):
    # /root/reference/test/runtests.jl:119-136; u = U*[1:nu] - K x (reference src/utils.jl:48-49)
    from oracle import mpc2mpqp as omm
    g = load_golden("prestab")
    K = g["K"]
    pn = omm.prestab_kat(False)
    qn = omm.mpc2mpqp(pn)
    nominal = lmpc.MPC(lmpc.MPQP(qn.H, qn.f, qn.f_theta, qn.A, qn.bu, qn.bl, qn.W, qn.senses), nx=2, nu=1, nr=2)
    prestab = lmpc.MPC(lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"]),
                       nx=2, nu=1, nr=2, K=K)
    unom = nominal.compute_control([0.0, 0.0], r=[1.0, 0.0])
    upre = prestab.compute_control([0.0, 0.0], r=[1.0, 0.0])
    assert np.linalg.norm(unom - upre) < 1e-10
    assert prestab.opt_model.kernel_name.endswith("wave") and prestab.opt_model.ms == 0      # bounds are general rows
    # batched path with K folded into the output map, against the oracle on the same pack
    cm = prestab.control_model()
    x, ef, it, act = _compare(cm, g["theta"])
    ok = (ef >= 1) & (g["ef_nominal"] >= 1)
    assert np.abs(x[ok, 0] - g["u_nominal"][ok]).max() < 1e-8
    U, efb = prestab.compute_control_batch(g["theta"][:, :2], R=g["theta"][:, 2:4], check=False)
    assert np.array_equal(U, x) and np.array_equal(efb, ef)


def test_K3_generalized_parameters_through_c_abi(lmpc):
    # /root/reference/test/runtests.jl:1250-1268: theta = [x; r; p]; u_nom = 1.0 (p = 0), u_tight = 0.25 (p = 0.75)
    from oracle import mpc2mpqp as omm
    prob = omm.generalized_parameter_kat()
    q = omm.mpc2mpqp(prob)
    mpc = lmpc.MPC(lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses), nx=1, nu=1, nr=1, np_=1)
    assert mpc.get_parameter_dims() == (1, 1, 0, 0, 1)
    u_nom = mpc.compute_control([0.0], r=[0.0], p=[0.0])
    u_tight = mpc.compute_control([0.0], r=[0.0], p=[0.75])
    assert abs(u_nom[0] - 1.0) < 1e-6 and abs(u_tight[0] - 0.25) < 1e-6
    rng = np.random.default_rng(2)
    theta = np.hstack([rng.uniform(-1, 1, (500, 1)), np.zeros((500, 1)), rng.uniform(-0.5, 1.5, (500, 1))])
    _compare(mpc.opt_model, theta)


def test_unconstrained_and_wide_parameter_problems(lmpc):
    rng = np.random.default_rng(21)
    # (a) no constraints at all (reference "Unconstrained" testset, test/runtests.jl:1327-1335):
    #     every problem is optimal after one iteration, x = -H^-1 f_theta theta
    n, nth = 4, 3
    Hh = rng.standard_normal((n, n)); H = Hh @ Hh.T + n * np.eye(n)
    f_theta = rng.standard_normal((n, nth))
    qp = lmpc.BatchedQP.from_mpqp(H, np.zeros(n), f_theta, np.zeros((0, n)), np.zeros(0), np.zeros(0),
                                  np.zeros((0, nth)), None)
    theta = rng.uniform(-3, 3, (700, nth))
    x, ef, it, act = _compare(qp, theta)
    assert np.all(ef == 1) and np.all(it == 1)
    assert np.abs(x + theta @ np.linalg.solve(H, f_theta).T).max() < 1e-10
    # (b) a parameter vector longer than the screening pass covers (nth > 32, e.g. reference preview
    #     over the horizon): the iterating kernel alone handles the batch
    n, mg, nth = 6, 10, 40
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth)
    qp = lmpc.BatchedQP.from_mpqp(H, f, 0.2 * f_theta, A, bu, bl, 0.1 * W, sense, nout=2)
    assert "lane" in qp.kernel_name
    theta = rng.uniform(-1, 1, (900, nth))
    x, ef, it, act = _compare(qp, theta)
    assert (ef == 1).mean() > 0.5 and it.max() > 1
    # (c) outputs that are not requested may be NULL
    x2, ef2, it2, act2 = qp.solve(theta, want_iters=False, want_active=False)
    assert it2 is None and act2 is None and np.array_equal(x2, x) and np.array_equal(ef2, ef)
    # (d) kernel-selection switches do not change a bit
    qp.set_option("screen", 0)
    x3, ef3, _, _ = qp.solve(theta)
    assert np.array_equal(x3, x) and np.array_equal(ef3, ef)
    with pytest.raises(lmpc.LmpcError):
        qp.set_option("no_such_option", 1)


def test_unsupported_shapes_are_refused_loudly(lmpc):
    rng = np.random.default_rng(22)
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, 130, 10, 3)      # n > 127
    with pytest.raises(lmpc.LmpcError) as e:
        lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense)
    assert e.value.code == -103
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, 70, 10, 3)       # branch and bound stops at n = 64
    sense = sense.copy(); sense[:4] |= 16
    with pytest.raises(lmpc.LmpcError) as e:
        lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense)
    assert e.value.code == -103
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, 8, 1020, 3)      # m > 1024
    with pytest.raises(lmpc.LmpcError) as e:
        lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense)
    assert e.value.code == -103


@pytest.mark.parametrize("n,mg,kernel", [(6, 58, "lane"), (6, 59, "wave"), (12, 30, "lane"), (12, 52, "wave"),
                                         (13, 3, "wave"), (20, 236, "wave"), (2, 1, "lane")])
def test_size_boundaries_between_kernels(lmpc, n, mg, kernel):
    # m = 64 is the last size the lane kernel's one-word masks cover, n = 12 its largest instantiation
    # (with general rows it is the default up to m*n < 600, then the wavefront kernel takes over),
    # m = 256 the last size of the 512-thread wavefront instantiations
    rng = np.random.default_rng(100 + n + mg)
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, 4)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, 3 * bu, 3 * bl, 0.2 * W, sense, nout=min(n, 3))
    assert kernel in qp.kernel_name and qp.m == n + mg
    theta = rng.uniform(-2, 2, (300, 4))
    x, ef, it, act = _compare(qp, theta)
    ok = ef >= 1
    if ok.sum() > 4:
        _compare(qp, theta[ok][:64], warm=act[ok][:64])


def test_problem_without_parameters(lmpc):
    # nth = 0: a plain QP solved N times (theta has no columns)
    rng = np.random.default_rng(31)
    n, mg = 5, 4
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, 0)
    f = rng.standard_normal(n) * 3
    qp = lmpc.BatchedQP.from_mpqp(H, f, np.zeros((n, 0)), A, bu, bl, np.zeros((n + mg, 0)), sense)
    x, ef, it, act = _compare(qp, np.zeros((130, 0)))
    assert np.all(ef == ef[0]) and np.all(x == x[0])


def test_broken_working_set_is_never_reported_optimal(lmpc):
    # BASELINE config 3 as worded (3 inputs, n = 30, m = 84 -> wavefront kernel).  Some infeasible
    # theta drive the dual iterates to ~1e15 through a nearly dependent working set; such a point
    # must come back with a failure flag, not as "optimal" (every reported optimum satisfies all
    # hard rows to primal_tol in the normalised constraint space)
    g = load_golden("mass_spring_3in")
    qp = _qp_from_golden(lmpc, g)
    assert qp.kernel_name.endswith("wave") and (qp.n, qp.m) == (30, 84)
    rng = np.random.default_rng(1234)
    theta = rng.uniform(-3, 3, (3000, 12))
    x, ef, it, act = _compare(qp, theta)
    assert (ef == 1).any() and (ef < 0).any()
    pk = qp.ldp()
    Afull = np.vstack([np.eye(30)[:30], g["A"]])
    ok = np.flatnonzero(ef >= 1)
    bu = g["bu"][None] + theta[ok] @ g["W"].T
    bl = g["bl"][None] + theta[ok] @ g["W"].T
    Ax = x[ok] @ Afull.T
    scale = np.linalg.norm(Afull @ np.linalg.inv(np.linalg.cholesky(g["H"]).T), axis=1)
    assert ((Ax - bu) / scale).max() < 1e-5 and ((bl - Ax) / scale).max() < 1e-5


# ------------------------------------------------------------------ hybrid MPC (binary rows, B&B)
@pytest.mark.parametrize("name", ["satellite4", "satellite20", "satellite20_preview"])
def test_hybrid_branch_and_bound_matches_oracle(lmpc, name):
    # /root/reference/test/runtests.jl:820-834; binaries of mpc_examples.jl:533-546
    g = load_golden(name)
    qp = _qp_from_golden(lmpc, g)
    assert qp.kernel_name.endswith("wave")
    x, ef, it, act = _compare(qp, g["theta"])
    assert np.all(ef == 1)
    bins = np.flatnonzero(g["senses"] & 16)
    assert np.all(np.minimum(np.abs(x[:, bins] - g["bu"][bins]), np.abs(x[:, bins] - g["bl"][bins])) < 1e-9)
    # against the committed answers (numpy-transformed pack: rounding-level differences only)
    assert np.array_equal(ef, g["exitflag"])
    assert np.abs(x - g["X"]).max() <= 1e-8


def test_hybrid_mpc_through_operator_interface(lmpc):
    g = load_golden("satellite20")
    mpc = lmpc.MPC(lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"],
                             has_binaries=True), nx=3, nu=3, nr=3)
    x = np.zeros(3)
    for k in range(40):
        u = mpc.compute_control(x, r=[0.5, 0.0, 0.0])
        assert np.abs(u - g["closed_loop_u"][k]).max() < 1e-8
        x = g["F"] @ x + g["G"] @ u
    assert abs(x[0] - 0.5) < 1e-3                                          # runtests.jl:829


def test_hybrid_closed_loop_batch_simulation(lmpc):
    from oracle import ldp as oldp
    g = load_golden("satellite20")
    qp = _qp_from_golden(lmpc, g, 3)
    L = oracle_ldp_from(qp.ldp())
    rng = np.random.default_rng(12)
    N, T = 24, 25
    x0 = np.hstack([rng.uniform(-0.1, 0.1, (N, 1)), np.zeros((N, 2))]); x0[0] = 0.0
    r = np.tile([0.5, 0.0, 0.0], (N, 1))
    ref = oldp.simulate(L, x0, T, g["F"], g["G"], r=r, warm=False)
    out = qp.simulate(x0, T, g["F"], g["G"], r=r, warm=False)
    assert np.array_equal(out["flag_min"], ref["flag_min"]) and np.all(out["flag_min"] == 1)
    assert np.abs(out["U"] - ref["U"]).max() <= TOL and np.abs(out["X"] - ref["X"]).max() <= TOL
    for b in (1, 2):                                                       # runtests.jl:831-834
        lo, hi = g["bl"][b], g["bu"][b]
        assert np.all((np.abs(out["U"][:, :, b] - lo) < 1e-5) | (np.abs(out["U"][:, :, b] - hi) < 1e-5))


def test_hybrid_random_problems_with_general_rows(lmpc):
    # binaries next to general inequality rows and soft rows; infeasible assignments must prune
    rng = np.random.default_rng(2024)
    nsolved = 0
    for trial in range(6):
        n, mg, nth = 6, 5, 3
        H, f, fth, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth, nsoft=(1 if trial % 2 else 0))
        sense = sense.copy()
        sense[:3] |= 16                                                    # first three bounds binary
        qp = lmpc.BatchedQP.from_mpqp(H, f, fth, A, bu, bl, W, sense)
        assert qp.kernel_name.endswith("wave")
        theta = rng.uniform(-1, 1, (200, nth))
        x, ef, it, act = _compare(qp, theta)
        ok = ef >= 1                                                       # trial 1 is infeasible throughout
        nsolved += int(ok.sum())
        xb = x[ok][:, :3]
        lo = (bl[:3] + theta[ok] @ W[:3].T)
        hi = (bu[:3] + theta[ok] @ W[:3].T)
        assert np.all(np.minimum(np.abs(xb - lo), np.abs(xb - hi)) < 1e-8)
    assert nsolved >= 800


# ------------------------------------------------------------------ binary32 path (codegen float_type="float")
def _copy_settings(lmpc, s):
    from oracle import ldp as oldp
    so = oldp.Settings()
    for f, _ in so._fields_:
        setattr(so, f, getattr(s, f, 0))
    return so


@pytest.mark.parametrize("name,rho", [("pendulum", None), ("mass_spring", None), ("mass_spring_3in", None),
                                      ("soft_doc", 1e-3), ("soft_doc", 1e-6), ("satellite4", None),
                                      ("satellite20", None)])
def test_f32_path_matches_f32_oracle(lmpc, name, rho):
    # the reference's single-precision build of this path: codegen.jl:19,31-37,82 (c_float = float,
    # DAQP_SINGLE_PRECISION).  Checker: the binary32 build of the oracle on the SAME pack rounded to
    # binary32; bar: identical flags / iteration counts / active sets, |dx| <= 1e-6 (observed 0).
    from oracle import ldp as oldp
    g = load_golden(name)
    s = lmpc.default_settings_f32()
    if rho is not None:
        s.rho_soft = rho
    qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"],
                                  settings=s)
    theta = g["theta"].astype(np.float32)
    x, ef, it, act = qp.solve_f32(theta)
    assert x.dtype == np.float32
    L = oracle_ldp_from(qp.ldp())
    xo, efo, ito, acto = oldp.solve_batch(L, theta, _copy_settings(lmpc, s), dtype=np.float32)
    assert np.array_equal(ef, efo) and np.array_equal(it, ito) and np.array_equal(act, acto)
    assert np.abs(x - xo).max() <= 1e-6
    # against the binary64 answers of the fixture: same outcome on (nearly) every problem, x to
    # single-precision accuracy where both solve
    ok = (ef >= 1) & (g["exitflag"] >= 1)
    assert ((ef >= 1) == (g["exitflag"] >= 1)).mean() > 0.9
    tol = 5e-3 if name == "soft_doc" else 2e-3
    assert np.abs(x[ok] - g["X"][ok]).max() <= tol * max(1.0, np.abs(g["X"][ok]).max())
    if name.startswith("satellite"):                                  # runtests.jl:831-834 (f32: +-1e-5)
        bins = np.flatnonzero(g["senses"] & 16)
        assert np.all(np.minimum(np.abs(x[:, bins] - g["bu"][bins]), np.abs(x[:, bins] - g["bl"][bins])) < 1e-5)


def test_f32_warm_start_and_device_path(lmpc):
    import torch
    from oracle import ldp as oldp
    g = load_golden("mass_spring_3in")
    s = lmpc.default_settings_f32()
    qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"],
                                  nout=3, settings=s)
    theta = g["theta"].astype(np.float32)
    x, ef, it, act = qp.solve_f32(theta)
    ok = ef >= 1
    L = oracle_ldp_from(qp.ldp())
    xw, efw, itw, actw = qp.solve_f32(theta[ok], warm=act[ok])
    xo, efo, ito, acto = oldp.solve_batch(L, theta[ok], _copy_settings(lmpc, s), warm=act[ok], dtype=np.float32)
    assert np.array_equal(efw, efo) and np.array_equal(itw, ito) and np.array_equal(actw, acto)
    assert np.abs(xw - xo).max() <= 1e-6
    assert itw.mean() < it[ok].mean()
    # device-resident float32 tensors through lmpc_solve_batch_f32_device
    th_d = torch.from_numpy(theta).cuda()
    x_d, ef_d = qp.solve_device(th_d)
    torch.cuda.synchronize()
    assert x_d.dtype == torch.float32
    assert np.array_equal(x_d.cpu().numpy(), x) and np.array_equal(ef_d.cpu().numpy(), ef)


def test_f32_refused_where_the_wave_kernel_does_not_reach(lmpc):
    # m = 0: only the lane kernel covers it -> the binary32 entry point must fail loudly
    H = np.eye(3)
    qp = lmpc.BatchedQP.from_mpqp(H, np.zeros(3), np.ones((3, 2)), np.zeros((0, 3)), [], [], np.zeros((0, 2)))
    with pytest.raises(lmpc.LmpcError) as e:
        qp.solve_f32(np.zeros((4, 2), np.float32))
    assert e.value.code == -103


# ------------------------------------------------------------------ previews (utils.jl:78-261) on the device
def test_form_parameter_device_matches_the_operator_interface(lmpc):
    import torch
    g = load_golden("satellite20_preview")
    Np, ny = 20, 3
    mpc = lmpc.MPC(lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"],
                             has_binaries=True), nx=3, nu=3, nr=ny * Np, Np=Np, reference_preview=True)
    mpc.setup()
    qp = mpc.opt_model
    rng = np.random.default_rng(5)
    N = 37
    X = rng.uniform(-1, 1, (N, 3))
    xd = torch.from_numpy(X).cuda()
    # (a) one short trajectory shared by all scenarios: padded with its last column (utils.jl:101-106)
    r_short = rng.uniform(-1, 1, (ny, 7))
    th = qp.form_parameter_device(xd, r=torch.from_numpy(r_short).cuda(), r_preview=Np)
    torch.cuda.synchronize()
    ref = np.stack([mpc.form_parameter(X[i], r=r_short) for i in range(N)])
    assert np.array_equal(th.cpu().numpy(), ref)
    # (b) a long trajectory per scenario, window starting at column k0 (simulation.jl:128-134)
    r_long = rng.uniform(-1, 1, (N, ny, 31))
    for k0 in (0, 5, 20, 30):
        th = qp.form_parameter_device(xd, r=torch.from_numpy(r_long).cuda(), r_preview=Np, k0=k0)
        torch.cuda.synchronize()
        ref = np.stack([mpc.form_parameter(X[i], r=r_long[i][:, k0:]) for i in range(N)])
        assert np.array_equal(th.cpu().numpy(), ref)
    # (c) a constant reference vector is repeated over the horizon (utils.jl:88-94); None gives zeros
    rv = rng.uniform(-1, 1, ny)
    th = qp.form_parameter_device(xd, r=torch.from_numpy(np.tile(rv[:, None], (1, 1))).cuda(), r_preview=Np)
    torch.cuda.synchronize()
    assert np.array_equal(th.cpu().numpy(), np.stack([mpc.form_parameter(X[i], r=rv) for i in range(N)]))
    # (d) non-preview handle: [x; r; uprev] with uprev per scenario
    gp = load_golden("pendulum")
    mp = lmpc.MPC(lmpc.MPQP(gp["H"], gp["f"], gp["f_theta"], gp["A"], gp["bu"], gp["bl"], gp["W"], gp["senses"]),
                  nx=4, nu=1, nr=2, nuprev=1).setup()
    X4 = rng.uniform(-1, 1, (N, 4)); up = rng.uniform(-1, 1, (N, 1)); r2 = rng.uniform(-1, 1, (N, 2, 1))
    th = mp.opt_model.form_parameter_device(torch.from_numpy(X4).cuda(), r=torch.from_numpy(r2).cuda(),
                                            uprev=torch.from_numpy(up).cuda())
    torch.cuda.synchronize()
    ref = np.stack([mp.form_parameter(X4[i], r=r2[i, :, 0], uprev=up[i]) for i in range(N)])
    assert np.array_equal(th.cpu().numpy(), ref)
    # blocks that do not add up to nth are refused
    with pytest.raises(lmpc.LmpcError):
        qp.form_parameter_device(xd, r=torch.from_numpy(r_short).cuda(), r_preview=Np - 1)


def test_hybrid_closed_loop_with_reference_preview(lmpc):
    # /root/reference/test/runtests.jl:820-834 as worded: reference_preview = true, a step in the
    # reference trajectory, 20 closed-loop steps; y -> 0.5 +- 1e-3, binary inputs on a bound
    g = load_golden("satellite20_preview")
    qp = _qp_from_golden(lmpc, g, 3)
    N = 6
    x0 = np.zeros((N, 3)); x0[1:, 0] = np.linspace(-0.02, 0.02, N - 1)
    out = qp.simulate_ref(x0, 20, g["F"], g["G"], g["rs"], preview=20)
    assert np.all(out["flag_min"] == 1)
    assert np.abs(out["U"][:, 0] - g["closed_loop_u"]).max() < 1e-8
    assert np.abs(out["X"][:20, 0] - g["closed_loop_y"]).max() < 1e-8
    assert abs(out["X"][19, 0, 0] - 0.5) < 1e-3                                       # runtests.jl:829
    for b, (lo, hi) in ((1, (0.0, 1.0)), (2, (-1.0, 0.0))):                           # runtests.jl:831-834
        ub = out["U"][:, :, b]
        assert np.all((np.abs(ub - lo) < 1e-5) | (np.abs(ub - hi) < 1e-5))
    # without preview the same entry point feeds column k of the trajectory: equals lmpc_simulate with
    # a constant reference when the trajectory is constant
    g0 = load_golden("satellite20")
    q0 = _qp_from_golden(lmpc, g0, 3)
    rc = np.tile(np.array([[0.5], [0.0], [0.0]]), (1, 4))
    a = q0.simulate_ref(x0, 8, g0["F"], g0["G"], rc, preview=0)
    b_ = q0.simulate(x0, 8, g0["F"], g0["G"], r=np.tile([0.5, 0.0, 0.0], (N, 1)), warm=False)
    assert np.array_equal(a["U"], b_["U"]) and np.array_equal(a["X"], b_["X"])


def test_form_parameter_device_all_blocks(lmpc):
    # theta = [x; r (preview); d (preview); uprev; p (constant)] -- every block of explicit.jl:54-63
    import torch
    rng = np.random.default_rng(8)
    nx, ny, nd, nu, npar, Np = 2, 2, 1, 1, 2, 4
    nth = nx + ny * Np + nd * Np + nu + npar
    n = 3
    H = np.eye(n)
    q = lmpc.MPQP(H, np.zeros(n), rng.normal(size=(n, nth)), np.zeros((0, n)), np.ones(n), -np.ones(n),
                  np.zeros((n, nth)), np.zeros(n, np.int32))
    mpc = lmpc.MPC(q, nx=nx, nu=nu, nr=ny * Np, nd=nd * Np, nuprev=nu, np_=npar, Np=Np,
                   reference_preview=True, disturbance_preview=True).setup()
    N = 50
    X = rng.normal(size=(N, nx)); R = rng.normal(size=(N, ny, 6)); D = rng.normal(size=(nd, 2))
    U = rng.normal(size=(N, nu)); Pm = rng.normal(size=(N, npar, 1))
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for k0 in (0, 1, 4):
        th = mpc.opt_model.form_parameter_device(cu(X), r=cu(R), d=cu(D), uprev=cu(U), p=cu(Pm),
                                                 r_preview=Np, d_preview=Np, k0=k0)
        torch.cuda.synchronize()
        ref = np.stack([mpc.form_parameter(X[i], r=R[i][:, min(k0, 5):], d=D[:, min(k0, 1):], uprev=U[i],
                                           p=Pm[i][:, 0]) for i in range(N)])
        assert np.array_equal(th.cpu().numpy(), ref)
    # and the formed batch solves like the host-formed one
    x1, ef1, _, _ = mpc.opt_model.solve(th.cpu().numpy())
    x2, ef2 = mpc.opt_model.solve_device(th)
    torch.cuda.synchronize()
    assert np.array_equal(x1, x2.cpu().numpy()) and np.array_equal(ef1, ef2.cpu().numpy())


# ------------------------------------------------------------------ K5: closed-loop end values
@pytest.mark.parametrize("name", ["x0unc_kat", "offset_kat", "moveblock_kat"])
def test_K5_fixtures_through_c_abi(lmpc, name):
    g = load_golden(name)
    qp = _qp_from_golden(lmpc, g)
    x, ef, it, act = _compare(qp, g["theta"])
    assert np.array_equal(ef, g["exitflag"]) and np.array_equal(act, g["active"])
    tol = 1e-4 if name == "x0unc_kat" else 1e-8      # soft rows: 1/rho amplifies pack rounding (see K8)
    assert np.abs(x - g["X"]).max() <= tol


def test_K5_closed_loops_on_the_gpu(lmpc):
    # (a) runtests.jl:1067-1074: x1 -> 0.4 (soft, tightened output bound), many scenarios at once
    g = load_golden("x0unc_kat")
    qp = _qp_from_golden(lmpc, g, 1)
    assert qp.kernel_name.endswith("wave")
    N = 16
    out = qp.simulate(np.zeros((N, 2)), 400, g["F"], g["G"], r=np.full((N, 1), 0.5), warm=False, want_x=False)
    assert np.all(out["flag_min"] >= 1) and np.abs(out["x"][:, 0] - 0.4).max() < 1e-6
    # (c) runtests.jl:1329-1335: move-blocked, unconstrained (m = 0, lane kernel): y = C x -> 5.0
    g = load_golden("moveblock_kat")
    qp = _qp_from_golden(lmpc, g, 1)
    out = qp.simulate(np.zeros((N, 1)), 20, g["F"], g["G"], r=np.full((N, 1), 5.0), warm=False)
    y19 = 2.211992169 * out["X"][19, :, 0]
    assert np.abs(y19 - 5.0).max() < 5e-8 * 5.0
    # (b) runtests.jl:1320-1327: offsets live in f; the recorded closed loop, solved as one batch
    g = load_golden("offset_kat")
    qp = _qp_from_golden(lmpc, g, 1)
    x, ef, _, _ = qp.solve(g["theta"][:50])
    assert np.all(ef == 1) and np.abs(x[:, 0] - g["us"][:, 0]).max() < 1e-9 and abs(x[49, 0] - 10.5) < 1e-7


def test_reference_preview_simulation_on_the_gpu(lmpc):
    # /root/reference/test/runtests.jl:276-327 through lmpc_simulate_ref_device (preview window
    # k+1 .. k+Np / column k), soft output bounds -> wavefront kernel; same four assertions, and the
    # trajectories of the closed loop restated on the host (tests/loop_reference.py), bit for bit
    import loop_reference as lr
    from oracle import mpc2mpqp as omm
    from test_oracle import _preview_sim
    N = 20
    outs = {}
    for prev in (True, False):
        p = omm.preview_sim_kat(prev)
        q = omm.mpc2mpqp(p)
        qp = lmpc.BatchedQP.from_mpqp(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, nout=1)
        us_o, ys_o, rt = _preview_sim(prev, N)
        x0 = np.tile([1.0, 0.0], (5, 1))
        out = qp.simulate_ref(x0, N, p.F, p.G, rt, preview=p.Np if prev else 0)
        assert np.all(out["flag_min"] >= 1)
        ref = lr.simulate_ref_reference(oracle_ldp_from(qp.ldp()), x0, N, p.F, p.G, rt, preview=p.Np if prev else 0)
        for key in ("U", "X", "x", "flag_min"):
            assert np.array_equal(out[key], ref[key]), (prev, key)
        assert out["uprev"] is None and ref["uprev"].size == 0
        assert np.abs(out["U"][:, 0, 0] - us_o[0]).max() < 1e-6 and np.abs(out["X"][:N, 0].T - ys_o).max() < 1e-6
        outs[prev] = (out["U"][:, 0].T, out["X"][:N, 0].T, rt)
    (up, yp, rt), (un, yn, _) = outs[True], outs[False]
    assert np.linalg.norm(up - un) > 1e-1
    ep, en = yp - rt, yn - rt
    assert np.linalg.norm(ep) / np.linalg.norm(en) < 0.9
    assert np.linalg.norm(ep[:, -1]) < 1e-3 and np.linalg.norm(en[:, -1]) < 1e-3


def test_generated_controller_entry_point(lmpc):
    # lmpc_compute_control == the reference's generated mpc_compute_control(control, state, reference,
    # disturbance) (codegen/mpc_update_qp.c:29-54, mpc_update_parameter.c) for N problems: control is
    # in (previous control) / out (u*).  K1 the way the reference runs it on its generated C
    # (runtests.jl:78-81), then a batch against solve(form_parameter(...)) -- same bits.
    g = load_golden("pendulum")
    mpc = lmpc.MPC(lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"]),
                   nx=4, nu=1, nr=2, nuprev=1)
    ctl = lmpc.GeneratedController(mpc)
    u = np.zeros((1, 1))
    ef = ctl.mpc_compute_control(u, np.array([[5.0, 5, 0, 0]]), np.zeros((1, 2)), None)
    assert ef[0] == 1 and abs(u[0, 0] - 1.7612519326) < 1e-6
    th = g["theta"][:3000]
    control = np.ascontiguousarray(th[:, 6:7].copy())
    ef = ctl.mpc_compute_control(control, th[:, :4], th[:, 4:6])
    x, efs, _, _ = mpc.control_model().solve(th)
    assert np.array_equal(ef, efs) and np.array_equal(control, x)
    # NULL reference = zeros (the C caller's NULL for an absent block)
    control = np.ascontiguousarray(th[:, 6:7].copy())
    ctl.mpc_compute_control(control, th[:, :4], None)
    th0 = th.copy()
    th0[:, 4:6] = 0
    assert np.array_equal(control, mpc.control_model().solve(th0)[0])
    # DAQP_WARMSTART build: second call starts from the first call's working sets, same answers
    warm = lmpc.GeneratedController(mpc, warm_start=True)
    c1 = np.ascontiguousarray(th[:, 6:7].copy())
    warm.mpc_compute_control(c1, th[:, :4], th[:, 4:6])
    c2 = np.ascontiguousarray(th[:, 6:7].copy())
    ef2 = warm.mpc_compute_control(c2, th[:, :4] + 1e-3, th[:, 4:6])
    th2 = th.copy()
    th2[:, :4] += 1e-3
    xs, efs2, _, _ = mpc.control_model().solve(th2)
    assert np.array_equal(ef2, efs2) and np.abs(c2 - xs).max() < 1e-9 and np.array_equal(c1, x)
    # errors: layout that does not add up to nth, entry point before a layout was given
    with pytest.raises(lmpc.LmpcError) as e:
        mpc.control_model().set_parameter_layout(4, 2, 0, 0, 0)
    assert e.value.code == -100
    qp = _qp_from_golden(lmpc, g, 1)
    with pytest.raises(lmpc.LmpcError):
        qp._layout = (4, 2, 0, 1, 0, 0)
        qp.compute_control(np.zeros((1, 1)), np.zeros((1, 4)))


def test_generated_controller_reference_condensation(lmpc):
    # /root/reference/test/runtests.jl:669-733: reference_preview + reference_condensation; the
    # generated controller receives the ny x Np trajectory and collapses it with traj2setpoint
    # (codegen/mpc_update_parameter.c:9-16).  Host and device entry points against the fixture.
    import torch
    g = load_golden("refcond_kat")
    mpc = lmpc.MPC(lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"]),
                   nx=2, nu=1, nr=2, Np=5, reference_preview=True, reference_condensation=True,
                   traj2setpoint=g["traj2setpoint"])
    # operator interface: compute_control(mpc, x; r = r_traj) condenses on the host (utils.jl:136-146)
    rt = np.array([[0.0, 0.5, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    assert np.abs(mpc.form_parameter([0.0, 0.0], r=rt) - g["theta"][0]).max() < 1e-12
    u_julia = mpc.compute_control([0.0, 0.0], r=rt)
    assert abs(u_julia[0] - g["X"][0, 0]) < 1e-9 and abs(u_julia[0] - float(g["u_full_preview"])) < 1e-5
    ctl = lmpc.GeneratedController(mpc)
    control = np.zeros((128, 1))
    ef = ctl.mpc_compute_control(control, g["state"], g["reference"], None)
    assert np.array_equal(ef, g["exitflag"])
    assert np.abs(control[:, 0] - g["X"][:, 0]).max() < 1e-10
    assert abs(control[0, 0] - u_julia[0]) < 1e-10                    # the reference's own assertion (:707)
    dev = torch.device("cuda", 0)
    cd = torch.zeros((128, 1), dtype=torch.float64, device=dev)
    efd = ctl.model.compute_control_device(cd, torch.from_numpy(g["state"]).to(dev),
                                           torch.from_numpy(np.ascontiguousarray(g["reference"])).to(dev))
    torch.cuda.synchronize()
    assert np.array_equal(cd.cpu().numpy(), control) and np.array_equal(efd.cpu().numpy(), ef)


def test_handles_are_independent_across_threads(lmpc):
    # include/lmpc_hip.h: calls on ONE handle must not overlap, DIFFERENT handles are independent (the
    # reference's DAQP workspace is one-per-MPC and not thread-safe either, types.jl:93-97,141): four
    # host threads, each with its own handle (two different problems), hammer the host-pointer entry
    # point at the same time; every answer must equal the single-threaded one
    import threading
    gp, gm = load_golden("pendulum"), load_golden("mass_spring")
    jobs = [(gp, gp["theta"][:4000]), (gm, gm["theta"][:600]), (gp, gp["theta"][4000:8000]), (gm, gm["theta"][300:900])]
    ref = []
    for g, th in jobs:
        ref.append(_qp_from_golden(lmpc, g, 1).solve(th))
    out = [None] * len(jobs)
    errs = []

    def work(i):
        try:
            g, th = jobs[i]
            qp = _qp_from_golden(lmpc, g, 1)
            for _ in range(8):
                out[i] = qp.solve(th)
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for (x, ef, it, act), (xr, efr, itr, actr) in zip(out, ref):
        assert np.array_equal(x, xr) and np.array_equal(ef, efr) and np.array_equal(it, itr) and np.array_equal(act, actr)


def test_generated_observer_entry_points(lmpc):
    # lmpc_predict_state / lmpc_correct_state == the generated mpc_predict_state / mpc_correct_state
    # (codegen/mpc_observer.c) for N scenarios; the reference checks them against predict!/correct! to
    # 1e-9 (runtests.jl:936-947, with a disturbance :977-987); here also against the C loops restated
    # term by term (same order, no fused multiply-add: identical bits asserted)
    import torch
    from oracle import observer as oobs
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    kd = oobs.kalman_filter([[1, 1], [0, 1.0]], [[0], [1.0]], [[1.0, 0], [0, 1.0]], Gd=[[0.5], [1.0]],
                            Dd=[[0.1], [0.0]], f_offset=[0.1, -0.2], h_offset=[0.3, 0.0], Q=[1.0, 1], R=[1e-2, 1.0])
    nx, nu, nd, ny = kd.dims
    dyn, meas, kt = kd.codegen_arrays()
    qp.set_observer(dyn, meas, kt, nx, nu, nd, ny)
    rng = np.random.default_rng(8)
    N = 1000
    x0, u, y, d = rng.standard_normal((N, nx)), rng.standard_normal((N, nu)), rng.standard_normal((N, ny)), rng.standard_normal((N, nd))
    xp = x0.copy()
    qp.predict_state(xp, u, d)
    ref = np.array([oobs.c_predict(dyn, x0[i], u[i], d[i], nx, nu, nd) for i in range(N)])
    assert np.array_equal(xp, ref)
    assert np.abs(xp - np.array([kd.predict(x0[i], u[i], d[i]) for i in range(N)])).max() < 1e-9
    xc = xp.copy()
    qp.correct_state(xc, y, d)
    ref = np.array([oobs.c_correct(meas, kt, xp[i], y[i], d[i], nx, ny, nd) for i in range(N)])
    assert np.array_equal(xc, ref)
    assert np.abs(xc - np.array([kd.correct(xp[i], y[i], d[i]) for i in range(N)])).max() < 1e-9
    # NULL disturbance = zeros (runtests.jl:942-946 passes C_NULL), device tensors in place
    xd = torch.from_numpy(x0).cuda()
    qp.predict_state(xd, torch.from_numpy(u).cuda(), None)
    torch.cuda.synchronize()
    ref0 = np.array([oobs.c_predict(dyn, x0[i], u[i], np.zeros(nd), nx, nu, nd) for i in range(N)])
    assert np.array_equal(xd.cpu().numpy(), ref0)
    with pytest.raises(lmpc.LmpcError):
        _qp_from_golden(lmpc, g, 1).predict_state(x0.copy(), u)        # no observer set


def test_observer_closed_loop_as_in_the_reference(lmpc):
    # /root/reference/test/runtests.jl:894-921 "Observer": invpend with Np = 100, move_block!([1,1,5,10,10]),
    # Kalman filter Q = 1e2*[1e-3,1,1e-3,1], R = [1,0.1]; 2000 closed-loop steps with measurement and
    # process noise: correct! -> compute_control(x_hat; r) -> predict! -> plant; x1 must settle within 1.0
    # of the reference 10.  Here for 64 noise realisations at once, every step through the generated
    # controller's three entry points on the device.
    import torch
    from oracle import mpc2mpqp as omm
    from oracle import observer as oobs
    p = omm.pendulum(Np=100, Nc=100).move_block([1, 1, 5, 10, 10])
    q = omm.mpc2mpqp(p)
    assert (q.n, q.nth) == (5, 7)
    mpc = lmpc.MPC(lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses), nx=4, nu=1, nr=2, nuprev=1)
    ctl = lmpc.GeneratedController(mpc)
    kf = oobs.kalman_filter(p.F, p.G, p.C, Q=1e2 * np.array([1e-3, 1, 1e-3, 1]), R=[1, 0.1])
    ctl.set_observer(*kf.codegen_arrays(), 4, 1, 0, 2)
    dev = torch.device("cuda", 0)
    S, T = 64, 2000
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    F = torch.from_numpy(p.F).to(dev)
    G = torch.from_numpy(p.G).to(dev)
    C = torch.from_numpy(p.C).to(dev)
    Wn = torch.tensor([[0, 0], [0.05, 0], [0, 0], [0, 0.005]], dtype=torch.float64, device=dev)
    vn = torch.tensor([0.05, 0.005], dtype=torch.float64, device=dev)
    x = torch.zeros((S, 4), dtype=torch.float64, device=dev)
    xhat = torch.zeros((S, 4), dtype=torch.float64, device=dev)
    u = torch.zeros((S, 1), dtype=torch.float64, device=dev)
    r0 = torch.zeros((S, 2), dtype=torch.float64, device=dev)
    r1 = torch.tensor([10.0, 0.0], dtype=torch.float64, device=dev).repeat(S, 1)
    flags = torch.empty(S, dtype=torch.int32, device=dev)
    worst = torch.ones(S, dtype=torch.int32, device=dev)
    x1_tail = []
    for k in range(T):
        y = x @ C.T + vn * torch.randn((S, 2), dtype=torch.float64, device=dev, generator=gen)
        ctl.model.correct_state(xhat, y.contiguous())
        ctl.model.compute_control_device(u, xhat, r0 if k < 20 else r1, exitflag=flags)
        worst = torch.minimum(worst, flags)
        ctl.model.predict_state(xhat, u)
        x = x @ F.T + u @ G.T + torch.randn((S, 2), dtype=torch.float64, device=dev, generator=gen) @ Wn.T
        if k >= T - 51:
            x1_tail.append(x[:, 0].clone())
    torch.cuda.synchronize()
    assert int(worst.min().item()) >= 1
    tail = torch.stack(x1_tail).cpu().numpy()
    assert np.all(np.abs(tail - 10.0) < 1.0), np.abs(tail - 10.0).max()


def test_randomized_differential_against_the_oracle(lmpc):
    # Sixty random problem shapes across every kernel family and row kind: n 1..14, 0..45 general rows,
    # 0..12 parameters, simple bounds present or not, SOFT / EQUALITY / IMMUTABLE / one-sided rows mixed in,
    # loose and tight bounds (feasible and infeasible batches), cold and warm starts -- each batch must
    # agree with the oracle in exit flags, iteration counts, active sets (bit for bit) and x (1e-10).
    from oracle import ldp as oldp
    rng = np.random.default_rng(20261003)
    kinds = {"lane": 0, "wave": 0}
    seen_flags = set()
    for trial in range(60):
        n = int(rng.integers(1, 15))
        mg = int(rng.integers(0, 46))
        ms = n if rng.random() < 0.7 else 0
        nth = int(rng.integers(0, 13))
        if ms + mg == 0:
            mg = 1
        nsoft = int(rng.integers(0, mg + 1)) if (mg and rng.random() < 0.4) else 0
        H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, max(nth, 1), nsoft, ms=ms)
        if nth == 0:
            f_theta, W = f_theta[:, :0], W[:, :0]
        scale = rng.choice([0.3, 1.0, 3.0])
        bu, bl = scale * bu, scale * bl
        m = ms + mg
        for j in range(m):                                   # sprinkle the other row kinds
            r = rng.random()
            if sense[j] == 0 and r < 0.08:
                bu[j], sense[j] = 1e30, 0                    # one-sided (lower bound only)
            elif sense[j] == 0 and r < 0.16:
                bl[j] = -1e30                                # one-sided (upper bound only)
            elif sense[j] == 0 and r < 0.20:
                bu[j], bl[j], sense[j] = 1e30, -1e30, 4      # IMMUTABLE: both bounds infinite
            elif sense[j] == 0 and j >= ms and r < 0.24 and n >= 3:
                v = rng.uniform(-0.2, 0.2)
                bu[j], bl[j], sense[j] = v, v, 5             # EQUALITY general row
        if (sense == 5).sum() > max(n - 1, 0):
            sense[sense == 5] = 0
        try:
            qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=min(n, 3))
        except lmpc.LmpcError as e:
            assert e.code in (-1, -6), e                     # setup flags of DAQP (infeasible bounds / dependent equalities)
            continue
        kinds["wave" if qp.kernel_name.endswith("wave") else "lane"] += 1
        theta = rng.uniform(-2, 2, (257, max(nth, 0))) if nth else np.zeros((257, 0))
        x, ef, it, act = _compare(qp, theta)
        seen_flags |= set(np.unique(ef).tolist())
        ok = ef >= 1
        if ok.sum() >= 8:
            _compare(qp, theta[ok][:64], warm=act[ok][:64])
    assert kinds["lane"] >= 10 and kinds["wave"] >= 10, kinds
    assert {1, -1} <= seen_flags and (2 in seen_flags), seen_flags


@pytest.mark.parametrize("layout", [(2, 1, 2, 1, 2), (3, 0, 0, 2, 0), (1, 2, 0, 0, 3), (4, 2, 1, 1, 1)])
def test_generated_controller_all_blocks_fused_and_unfused(lmpc, layout):
    # theta = [state; reference; disturbance; control[0:nup]; affine_parameter] assembled inside the
    # screening kernel (default on the lane path) or by update_parameter_kernel ("cc_fused" 0): both must
    # equal solve(theta) bit for bit, with NULL blocks standing for zeros and with the DAQP_WARMSTART mode
    nx, nr, nd, nup, npar = layout
    nth = nx + nr + nd + nup + npar
    nu = max(nup, 1) + 1
    rng = np.random.default_rng(sum(layout))
    n, mg = 2 * nu, 6
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth)
    N = 3000
    blocks = [rng.uniform(-1.5, 1.5, (N, w)) for w in (nx, nr, nd, nu, npar)]
    theta = np.ascontiguousarray(np.hstack([blocks[0], blocks[1], blocks[2], blocks[3][:, :nup], blocks[4]]))
    ref_qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=nu)
    xr, efr, _, actr = ref_qp.solve(theta)
    assert "lane" in ref_qp.kernel_name and (efr >= 1).mean() > 0.3
    for fused in (1, 0):
        qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=nu)
        qp.set_option("cc_fused", fused)
        qp.set_parameter_layout(nx, nr, nd, nup, npar)
        control = np.ascontiguousarray(blocks[3].copy())
        ef = qp.compute_control(control, blocks[0], blocks[1] if nr else None, blocks[2] if nd else None,
                                blocks[4] if npar else None)
        assert np.array_equal(ef, efr) and np.array_equal(control, xr)
        # warm: the second call starts from the first call's working sets
        control = np.ascontiguousarray(blocks[3].copy())
        qp.compute_control(control, blocks[0], blocks[1] if nr else None, blocks[2] if nd else None,
                           blocks[4] if npar else None, warm=True)
        c2 = np.ascontiguousarray(blocks[3].copy())
        ef2 = qp.compute_control(c2, blocks[0], blocks[1] if nr else None, blocks[2] if nd else None,
                                 blocks[4] if npar else None, warm=True)
        xw, efw, _, _ = ref_qp.solve(theta, warm=actr)
        assert np.array_equal(ef2, efw) and np.array_equal(c2, xw)
    # NULL blocks = zeros
    if nr or nd or npar:
        th0 = theta.copy()
        th0[:, nx:nx + nr + nd] = 0
        th0[:, nx + nr + nd + nup:] = 0
        control = np.ascontiguousarray(blocks[3].copy())
        qp.set_option("cc_fused", 1)
        qp.compute_control(control, blocks[0], None, None, None)
        assert np.array_equal(control, ref_qp.solve(th0)[0])


@pytest.mark.parametrize("name", ["pendulum", "mass_spring", "soft_doc"])
def test_warm_masks_in_place(lmpc, name):
    # the closed loop and the generated controller keep ONE mask buffer per handle: the previous call's
    # final working sets are read (warm) and this call's are written (active) in the same place -- lane /
    # screening path and wavefront path alike; results must equal the two-buffer call
    import torch
    g = load_golden(name)
    qp = _qp_from_golden(lmpc, g, 1)
    theta = g["theta"]
    x0, ef0, it0, act0 = qp.solve(theta)
    xw, efw, itw, actw = qp.solve(theta, warm=act0)
    dev = torch.device("cuda", 0)
    th = torch.from_numpy(theta).to(dev)
    buf = torch.from_numpy(act0.view(np.int64).copy()).to(dev)
    it = torch.empty(len(theta), dtype=torch.int32, device=dev)
    x, ef = qp.solve_device(th, iters=it, active=buf, warm=buf)
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), xw) and np.array_equal(ef.cpu().numpy(), efw)
    assert np.array_equal(it.cpu().numpy(), itw) and np.array_equal(buf.cpu().numpy().view(np.uint64), actw)


@pytest.mark.parametrize("name,warm", [("pendulum", False), ("pendulum", True), ("soft_doc", True)])
def test_f32_closed_loop_matches_the_f32_oracle(lmpc, name, warm):
    # lmpc_simulate_f32: the reference's float_type="float" controller (codegen.jl:19,31-37) in a closed
    # loop; checker: the binary32 build of the oracle's closed loop on the same rounded pack and plant
    from oracle import ldp as oldp
    from oracle import mpc2mpqp as omm
    g = load_golden(name)
    prob = omm.pendulum() if name == "pendulum" else omm.doc_simple_soft()
    s32 = lmpc.default_settings_f32()
    qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"],
                                  nout=int(g["nu"]), settings=s32)
    nx = prob.F.shape[0]
    rng = np.random.default_rng(12)
    N, T = 96, 25
    th = g["theta"][:N]
    x0 = th[:, :nx].astype(np.float32)
    nr = qp.nth - nx - int(g["nu"])
    r = th[:, nx:nx + nr].astype(np.float32)
    out = qp.simulate_f32(x0, T, prob.F, prob.G, r=r, warm=warm)
    ref = oldp.simulate(oracle_ldp_from(qp.ldp()), x0, T, prob.F, prob.G, r=r, settings=_copy_settings(lmpc, s32),
                        warm=warm, dtype=np.float32)
    assert np.array_equal(out["flag_min"], ref["flag_min"])
    assert np.abs(out["U"] - ref["U"]).max() <= 1e-6 and np.abs(out["X"] - ref["X"]).max() <= 1e-5
    assert np.array_equal(out["U"], ref["U"]) and np.array_equal(out["X"], ref["X"])      # observed: identical bits


def test_offset_free_observer_controller_call(lmpc):
    # generated mpc_compute_control_observer (reference src/observer.jl:156-196): the controller reads the
    # state and the estimated disturbance out of the augmented observer state.  Layout here: nx = 2, one
    # measured + one estimated disturbance (nd = 2), nr = 1, nuprev = 1.
    import torch
    nx, nr, ndm, ndo, nup = 2, 1, 1, 1, 1
    nth = nx + nr + ndm + ndo + nup
    rng = np.random.default_rng(77)
    n, mg, nu = 4, 5, 2
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=nu)
    qp.set_parameter_layout(nx, nr, ndm + ndo, nup, 0)
    N = 2000
    xaug = rng.uniform(-1, 1, (N, nx + ndo))
    ref = rng.uniform(-1, 1, (N, nr))
    dm = rng.uniform(-1, 1, (N, ndm))
    u0 = rng.uniform(-1, 1, (N, nu))
    theta = np.ascontiguousarray(np.hstack([xaug[:, :nx], ref, dm, xaug[:, nx:], u0[:, :nup]]))
    xr, efr, _, _ = qp.solve(theta)
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(u0.copy()).to(dev)
    ef = qp.compute_control_observer_device(c, torch.from_numpy(xaug).to(dev), ndm, torch.from_numpy(ref).to(dev),
                                            torch.from_numpy(dm).to(dev))
    torch.cuda.synchronize()
    assert np.array_equal(ef.cpu().numpy(), efr) and np.array_equal(c.cpu().numpy(), xr)
    # measured disturbance NULL = zeros (the generated code's `measured_disturbance ? ... : 0`)
    th0 = theta.copy()
    th0[:, nx + nr:nx + nr + ndm] = 0
    c = torch.from_numpy(u0.copy()).to(dev)
    qp.compute_control_observer_device(c, torch.from_numpy(xaug).to(dev), ndm, torch.from_numpy(ref).to(dev), None)
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy(), qp.solve(th0)[0])


def test_c_client_solves_on_the_gpu(lmpc, tmp_path):
    # examples/abi_check.c, the plain-C99 client of the shared library, on a box with a GPU: setup, a batch
    # through lmpc_solve_batch and through the generated controller's lmpc_compute_control, closed-form check
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    libdir = os.path.dirname(lmpc.LIB_PATH)
    exe = tmp_path / "abi_check"
    subprocess.run([shutil.which("gcc"), "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "abi_check.c"), "-o", str(exe), "-L", libdir, "-llmpc_hip",
                    f"-Wl,-rpath,{libdir}", "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "solved through the C ABI on a HIP device" in out.stdout


def test_measured_disturbance_closed_loop_with_observer_on_the_gpu(lmpc):
    # /root/reference/test/runtests.jl:951-961 "Observer + disturbance" for 128 noise realisations at once,
    # every step through lmpc_correct_state_device(y, d) -> lmpc_compute_control_device(xhat, r, d) ->
    # lmpc_predict_state_device(u, d); the reference's assertion |mean(ys[end-20:end])| < 1e-2 per realisation
    import torch
    from oracle import mpc2mpqp as omm
    from oracle import observer as oobs
    p = omm.observer_disturbance_kat()
    q = omm.mpc2mpqp(p)
    mpc = lmpc.MPC(lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses), nx=2, nu=1, nr=1, nd=2)
    ctl = lmpc.GeneratedController(mpc)
    kf = oobs.kalman_filter(p.F, p.G, p.C, Gd=p.Gd, Dd=p.Dd, Q=[1.0, 1], R=[1e-2])
    ctl.set_observer(*kf.codegen_arrays(), 2, 1, 2, 1)
    dev = torch.device("cuda", 0)
    S, T = 128, 100
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    t64 = dict(dtype=torch.float64, device=dev)
    F, G, Gd = (torch.from_numpy(np.asarray(a, float)).to(dev) for a in (p.F, p.G, p.Gd))
    x = torch.tensor([1.0, 0.0], **t64).repeat(S, 1)
    xhat = x.clone()
    d = torch.ones((S, 2), **t64)
    r = torch.zeros((S, 1), **t64)
    u = torch.zeros((S, 1), **t64)
    flags = torch.empty(S, dtype=torch.int32, device=dev)
    ys = []
    for k in range(T):
        ys.append((x[:, 0] + d[:, 1]).clone())                               # y = C x + Dd d
        ym = (x[:, :1] + d[:, 1:2] + 0.01 * torch.randn((S, 1), generator=gen, **t64)).contiguous()
        ctl.model.correct_state(xhat, ym, d)
        ctl.model.compute_control_device(u, xhat, r, d, exitflag=flags)
        assert int(flags.min().item()) >= 1
        ctl.model.predict_state(xhat, u, d)
        x = x @ F.T + u @ G.T + d @ Gd.T
    torch.cuda.synchronize()
    tail = torch.stack(ys[-21:]).mean(0).cpu().numpy()
    assert np.abs(tail).max() < 1e-2


def test_generated_controller_disturbance_preview(lmpc):
    # /root/reference/test/runtests.jl:735-774: the generated controller takes the nd x Np disturbance
    # trajectory as its `disturbance` argument (N_DISTURBANCE = nd*Np, mpc_update_parameter.c:19-21)
    g = load_golden("dist_preview_kat")
    mpc = lmpc.MPC(lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"]),
                   nx=2, nu=1, nr=1, nd=4, Np=4, disturbance_preview=True)
    # operator interface: compute_control(mpc, x; r, d = d_traj)
    d_traj = np.array([[0.0, 1.0, 1.0, 1.0]])
    assert np.array_equal(mpc.form_parameter([0.0, 0.0], r=[0.0], d=d_traj), g["theta"][0])
    u_julia = mpc.compute_control([0.0, 0.0], r=[0.0], d=d_traj)
    assert abs(u_julia[0] - g["X"][0, 0]) < 1e-10
    ctl = lmpc.GeneratedController(mpc)
    control = np.zeros((128, 1))
    ef = ctl.mpc_compute_control(control, g["state"], g["reference"], g["disturbance"])
    assert np.array_equal(ef, g["exitflag"]) and np.abs(control[:, 0] - g["X"][:, 0]).max() < 1e-10
    assert abs(control[0, 0] - u_julia[0]) < 1e-10                    # the reference's own assertion (:772)


def test_generated_controller_parameter_preview(lmpc):
    # /root/reference/test/runtests.jl:1270-1304 "Generalized Parameter Codegen for Explicit Preview": the
    # generated controller's affine_parameter argument carries one parameter per predicted step; closed form
    # u_0 = clip(2 p_0, 0, 2) (x = 0, r = 0, p = [0.5, 0, 0] -> u = 1)
    from oracle import mpc2mpqp as omm
    p = omm.parameter_preview_kat()
    q = omm.mpc2mpqp(p)
    mpc = lmpc.MPC(lmpc.MPQP(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses), nx=1, nu=1, nr=1, np_=3, Np=3,
                   parameter_preview=True)
    u_julia = mpc.compute_control([0.0], r=[0.0], p=[0.5, 0.0, 0.0])
    assert abs(u_julia[0] - 1.0) < 1e-12
    ctl = lmpc.GeneratedController(mpc)
    rng = np.random.default_rng(9)
    N = 500
    P = rng.uniform(-0.5, 1.5, (N, 3))
    P[0] = [0.5, 0.0, 0.0]
    control = np.zeros((N, 1))
    ef = ctl.mpc_compute_control(control, np.zeros((N, 1)), np.zeros((N, 1)), None, P)
    assert np.all(ef == 1) and np.abs(control[:, 0] - np.clip(2 * P[:, 0], 0, 2)).max() < 1e-12
    assert abs(control[0, 0] - u_julia[0]) < 1e-12


# ------------------------------------------------------------------ host pipeline, several GPUs behind one call
@pytest.mark.parametrize("chunk", [1024, 4096, 131072])
def test_host_pipeline_chunks_do_not_change_results(lmpc, chunk):
    # lmpc_solve_batch moves the batch through H2D / kernels / D2H in chunks; any chunk size, ragged last
    # chunk included, gives the bits of the device-resident call on the whole batch
    import torch
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    rng = np.random.default_rng(11)
    N = 3 * 4096 + 77
    theta = np.hstack([rng.uniform(-6, 6, (N, 4)), rng.uniform(-5, 5, (N, 1)), np.zeros((N, 1)), rng.uniform(-2, 2, (N, 1))])
    qp.set_option("host_chunk", chunk)
    x, ef, it, act = qp.solve(theta)
    th_d = torch.from_numpy(theta).cuda()
    it_d = torch.empty(N, dtype=torch.int32, device="cuda")
    ac_d = torch.zeros((N, qp.words), dtype=torch.int64, device="cuda")
    x_d, ef_d = qp.solve_device(th_d, iters=it_d, active=ac_d)
    torch.cuda.synchronize()
    assert np.array_equal(x, x_d.cpu().numpy()) and np.array_equal(ef, ef_d.cpu().numpy())
    assert np.array_equal(it, it_d.cpu().numpy()) and np.array_equal(act, ac_d.cpu().numpy().view(np.uint64))
    # unpinned copies (host_register 0) and a warm start through the pipeline
    qp.set_option("host_register", 0)
    x2, ef2, it2, act2 = qp.solve(theta, warm=act)
    assert np.array_equal(ef2, ef) and np.abs(x2 - x).max() <= TOL and np.array_equal(act2, act)
    _compare(qp, theta[:2000], warm=act[:2000])


def test_multi_device_entry_points(lmpc):
    # lmpc_setup_multi / lmpc_solve_batch_multi / lmpc_solve_batch_multi_device with however many GPUs this
    # box shows (one is fine): the sharded call returns the bits of the single-device call
    import torch
    g = load_golden("pendulum")
    nd = torch.cuda.device_count()
    mq = lmpc.MultiQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1)
    assert mq.ndev == nd and mq.nth == 7
    qp = _qp_from_golden(lmpc, g, 1)
    rng = np.random.default_rng(12)
    N = 200_003
    theta = np.hstack([rng.uniform(-6, 6, (N, 4)), rng.uniform(-5, 5, (N, 1)), np.zeros((N, 1)), rng.uniform(-2, 2, (N, 1))])
    x1, ef1, it1, act1 = qp.solve(theta)
    for q_ in mq.parts:
        q_.set_option("host_chunk", 30000)
    x, ef, it, act = mq.solve(theta)
    assert np.array_equal(x, x1) and np.array_equal(ef, ef1) and np.array_equal(it, it1) and np.array_equal(act, act1)
    # device-resident shards + gather to the first device
    off = lmpc.MultiQP.partition(N, nd)
    shards = [torch.from_numpy(theta[off[d]:off[d + 1]]).to(f"cuda:{d}") for d in range(nd)]
    xs, fs, xr, fr = mq.solve_device(shards, gather=True)
    assert np.array_equal(xr.cpu().numpy(), x1) and np.array_equal(fr.cpu().numpy(), ef1)
    for d in range(nd):
        assert np.array_equal(xs[d].cpu().numpy(), x1[off[d]:off[d + 1]])
    # the caller's current device is left alone by every entry point
    assert torch.cuda.current_device() == 0
    mq.close()


def test_mixed_controller_entry_points_on_one_handle(lmpc):
    # compute_control_observer_device, then the host compute_control (regrows its staging
    # block), then the observer call again -- the observer scratch must survive
    import torch
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    qp.set_parameter_layout(4, 2, 0, 1, 0)
    rng = np.random.default_rng(13)
    N = 3000
    state = rng.uniform(-3, 3, (N, 4)); ref = rng.uniform(-2, 2, (N, 2)); ctrl0 = rng.uniform(-1, 1, (N, 1))

    def observer_call():
        c = torch.from_numpy(ctrl0.copy()).cuda()
        ef = qp.compute_control_observer_device(c, torch.from_numpy(state).cuda(), 0, reference=torch.from_numpy(ref).cuda())
        torch.cuda.synchronize()
        return c.cpu().numpy(), ef.cpu().numpy()

    c1, e1 = observer_call()
    big = 3 * N                                              # larger batch: the host staging block regrows
    ch = np.tile(ctrl0, (3, 1)).copy()
    efh = qp.compute_control(ch, np.tile(state, (3, 1)), np.tile(ref, (3, 1)))
    c2, e2 = observer_call()
    assert np.array_equal(c1, c2) and np.array_equal(e1, e2)
    assert np.array_equal(ch[:N], c1) and np.array_equal(efh[:N], e1) and big == len(ch)


# ------------------------------------------------------------------ one-launch kernel (lmpc_fast_kernel.hpp)
def _boxed_problem(rng, n, nth, spread):
    """Random strictly convex QP with the n simple bounds as its only constraints (the input-bounded MPC shape)."""
    Rm = rng.normal(size=(n, n))
    H = Rm @ Rm.T + n * np.eye(n) * rng.uniform(0.05, 1.0)
    f_theta = rng.normal(size=(n, nth)) * spread
    f = rng.normal(size=n) * 0.3
    bu = rng.uniform(0.2, 1.5, n)
    bl = -rng.uniform(0.2, 1.5, n)
    W = rng.normal(size=(n, nth)) * 0.2 * (rng.uniform() < 0.5)
    return H, f, f_theta, bu, bl, W


@pytest.mark.parametrize("n,nth", [(2, 1), (3, 5), (4, 16), (5, 7), (5, 8), (4, 9), (5, 3)])
def test_one_launch_kernel_matches_two_kernel_form_and_oracle(lmpc, n, nth):
    # small boxed problems, cold start: ONE kernel (streaming pass + straight-line tiers + generic loop for the
    # rest) against the two-kernel form ("fast" 0) and against the oracle, with parameter spreads from "hardly
    # ever iterates" to "most problems iterate"; ragged batch sizes around the tile and workgroup sizes; one and
    # n outputs.  On this problem family rows are almost only ever ADDED (the oracle on _boxed_problem at all 56
    # instantiated pairs x these three spreads: no point with iters > |active set| + 1 at 53 pairs, 2.1 % at
    # most): the straight-line tiers finish nearly every point, the generic loop behind them (fast_fallback)
    # hardly runs here.  tests/test_gpu_fast.py has the problems on which it does, at every pair.
    import torch
    rng = np.random.default_rng(100 * n + nth)
    for spread, nout in ((0.3, 1), (1.5, n), (6.0, 1)):
        H, f, f_theta, bu, bl, W = _boxed_problem(rng, n, nth, spread)
        qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, np.zeros((0, n)), bu, bl, W, nout=nout)
        assert qp.kernel_name.startswith(f"fast<{n}>|screen+lane")
        for N in (1, 63, 64, 65, 1500, 30011):
            theta = rng.normal(size=(N, nth))
            x, ef, it, act = _compare(qp, theta)                     # (fast path on by default) vs the oracle
            qp.set_option("fast", 0)
            x0, ef0, it0, act0 = qp.solve(theta)
            qp.set_option("fast", 1)
            assert np.array_equal(x, x0) and np.array_equal(ef, ef0) and np.array_equal(it, it0) and np.array_equal(act, act0)
        for nstr in (1, 2, 4):                                        # any split of streaming / solving wavefronts
            qp.set_option("fast_nstr", nstr)
            qp.set_option("fast_tiles", 8 if nstr == 2 else 0)
            x1, ef1, it1, act1 = qp.solve(theta)
            assert np.array_equal(x1, x) and np.array_equal(ef1, ef) and np.array_equal(it1, it) and np.array_equal(act1, act)
        # device-resident call without the optional outputs
        th_d = torch.from_numpy(theta).cuda()
        xd, efd = qp.solve_device(th_d)
        torch.cuda.synchronize()
        assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(efd.cpu().numpy(), ef)
        if spread == 6.0:
            assert it.max() >= 3 and (it >= 2).mean() > 0.5, "the hard spread should make most problems iterate"


def test_one_launch_kernel_respects_the_solver_guards(lmpc):
    # an iteration limit or cycle tolerance that could fire inside the straight-line tiers switches them off
    # (host-side check): flags and iteration counts stay those of the oracle
    g = load_golden("pendulum")
    rng = np.random.default_rng(21)
    N = 5000
    theta = np.hstack([rng.uniform(-20, 20, (N, 4)), rng.uniform(-20, 20, (N, 1)), np.zeros((N, 1)), rng.uniform(-2, 2, (N, 1))])
    from oracle import ldp as oldp
    for lim, cyc in ((3, 10), (5, 10), (10000, 2)):
        s = lmpc.default_settings()
        s.iter_limit, s.cycle_tol = lim, cyc
        so = oldp.default_settings()
        so.iter_limit, so.cycle_tol = lim, cyc
        qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"],
                                      nout=1, settings=s)
        x, ef, it, act = _compare(qp, theta, settings=so)
        if lim == 3:
            assert (ef == -4).any()


def test_one_launch_kernel_failure_is_visible(lmpc):
    """The one-launch kernel's bounded waits are never expected to run out; if one does, nothing may look like
    success (/root/reference/src/utils.jl:46 asserts exitflag >= 1): every queued problem carries the provisional
    flag -8 until its solving lane overwrites it, and the handle reports LMPC_ERR_HIP at its next check.  The test
    hook "fast_spin_limit" makes the waits give up at their first poll."""
    import torch
    from oracle import ldp as oldp
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    assert "fast" in qp.kernel_name
    L = oracle_ldp_from(qp.ldp())
    rng = np.random.default_rng(33)
    N = 200_000
    theta = np.hstack([rng.uniform(-20, 20, (N, 4)), rng.uniform(-20, 20, (N, 1)), np.zeros((N, 1)), rng.uniform(-2, 2, (N, 1))])
    xo, efo, ito, acto = oldp.solve_batch(L, theta)
    th_d = torch.from_numpy(theta).to("cuda:0")
    raised = 0
    for trial in range(6):
        qp.set_option("fast_spin_limit", 1)              # give up at the first poll that finds nothing to claim
        x_d = torch.full((N, 1), float("nan"), dtype=torch.float64, device="cuda:0")
        ef_d = torch.full((N,), 12345, dtype=torch.int32, device="cuda:0")
        qp.solve_device(th_d, x=x_d, exitflag=ef_d)
        try:
            qp.check()                                   # waits for the GPU, then reports the kernel's error word
            err = None
        except lmpc.LmpcError as e:
            err = e
        ef, x = ef_d.cpu().numpy(), x_d.cpu().numpy()
        assert not (ef == 12345).any()                   # every problem has a flag of this call
        done = ef != -8
        assert np.array_equal(ef[done], efo[done]) and np.array_equal(x[done], xo[done])
        if err is not None:
            raised += 1
            assert err.code == -102 and "one-launch kernel" in str(err)
        else:
            assert done.all()                            # no error word => nothing left unfinished
        if not done.all():
            assert err is not None                       # unfinished problems never come without the error
        qp.check()                                       # reported once
    assert raised >= 1
    # the error also stops the NEXT call on the handle when nobody checked in between
    qp.set_option("fast_spin_limit", 1)
    for _ in range(20):
        qp.solve_device(th_d, x=x_d, exitflag=ef_d)
        torch.cuda.synchronize()
        qp.set_option("fast_spin_limit", 0)
        try:
            qp.solve_device(th_d, x=x_d, exitflag=ef_d)
        except lmpc.LmpcError as e:
            assert e.code == -102
            break
        qp.set_option("fast_spin_limit", 1)
    else:
        raise AssertionError("the error word was never raised")
    # back to normal
    qp.set_option("fast_spin_limit", 0)
    qp.solve_device(th_d, x=x_d, exitflag=ef_d)
    qp.check()
    assert np.array_equal(ef_d.cpu().numpy(), efo) and np.array_equal(x_d.cpu().numpy(), xo)
    # host-pointer entry point: the failure comes back from the call itself
    qp.set_option("fast_spin_limit", 1)
    seen = 0
    for _ in range(10):
        try:
            qp.solve(theta)
        except lmpc.LmpcError as e:
            assert e.code == -102
            seen += 1
    assert seen >= 1
    qp.set_option("fast_spin_limit", 0)
    x, ef, it, act = qp.solve(theta)
    assert np.array_equal(ef, efo) and np.array_equal(x, xo)


def test_one_launch_kernel_very_large_batch(lmpc):
    """3e7 points in one call: the workgroup's LDS queue is capped (96 tiles) and the grid grows past one resident
    round instead of the queue past the LDS limit.  Size-independent checks + an oracle sample."""
    import torch
    from oracle import ldp as oldp
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    L = oracle_ldp_from(qp.ldp())
    N = 30_000_011
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(5)
    lo = torch.tensor([-5, -5, -0.3, -2, -5, 0, -2], dtype=torch.float64, device="cuda:0")
    hi = torch.tensor([5, 5, 0.3, 2, 5, 0, 2], dtype=torch.float64, device="cuda:0")
    th_d = lo + (hi - lo) * torch.rand((N, 7), dtype=torch.float64, device="cuda:0", generator=gen)
    x_d = torch.full((N, 1), float("nan"), dtype=torch.float64, device="cuda:0")
    ef_d = torch.full((N,), 12345, dtype=torch.int32, device="cuda:0")
    qp.solve_device(th_d, x=x_d, exitflag=ef_d)
    qp.check()
    assert bool((ef_d == 1).all()) and bool(torch.isfinite(x_d).all())
    assert float(x_d.abs().max()) <= 2.0 + 1e-5                       # |u| <= 2 (input bound of the example) up to primal_tol
    idx = torch.cat([torch.arange(0, 4000, device="cuda:0"), torch.arange(N - 4000, N, device="cuda:0"),
                     torch.randint(0, N, (12000,), device="cuda:0", generator=gen)])
    xo, efo, _, _ = oldp.solve_batch(L, th_d[idx].cpu().numpy())
    assert np.array_equal(x_d[idx].cpu().numpy(), xo) and np.array_equal(ef_d[idx].cpu().numpy(), efo)
    qp.set_option("fast_tiles", 256)                                  # the option is clamped to the same cap
    x2 = torch.empty_like(x_d); f2 = torch.empty_like(ef_d)
    qp.solve_device(th_d[:3_000_000], x=x2[:3_000_000], exitflag=f2[:3_000_000])
    qp.check()
    assert bool((x2[:3_000_000] == x_d[:3_000_000]).all())


# ------------------------------------------------------------------ reference-held vectors through the device path
def test_reference_formatting_vectors_on_the_device(lmpc):
    """/root/reference/test/runtests.jl:1401-1428, number for number, through lmpc_form_parameter_device: the
    reference / disturbance block of theta the device forms is the vector the reference's test expects."""
    import torch

    def handle(nx, ny, nd, Np, rp, dp):
        nth = nx + ny * (Np if rp else 1) + nd * (Np if dp else 1)
        return lmpc.BatchedQP.from_mpqp(np.eye(1), np.zeros(1), np.zeros((1, nth)), np.zeros((0, 1)), np.ones(1),
                                        -np.ones(1), np.zeros((1, nth)), nout=1)

    cu = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, float))).cuda()
    x2 = cu(np.array([[0.25, -0.5], [1.0, 2.0], [3.0, 4.0]]))
    qp = handle(2, 2, 0, 4, True, False)
    for r, want in (([1.0, 2.0], np.tile([1.0, 2.0], 4)),                                                      # :1406
                    ([[1.0, 2, 3, 4, 5], [10.0, 20, 30, 40, 50]], [1.0, 10.0, 2.0, 20.0, 3.0, 30.0, 4.0, 40.0]),  # :1407
                    ([[1.0, 2.0], [10.0, 20.0]], [1.0, 10.0, 2.0, 20.0, 2.0, 20.0, 2.0, 20.0])):                # :1409
        th = qp.form_parameter_device(x2, r=cu(r), r_preview=4)
        torch.cuda.synchronize()
        assert np.array_equal(th.cpu().numpy(), np.hstack([x2.cpu().numpy(), np.tile(want, (3, 1))]))
    plain = handle(2, 2, 0, 4, False, False)
    th = plain.form_parameter_device(x2, r=cu([[7.0, 8.0, 9.0], [1.0, 2.0, 3.0]]))                              # :1416
    torch.cuda.synchronize()
    assert np.array_equal(th.cpu().numpy()[:, 2:], np.tile([7.0, 1.0], (3, 1)))
    x1 = cu(np.array([[0.5], [1.5]]))
    dq = handle(1, 1, 1, 4, False, True)
    r0 = cu([0.0])
    for d, want in (([3.0], [3.0, 3.0, 3.0, 3.0]), ([[1.0, 2.0]], [1.0, 2.0, 2.0, 2.0])):                       # :1421-1422
        th = dq.form_parameter_device(x1, r=r0, d=cu(d), d_preview=4)
        torch.cuda.synchronize()
        assert np.array_equal(th.cpu().numpy()[:, 2:], np.tile(want, (2, 1)))
    dplain = handle(1, 1, 1, 4, False, False)
    th = dplain.form_parameter_device(x1, r=r0, d=cu([[7.0, 8.0, 9.0]]))                                       # :1427
    torch.cuda.synchronize()
    assert np.array_equal(th.cpu().numpy()[:, 2:], np.tile([7.0], (2, 1)))
    # a block of the wrong width is refused (the reference throws, :1411-1413 / :1423-1424)
    with pytest.raises(lmpc.LmpcError):
        qp.form_parameter_device(x2, r=cu([1.0]), r_preview=4)
    with pytest.raises(lmpc.LmpcError):
        dq.form_parameter_device(x1, r=r0, d=cu(np.ones((2, 2))), d_preview=4)


def test_reference_preview_controller_three_ways(lmpc):
    """/root/reference/test/runtests.jl:627-667 "Codegen Reference Preview - Full": the reference asserts that
    its Julia path and its generated C agree to 1e-10 on this controller and this trajectory.  Here the same
    controller through (a) lmpc_setup on the mpQP, (b) lmpc_setup_ldp on the arrays the generator would write
    (the oracle's numpy transform), (c) the oracle itself -- and (d) the generated controller's entry point fed
    with the trajectory exactly as the reference's ccall passes it (r_traj, column by column)."""
    from oracle import ldp as oldp
    g = load_golden("refprev_full_kat")
    theta = g["theta"]
    qa = _qp_from_golden(lmpc, g, 1)
    xa, efa, ita, acta = _compare(qa, theta)                       # (a) vs (c) on the library's own pack
    L = oldp.qp2ldp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1)
    qb = lmpc.BatchedQP.from_ldp(L.M, L.du0, L.dl0, L.Dth, L.Rout, L.x0, L.Xth, L.sense, ms=L.ms)
    xb, efb, itb, actb = _compare(qb, theta)                       # (b) vs (c) on the numpy pack
    assert np.array_equal(efa, efb) and np.array_equal(acta, actb)
    assert np.abs(xa - xb).max() < 1e-10                           # the bar the reference's test sets
    assert np.abs(xa[:, 0] - g["X"][:, 0]).max() < 1e-10           # ... and the committed answers
    assert abs(xa[0, 0] - g["u_julia_equals_c"][0]) < 1e-10
    # (d) mpc_compute_control(u, x, r_traj, d) as at runtests.jl:659
    qa.set_parameter_layout(2, 10, 0, 0, 0)
    N = theta.shape[0]
    ctrl = np.zeros((N, 1))
    ef = qa.compute_control(ctrl, theta[:, :2].copy(), reference=theta[:, 2:].copy())
    assert np.array_equal(ef, efa) and np.array_equal(ctrl, xa)
    assert np.array_equal(theta[0, 2:], g["r_traj"].T.reshape(-1))


def test_release_scratch_between_batches(lmpc):
    # staging buffers only grow; lmpc_release_scratch gives them back and the next call allocates again
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    theta = g["theta"]
    a = qp.solve(theta)
    out = qp.simulate(theta[:500, :4], 5, np.eye(4), np.zeros((4, 1)), r=theta[:500, 4:6])
    qp.release_scratch()
    b = qp.solve(theta)
    out2 = qp.simulate(theta[:500, :4], 5, np.eye(4), np.zeros((4, 1)), r=theta[:500, 4:6])
    assert all(np.array_equal(p_, q_) for p_, q_ in zip(a, b))
    assert np.array_equal(out["U"], out2["U"]) and np.array_equal(out["x"], out2["x"])


def test_caller_pinned_arrays(lmpc):
    # lmpc_pin_host: a caller that reuses its arrays pins them once; the host pipeline then leaves them alone,
    # a second pin of the same pages is refused (the runtime would abort on a doubly registered page)
    import ctypes
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    L = lmpc.lib()
    rng = np.random.default_rng(31)
    N = 300_000
    theta = np.ascontiguousarray(np.hstack([rng.uniform(-6, 6, (N, 4)), rng.uniform(-5, 5, (N, 1)), np.zeros((N, 1)),
                                            rng.uniform(-2, 2, (N, 1))]))
    import mmap

    def paged(shape, dtype):          # page-aligned, pages of its own (what lmpc_pin_host asks of the caller)
        a_ = np.frombuffer(mmap.mmap(-1, int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape)
        a_[...] = 0
        return a_

    th_p = paged(theta.shape, np.float64); th_p[...] = theta; theta = th_p
    x = paged((N, 1), np.float64); ef = paged((N,), np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    x_ref, ef_ref, _, _ = qp.solve(theta, want_iters=False, want_active=False)
    for a_ in (theta, x, ef):
        assert L.lmpc_pin_host(vp(a_), a_.nbytes) == 1
    assert L.lmpc_pin_host(vp(theta), 4096) == -100            # same pages again
    for _ in range(3):
        assert L.lmpc_solve_batch(qp._h, N, vp(theta), vp(x), vp(ef), None, None, None) == 1
        assert np.array_equal(x, x_ref) and np.array_equal(ef, ef_ref)
    for a_ in (theta, x, ef):
        assert L.lmpc_unpin_host(vp(a_)) == 1
    assert L.lmpc_unpin_host(vp(theta)) == -100


# ------------------------------------------------------------------ long horizons: 64 <= n <= 127 (two variable slots per lane)
@pytest.mark.parametrize("N", [50, 75, 100, 125])
def test_reference_benchmark_class_long_horizons(lmpc, N):
    """The reference's published benchmark sweeps the pendulum's horizons together, Np = Nc = N in {50, 75, 100,
    125}, with input and state constraints (docs/src/manual/benchmark.md:4-16): n = N variables, 3N - 2 rows,
    2N - 2 of them soft.  theta: the closed loops of the example's scenarios plus perturbed copies (fixture)."""
    g = load_golden(f"pendulum_N{N}")
    theta = g["theta"]
    qp = _qp_from_golden(lmpc, g, 1)
    assert qp.kernel_name.endswith("wave") and qp.n == N and qp.m == 3 * N - 2
    x, ef, it, act = _compare(qp, theta)                         # bit-level against the oracle on the library's pack
    assert np.all(ef >= 1)
    # against the committed answers (oracle on the numpy pack: 1/rho = 1e6 amplifies the 1e-16 between the packs)
    assert np.array_equal(ef, g["exitflag"]) and np.abs(x[:, 0] - g["X"][:, 0]).max() < 1e-5
    # the whole trajectory (nout = n > 64: outputs in blocks of 64 lanes) and a warm start from the final sets
    qt = _qp_from_golden(lmpc, g)
    xt, eft, itt, actt = _compare(qt, theta[:200])
    assert np.array_equal(xt[:, 0], x[:200, 0]) and np.array_equal(actt, act[:200])
    _compare(qt, theta[:200], warm=actt)
    # binary32 on the same kernel
    from oracle import ldp as oldp
    q32 = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1,
                                   settings=lmpc.default_settings_f32())
    th32 = theta[:256].astype(np.float32)
    x32, ef32, it32, act32 = q32.solve_f32(th32)
    xo, efo, ito, acto = oldp.solve_batch(oracle_ldp_from(q32.ldp()), th32, oldp.default_settings_f32(), dtype=np.float32)
    assert np.array_equal(ef32, efo) and np.array_equal(it32, ito) and np.array_equal(act32, acto) and np.array_equal(x32, xo)


@pytest.mark.parametrize("n,mg,nsoft", [(64, 20, 0), (65, 10, 3), (90, 200, 20), (127, 60, 0)])
def test_wave_kernel_two_variable_slots_random_problems(lmpc, n, mg, nsoft):
    # random problems around the slot boundary (n = 64 is the last single-slot size), hard and soft general rows,
    # feasible and infeasible points, iteration counts and masks against the oracle
    rng = np.random.default_rng(7 * n + mg)
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, 5)
    sense = sense.copy()
    sense[n:n + nsoft] |= 8
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, 2 * bu, 2 * bl, 0.3 * W, sense, nout=min(n, 70))
    assert qp.kernel_name.endswith("wave")
    theta = rng.uniform(-1.5, 1.5, (160, 5))
    x, ef, it, act = _compare(qp, theta)
    ok = ef >= 1
    if ok.sum() > 4:
        _compare(qp, theta[ok][:48], warm=act[ok][:48])


# ------------------------------------------------------------------ BASELINE configs 3 and 5 at the sizes the bench runs
def test_mass_spring_3in_full_size_properties(lmpc):
    """BASELINE config 3 as worded (oscillating masses, 12 states / 3 inputs, Nc = 10) at its full 10^6 points,
    through size-independent properties: every solved point satisfies all 84 two-sided constraints to primal_tol
    (in the normalised units the solver works in) and is stationary on its reported active set; unsolved points
    carry a DAQP failure flag; a strided sample of 3000 points agrees with the oracle bit for bit."""
    import torch
    import bench
    from oracle import ldp as oldp
    g = load_golden("mass_spring_3in")
    n, N = g["H"].shape[0], 1_000_000
    qp = _qp_from_golden(lmpc, g)
    theta = bench.make_theta("mass_spring_3in", N, 77)
    th_d = torch.from_numpy(theta).cuda()
    it_d = torch.empty(N, dtype=torch.int32, device="cuda")
    ac_d = torch.zeros((N, qp.words), dtype=torch.int64, device="cuda")
    x_d, ef_d = qp.solve_device(th_d, iters=it_d, active=ac_d)
    torch.cuda.synchronize()
    x, ef = x_d.cpu().numpy(), ef_d.cpu().numpy()
    assert set(np.unique(ef)) <= {1, -1, -2}, np.unique(ef)
    ok = ef == 1
    assert 0.2 < ok.mean() < 0.4                      # the bench line's solved_fraction (0.28) for this sampling
    Afull = np.vstack([np.eye(n)[:qp.ms], g["A"]])
    sc = np.linalg.norm(Afull @ np.linalg.inv(np.linalg.cholesky(g["H"]).T), axis=1)     # row norms of M before scaling
    V = x[ok] @ Afull.T
    hi = (g["bu"] + theta[ok] @ g["W"].T - V) / sc
    lo = (V - (g["bl"] + theta[ok] @ g["W"].T)) / sc
    assert min(hi.min(), lo.min()) > -1.01e-6
    # stationarity on the reported active set, on a sample (dense KKT solve per point)
    bits = ac_d.cpu().numpy().view(np.uint64)
    idx = np.nonzero(ok)[0][::997][:300]
    m = qp.m
    for i in idx:
        rows = [j for j in range(m) if (int(bits[i, j >> 6]) >> (j & 63)) & 1 or (int(bits[i, (m + j) >> 6]) >> ((m + j) & 63)) & 1]
        grad = g["H"] @ x[i] + g["f"] + g["f_theta"] @ theta[i]
        if rows:
            lam = np.linalg.lstsq(Afull[rows].T, -grad, rcond=None)[0]
            grad = grad + Afull[rows].T @ lam
        assert np.abs(grad).max() < 1e-6 * max(1.0, np.abs(g["H"]).max())
    sel = np.arange(0, N, 333)[:3000]
    L = oracle_ldp_from(qp.ldp())
    xo, efo, ito, acto = oldp.solve_batch(L, theta[sel])
    assert np.array_equal(ef[sel], efo) and np.array_equal(it_d.cpu().numpy()[sel], ito) and np.array_equal(bits[sel], acto)
    assert np.abs(x[sel] - xo).max() <= TOL


def test_hybrid_f32_bench_size_properties(lmpc):
    """BASELINE config 5 (hybrid MPC, binary32) at the bench's 10^5 points: every point solved, every binary input
    on one of its bounds (the reference's own assertion, runtests.jl:831-834, at 1e-5), a sample bit-identical to
    the binary32 oracle."""
    import bench
    from oracle import ldp as oldp
    g = load_golden("satellite20")
    qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"],
                                  nout=g["H"].shape[0], settings=lmpc.default_settings_f32())
    N = 100_000
    theta = bench.make_theta("satellite20", N, 78).astype(np.float32)
    x, ef, it, act = qp.solve_f32(theta)
    assert np.all(ef == 1)
    binary = (g["senses"] & 16) != 0
    xb = x[:, :len(binary)][:, binary[:x.shape[1]]]
    bu, bl = g["bu"][binary], g["bl"][binary]
    assert np.all((np.abs(xb - bu) < 1e-5) | (np.abs(xb - bl) < 1e-5))
    sel = np.arange(0, N, 211)[:400]
    xo, efo, ito, acto = oldp.solve_batch(oracle_ldp_from(qp.ldp()), theta[sel], oldp.default_settings_f32(), dtype=np.float32)
    assert np.array_equal(ef[sel], efo) and np.array_equal(it[sel], ito) and np.array_equal(act[sel], acto)
    assert np.array_equal(x[sel], xo)


def test_branch_and_bound_in_two_passes_is_the_same_search(lmpc):
    """Round 4: a hybrid batch first runs at a smaller working-set capacity (more wavefronts resident) and the points
    that outgrow it are searched again at the full one (lmpc_wave_launch.hpp, bnb_first_pass_cap).  One pass
    ("wave_two_pass" 0), the default split (48 rows for the satellite's 40 binaries: nothing overflows) and a first
    pass forced so small that most points overflow (42 rows) must return the same arrays, binary64 and binary32; a
    sample against the oracle's search.  Also the lazy snapshots of a node's factor (written only when a removal
    would break the leading-block property) against the oracle's eager ones."""
    import bench
    from oracle import ldp as oldp
    g = load_golden("satellite20")
    N = 12_288
    theta = bench.make_theta("satellite20", N, 5)
    outs = {}
    for name, opts in (("one", {"wave_two_pass": 0}), ("default", {}), ("forced42", {"wave_two_pass": 1, "wave_cap1": 42})):
        qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=3)
        for k, v in opts.items():
            qp.set_option(k, v)
        outs[name] = qp.solve(theta)
        qp32 = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=3,
                                        settings=lmpc.default_settings_f32())
        for k, v in opts.items():
            qp32.set_option(k, v)
        outs[name + "32"] = qp32.solve_f32(theta.astype(np.float32))
        if name == "one":
            L = oracle_ldp_from(qp.ldp())
        qp.close(); qp32.close()
    for suf in ("", "32"):
        a = outs["one" + suf]
        assert np.all(a[1] == 1)
        for other in ("default", "forced42"):
            b = outs[other + suf]
            for u, v in zip(a, b):
                assert np.array_equal(u, v), (other, suf)
    sel = np.arange(0, N, 97)[:100]
    xo, efo, ito, acto = oldp.solve_batch(L, theta[sel])
    x, ef, it, act = outs["default"]
    assert np.array_equal(x[sel], xo) and np.array_equal(ef[sel], efo) and np.array_equal(it[sel], ito) and np.array_equal(act[sel], acto)


# ------------------------------------------------------------------ screening pass in front of the wavefront kernel
@pytest.mark.parametrize("n,mg,nth,nsoft,nout,imm,seed", [
    (20, 30, 6, 0, 1, False, 0),       # m = 50: one constraint slot per lane
    (16, 120, 7, 12, 3, True, 1),      # m = 136, soft rows, immutable rows below and above row 64, transposed stores
    (40, 300, 20, 0, 20, True, 2),     # m = 340, padded parameter columns (nth > 16), more than 16 outputs
    (100, 60, 5, 0, 2, False, 3),      # two variable slots per lane
    (13, 3, 1, 1, 1, False, 4),        # one parameter
])
def test_screening_pass_in_front_of_wave_kernel(lmpc, n, mg, nth, nsoft, nout, imm, seed):
    # A wavefront-kernel problem whose unconstrained optimum is feasible ends in its first iteration; the streaming
    # pass finishes those and hands the wavefront kernel a work list of the others.  Which kernel finishes a problem
    # must not change one bit: screened == unscreened == oracle, cold and warm, at batch sizes around the tile edges.
    rng = np.random.default_rng(4200 + seed)
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth, nsoft=nsoft)
    if imm:
        sense[[3, n + 70, n + mg - 1]] |= 4        # IMMUTABLE: never enters the working set, may be violated
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=nout)
    assert qp.kernel_name.endswith("wave")
    for N in (1, 63, 257, 3000):
        # a mix: most points close to the origin (nothing violated), some far out (iterations needed)
        theta = rng.standard_normal((N, nth)) * np.where(rng.random(N) < 0.6, 0.05, 1.5)[:, None]
        qp.set_option("screen_wave", 0)
        x0, ef0, it0, act0 = qp.solve(theta)
        qp.set_option("screen_wave", 1)
        x1, ef1, it1, act1 = _compare(qp, theta)
        assert np.array_equal(x0, x1) and np.array_equal(ef0, ef1) and np.array_equal(it0, it1)
        assert np.array_equal(act0, act1)
        if N == 3000:
            settled = (it1 == 1) & (ef1 == 1)
            assert 0.1 < settled.mean() < 0.99, settled.mean()     # both kernels had work
            ok = ef1 >= 1
            xw, efw, itw, actw = _compare(qp, theta[ok], warm=act1[ok])
            assert np.array_equal(efw, ef1[ok])
    # consecutive calls alternate the two counter sets; a batch with nothing to iterate leaves an empty list
    xz, efz, itz, actz = qp.solve(np.zeros((500, nth)))
    assert np.all(efz == 1) and np.all(itz == 1) and not actz.any()
    _compare(qp, rng.standard_normal((200, nth)) * 2.0)


def test_benched_configuration_is_parity_checked(lmpc):
    """The exact shape bench.py times: three handles on three HIP streams, each told
    `in_flight = 3`, six rotating 1e6-point batches and as many output buffers, launches enqueued back to back
    without synchronisation in between -- then every buffer against the oracle on a sample, and two full batches
    against the one-call-at-a-time results of a fresh handle on library defaults."""
    import torch
    import bench
    dev = torch.device("cuda", 0)
    W = bench.Workload(torch, lmpc, "pendulum", bench.BATCH, dev, 0, 0, 3, options={"in_flight": 3})
    assert W.nrot >= 6 and W.nstreams == 3 and "fast" in W.kernel
    steps = 2 * W.nbuf + 1
    for k in range(steps):
        W.launch(k)
    torch.cuda.synchronize(dev)
    for q_ in W.qps:
        q_.check()
    ver = W.verify_steps(list(range(steps - W.nbuf, steps)), per_step=3000)
    assert ver["verified"] and ver["exit_flag_mismatches"] == 0 and ver["max_abs_dx"] == 0.0
    ref = _qp_from_golden(lmpc, load_golden("pendulum"), 1)
    for k in (steps - 1, steps - 2):
        xr, fr = ref.solve_device(W.thetas[k % W.nrot])
        torch.cuda.synchronize(dev)
        assert bool((xr == W.xbuf[k % W.nbuf]).all()) and bool((fr == W.fbuf[k % W.nbuf]).all())
    W.close()


def test_multi_device_rccl_gather_with_several_gpus(lmpc):
    """lmpc_solve_batch_multi_device with MORE than one device: ncclCommInitAll in this process, one ncclSend /
    ncclRecv pair per shard inside a group, gather to the first device (csrc/lmpc_multi.hip).  Needs at least two
    visible GPUs; the single-GPU boxes of this pool skip it (bench.py runs the same check as config.multi_abi)."""
    import torch
    nd = torch.cuda.device_count()
    if nd < 2:
        pytest.skip("one visible GPU: the nd > 1 branch of lmpc_solve_batch_multi_device cannot run here")
    import bench
    g = load_golden("pendulum")
    out = bench.multi_abi_isolated(torch, 300_000)           # (a child process: a first-ever run may crash)
    assert "error" not in out, out
    assert out["n_devices"] == nd and out["identical"] and out["oracle_sample_identical"]


def test_multi_device_control_flow_on_one_gpu(lmpc, monkeypatch):
    """The n_devices > 1 code of csrc/lmpc_multi.hip -- partitioning, one handle / stream / host thread per shard,
    gather offsets, events -- executed on ONE GPU: with LMPC_MULTI_TRANSPORT=copy the device list may repeat a device
    and the gather runs as event-ordered peer copies instead of ncclSend / ncclRecv (the only part left to a machine
    with several GPUs, test_multi_device_rccl_gather_with_several_gpus).  Three shards of unequal size, incl. an empty
    one, bit for bit against the single-device call; RCCL on a repeated device is refused."""
    import torch
    g = load_golden("pendulum")
    monkeypatch.setenv("LMPC_MULTI_TRANSPORT", "copy")
    mq = lmpc.MultiQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1,
                                devices=[0, 0, 0])
    monkeypatch.delenv("LMPC_MULTI_TRANSPORT")
    assert mq.ndev == 3
    with pytest.raises(lmpc.LmpcError):
        mq.set_option("transport", 0)                       # RCCL needs distinct devices
    with pytest.raises(lmpc.LmpcError):                     # ... and without the hook a repeated device is an error
        lmpc.MultiQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1, devices=[0, 0])
    qp = _qp_from_golden(lmpc, g, 1)
    rng = np.random.default_rng(13)
    N = 300_001
    theta = np.hstack([rng.uniform(-6, 6, (N, 4)), rng.uniform(-5, 5, (N, 1)), np.zeros((N, 1)), rng.uniform(-2, 2, (N, 1))])
    x1, ef1, it1, act1 = qp.solve(theta)
    # host arrays, three shards through the chunked pipelines of three handles
    for q_ in mq.parts:
        q_.set_option("host_chunk", 20000)
    x, ef, it, act = mq.solve(theta)
    assert np.array_equal(x, x1) and np.array_equal(ef, ef1) and np.array_equal(it, it1) and np.array_equal(act, act1)
    off = lmpc.MultiQP.partition(N, 3)
    assert off == [0, 100001, 200001, 300001]
    # resident shards of unequal sizes (one of them empty), gathered on the "first device"
    for cuts in ([0, 150000, 150000, N], [0, 1, 200000, N], off):
        shards = [torch.from_numpy(theta[cuts[d]:cuts[d + 1]]).to("cuda:0") for d in range(3)]
        xs, fs, xr, fr = mq.solve_device(shards, gather=True)
        assert np.array_equal(xr.cpu().numpy(), x1) and np.array_equal(fr.cpu().numpy(), ef1), cuts
        for d in range(3):
            assert np.array_equal(xs[d].cpu().numpy(), x1[cuts[d]:cuts[d + 1]])
    # no gather asked for: shards only
    xs, fs, xr, fr = mq.solve_device(shards, gather=False)
    assert xr is None and np.array_equal(fs[2].cpu().numpy(), ef1[off[2]:])
    mq.close()


def test_rccl_calls_of_the_gather_on_one_gpu():
    """The RCCL half of the multi-device gather has never met a machine with several GPUs.  What one GPU can check: the
    library loads librccl, resolves every symbol it calls, ncclCommInitAll succeeds, and a grouped ncclSend / ncclRecv
    pair with the data types and counts of the gather moves a shard correctly -- to itself (LMPC_MULTI_TRANSPORT=rccl_self:
    shard 0's local copy goes through RCCL).  In a child process with a time limit: a first-ever call into a
    communication library must not be able to take the test run with it."""
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import os, sys
        os.environ["LMPC_MULTI_TRANSPORT"] = "rccl_self"
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        import numpy as np, torch
        import linearmpc_jl_amd as lmpc
        from conftest import load_golden
        g = load_golden("pendulum")
        mq = lmpc.MultiQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1, devices=[0])
        qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1)
        rng = np.random.default_rng(3)
        N = 100003
        th = np.hstack([rng.uniform(-6, 6, (N, 4)), rng.uniform(-5, 5, (N, 1)), np.zeros((N, 1)), rng.uniform(-2, 2, (N, 1))])
        td = torch.from_numpy(th).to("cuda:0")
        xs, fs, xr, fr = mq.solve_device([td], gather=True)
        x1, f1 = qp.solve_device(td)
        torch.cuda.synchronize()
        assert torch.equal(xr, x1) and torch.equal(fr, f1) and torch.equal(xs[0], x1)
        print("RCCL_SELF_OK")
    """) % (ROOT_DIR, ROOT_DIR)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert "RCCL_SELF_OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-1500:])


def test_solve_mpc_theta_drop_in_and_user_settings(lmpc):
    """`solve(mpc, θ)` (/root/reference/src/utils.jl:268-283) for one parameter vector returns DAQP.solve's tuple
    (x*, fval, exitflag, info) through lmpc_solve_one -- what the glue's LinearMPC.solve(mpc::MPC, θ::AbstractVector)
    calls -- and `compute_control` (utils.jl:43-51) runs on it unchanged; solver settings the user changes
    (`DAQP.settings(mpc.opt_model, Dict(...))`, docs/src/manual/solver.md:19-22) reach the handle."""
    from oracle import ldp as oldp
    g = load_golden("pendulum")
    q = lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"])
    mpc = lmpc.MPC(q, nx=4, nu=1, nr=2, nuprev=1)
    th = mpc.form_parameter([5.0, 5, 0, 0], uprev=[0.0])
    x, fval, flag, info = mpc.solve(th)
    assert flag == 1 and info["status"] == "Solved" and abs(x[0] - 1.7612519326) < 1e-6      # K1, runtests.jl:62-66
    # fval is the QP's objective at x*, and x* minimises it over the feasible set: any feasible perturbation is worse
    obj = lambda z: 0.5 * z @ q.H @ z + (q.f + q.f_theta @ th) @ z
    assert abs(fval - obj(x)) < 1e-12
    L = oracle_ldp_from(mpc.opt_model.ldp())
    xo, efo, _, _ = oldp.solve_batch(L, th[None])
    assert np.array_equal(x, xo[0]) and flag == efo[0]
    rng = np.random.default_rng(0)
    for _ in range(50):
        z = np.clip(x + 1e-3 * rng.standard_normal(5), g["bl"][:5], g["bu"][:5])
        assert obj(z) >= fval - 1e-12
    # the user's solver settings are the handle's: an iteration limit of 2 makes this 3-iteration point fail
    assert mpc.solver_settings()["iter_limit"] == 10000
    mpc.solver_settings(iter_limit=2)
    _, _, flag2, info2 = mpc.solve(th)
    assert flag2 == -4 and info2["status"] == "Failed"
    with pytest.raises(AssertionError):
        mpc.compute_control([5.0, 5, 0, 0])                       # @assert exitflag >= 1, utils.jl:46
    mpc.solver_settings(iter_limit=2000, primal_tol=1e-8)
    u = mpc.compute_control([5.0, 5, 0, 0])
    assert abs(u[0] - 1.7612519326) < 1e-6
    with pytest.raises(KeyError):
        mpc.solver_settings(pivot_tol=1e-3)                       # a DAQP setting without a counterpart here


def test_glue_cache_follows_the_mpqp_object_and_the_model_settings(lmpc):
    """The two traps of a per-MPC handle cache (integration/LmpcHipExt.jl `_model_for`, mirrored by MPC._model_for):
    (1) set_bounds! / set_objective! clear mpc.mpqp_issetup and the next setup! -- whoever calls it -- builds a NEW
    mpQP of the SAME dimensions (/root/reference/src/setup.jl:9,36-160; utils.jl:269): the handle must follow the
    object, not the dimensions; (2) DAQP.settings(mpc.opt_model, Dict(...)) after the first solve must reach the
    handle.  Here: solve, change a bound, solve -> the new answer (both orders of `setup!`), then a setting written
    straight onto the model's settings object."""
    g = load_golden("pendulum")
    mk = lambda ub: lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], np.full(5, ub), np.full(5, -ub), g["W"], g["senses"])
    mpc = lmpc.MPC(mk(2.0), nx=4, nu=1, nr=2, nuprev=1)
    u2 = mpc.compute_control([5.0, 5, 0, 0], uprev=[0.0])
    assert abs(u2[0] - 1.7612519326) < 1e-6
    first_handle = mpc.opt_model
    # set_bounds!(mpc; umax = 1): the reference only clears the flag; the next solve sets up again (utils.jl:269)
    mpc.mpQP = mk(1.0)
    mpc.mpqp_issetup = False
    u1 = mpc.compute_control([5.0, 5, 0, 0], uprev=[0.0])
    assert abs(u1[0] - 1.0) < 1e-9 and mpc.opt_model is not first_handle and first_handle._h is None   # rebuilt, old one freed
    # the user calls setup!(mpc) THEMSELVES after another change: flag true again, mpQP new, same dimensions --
    # exactly the sequence a dimension-keyed cache answers with the OLD bounds
    mpc.mpQP = mk(0.5)
    mpc.mpqp_issetup = True
    u05 = mpc.compute_control([5.0, 5, 0, 0], uprev=[0.0])
    assert abs(u05[0] - 0.5) < 1e-9
    Ub, efb = mpc.compute_control_batch(np.array([[5.0, 5, 0, 0]]), Uprev=np.zeros((1, 1)))
    assert abs(Ub[0, 0] - 0.5) < 1e-9                                 # the batched control handle followed too
    mpc.mpQP = mk(2.0)
    mpc.mpqp_issetup = True
    Ub, efb = mpc.compute_control_batch(np.array([[5.0, 5, 0, 0]]), Uprev=np.zeros((1, 1)))
    assert abs(Ub[0, 0] - 1.7612519326) < 1e-6
    # DAQP.settings(mpc.opt_model, Dict(:iter_limit => 2)) after the first solve: written on the model, not through
    # any method of ours -- the next solve must see it
    mpc.settings.iter_limit = 2
    _, _, flag, _ = mpc.solve(mpc.form_parameter([5.0, 5, 0, 0], uprev=[0.0]))
    assert flag == -4
    mpc.settings.iter_limit = 10000
    assert mpc.solve(mpc.form_parameter([5.0, 5, 0, 0], uprev=[0.0]))[2] == 1


def test_region_discovery_device_pipeline(lmpc):
    """BASELINE config 4 with the per-sample part on the GPU: sample drawn on the device, solved
    with the masks kept there, reduced to the distinct masks by lmpc_distinct_active_sets_device -- against the host
    path (np.unique over all masks) on the SAME sample: same sets, same counts, same representative samples."""
    import torch
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g)
    lb = np.array([-20.0] * 4 + [-20.0, 0.0] + [-2.0])
    ub = np.array([20.0] * 4 + [20.0, 0.0] + [2.0])
    out = lmpc.explicit.discover_regions_device(qp, lb, ub, 1_000_000, seed=3)
    theta = out["theta"].cpu().numpy()
    ref = lmpc.explicit.discover_regions(qp.solve, theta)
    assert out["n_solved"] == ref["n_solved"] == 1_000_000 and 44 <= len(out["masks"]) <= 243
    assert np.array_equal(out["counts"], ref["counts"][np.lexsort((ref["first_index"], -ref["counts"]))])
    key = lambda d: sorted((tuple(int(w) for w in m), int(c), int(f)) for m, c, f in zip(d["masks"], d["counts"], d["first_index"]))
    assert key(out) == key(ref)
    # law of the most frequent region reproduces the solver at its representative sample (KKT law check)
    i = int(out["first_index"][0])
    Fz, gz = lmpc.explicit.affine_law(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], out["masks"][0])
    x, ef, _, act = qp.solve(theta[i][None])
    assert np.array_equal(act[0], out["masks"][0]) and np.abs(Fz @ theta[i] + gz - x[0]).max() < 1e-8
    # a small capacity overflows and is retried with more room; failed problems do not count
    m2, c2, f2 = qp.distinct_active_sets_device(torch.from_numpy(np.ascontiguousarray(ref_act(qp, theta[:50000]))).to("cuda:0"),
                                                capacity=8)
    assert len(m2) == len(np.unique(ref_act(qp, theta[:50000]), axis=0)) and c2.sum() == 50000
    # one-word masks of a large batch take the lock-free per-lane reduction (round 4): both forms give the same sets, with
    # a capacity that overflows and is retried, and with problems excluded by their exit flag
    act_all = torch.from_numpy(np.ascontiguousarray(ref_act(qp, theta))).to("cuda:0")
    flags = torch.ones(len(theta), dtype=torch.int32, device="cuda:0")
    flags[::3] = -1
    keep = np.ones(len(theta), bool); keep[::3] = False
    want_all = key(ref)
    um, ui, uc = np.unique(ref_act(qp, theta)[keep], axis=0, return_index=True, return_counts=True)
    want_kept = sorted((tuple(int(w) for w in m), int(c), int(np.flatnonzero(keep)[i])) for m, c, i in zip(um.view(np.uint64), uc, ui))
    for lockfree in (1, 0):
        qp.set_option("region_lockfree", lockfree)
        for rep in range(2):             # (twice: the tables are handed over clean between calls)
            m3, c3, f3 = qp.distinct_active_sets_device(act_all, capacity=8)
            assert sorted((tuple(int(w) for w in m), int(c), int(f)) for m, c, f in zip(m3, c3, f3)) == want_all, (lockfree, rep)
        m4, c4, f4 = qp.distinct_active_sets_device(act_all, exitflag=flags, capacity=4096)
        assert sorted((tuple(int(w) for w in m), int(c), int(f)) for m, c, f in zip(m4, c4, f4)) == want_kept, lockfree
    qp.set_option("region_lockfree", 1)
    # multi-word masks (m = 84 rows: three words) with infeasible points in the batch
    g3 = load_golden("mass_spring_3in")
    q3 = _qp_from_golden(lmpc, g3)
    th3 = torch.from_numpy(np.ascontiguousarray(np.random.default_rng(5).uniform(-4, 4, (60000, 12)))).to("cuda:0")
    o3 = lmpc.explicit.discover_regions_device(q3, None, None, 0, theta=th3)
    r3 = lmpc.explicit.discover_regions(q3.solve, th3.cpu().numpy())
    assert q3.words == 3 and key(o3) == key(r3) and o3["n_solved"] == r3["n_solved"] < 60000


def ref_act(qp, theta):
    return qp.solve(theta)[3].view(np.int64)


@pytest.mark.parametrize("opts", [{"fast_dyn": 4}, {"fast_dyn": 6, "fast_dma": 0}, {"fast_dyn": 3, "fast_dma": 3},
                                  {"fast_dma": 0}, {"fast_dma": 3}, {"fast_dyn": 4, "fast_nstr": 4, "fast_tiles": 28}])
def test_one_launch_kernel_record_paths_and_dynamic_tail(lmpc, opts):
    """The one-launch kernel's ways of taking its records -- through registers, by LDS-DMA into a ring of two or three
    tiles -- and of splitting the batch -- static, or a static share plus a dynamic tail of tiles handed out through
    global tickets -- change the execution order only: every combination gives the oracle's bits, at batch sizes
    with and without a partial last tile and with fewer tiles than workgroups could hold."""
    from oracle import ldp as oldp
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    for k, v in opts.items():
        qp.set_option(k, v)
    L = oracle_ldp_from(qp.ldp())
    rng = np.random.default_rng(44)
    for N in (63, 64, 1000, 30011, 400_000, 1_000_003):
        theta = np.hstack([rng.uniform(-9, 9, (N, 4)), rng.uniform(-9, 9, (N, 1)), np.zeros((N, 1)), rng.uniform(-2, 2, (N, 1))])
        x, ef, it, act = qp.solve(theta)
        sel = np.arange(N) if N <= 30011 else np.concatenate([np.arange(3000), np.arange(N - 3000, N), rng.integers(0, N, 6000)])
        xo, efo, ito, acto = oldp.solve_batch(L, theta[sel])
        assert np.array_equal(x[sel], xo) and np.array_equal(ef[sel], efo) and np.array_equal(it[sel], ito)
        assert np.array_equal(act[sel], acto)
        assert (ef >= 1).all()
    qp.check()


def test_one_launch_kernel_unaligned_batch(lmpc):
    # a batch that starts 8 bytes into an allocation (a view): the LDS-DMA pieces need 16-byte alignment, the library
    # falls back to the register path by itself; results are the oracle's either way
    import torch
    from oracle import ldp as oldp
    g = load_golden("pendulum")
    qp = _qp_from_golden(lmpc, g, 1)
    L = oracle_ldp_from(qp.ldp())
    rng = np.random.default_rng(8)
    N = 100_003
    theta = np.hstack([rng.uniform(-9, 9, (N, 4)), rng.uniform(-9, 9, (N, 1)), np.zeros((N, 1)), rng.uniform(-2, 2, (N, 1))])
    flat = torch.zeros(N * 7 + 1, dtype=torch.float64, device="cuda:0")
    flat[1:] = torch.from_numpy(theta.reshape(-1)).to("cuda:0")
    view = flat[1:].view(N, 7)
    assert view.data_ptr() % 16 == 8
    x, ef = qp.solve_device(view)
    qp.check()
    xo, efo, _, _ = oldp.solve_batch(L, theta)
    assert np.array_equal(x.cpu().numpy(), xo) and np.array_equal(ef.cpu().numpy(), efo)


def test_distinct_active_sets_edge_cases(lmpc):
    import torch
    g = load_golden("mass_spring")
    qp = _qp_from_golden(lmpc, g, 1)
    # empty batch
    act0 = torch.zeros((0, qp.words), dtype=torch.int64, device="cuda:0")
    m0, c0, f0 = qp.distinct_active_sets_device(act0)
    assert len(m0) == 0 and len(c0) == 0
    # no exit flags given: every row counts, duplicates far apart in the batch are merged
    rng = np.random.default_rng(2)
    base = rng.integers(0, 2 ** 62, (7, qp.words)).astype(np.int64)
    pick = rng.integers(0, 7, 100_000)
    act = torch.from_numpy(base[pick]).to("cuda:0")
    m1, c1, f1 = qp.distinct_active_sets_device(act, capacity=16)
    assert len(m1) == len(np.unique(pick)) and c1.sum() == 100_000
    for mask, cnt, first in zip(m1, c1, f1):
        k = int(np.flatnonzero((base.view(np.uint64) == mask).all(axis=1))[0])
        assert cnt == (pick == k).sum() and first == np.flatnonzero(pick == k)[0]
    # every problem failed: nothing to report
    ef = torch.full((100_000,), -1, dtype=torch.int32, device="cuda:0")
    m2, c2, f2 = qp.distinct_active_sets_device(act, ef)
    assert len(m2) == 0


# ------------------------------------------------------------------ variational objective (is_avi)
def _avi_oracle_pack(qp):
    from oracle import avi as oavi
    pk = qp.avi_pack()
    return oavi.AVI(pk["n"], pk["m"], pk["ms"], pk["nth"], pk["nout"], pk["ML"], pk["MR"], pk["G"], pk["du"], pk["dl"],
                    pk["Dth"], pk["Rout"], pk["x0"], pk["Xth"], pk["sense"], np.ones(pk["m"])).contiguous()


def test_game_theoretic_mpc_golden_vectors_and_same_pack_parity(lmpc):
    """The reference's game-theoretic MPC (test/runtests.jl:1337-1358; non-symmetric H -> is_avi, setup.jl:13)
    through lmpc_setup (which decides is_avi from H as the reference does): kernel `avi`, the committed answers to
    1e-10 with identical active sets, and bit-identical to the oracle on the handle's own pack, cold and warm."""
    from oracle import avi as oavi
    g = load_golden("game_kat")
    qp = _qp_from_golden(lmpc, g)
    assert qp.is_avi and qp.kernel_name == "avi_tiers<6>|avi"
    x, ef, it, act = qp.solve(g["theta"])
    assert np.array_equal(ef, g["exitflag"]) and np.array_equal(act, g["active"])
    assert np.abs(x - g["X"]).max() <= TOL
    P = _avi_oracle_pack(qp)
    xo, efo, ito, acto = oavi.solve_batch(P, g["theta"])
    assert np.array_equal(ef, efo) and np.array_equal(it, ito) and np.array_equal(act, acto) and np.array_equal(x, xo)
    # warm start from a shuffled neighbour's active set: same answers, the oracle's iteration counts
    warm = np.roll(act, 7, axis=0)
    xw, efw, itw, actw = qp.solve(g["theta"], warm=warm)
    xow, efow, itow, actow = oavi.solve_batch(P, g["theta"], warm=warm)
    assert np.array_equal(efw, efow) and np.array_equal(itw, itow) and np.array_equal(actw, actow) and np.array_equal(xw, xow)
    assert np.abs(xw - x).max() <= 1e-9
    # ragged sizes: 1, 63, 64, 65 problems
    for nq in (1, 63, 64, 65):
        xq, efq, _, _ = qp.solve(g["theta"][:nq])
        assert np.array_equal(xq, x[:nq]) and np.array_equal(efq, ef[:nq])
    # explicit keyword form of the reference's DAQP.setup call
    qp2 = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"],
                                   break_points=np.zeros(0, np.int32), is_avi=True)
    x2, ef2, _, _ = qp2.solve(g["theta"][:500])
    assert np.array_equal(x2, x[:500])
    with pytest.raises(lmpc.LmpcError):                               # no binary32 build of this mode
        qp.solve_f32(g["theta"][:4].astype(np.float32))


def test_game_theoretic_mpc_closed_loop_reproduces_the_reference_pins(lmpc):
    """test/runtests.jl:1345-1354: Simulation(mpc; x0 = 10*ones(2), r = [10,0], N = 500) ends at y = [10, 0] (atol
    1e-4).  Three ways: the literal one-theta drop-in (MPC.compute_control -> solve -> lmpc_solve_one, step by step
    on the host like the reference's Simulation), the batched closed loop on the device (lmpc_simulate, 256 scenarios
    around the reference's start), and the oracle's closed loop -- the last two bit for bit."""
    from oracle import avi as oavi
    g = load_golden("game_kat")
    F, G = g["F"], g["G"]
    q = lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], is_symmetric=False)
    mpc = lmpc.MPC(q, nx=2, nu=2, nr=2, nuprev=2)
    x = np.array([10.0, 10.0])
    ys = []
    for _ in range(500):
        ys.append(x.copy())
        u = mpc.compute_control(x, r=[10.0, 0.0])
        x = F @ x + G @ u
    assert abs(ys[-1][0] - 10.0) < 1e-4 and abs(ys[-1][1]) < 1e-4
    assert np.abs(ys[-1] - g["y_end"]).max() < 1e-9
    rng = np.random.default_rng(2)
    N = 256
    x0 = np.array([10.0, 10.0]) + rng.normal(size=(N, 2)); x0[0] = [10.0, 10.0]
    r = np.tile([10.0, 0.0], (N, 1))
    qp = mpc.control_model()
    assert qp.is_avi
    for warm in (False, True):
        out = qp.simulate(x0, 500, F, G, r=r, uprev=np.zeros((N, 2)), warm=warm)
        ref = oavi.simulate(_avi_oracle_pack(qp), x0, 500, F, G, r=r, uprev=np.zeros((N, 2)), warm=warm)
        assert np.array_equal(out["x"], ref["x"]) and np.array_equal(out["U"], ref["U"])
        assert np.array_equal(out["flag_min"], ref["flag_min"]) and (out["flag_min"] == 1).all()
        assert abs(out["X"][499, 0, 0] - 10.0) < 1e-4 and abs(out["X"][499, 0, 1]) < 1e-4
        assert np.abs(out["X"][499] - [10.0, 0.0]).max() < 1e-3         # every scenario settles at the reference


def test_generated_controller_call_on_a_variational_handle(lmpc):
    """The batched `mpc_compute_control(control, state, reference, ...)` (reference codegen/mpc_update_qp.c:29-54) and
    the multi-device entry points on an is_avi handle: same numbers as solving the assembled theta directly."""
    import torch
    g = load_golden("game_kat")
    q = lmpc.MPQP(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], is_symmetric=False)
    mpc = lmpc.MPC(q, nx=2, nu=2, nr=2, nuprev=2)
    gc = lmpc.GeneratedController(mpc)
    rng = np.random.default_rng(8)
    N = 5000
    state = rng.uniform(-20, 20, (N, 2)); ref = rng.uniform(-20, 20, (N, 2)); prev = rng.uniform(-1, 1, (N, 2))
    control = prev.copy()
    ef = gc.mpc_compute_control(control, state, ref)
    theta = np.hstack([state, ref, prev])
    x, ef2, _, _ = mpc.control_model().solve(theta)
    assert np.array_equal(ef, ef2) and np.all(ef == 1) and np.array_equal(control, x)
    U, efb = mpc.compute_control_batch(state, R=ref, Uprev=prev)
    assert np.array_equal(U, x)
    # every GPU behind one call (here: however many this box shows) on the same problem
    mq = lmpc.MultiQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=2)
    xm, efm, _, _ = mq.solve(theta)
    assert np.array_equal(xm, x) and np.array_equal(efm, ef)
    mq.close()
    # distinct optimal active sets of the sample, reduced on the device (region discovery works on this mode too)
    out = lmpc.explicit.discover_regions_device(mpc.control_model(), None, None, 0, theta=torch.from_numpy(theta).to("cuda:0"))
    _, _, _, act = mpc.control_model().solve(theta)
    assert len(out["masks"]) == len(np.unique(act, axis=0)) and out["n_solved"] == N


def test_proximal_point_mode_for_a_semidefinite_hessian(lmpc):
    """eps_prox > 0 (DAQP's proximal-point setting; a semidefinite H is -5 without it): the kernel's outer iteration
    against the oracle's on the same pack -- x, exit flags, summed iteration counts, final active sets bit for bit --
    on rank-deficient problems with bounded variables and general rows; eps_prox reaches the handle through the settings
    struct, changing it on the MPC rebuilds the handle, changing it on a live handle is refused."""
    from oracle import avi as oavi
    rng = np.random.default_rng(17)
    for trial in range(8):
        n = int(rng.integers(3, 10)); r = int(rng.integers(1, n)); mg = int(rng.integers(0, 9)); nth = int(rng.integers(1, 5))
        B = rng.normal(size=(n, r)); H = B @ B.T
        f, fth = rng.normal(size=n), rng.normal(size=(n, nth))
        A = rng.normal(size=(mg, n)); m = n + mg
        bu, bl = rng.uniform(0.5, 2, m), -rng.uniform(0.5, 2, m)
        W = rng.normal(size=(m, nth)) * 0.2; W[:n] = 0
        sense = np.zeros(m, np.int32)
        s = lmpc.default_settings(); s.eps_prox = 1e-4; s.eta_prox = 1e-9
        nout = min(n, 3)
        qp = lmpc.BatchedQP.from_mpqp(H, f, fth, A, bu, bl, W, sense, nout=nout, settings=s)
        assert qp.kernel_name == "avi+prox"
        th = rng.normal(size=(1500, nth))
        x, ef, it, act = qp.solve(th)
        pk = qp.avi_pack()
        P = oavi.AVI(pk["n"], pk["m"], pk["ms"], pk["nth"], pk["nout"], pk["ML"], pk["MR"], pk["G"], pk["du"], pk["dl"],
                     pk["Dth"], pk["Rout"], pk["x0"], pk["Xth"], pk["sense"], np.ones(pk["m"])).contiguous()
        # the library's own transform (qp_to_prox: H + eps I, its inverse, the affine map, the outputs' feedback term)
        # against the independent restatement in oracle/avi.py -- the kernel and the checker below share the handle's pack,
        # so an error in the transform would cancel there
        Pq, px = oavi.qp2prox(H, f, fth, A, bu, bl, W, sense, nout=nout, eps=1e-4)
        hp = qp.prox_pack()
        for k in ("Hinv", "x0f", "Xthf", "Kth"):
            assert np.allclose(hp[k], px[k], rtol=1e-9, atol=1e-11), (trial, k)
        for k, ref in (("ML", Pq.ML), ("MR", Pq.MR), ("du", Pq.du0), ("dl", Pq.dl0), ("Dth", Pq.Dth), ("Rout", Pq.Rout),
                       ("x0", Pq.x0), ("Xth", Pq.Xth)):
            assert np.allclose(np.asarray(pk[k]).reshape(-1), np.asarray(ref).reshape(-1), rtol=1e-8, atol=1e-10), (trial, k)
        xo, efo, ito, acto = oavi.prox_solve_batch(P, hp, th, 1e-4, 1e-9)
        # ... and the limit is a KKT point of the ORIGINAL (semidefinite) problem: full-length x from a second handle
        qf = lmpc.BatchedQP.from_mpqp(H, f, fth, A, bu, bl, W, sense, nout=n, settings=s)
        xf, eff, _, actf = qf.solve(th[:200])
        for i in np.flatnonzero(eff == 1)[:40]:
            r_st, r_pr, r_sg = oavi.kkt_residual(H, f, fth, A, bu, bl, W, sense, th[i], xf[i], actf[i])
            assert r_st < 1e-6 and r_pr < 1e-6 and r_sg < 1e-6, (trial, i, r_st, r_pr, r_sg)
        qf.close()
        assert set(np.unique(efo)) <= {1, -1} and (efo == 1).mean() > 0.5        # (some points' rows are infeasible)
        assert np.array_equal(ef, efo) and np.array_equal(it, ito) and np.array_equal(act, acto) and np.array_equal(x, xo), trial
        bad = lmpc.default_settings(); bad.eps_prox = 1e-3
        with pytest.raises(lmpc.LmpcError):
            qp.set_settings(bad)
        qp.close()
    # through the MPC mirror: eps_prox set on the model's settings -> the next solve sets the handle up again
    q = lmpc.MPQP(H, f, fth, A, bu, bl, W, sense)
    mpc = lmpc.MPC(q, nx=1, nu=1, nr=nth - 1 if nth > 1 else 0)
    mpc.nx, mpc.nr = 1, nth - 1
    with pytest.raises(lmpc.LmpcError) as e:
        mpc.solve(th[0])
    assert e.value.code == -5
    mpc.solver_settings(eps_prox=1e-4, eta_prox=1e-9)
    xs, fval, flag, info = mpc.solve(th[0])
    assert flag == 1 and mpc.opt_model.kernel_name == "avi+prox"


def test_variational_problems_with_general_and_soft_rows(lmpc):
    """Random non-symmetric problems with general, one-sided and SOFT rows, feasible and infeasible points: the AVI
    kernel against the oracle on the handle's pack, bit for bit (flags incl. -1, iterations, active sets, x)."""
    from oracle import avi as oavi
    rng = np.random.default_rng(21)
    for trial in range(12):
        n = int(rng.integers(2, 13)); mg = int(rng.integers(1, 20)); ms = int(rng.integers(0, n + 1)); nth = int(rng.integers(1, 6))
        B = rng.normal(size=(n, n)); K = rng.normal(size=(n, n)) * rng.uniform(0, 2)
        H = B @ B.T + 0.3 * np.eye(n) + (K - K.T)
        A = rng.normal(size=(mg, n)); m = ms + mg
        bu, bl = rng.uniform(0.1, 2, m), -rng.uniform(0.1, 2, m)
        bl[rng.random(m) < 0.2] = -1e30
        sense = np.zeros(m, np.int32); sense[ms:][rng.random(mg) < 0.3] = 8
        qp = lmpc.BatchedQP.from_mpqp(H, rng.normal(size=n), rng.normal(size=(n, nth)), A, bu, bl,
                                      rng.normal(size=(m, nth)) * 0.3, sense, nout=min(n, 3))
        assert qp.is_avi
        th = rng.normal(size=(777, nth)) * rng.uniform(0.5, 4)
        x, ef, it, act = qp.solve(th)
        xo, efo, ito, acto = oavi.solve_batch(_avi_oracle_pack(qp), th)
        assert np.array_equal(ef, efo) and np.array_equal(it, ito) and np.array_equal(act, acto), trial
        ok = efo >= 1
        assert np.array_equal(x[ok], xo[ok]), trial
        qp.close()


def test_register_resident_variational_kernels_against_generic_kernel_and_oracle(lmpc):
    """Small box-constrained variational problems (n = 2 .. 8, bounds only: the shape of the reference's game-theoretic
    MPC, test/runtests.jl:1337-1358) run a chain of register-resident kernels in front of the generic one
    (avi_tiers -> avi_lane -> avi).  Every depth of the first pass (0 = the complete lane kernel over the whole batch),
    the generic kernel alone and the oracle agree bit for bit on x, flags, iteration counts and active sets --
    on samplings with few and with many active bounds (removals), ragged batch sizes, several calls in a row (the
    work lists' counters are handed over between calls), and with an iteration limit the chain must hand down."""
    import torch
    from oracle import avi as oavi, ldp as oldp
    rng = np.random.default_rng(77)
    dev = torch.device("cuda", 0)
    for trial in range(14):
        n = 2 + trial % 7
        nth = int(rng.integers(1, 8)); nout = int(rng.integers(1, n + 1))
        B = rng.normal(size=(n, n)); K = rng.normal(size=(n, n)) * rng.uniform(0.2, 2)
        H = B @ B.T + 0.3 * np.eye(n) + (K - K.T)
        bu, bl = rng.uniform(0.1, 2, n), -rng.uniform(0.1, 2, n)
        qp = lmpc.BatchedQP.from_mpqp(H, rng.normal(size=n), rng.normal(size=(n, nth)), np.zeros((0, n)), bu, bl,
                                      rng.normal(size=(n, nth)) * 0.3, np.zeros(n, np.int32), nout=nout)
        assert qp.is_avi and qp.kernel_name.startswith("avi_tiers<%d>" % n), qp.kernel_name
        P = _avi_oracle_pack(qp)
        for N, scale in ((5000, 1.0), (4097, 6.0), (63, 3.0), (1, 2.0)):
            th = np.ascontiguousarray(rng.normal(size=(N, nth)) * scale)
            xo, efo, ito, acto = oavi.solve_batch(P, th)
            assert (efo >= 1).all()
            t = torch.from_numpy(th).to(dev)
            for first in (2, 0, 1, 3, -1):
                qp.set_option("avi_tiers", 0 if first < 0 else 1)
                if first >= 0:
                    qp.set_option("avi_tiers_first", first)
                it = torch.full((N,), -77, dtype=torch.int32, device=dev)
                act = torch.full((N, qp.words), -1, dtype=torch.int64, device=dev)
                x, ef = qp.solve_device(t, iters=it, active=act)
                torch.cuda.synchronize()
                assert np.array_equal(ef.cpu().numpy(), efo), (trial, N, first)
                assert np.array_equal(it.cpu().numpy(), ito), (trial, N, first)
                assert np.array_equal(act.cpu().numpy().view(np.uint64), acto.view(np.uint64)), (trial, N, first)
                assert np.array_equal(x.cpu().numpy(), xo), (trial, N, first)
        # an iteration limit inside the chain's reach: what it cannot finish goes down to the generic kernel, which
        # reports the limit exactly as it does alone
        th = np.ascontiguousarray(rng.normal(size=(3000, nth)) * 6.0)
        qp.set_option("avi_tiers", 1); qp.set_option("avi_tiers_first", 2)
        for limit in (n + 2, 3):         # (3 <= n + 1: the chain is not used at all)
            s = lmpc.default_settings(); s.iter_limit = limit; qp.set_settings(s)
            so = oldp.default_settings(); so.iter_limit = limit
            xo, efo, ito, acto = oavi.solve_batch(P, th, settings=so)
            x, ef, it, act = qp.solve(th)
            assert np.array_equal(ef, efo) and np.array_equal(it, ito), (trial, limit)
            ok = efo >= 1
            assert np.array_equal(x[ok], xo[ok]) and np.array_equal(act[ok], acto[ok]), (trial, limit)
        qp.close()


def test_tiers_pass_in_front_of_the_wavefront_kernel(lmpc):
    """Small problems with many plain hard rows on the wavefront path (the reference's mass_spring example is the model:
    n = 10, m = 63) first go through straight-line tiers, one problem per lane (lmpc_qp_tiers_kernel.hpp), which finish
    every problem on an append-only path -- optimal (1) or infeasible (-1) -- and queue the rest for the wavefront
    kernel.  n = 2 .. 12 (forced onto the wavefront path where the lane kernels would be the default), m up to 64,
    wide and narrow theta ranges, ragged batches: the same bits as the path without the pass and as the oracle --
    x also on the failed points, flags, iteration counts, active sets; settings that rule the pass out (an iteration
    limit inside its reach, a warm start) fall back by themselves.  The same pass runs in front of the LANE kernel where
    that one is the default for general rows ("wave" 0)."""
    import torch
    from oracle import ldp as oldp
    rng = np.random.default_rng(404)
    dev = torch.device("cuda", 0)
    for trial in range(22):
        n = 2 + trial % 11
        mg = int(rng.integers(1, 64 - n + 1)); nth = int(rng.integers(1, 17))
        H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth)
        scale = rng.choice([0.5, 1.0, 3.0])
        qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, scale * bu, scale * bl, W, sense, nout=int(rng.integers(1, n + 1)))
        qp.set_option("wave", 1)
        assert qp.kernel_name == "qp_tiers<%d>|wave" % n, qp.kernel_name
        L = oracle_ldp_from(qp.ldp())
        for N, amp in ((3000, 2.0), (4097, 8.0), (65, 1.0), (1, 4.0)):
            th = np.ascontiguousarray(rng.uniform(-amp, amp, (N, nth)))
            xo, efo, ito, acto = oldp.solve_batch(L, th)
            t = torch.from_numpy(th).to(dev)
            for tiers, wave in ((1, 1), (0, 1), (1, 0), (0, 0)):          # (in front of the wavefront kernel / the lane kernel)
                qp.set_option("qp_tiers", tiers)
                qp.set_option("wave", wave)
                it = torch.full((N,), -77, dtype=torch.int32, device=dev)
                act = torch.full((N, qp.words), -1, dtype=torch.int64, device=dev)
                x, ef = qp.solve_device(t, iters=it, active=act)
                torch.cuda.synchronize()
                assert np.array_equal(ef.cpu().numpy(), efo), (trial, N, tiers)
                assert np.array_equal(it.cpu().numpy(), ito), (trial, N, tiers)
                assert np.array_equal(act.cpu().numpy().view(np.uint64), acto.view(np.uint64)), (trial, N, tiers)
                assert np.array_equal(x.cpu().numpy(), xo), (trial, N, tiers)
        qp.set_option("qp_tiers", 1)
        qp.set_option("wave", 1)
        th = np.ascontiguousarray(rng.uniform(-6, 6, (2000, nth)))
        s = lmpc.default_settings(); s.iter_limit = n + 2; qp.set_settings(s)          # the pass needs iter_limit > n + 2
        so = oldp.default_settings(); so.iter_limit = n + 2
        _compare(qp, th, settings=so)
        s.iter_limit = 10000; qp.set_settings(s)
        x, ef, it, act = _compare(qp, th)
        _compare(qp, th, warm=act)                                                       # warm: wavefront kernel alone
        qp.close()
    # large batches in the default mode: the handle times one call with the pass and one without, then keeps the faster
    # -- whichever call it is, the arrays are the same
    gm = load_golden("mass_spring")
    qm = _qp_from_golden(lmpc, gm)
    thm = np.ascontiguousarray(rng.uniform(-4, 4, (70_000, 12)))
    tm = torch.from_numpy(thm).to(dev)
    ref = None
    for call in range(6):
        x, ef = qm.solve_device(tm)
        torch.cuda.synchronize()
        cur = (x.cpu().numpy(), ef.cpu().numpy())
        assert ref is None or (np.array_equal(cur[0], ref[0]) and np.array_equal(cur[1], ref[1])), call
        ref = cur
    sel = rng.integers(0, len(thm), 4000)
    xo, efo, _, _ = oldp.solve_batch(oracle_ldp_from(qm.ldp()), thm[sel])
    assert np.array_equal(ref[1][sel], efo) and np.array_equal(ref[0][sel], xo)
    qm.close()
    # SOFT rows (the reference's default for output bounds, setup.jl:94): slack weighted 1 / rho_soft, exit flag 2 when a
    # soft row is violated at the optimum -- the pass finishes those too; the reference's soft-constraint document example
    cases = []
    for trial in range(10):
        n = 3 + trial % 10
        mg = int(rng.integers(4, 64 - n + 1)); nth = int(rng.integers(1, 9)); nsoft = int(rng.integers(1, mg + 1))
        H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth, nsoft=nsoft)
        sc = rng.choice([0.3, 1.0])
        cases.append((lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, sc * bu, sc * bl, W, sense, nout=min(n, 2)), nth, 3.0))
    seen_soft_optimal = False
    gs = load_golden("soft_doc")
    cases.append((_qp_from_golden(lmpc, gs), gs["theta"].shape[1], None))
    for qp, nth, amp in cases:
        assert qp.kernel_name.startswith("qp_tiers<") and qp.kernel_name.endswith("wave"), qp.kernel_name
        L = oracle_ldp_from(qp.ldp())
        th = np.ascontiguousarray(rng.uniform(-amp, amp, (5000, nth))) if amp else np.ascontiguousarray(gs["theta"])
        xo, efo, ito, acto = oldp.solve_batch(L, th)
        t = torch.from_numpy(th).to(dev)
        N = len(th)
        for tiers in (1, 0):
            qp.set_option("qp_tiers", tiers)
            it = torch.full((N,), -77, dtype=torch.int32, device=dev)
            act = torch.full((N, qp.words), -1, dtype=torch.int64, device=dev)
            x, ef = qp.solve_device(t, iters=it, active=act)
            torch.cuda.synchronize()
            assert np.array_equal(ef.cpu().numpy(), efo) and np.array_equal(it.cpu().numpy(), ito), tiers
            assert np.array_equal(act.cpu().numpy().view(np.uint64), acto.view(np.uint64)), tiers
            assert np.array_equal(x.cpu().numpy(), xo), tiers
        seen_soft_optimal = seen_soft_optimal or bool((efo == 2).any())
        qp.close()
    assert seen_soft_optimal



# ------------------------------------------------------------------ four problems per wavefront (lmpc_row_kernel.hpp)
def _row_launches(qp, since=None):
    """Row-kernel launches in the handle's record (lmpc_row_launch_info): the last running number, or -- with `since` --
    the launches made after it."""
    if since is None:
        r = qp.row_launch_info()
        return r[-1]["seq"] if r else 0
    return qp.row_launch_info(since)


def _row_vs_wave_vs_oracle(lmpc, qp, theta, settings=None, row=True):
    """The row kernel (forced), the wavefront kernel (row kernel off) and the oracle on the same points: identical
    x, exit flags, iteration counts and active sets.  The handle's launch record must show a row-kernel launch with
    "row_kernel" 1 (`row` = False: a handle the row kernel does not take -- none) and none with 0."""
    qp.set_option("row_kernel", 0)
    seq = _row_launches(qp)
    ref = qp.solve(theta)
    assert not _row_launches(qp, seq), "a row-kernel launch with \"row_kernel\" 0"
    qp.set_option("row_kernel", 1)
    got = _compare(qp, theta, settings=settings)
    assert bool(_row_launches(qp, seq)) == row, ("row-kernel launches with \"row_kernel\" 1", _row_launches(qp, seq))
    for a, b in zip(ref, got):
        assert np.array_equal(a, b, equal_nan=True)
    return got


@pytest.mark.parametrize("name", ["mass_spring_3in", "mass_spring", "soft_doc", "pendulum_N50"])
def test_row_kernel_matches_the_wavefront_kernel_and_the_oracle(lmpc, name):
    # BASELINE config 3 (n = 30, m = 84: two slots of positions), the reference's mass_spring example (one slot, behind
    # the tiers pass: work-list mode), a problem with SOFT rows, the benchmark class at N = 50 (ten constraint slots; first
    # of two passes at 32 rows, the wavefront kernel takes what outgrows it)
    import bench
    g = load_golden(name)
    qp = _qp_from_golden(lmpc, g, nout=int(g["nu"]) if "nu" in g else None)
    theta = bench.make_theta(name, 3001, 5)            # (ragged: 3001 = 46 wavefronts of 64 + 57)
    x, ef, it, act = _row_vs_wave_vs_oracle(lmpc, qp, theta)
    assert (ef != -7).all()
    # trajectories: every output slot
    qp2 = _qp_from_golden(lmpc, g)
    _row_vs_wave_vs_oracle(lmpc, qp2, theta[:777])


@pytest.mark.parametrize("n,mg,nth,nsoft,seed", [(6, 20, 3, 0, 31), (14, 40, 5, 6, 32), (16, 48, 16, 0, 33), (20, 30, 6, 0, 34),
                                                 (30, 60, 8, 10, 35), (31, 65, 12, 0, 36), (32, 64, 7, 4, 37),
                                                 (40, 100, 5, 0, 38), (60, 100, 17, 12, 39)])
def test_row_kernel_random_problems(lmpc, n, mg, nth, nsoft, seed):
    # every instantiation, full and partial slots, SOFT rows, records longer than the 16 parameters fetched in one batch;
    # capacities beyond 32 rows run the row kernel as the first of two passes (what outgrows 32 rows goes to the
    # wavefront kernel)
    rng = np.random.default_rng(seed)
    H, f, f_theta, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth, nsoft)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=min(n, 4))
    # (n = 6, m = 26 is a lane-kernel handle by default, where "row_kernel" 1 asks for nothing: the launch record showed
    # that this case had never reached the row kernel)
    qp.set_option("wave", 1)
    theta = rng.uniform(-2, 2, (1500, nth)) * (0.4 if nth >= 12 else 1.0)
    x, ef, it, act = _row_vs_wave_vs_oracle(lmpc, qp, theta)
    assert (ef >= 1).any() and (ef != -7).all()


def test_row_kernel_guards_and_small_batches(lmpc):
    # iteration limit, infeasible and singular paths, one to five problems (rows of a wavefront without a problem)
    g = load_golden("mass_spring_3in")
    qp = _qp_from_golden(lmpc, g, nout=3)
    import bench
    theta = bench.make_theta("mass_spring_3in", 700, 9)
    for N in (1, 2, 3, 5, 63, 65, 700):
        _row_vs_wave_vs_oracle(lmpc, qp, theta[:N])
    s = lmpc.default_settings()
    s.iter_limit = 12
    qp.set_settings(s)
    x, ef, it, act = _row_vs_wave_vs_oracle(lmpc, qp, theta, settings=_copy_settings(lmpc, s))
    assert (ef == -4).any() and (it[ef == -4] == 12).all()
    # the default: large cold batches take the row kernel, small ones the wavefront kernel; same answers either way
    qp.set_settings(lmpc.default_settings())
    qp.set_option("row_kernel", -1)
    assert qp.kernel_name == "row|wave"
    big = np.tile(theta, (13, 1))
    xa = qp.solve(big)
    qp.set_option("row_kernel", 0)
    xb = qp.solve(big)
    for a, b in zip(xa, xb):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name,N", [("pendulum", 100_003), ("pendulum", 777), ("refcond_kat", 50_000), ("mass_spring_3in", 4000)])
def test_several_batches_in_one_call(lmpc, name, N):
    """lmpc_solve_batches_device: one to nine batches in one call (one kernel launch for up to eight of them on the
    handles the one-launch kernel covers, a loop of single-batch launches elsewhere) against the single-batch call on the
    same buffers: bit-identical x and exit flags; a sample against the oracle."""
    import torch
    import bench
    from oracle import ldp as oldp
    g = load_golden(name)
    qp = _qp_from_golden(lmpc, g, nout=1)
    rng = np.random.default_rng(3)
    if name in ("pendulum", "mass_spring_3in"):
        ths = [bench.make_theta(name, N, 100 + b, hard=(b % 2 == 1) if name == "pendulum" else False) for b in range(9)]
    else:
        base = g["theta"]
        ths = [np.ascontiguousarray(base[rng.integers(0, len(base), N)] * rng.uniform(0.5, 1.5)) for _ in range(9)]
    th_d = [torch.from_numpy(t).cuda() for t in ths]
    singles = [qp.solve_device(t) for t in th_d]
    torch.cuda.synchronize()
    for nb in (1, 2, 3, 8, 9):
        xs, fs = qp.solve_batches_device(th_d[:nb])
        torch.cuda.synchronize()
        qp.check()
        for b in range(nb):
            assert torch.equal(xs[b], singles[b][0]) and torch.equal(fs[b], singles[b][1]), (nb, b)
    L = oracle_ldp_from(qp.ldp())
    sel = np.arange(0, N, max(1, N // 500))
    xo, efo, _, _ = oldp.solve_batch(L, ths[2][sel])
    assert np.array_equal(singles[2][1].cpu().numpy()[sel], efo) and np.abs(singles[2][0].cpu().numpy()[sel] - xo).max() <= TOL


def test_row_kernel_immutable_one_sided_and_duplicated_rows(lmpc):
    """IMMUTABLE rows (both bounds infinite: never enter a working set), one-sided rows, duplicated and opposing general
    rows (the singular-direction branch, infeasible points) on the row kernel; a problem with an equality row (flagged
    ACTIVE) is left to the wavefront kernel even when the row kernel is asked for."""
    rng = np.random.default_rng(41)
    n, nth, mg = 14, 4, 30
    Hh = rng.standard_normal((n, n)); H = Hh @ Hh.T + n * np.eye(n)
    A = rng.standard_normal((mg, n))
    A[5] = A[4]; A[7] = -A[6]                               # duplicated / opposing rows
    m = n + mg
    bu = rng.uniform(0.3, 1.5, m); bl = -rng.uniform(0.3, 1.5, m)
    sense = np.zeros(m, np.int32)
    for j in (1, 3, n + 2, n + 9):                          # both bounds infinite
        bu[j], bl[j], sense[j] = 1e30, -1e30, 4
    for j in (2, n + 1, n + 10):                            # one-sided
        bl[j] = -1e30
    bu[n + 7] = -bl[n + 6] - 0.4                            # opposing rows that cannot both hold for some theta
    W = 0.4 * rng.standard_normal((m, nth)); W[:n] = 0
    qp = lmpc.BatchedQP.from_mpqp(H, np.zeros(n), rng.standard_normal((n, nth)), A, bu, bl, W, sense, nout=3)
    theta = rng.uniform(-2, 2, (2000, nth))
    x, ef, it, act = _row_vs_wave_vs_oracle(lmpc, qp, theta)
    assert (ef >= 1).any() and (ef < 0).any()
    bits = act.view(np.uint64)
    for j in (1, 3, n + 2, n + 9):                          # an IMMUTABLE row is in no final active set
        assert not (((bits[:, j >> 6] >> np.uint64(j & 63)) & np.uint64(1)).any() or
                    ((bits[:, (m + j) >> 6] >> np.uint64((m + j) & 63)) & np.uint64(1)).any())
    # an equality row: flagged ACTIVE by the setup -> not the row kernel's (same answers through the option either way)
    bu2, bl2, s2 = bu.copy(), bl.copy(), sense.copy()
    bu2[n + 12] = bl2[n + 12] = 0.1; s2[n + 12] = 5
    q2 = lmpc.BatchedQP.from_mpqp(H, np.zeros(n), rng.standard_normal((n, nth)), A, bu2, bl2, W, s2, nout=3)
    assert q2.kernel_name == "wave"
    _row_vs_wave_vs_oracle(lmpc, q2, theta[:500], row=False)


# ------------------------------------------------------------------ branch and bound on the row kernel (binary32)
def _bnb_row_vs_wave_vs_oracle(lmpc, qp, s, theta, nsample=200):
    """Binary32 search on the row kernel (four searches per wavefront, "row_kernel" 1) against the wavefront kernel (0) --
    every output identical -- and a sample against the binary32 oracle."""
    import torch
    from oracle import ldp as oldp
    N = len(theta)
    th_d = torch.from_numpy(theta).cuda()
    out = {}
    for mode in (0, 1):
        qp.set_option("row_kernel", mode)
        seq = _row_launches(qp)
        it_d = torch.empty(N, dtype=torch.int32, device="cuda")
        ac_d = torch.zeros((N, qp.words), dtype=torch.int64, device="cuda")
        x_d, ef_d = qp.solve_device(th_d, iters=it_d, active=ac_d)
        torch.cuda.synchronize()
        qp.check()
        assert bool(_row_launches(qp, seq)) == bool(mode), (mode, _row_launches(qp, seq))
        out[mode] = (x_d.cpu().numpy(), ef_d.cpu().numpy(), it_d.cpu().numpy(), ac_d.cpu().numpy().view(np.uint64))
    for q in range(4):
        assert np.array_equal(out[0][q], out[1][q], equal_nan=(q == 0)), ("x", "exitflag", "iters", "active")[q]
    sel = np.arange(0, N, max(1, N // nsample))
    xo, efo, ito, acto = oldp.solve_batch(oracle_ldp_from(qp.ldp()), theta[sel], _copy_settings(lmpc, s), dtype=np.float32)
    x, ef, it, act = out[1]
    assert np.array_equal(ef[sel], efo) and np.array_equal(it[sel], ito) and np.array_equal(act[sel], acto)
    assert np.abs(x[sel] - xo).max() == 0.0
    return out[1]


@pytest.mark.parametrize("name", ["satellite4", "satellite20"])
def test_row_kernel_branch_and_bound_f32(lmpc, name):
    # the hybrid example of /root/reference/test/runtests.jl:820-834 (binaries: mpc_examples.jl:533-546), single precision
    # (codegen.jl:19 float_type="float"); satellite20 = BASELINE config 5: first pass of 48 rows on the row kernel, what
    # outgrows it listed for the wavefront kernel
    g = load_golden(name)
    s = lmpc.default_settings_f32()
    qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], settings=s)
    rng = np.random.default_rng(8)
    base = g["theta"]
    N = 3000 if name == "satellite20" else 6000
    theta = base[rng.integers(0, len(base), N)] * rng.uniform(0.2, 1.6, (N, 1)) + rng.normal(0, 0.01, (N, base.shape[1]))
    theta[: len(base)] = base[:N]
    theta = theta.astype(np.float32)
    x, ef, it, act = _bnb_row_vs_wave_vs_oracle(lmpc, qp, s, theta)
    assert (ef == 1).mean() > 0.9
    ok = ef == 1
    bins = np.flatnonzero(g["senses"] & 16)                            # runtests.jl:831-834 (f32: +-1e-5)
    assert np.all(np.minimum(np.abs(x[ok][:, bins] - g["bu"][bins]), np.abs(x[ok][:, bins] - g["bl"][bins])) < 1e-5)


def test_row_kernel_branch_and_bound_overflow_is_listed(lmpc):
    # a first pass too small for many of the searches ("wave_cap1" 42 rows for 40 binaries): those points are listed and
    # searched again by the wavefront kernel at the full capacity -- same answers as without the split
    g = load_golden("satellite20")
    s = lmpc.default_settings_f32()
    qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], settings=s)
    qp.set_option("wave_two_pass", 1)
    qp.set_option("wave_cap1", 42)
    rng = np.random.default_rng(9)
    base = g["theta"]
    theta = (base[rng.integers(0, len(base), 1500)] * rng.uniform(0.5, 1.6, (1500, 1))).astype(np.float32)
    x, ef, it, act = _bnb_row_vs_wave_vs_oracle(lmpc, qp, s, theta, nsample=100)
    assert (ef == 1).mean() > 0.9


def test_row_kernel_branch_and_bound_random_problems(lmpc):
    # binaries next to general rows and soft rows (n = 6, m = 11: the one-slot instantiation); infeasible assignments
    # prune, an infeasible problem ends with the search's flag
    rng = np.random.default_rng(2025)
    s = lmpc.default_settings_f32()
    nsolved = 0
    for trial in range(6):
        n, mg, nth = 6, 5, 3
        H, f, fth, A, bu, bl, W, sense = _random_qp(rng, n, mg, nth, nsoft=(1 if trial % 2 else 0))
        sense = sense.copy()
        sense[:3] |= 16
        qp = lmpc.BatchedQP.from_mpqp(H, f, fth, A, bu, bl, W, sense, settings=s)
        theta = rng.uniform(-1, 1, (1200, nth)).astype(np.float32)
        x, ef, it, act = _bnb_row_vs_wave_vs_oracle(lmpc, qp, s, theta)
        ok = ef >= 1
        nsolved += int(ok.sum())
        xb = x[ok][:, :3]
        lo = (bl[:3] + theta[ok] @ W[:3].T)
        hi = (bu[:3] + theta[ok] @ W[:3].T)
        assert np.all(np.minimum(np.abs(xb - lo), np.abs(xb - hi)) < 1e-4)
    assert nsolved >= 3000


def test_row_kernel_branch_and_bound_fuzz(lmpc):
    # random hybrid problems in both instantiations (tools/fuzz_row_bnb.py): the row kernel bit-identical to the
    # wavefront kernel, a sample of every trial identical to the binary32 oracle.  Seed 3 holds the problem (trial 37:
    # n = 24, 2 soft rows, 6 binaries) whose searches reach n + 2 + #soft rows in a working set -- one more than a plain
    # solve can: the kernels used to give those points up with exit flag -7 where the oracle solves them
    import importlib.util
    from oracle import ldp as oldp
    spec = importlib.util.spec_from_file_location("fuzz_row_bnb", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_row_bnb.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    rng = np.random.default_rng(3)
    s = lmpc.default_settings_f32()
    for t in range(40):
        same, ok, n, m, nb, solved, its = fz.run_trial(rng, t % 2 == 1, 1500, s, oldp.Settings)
        assert same and ok, (t, n, m, nb)


@pytest.mark.parametrize("name", ["mass_spring_3in", "soft_doc", "mass_spring"])
def test_row_kernel_binary32_plain_solves(lmpc, name):
    # binary32 (codegen.jl:19 float_type="float") on the row kernel: identical to the wavefront kernel, a sample identical
    # to the binary32 oracle
    import torch
    from oracle import ldp as oldp
    g = load_golden(name)
    s = lmpc.default_settings_f32()
    qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], settings=s)
    rng = np.random.default_rng(12)
    base = g["theta"]
    N = 20000
    theta = (base[rng.integers(0, len(base), N)] * rng.uniform(0.3, 1.5, (N, 1))).astype(np.float32)
    th_d = torch.from_numpy(theta).cuda()
    out = {}
    for mode in (0, 1):
        qp.set_option("row_kernel", mode)
        seq = _row_launches(qp)
        it_d = torch.empty(N, dtype=torch.int32, device="cuda")
        ac_d = torch.zeros((N, qp.words), dtype=torch.int64, device="cuda")
        x_d, ef_d = qp.solve_device(th_d, iters=it_d, active=ac_d)
        torch.cuda.synchronize()
        qp.check()
        assert bool(_row_launches(qp, seq)) == bool(mode), (mode, _row_launches(qp, seq))
        out[mode] = (x_d.cpu().numpy(), ef_d.cpu().numpy(), it_d.cpu().numpy(), ac_d.cpu().numpy().view(np.uint64))
    for q in range(4):
        assert np.array_equal(out[0][q], out[1][q], equal_nan=(q == 0))
    sel = np.arange(0, N, 40)
    xo, efo, ito, acto = oldp.solve_batch(oracle_ldp_from(qp.ldp()), theta[sel], _copy_settings(lmpc, s), dtype=np.float32)
    x, ef, it, act = out[1]
    assert np.array_equal(ef[sel], efo) and np.array_equal(it[sel], ito) and np.array_equal(act[sel], acto)
    assert np.abs(x[sel] - xo).max() == 0.0
    assert (ef >= 1).any()


def test_row_kernel_branch_and_bound_scratch_and_streams(lmpc):
    # the search's snapshot scratch is per handle and sized by the grid: released and allocated again between calls, and two
    # handles searching at once on two streams, the answers stay the same
    import torch
    g = load_golden("satellite20")
    s = lmpc.default_settings_f32()
    rng = np.random.default_rng(21)
    base = g["theta"]
    N = 12000
    theta = (base[rng.integers(0, len(base), N)] * rng.uniform(0.4, 1.5, (N, 1))).astype(np.float32)
    th_d = torch.from_numpy(theta).cuda()
    qps = [lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], settings=s)
           for _ in range(2)]
    x0, ef0 = qps[0].solve_device(th_d)                      # (N >= 8192: the row kernel by default)
    torch.cuda.synchronize()
    ref = (x0.cpu().numpy(), ef0.cpu().numpy())
    qps[0].release_scratch()
    x1, ef1 = qps[0].solve_device(th_d)
    torch.cuda.synchronize()
    assert np.array_equal(x1.cpu().numpy(), ref[0]) and np.array_equal(ef1.cpu().numpy(), ref[1])
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = []
    for r in range(3):
        for q, st in zip(qps, streams):
            outs.append(q.solve_device(th_d, stream=st.cuda_stream))
    torch.cuda.synchronize()
    for x, ef in outs:
        assert np.array_equal(x.cpu().numpy(), ref[0]) and np.array_equal(ef.cpu().numpy(), ref[1])
    qps[0].set_option("row_kernel", 0)
    xw, efw = qps[0].solve_device(th_d)
    torch.cuda.synchronize()
    assert np.array_equal(xw.cpu().numpy(), ref[0]) and np.array_equal(efw.cpu().numpy(), ref[1])


@pytest.mark.parametrize("name", ["satellite4", "satellite20"])
def test_row_kernel_branch_and_bound_f64(lmpc, name):
    # binary64 searches on the row kernel (one wavefront per SIMD: 336 registers): identical to the wavefront kernel and, on
    # a sample, to the oracle
    import torch
    from oracle import ldp as oldp
    g = load_golden(name)
    qp = _qp_from_golden(lmpc, g)
    rng = np.random.default_rng(18)
    base = g["theta"]
    N = 3000 if name == "satellite20" else 6000
    theta = base[rng.integers(0, len(base), N)] * rng.uniform(0.2, 1.6, (N, 1)) + rng.normal(0, 0.01, (N, base.shape[1]))
    theta[: len(base)] = base[:N]
    th_d = torch.from_numpy(theta).cuda()
    out = {}
    for mode in (0, 1):
        qp.set_option("row_kernel", mode)
        seq = _row_launches(qp)
        it_d = torch.empty(N, dtype=torch.int32, device="cuda")
        ac_d = torch.zeros((N, qp.words), dtype=torch.int64, device="cuda")
        x_d, ef_d = qp.solve_device(th_d, iters=it_d, active=ac_d)
        torch.cuda.synchronize()
        qp.check()
        assert bool(_row_launches(qp, seq)) == bool(mode), (mode, _row_launches(qp, seq))
        out[mode] = (x_d.cpu().numpy(), ef_d.cpu().numpy(), it_d.cpu().numpy(), ac_d.cpu().numpy().view(np.uint64))
    for q in range(4):
        assert np.array_equal(out[0][q], out[1][q], equal_nan=(q == 0))
    sel = np.arange(0, N, max(1, N // 150))
    xo, efo, ito, acto = oldp.solve_batch(oracle_ldp_from(qp.ldp()), theta[sel])
    x, ef, it, act = out[1]
    assert np.array_equal(ef[sel], efo) and np.array_equal(it[sel], ito) and np.array_equal(act[sel], acto)
    assert np.abs(x[sel] - xo).max() == 0.0
    assert (ef == 1).mean() > 0.9


def test_row_kernel_branch_and_bound_fuzz_f64(lmpc):
    import importlib.util
    from oracle import ldp as oldp
    spec = importlib.util.spec_from_file_location("fuzz_row_bnb", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_row_bnb.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    rng = np.random.default_rng(14)
    for t in range(24):
        same, ok, n, m, nb, solved, its = fz.run_trial(rng, t % 2 == 1, 1500, None, oldp.Settings, True)
        assert same and ok, (t, n, m, nb)


def test_row_kernel_fuzz_plain_solves(lmpc):
    # random plain problems over all instantiations, binary64 and binary32 alternating (tools/fuzz_row.py): the row kernel
    # identical to the wavefront kernel, a sample of every trial identical to the oracle.  Seed 5 holds the problem (trial
    # 297: binary32, n = 13, one soft row) whose working sets reach n + 2 + #soft rows: those points now go through the
    # slow path and end with the oracle's flag (they used to keep exit flag -7)
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_row", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_row.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    rng = np.random.default_rng(5)
    for t in range(300):
        same, ok, n, m, kn, solved, its, nlim = fz.run_trial(rng, t % 2 == 1, 3000)
        assert same and ok and nlim == 0, (t, n, m, kn, nlim)


def test_row_kernel_calls_captured_in_a_graph(lmpc):
    # lmpc_reserve, then an even number of calls captured in a hipGraph and replayed: the row kernel (plain solves as the
    # first of two passes, the second pass and the slow path behind it) allocates nothing inside the capture
    import torch
    g = load_golden("mass_spring_3in")
    qp = _qp_from_golden(lmpc, g, 3)
    assert qp.kernel_name == "row|wave"
    rng = np.random.default_rng(31)
    N = 4096
    theta = g["theta"][rng.integers(0, len(g["theta"]), N)] * rng.uniform(0.3, 1.3, (N, 1))
    th_d = torch.from_numpy(theta).cuda()
    x_ref, ef_ref = qp.solve_device(th_d)
    torch.cuda.synchronize()
    x_ref, ef_ref = x_ref.clone(), ef_ref.clone()
    qp = _qp_from_golden(lmpc, g, 3)                       # a fresh handle: its first calls are the captured ones
    qp.reserve(N)
    xs = [torch.zeros((N, qp.nout), dtype=torch.float64, device="cuda") for _ in range(2)]
    fs = [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in range(2)]
    st = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            for q in range(2):
                qp.solve_device(th_d, x=xs[q], exitflag=fs[q], stream=st.cuda_stream)
    for rep in range(3):
        for q in range(2):
            xs[q].zero_(); fs[q].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for q in range(2):
            assert torch.equal(xs[q], x_ref) and torch.equal(fs[q], ef_ref)
    qp.check()


def test_row_kernel_sixteen_row_first_pass_of_the_benchmark_class(lmpc):
    # pendulum_N50 (the reference's published benchmark class, docs/src/manual/benchmark.md:4-16): the one-slot shape with
    # ten constraint slots as a first pass of 16 rows (forced here; by default the handle's statistics choose it), what
    # outgrows it listed for the wavefront kernel -- identical to the wavefront kernel alone and to the oracle
    g = load_golden("pendulum_N50")
    qp = _qp_from_golden(lmpc, g, int(g["nu"]))
    rng = np.random.default_rng(51)
    base = g["theta"]
    N = 6000
    theta = base[rng.integers(0, len(base), N)] * rng.uniform(0.6, 1.8, (N, 1))
    qp.set_option("wave_two_pass", 1)
    qp.set_option("wave_cap1", 16)
    x, ef, it, act = _row_vs_wave_vs_oracle(lmpc, qp, theta)
    assert (ef >= 1).mean() > 0.9 and it.max() > 17          # (some points do outgrow 16 rows)
