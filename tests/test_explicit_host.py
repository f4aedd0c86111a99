"""Explicit MPC built on the host (lmpc_explicit_build_ldp): no GPU.  Packs come from the numpy restatement of the
QP -> LDP transform on the golden fixtures, training samples from the CPU oracle; the controller's laws, halfspaces,
serialised tree and host-side evaluation (the kernel's arithmetic) are checked against them."""
import numpy as np
import pytest

from conftest import load_golden


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


def _pack(name, nout=None):
    from oracle import ldp as oldp
    g = load_golden(name)
    n = g["H"].shape[0]
    L = oldp.qp2ldp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=n if nout is None else nout)
    pk = dict(M=L.M, du=L.du0, dl=L.dl0, Dth=L.Dth, Rout=L.Rout, x0=L.x0, Xth=L.Xth, sense=L.sense, ms=L.ms)
    return g, L, pk


_CACHE = {}


def _built(lmpc, name, N, hard=False, **opts):
    import bench
    from oracle import ldp as oldp
    key = (name, N, hard, tuple(sorted(opts.items())))
    if key not in _CACHE:
        g, L, pk = _pack(name)
        th = bench.make_theta(name, N, 11, hard)
        X, ef, _, act = oldp.solve_batch(L, th)
        ec = lmpc.explicit.ExplicitController.build_ldp(pk, th, act, ef, **opts)
        _CACHE[key] = (g, L, pk, th, X, ef, act, ec)
    return _CACHE[key]


@pytest.mark.parametrize("name,N", [("pendulum", 40000), ("soft_doc", 20000), ("pendulum_N50", 4000)])
def test_region_laws_equal_the_kkt_law(lmpc, name, N):
    # regions without active SOFT rows: the law against the QP-form KKT solve in numpy (explicit.affine_law);
    # regions with active SOFT rows (the LDP relaxes them): the law at a training point of the region against the
    # oracle's x there
    g, L, pk, th, X, ef, act, ec = _built(lmpc, name, N)
    lab, _ = ec.training(len(ef))
    info = ec.info()
    assert info["regions"] > 0 and info["regions"] + info["dropped_singular"] + info["dropped_capacity"] == info["distinct_sets"]
    soft = (L.sense & 8) != 0
    n_soft = 0
    for r in range(info["regions"]):
        reg = ec.region(r)
        up, lo = lmpc.explicit.mask_to_sets(reg["mask"], L.m)
        if soft[up + lo].any():
            n_soft += 1
            i = int(np.flatnonzero(lab == r)[0])
            xl = reg["F"] @ th[i] + reg["g"]
            assert np.abs(xl - X[i]).max() <= 1e-6 * (1 + np.abs(X[i]).max()), (r, xl, X[i])
        else:
            Fz, gz = lmpc.explicit.affine_law(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], reg["mask"])
            scale = 1 + max(np.abs(Fz).max(), np.abs(gz).max())
            assert np.abs(reg["F"] - Fz).max() <= 1e-9 * scale and np.abs(reg["g"] - gz).max() <= 1e-9 * scale, r
    if name != "pendulum":
        assert n_soft > 0


@pytest.mark.parametrize("name,N", [("pendulum", 40000), ("soft_doc", 20000), ("pendulum_N50", 4000)])
def test_training_points_satisfy_their_region(lmpc, name, N):
    # the solver stops once every inactive row is violated by less than primal_tol (1e-6, in the rows' normalised
    # units) and every multiplier has the right sign to dual_tol: a training point may sit that far outside its
    # region's exact halfspaces, and no farther
    g, L, pk, th, X, ef, act, ec = _built(lmpc, name, N)
    lab, _ = ec.training(len(ef))
    worst = 0.0
    for r in range(ec.info()["regions"]):
        reg = ec.region(r)
        pts = th[lab == r]
        viol = pts @ reg["A"].T - reg["b"]
        scale = 1 + np.abs(pts) @ np.abs(reg["A"]).T + np.abs(reg["b"])
        worst = max(worst, (viol / scale).max() if viol.size else 0.0)
    assert worst <= 1e-6


def _walk(blob, theta):
    head = blob[:128].view(np.int64)
    nth, nodes_n = int(head[0]), int(head[3])
    nodes = blob[head[6]:head[6] + 16 * nodes_n].view(np.int32).reshape(-1, 4)
    rows = blob[head[9]:head[10]].view(np.float64).reshape(-1, nth + 1)
    node = np.zeros(len(theta), np.int64)
    while True:
        inner = nodes[node, 0] >= 0
        if not inner.any():
            return node
        r = nodes[node[inner], 0]
        right = np.einsum("ij,ij->i", rows[r, :nth], theta[inner]) > rows[r, nth]
        node[inner] = np.where(right, nodes[node[inner], 2], nodes[node[inner], 1])


def test_blob_walk_reproduces_the_builders_tree_and_the_tree_only_misses(lmpc):
    import bench
    from oracle import ldp as oldp
    g, L, pk, th, X, ef, act, ec = _built(lmpc, "pendulum_N50", 4000)
    lab, leaf = ec.training(len(ef))
    lab_pts = lab >= 0
    walked = _walk(ec.blob(), th[lab_pts])
    assert np.mean(walked != leaf[lab_pts]) <= 1e-4
    assert ec.info()["depth"] >= 2
    # a fresh sample: every point the tree locates is located by the max_depth = 0 scan, in a region whose
    # halfspaces it satisfies; the tree's misses are few
    flat = lmpc.explicit.ExplicitController.build_ldp(pk, th, act, ef, max_depth=0)
    assert flat.info()["nodes"] == 1 and flat.info()["regions"] == ec.info()["regions"]
    th2 = bench.make_theta("pendulum_N50", 4000, 12)
    xd, fd, rd, _ = ec.locate_host(th2)
    xf, ff, rf, _ = flat.locate_host(th2)
    assert np.all(rf[rd >= 0] >= 0)
    for i in np.flatnonzero(rd >= 0):
        reg = ec.region(int(rd[i]))
        assert np.all(reg["A"] @ th2[i] <= reg["b"] + 1e-12 * (1 + np.abs(reg["b"])))
    both = (rd >= 0) & (rd == rf)
    assert np.array_equal(xd[both], xf[both]) and np.array_equal(fd[rd >= 0], ff[rd >= 0])
    misses = np.mean((rf >= 0) & (rd < 0))
    assert misses < 0.02, misses


def test_host_evaluation_matches_the_oracle(lmpc):
    # located points: the oracle's exit flag; its x to rounding where the region is the oracle's final active set
    import bench
    from oracle import ldp as oldp
    for name, hard in (("pendulum", False), ("pendulum", True), ("soft_doc", False)):
        g, L, pk, th, X, ef, act, ec = _built(lmpc, name, 40000 if name == "pendulum" else 20000, hard)
        th2 = bench.make_theta(name, 20000, 13, hard)
        X2, ef2, _, act2 = oldp.solve_batch(L, th2)
        x, f, r, rows = ec.locate_host(th2)
        loc = r >= 0
        assert loc.mean() >= (0.99 if name == "pendulum" else 0.4)
        assert np.array_equal(f[loc], ef2[loc]) and np.all(ef2[loc] >= 1)
        masks = np.array([ec.region(k)["mask"] for k in range(ec.info()["regions"])])
        same = loc.copy()
        same[loc] = (masks[r[loc]] == act2[loc]).all(1)
        tol = 1e-8 if name == "pendulum" else 1e-5      # soft_doc's reduced systems reach condition 1e11
        assert np.all(np.abs(x[same] - X2[same]) <= tol * (1 + np.abs(X2[same])))
        assert np.all(np.isnan(x[~loc])) and np.all(f[~loc] == 0)


def test_constant_law_without_parameters(lmpc):
    from oracle import ldp as oldp
    g, L, pk = _pack("pendulum")
    pk0 = dict(pk, Dth=np.zeros((L.m, 0)), Xth=np.zeros((L.nout, 0)))
    L0 = oldp.LDP(L.n, L.m, L.ms, 0, L.nout, L.M, L.du0 + 0.3, L.dl0 + 0.3, np.zeros((L.m, 0)), L.Rout, L.x0,
                  np.zeros((L.nout, 0)), L.sense, L.scale).contiguous()
    pk0.update(du=L0.du0, dl=L0.dl0)
    X, ef, _, act = oldp.solve_batch(L0, np.zeros((5, 0)))
    ec = lmpc.explicit.ExplicitController.build_ldp(pk0, np.zeros((5, 0)), act, ef)
    x, f, r, _ = ec.locate_host(np.zeros((3, 0)))
    assert np.all(r == 0) and np.all(f == ef[0]) and np.abs(x - X[0]).max() <= 1e-12


def test_capacity_cap_is_reported(lmpc):
    import bench
    from oracle import ldp as oldp
    g, L, pk = _pack("mass_spring_3in", nout=3)
    th = bench.make_theta("mass_spring_3in", 3000, 5, "feasible")
    X, ef, _, act = oldp.solve_batch(L, th)
    ec = lmpc.explicit.ExplicitController.build_ldp(pk, th, act, ef, max_regions=20)
    info = ec.info()
    assert info["regions"] == 20 and info["dropped_capacity"] > 100
    x, f, r, _ = ec.locate_host(th)
    assert np.all(r < 20) and np.array_equal(f[r >= 0], ef[r >= 0])


def test_refusals(lmpc):
    g, L, pk = _pack("satellite20")
    assert np.any(L.sense & 16)
    with pytest.raises(lmpc.LmpcError) as e:
        lmpc.explicit.ExplicitController.build_ldp(pk, np.zeros((1, L.nth)), np.zeros((1, (2 * L.m + 63) // 64), np.uint64),
                                                   np.ones(1, np.int32))
    assert e.value.code == -103 and "BINARY" in str(e.value)
    from oracle import mpc2mpqp as omm, ldp as oldp
    q = omm.mpc2mpqp(omm.game_kat())
    La = oldp.qp2ldp(q.H, q.f, q.f_theta, q.A, q.bu, q.bl, q.W, q.senses, nout=2)
    pka = dict(M=La.M, du=La.du0, dl=La.dl0, Dth=La.Dth, Rout=La.Rout, x0=La.x0, Xth=La.Xth, sense=La.sense, ms=La.ms)
    with pytest.raises(lmpc.LmpcError) as e:
        lmpc.explicit.ExplicitController.build_ldp(pka, np.zeros((1, La.nth)), np.zeros((1, 1), np.uint64),
                                                   np.ones(1, np.int32), is_avi=True)
    assert e.value.code == -103 and "is_avi" in str(e.value)
    g, L, pk = _pack("pendulum")
    big = dict(pk, Dth=np.zeros((L.m, 33)), Xth=np.zeros((L.nout, 33)))
    with pytest.raises(lmpc.LmpcError) as e:
        lmpc.explicit.ExplicitController.build_ldp(big, np.zeros((1, 33)), np.zeros((1, 1), np.uint64), np.ones(1, np.int32))
    assert e.value.code == -103 and "nth = 33" in str(e.value)
