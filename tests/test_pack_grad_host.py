"""Gradient with respect to the pack on the host (lmpc_solve_pack_vjp_host, lmpc_transform_vjp): no GPU.  The host twin
runs the kernels' per-point arithmetic and the contract's tree; it is held value for value (np.array_equal) to the
numpy restatement of the contract (pack_grad_reference.py) on every case of pack_grad_cases.py, and the contract itself
to the truth: the formulas evaluated densely in extended precision, central differences of the transform, and central
differences of the oracle's solve from the QP data."""
import ast
import ctypes
import os

import numpy as np
import pytest

import pack_grad_cases as pc
import pack_grad_reference as pr
import sens_cases as sc
import sens_reference as sr
import sens_truth as st
from conftest import load_golden
from oracle import ldp as oldp

HERE = os.path.dirname(os.path.abspath(__file__))
N_NULL = 257                    # the NULL-output and forced-flag repeats run on this prefix of a batch


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


_CACHE = {}


def _data(lmpc, case):
    """pack, batch and the reference's results of a case (computed once)."""
    if case.name not in _CACHE:
        S = lmpc.default_settings()
        pack = sc.host_pack(case)
        b = pc.build(case, pack)
        cache = pr.derived(pack)
        ref = pr.pack_vjp(pack, b["theta"], b["active"], b["exitflag"], b["xbar"], S.rho_soft, S.zero_tol, cache)
        _CACHE[case.name] = dict(pack=pack, batch=b, cache=cache, ref=ref, S=S)
    return _CACHE[case.name]


def _host_call(lmpc, pack, b, N, want=pc.NAMES, want_thbar=True, want_status=True, settings=None):
    """The host twin on guarded outputs: dict of results after checking the guards and that no sentinel is left."""
    L = lmpc.lib()
    n, m, ms, nth, nout = (int(pack[k]) for k in ("n", "m", "ms", "nth", "nout"))
    G = sc.GUARD
    shp = pc.shapes(pack)
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    bufs = {k: np.full(int(np.prod(shp[k])) + 2 * G, sc.SENT) for k in want}
    thbar = np.full((N + 2 * G, nth), sc.SENT) if want_thbar else None
    status = np.full(N + 2 * G, sc.SENT_I, np.int32) if want_status else None
    arrs = [np.ascontiguousarray(pack[k], dtype=np.float64) for k in pc.NAMES]
    sense = np.ascontiguousarray(pack["sense"], dtype=np.int32)
    ins = [np.ascontiguousarray(b["theta"][:N], dtype=np.float64), np.ascontiguousarray(b["active"][:N], dtype=np.uint64),
           np.ascontiguousarray(b["exitflag"][:N], dtype=np.int32), np.ascontiguousarray(b["xbar"][:N], dtype=np.float64)]
    sp = ctypes.cast(ctypes.pointer(settings), ctypes.c_void_p) if settings is not None else None
    rc = L.lmpc_solve_pack_vjp_host(n, m, ms, nth, nout, *[vp(a) for a in arrs], vp(sense), sp, 0, N, *[vp(a) for a in ins],
                                    *[vp(bufs[k][G:]) if k in bufs else None for k in pc.NAMES],
                                    vp(thbar[G:]) if want_thbar else None, vp(status[G:]) if want_status else None)
    assert rc == 1, lmpc._cabi.last_error()
    out = {}
    for k, a in bufs.items():
        assert (a[:G] == sc.SENT).all() and (a[len(a) - G:] == sc.SENT).all(), f"a guard of {k}-bar was written"
        assert not (a[G:len(a) - G] == sc.SENT).any(), f"an entry of {k}-bar was not written"
        out[k] = a[G:len(a) - G].reshape(shp[k])
    if want_thbar:
        assert (thbar[:G] == sc.SENT).all() and (thbar[N + G:] == sc.SENT).all() and not (thbar[G:N + G] == sc.SENT).any()
        out["thbar"] = thbar[G:N + G]
    if want_status:
        assert (status[:G] == sc.SENT_I).all() and (status[N + G:] == sc.SENT_I).all() and not (status[G:N + G] == sc.SENT_I).any()
        out["status"] = status[G:N + G]
    return out


def _same(got, ref, names=pc.NAMES + ("thbar", "status")):
    for k in names:
        if k in got:
            assert np.array_equal(got[k], ref[k]), k


def test_reference_imports_nothing_of_the_library():
    allowed = {"numpy", "types"}
    for mod in ("pack_grad_reference.py",):
        tree = ast.parse(open(os.path.join(HERE, mod)).read())
        for node in ast.walk(tree):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else \
                [node.module] if isinstance(node, ast.ImportFrom) else []
            for nm in names:
                assert nm.split(".")[0] in allowed, f"{mod} imports {nm}"
    src = open(os.path.join(HERE, "pack_grad_reference.py")).read()
    assert "linearmpc" not in src and "ctypes" not in src and "lmpc." not in src


def test_reference_fma_equals_libm():
    from loop_reference import fma as fma_libm
    rng = np.random.default_rng(0)
    n = 60000
    a, b, c = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n) for _ in range(3))
    c[:20000] = -(a * b)[:20000] * (1 + rng.integers(-4, 5, 20000) * 2.0 ** -52)          # cancelling sums
    c[20000:25000] = 0.0
    a[25000:30000] = 0.0
    c[30000:40000] = (a * b)[30000:40000] * 2.0 ** rng.integers(-60, 60, 10000)             # every distance of exponents
    assert np.array_equal(pr.fma(a, b, c), fma_libm(a, b, c))


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_case_conditions(lmpc, case):
    d = _data(lmpc, case)
    pc.check_conditions(case, d["pack"], d["batch"], d["ref"])
    assert set(d["ref"]["status"].tolist()) >= {1, 0}


def test_conditions_reject_batches_that_miss_them(lmpc):
    case = pc.BY_NAME["own-n12-m76-nth17"]
    d = _data(lmpc, case)
    pack, b, S = d["pack"], d["batch"], d["S"]
    N = pc.N_COND

    def run(bb, n=1000, slab=pc.SLAB_MIN):                                  # (a prefix with both special blocks: quicker)
        bb = {k: (v[:n] if isinstance(v, np.ndarray) and len(v) == N else v) for k, v in bb.items()}
        ref = pr.pack_vjp(pack, bb["theta"], bb["active"], bb["exitflag"], bb["xbar"], S.rho_soft, S.zero_tol, d["cache"])
        pc.check_conditions(case, pack, bb, ref, slab)

    run(b)
    with pytest.raises(AssertionError, match="all zero"):                   # no cotangent at all
        run(dict(b, xbar=np.zeros_like(b["xbar"])))
    with pytest.raises(AssertionError, match="dl-bar"):           # every lower side moved to the upper side
        a = b["active"].copy()
        m = pack["m"]
        bits = np.unpackbits(a.view(np.uint8), axis=1, bitorder="little")
        bits[:, :m] |= bits[:, m:2 * m]
        bits[:, m:2 * m] = 0
        run(dict(b, active=np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view(np.uint64))))
    with pytest.raises(AssertionError, match="without an active row"):      # the empty block given the sets of block 0
        a = b["active"].copy()
        a[64 * pc.EMPTY_BLOCK:64 * pc.EMPTY_BLOCK + 64] = a[128:192]
        run(dict(b, active=a))
    with pytest.raises(AssertionError, match="status != 1 only"):           # the failed block solved
        e = b["exitflag"].copy()
        e[64 * pc.FAILED_BLOCK:64 * pc.FAILED_BLOCK + 64] = 1
        e[e < 1] = 1
        run(dict(b, exitflag=e, active=np.where((sc.set_sizes(b["active"], pack["m"]) > 64)[:, None], 0, b["active"])))
    with pytest.raises(AssertionError, match="power of two"):
        run(b, n=1024)
    with pytest.raises(AssertionError, match="3 slabs"):
        run(b, slab=12)


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_host_twin_equals_the_reference(lmpc, case):
    d = _data(lmpc, case)
    got = _host_call(lmpc, d["pack"], d["batch"], pc.N_COND)
    _same(got, d["ref"])
    assert (got["thbar"][got["status"] != 1] == 0).all()
    # the Python wrapper
    b = d["batch"]
    w = lmpc.pack_vjp_host(d["pack"], b["theta"], b["active"], b["exitflag"], b["xbar"])
    _same(w, d["ref"])


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_outputs_null_one_at_a_time_and_failed_flags(lmpc, case):
    d = _data(lmpc, case)
    pack, b, S = d["pack"], d["batch"], d["S"]
    cut = {k: (v[:N_NULL] if isinstance(v, np.ndarray) and len(v) == pc.N_COND else v) for k, v in b.items()}
    ref = pr.pack_vjp(pack, cut["theta"], cut["active"], cut["exitflag"], cut["xbar"], S.rho_soft, S.zero_tol, d["cache"])
    for skip in pc.NAMES:
        _same(_host_call(lmpc, pack, cut, N_NULL, want=tuple(k for k in pc.NAMES if k != skip)), ref)
    _same(_host_call(lmpc, pack, cut, N_NULL, want_thbar=False, want_status=False), ref)
    failed = dict(cut, exitflag=np.full(N_NULL, -1, np.int32))
    got = _host_call(lmpc, pack, failed, N_NULL)
    assert (got["status"] == 0).all() and (got["thbar"] == 0).all()
    for k in pc.NAMES:
        assert (got[k] == 0).all(), k


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_thbar_and_status_equal_the_vjp_twin(lmpc, case):
    d = _data(lmpc, case)
    b = d["batch"]
    v, s = lmpc.solver.sens_host(d["pack"], b["active"], b["exitflag"], b["xbar"])
    assert np.array_equal(d["ref"]["thbar"], v) and np.array_equal(d["ref"]["status"], s)
    got = _host_call(lmpc, d["pack"], b, pc.N_COND, want=())
    assert np.array_equal(got["thbar"], v) and np.array_equal(got["status"], s)


def test_batch_sum_equals_the_tree_of_one_point_calls(lmpc):
    case = pc.BY_NAME["own-n5-m80-nth17"]
    d = _data(lmpc, case)
    pack, b = d["pack"], d["batch"]
    lo, N = 40, 37
    pick = lambda i, n: {k: (v[lo + i:lo + i + n] if isinstance(v, np.ndarray) and len(v) == pc.N_COND else v) for k, v in b.items()}
    whole = _host_call(lmpc, pack, pick(0, N), N)
    ones = [_host_call(lmpc, pack, pick(i, 1), 1) for i in range(N)]
    assert any((o["status"] != 1).any() for o in ones) and sum(int(o["status"][0] == 1) for o in ones) > 20
    for k in pc.NAMES:
        assert np.array_equal(whole[k], pr.tree_sum(np.stack([o[k] for o in ones]))), k


def test_tree_sum_pairs_neighbours_first():
    x = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 0.0, 1.0])
    assert pr.tree_sum(x) == ((1.0 + 2.0 ** -53) + (2.0 ** -53 + 0.0)) + ((1.0 + 0.0) + (0.0 + 0.0))
    y = np.array([2.0 ** -53, 2.0 ** -53, 1.0])
    assert pr.tree_sum(y) == (2.0 ** -53 + 2.0 ** -53) + (1.0 + 0.0) and pr.tree_sum(y) != (2.0 ** -53 + 1.0) + 2.0 ** -53


def test_every_new_symbol_is_declared_and_exported(lmpc):
    new = ("lmpc_solve_pack_vjp_device", "lmpc_solve_pack_vjp", "lmpc_solve_pack_vjp_host", "lmpc_pack_grad_launch_info",
           "lmpc_transform_vjp")
    header = open(os.path.join(HERE, "..", "include", "lmpc_hip.h")).read()
    for name in new:
        assert name in lmpc.SYMBOLS and hasattr(lmpc.lib(), name) and f"int {name}(" in header, name
    assert lmpc.lib().lmpc_abi_version() == 2
    assert lmpc.lib().lmpc_pack_grad_launch_info(None, None, 0) == -100


def test_refusals_and_argument_errors(lmpc):
    case = pc.BY_NAME["own-n5-m25-nth1"]
    pack = sc.host_pack(case)
    act = np.zeros((3, case.words), np.uint64)
    ef = np.ones(3, np.int32)
    th, xb = np.ones((3, pack["nth"])), np.ones((3, pack["nout"]))

    def code(**kw):
        p = dict(pack)
        args = dict(theta=th, active=act, exitflag=ef, xbar=xb)
        for k, v in kw.items():
            (args if k in ("theta", "active", "exitflag", "xbar", "settings", "is_avi") else p)[k] = v
        with pytest.raises(lmpc.LmpcError) as e:
            lmpc.pack_vjp_host(p, **args)
        return e.value.code

    binary = pack["sense"].copy()
    binary[0] |= 16
    assert code(sense=binary) == -103
    assert code(is_avi=True) == -103
    prox = lmpc.default_settings()
    prox.eps_prox = 1e-3
    assert code(settings=prox) == -103
    assert code(nth=0, Dth=np.zeros((pack["m"], 0)), Xth=np.zeros((pack["nout"], 0)), theta=np.zeros((3, 0))) == -100
    L = lmpc.lib()
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    arrs = [np.ascontiguousarray(pack[k], dtype=np.float64) for k in pc.NAMES]
    head = [int(pack[k]) for k in ("n", "m", "ms", "nth", "nout")] + [vp(a) for a in arrs] + [vp(pack["sense"]), None, 0]
    none7 = [None] * 7
    assert L.lmpc_solve_pack_vjp_host(*head, 3, None, vp(act), vp(ef), vp(xb), *none7, None, None) == -100       # theta NULL
    assert L.lmpc_solve_pack_vjp_host(*head, 3, vp(th), vp(act), vp(ef), None, *none7, None, None) == -100       # xbar NULL
    assert L.lmpc_solve_pack_vjp_host(*head, -1, vp(th), vp(act), vp(ef), vp(xb), *none7, None, None) == -100
    assert L.lmpc_solve_pack_vjp_host(*head, 0, None, None, None, None, *none7, None, None) == 1
    assert L.lmpc_solve_pack_vjp_host(*head, 3, vp(th), vp(act), vp(ef), vp(xb), *none7, None, None) == 1        # every output NULL
    # a different rho_soft / zero_tol is used
    S = lmpc.default_settings()
    S.rho_soft, S.zero_tol = 1e-3, 1e-9
    d = _data(lmpc, case)
    b = {k: (v[:257] if isinstance(v, np.ndarray) and len(v) == pc.N_COND else v) for k, v in d["batch"].items()}
    got = _host_call(lmpc, pack, b, 257, settings=S)
    ref = pr.pack_vjp(pack, b["theta"], b["active"], b["exitflag"], b["xbar"], 1e-3, 1e-9, d["cache"])
    _same(got, ref)
    assert not np.array_equal(got["M"], d["ref"]["M"])


# ---------------------------------------------------------------------------------------------------------------- truth
def _dense_point(pack, rows, upper, theta, xbar, rho_soft):
    """The point's contributions by the formulas in np.longdouble (dict of arrays), cond(K_A), and the summed magnitudes
    of the terms of the whole inner product (the measure's scale)."""
    ld = np.longdouble
    n, m, nth, nout = (int(pack[k]) for k in ("n", "m", "nth", "nout"))
    M, Rout = np.asarray(pack["M"], ld), np.asarray(pack["Rout"], ld)
    Dth = np.asarray(pack["Dth"], ld).reshape(m, nth)
    th, xb = np.asarray(theta, ld), np.asarray(xbar, ld)
    out = {k: np.zeros(s, ld) for k, s in pc.shapes(pack).items()}
    out["x0"] = xb.copy()
    out["Xth"] = np.outer(xb, th)
    scale = float(np.abs(xb).sum() * (1 + np.abs(th).sum()))
    cond = 1.0
    if len(rows):
        MA = M[rows]
        soft = (np.asarray(pack["sense"])[rows] & st.SENSE_SOFT) != 0
        K = MA @ MA.T + np.diag(np.where(soft, ld(rho_soft), ld(0)))
        d = np.where(upper, np.asarray(pack["du"], ld)[rows], np.asarray(pack["dl"], ld)[rows]) + Dth[rows] @ th
        sol = st.solve_ld(K, np.stack([d, MA @ (Rout.T @ xb)], axis=1))
        lam, y = sol[:, 0], sol[:, 1]
        v, w, vb = MA.T @ lam, MA.T @ y, Rout.T @ xb
        out["M"][rows] = np.outer(lam, vb - w) - np.outer(y, v)
        out["du"][rows] = np.where(upper, y, 0)
        out["dl"][rows] = np.where(upper, 0, y)
        out["Dth"][rows] = np.outer(y, th)
        out["Rout"] = np.outer(xb, v)
        cond = float(np.linalg.cond(K.astype(np.float64)))
        aw, av = np.abs(MA).T @ np.abs(y), np.abs(MA).T @ np.abs(lam)
        scale += float(np.abs(lam).sum() * (np.abs(vb) + aw).sum() + np.abs(y).sum() * av.sum()
                       + np.abs(y).sum() * (1 + np.abs(th).sum()) + np.abs(xb).sum() * av.sum())
    return out, cond, scale


# Per point, as one-point calls: max over the seven arrays of |contribution - true contribution| / (eps x cond(K_A) x the
# summed magnitudes of the terms of the point's whole inner product), the true contribution being the formulas in
# np.longdouble; worst point of a case over one point per distinct active set with status 1 of the whole batch (every set
# size and special).  Measured with the numpy reference (pack_grad_reference.pack_vjp on one point at a time):
#     cases without SOFT rows (hard):  0.721 (fast-n5-nth7, 19 sets)
#     cases with SOFT rows:            0.243 (own-n127-m140-nth17, 111 sets; the K form at rho_soft = 1e-6, cond to 1e11)
# each bound the next power of two at or above 8 x the measured maximum (sens_truth.next_pow2_bound).
TRUTH_MEASURED = {"hard": 0.721, "soft": 0.243}          # fast-n5-nth7, own-n127-m140-nth17 -> bounds 8 and 2
TRUTH_BOUND = {k: st.next_pow2_bound(v) for k, v in TRUTH_MEASURED.items()}
assert TRUTH_BOUND == {"hard": 8.0, "soft": 2.0}


def truth_points(pack, b, status):
    """One point per distinct active set among the points of status 1 with a non-zero cotangent."""
    rows = sr.rows_of(b["active"], pack["m"])
    done = np.nonzero((status == 1) & np.any(b["xbar"] != 0.0, axis=1))[0]
    _, first = np.unique(rows[done], axis=0, return_index=True)
    return done[np.sort(first)]


def truth_error(pack, b, points, one_point, rho_soft):
    """Worst scaled error over `points`; one_point(p) = the seven contributions of point p alone (dict)."""
    rows = sr.rows_of(b["active"], pack["m"])
    up = pr.upper_bits(b["active"], pack["m"])
    worst = 0.0
    for p in points:
        r = np.nonzero(rows[p])[0]
        c, cond, scale = _dense_point(pack, r, up[p, r], b["theta"][p], b["xbar"][p], rho_soft)
        got = one_point(p)
        err = max(float(np.abs(np.asarray(got[k], np.longdouble) - c[k]).max()) for k in c if c[k].size)
        worst = max(worst, err / (st.EPS * cond * scale))
    return worst


def _one(b, p):
    return {k: (v[p:p + 1] if isinstance(v, np.ndarray) and len(v) == pc.N_COND else v) for k, v in b.items()}


def _kind(case):
    return "soft" if case.nsoft else "hard"


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_contributions_against_the_formulas_in_extended_precision(lmpc, case):
    d = _data(lmpc, case)
    pack, b = d["pack"], d["batch"]
    pts = truth_points(pack, b, d["ref"]["status"])
    e = truth_error(pack, b, pts, lambda p: _host_call(lmpc, pack, _one(b, p), 1), d["S"].rho_soft)
    print(f"{case.name} ({_kind(case)}): {len(pts)} sets, scaled error {e:.3g}")
    assert len(pts) >= 4
    assert e <= TRUTH_BOUND[_kind(case)]


# lmpc_transform_vjp against central differences of lmpc_transform: <bars, transform(data + h D) - transform(data - h D)>
# / 2h against <transform_vjp(bars), D> for random bars and random directions D (symmetric for H), relative to the sum
# of the magnitudes of the terms of the second inner product, worst of TRANSFORM_SEEDS draws of bars and directions.
# Measured with the numpy adjoint (pack_grad_reference.transform_vjp) in the place of the library's: TRANSFORM_MEASURED,
# the bound the next power of two at or above 8 x that.
TRANSFORM_SEEDS = (1, 2, 3, 4, 5, 6)
TRANSFORM_MEASURED = 8.77e-9                               # soft_doc; pendulum 1.8e-9, mass_spring 1.4e-9, prestab 6.9e-9, random 1.2e-9
TRANSFORM_BOUND = st.next_pow2_bound(TRANSFORM_MEASURED)
assert TRANSFORM_BOUND == 2.0 ** -23
QP_KEYS = ("H", "f", "f_theta", "A", "bu", "bl", "W")


def _direction(rng, qp, key, x0):
    """A random direction of `key` along which the transform stays differentiable and feasible, and the step's scale (1):
    every entry moves in proportion to max(|entry|, 1) (mass_spring's W spans nine decades); symmetric for H; zero on a
    zero row of A (scaling sets in at any non-zero norm), on bounds that stand for infinity and on the bounds of rows
    whose two bounds (nearly) meet (a step would cross the other bound)."""
    D = rng.standard_normal(np.shape(x0))
    if key == "H":
        D = D + D.T
    fin = np.abs(x0) < 1e20
    D = D * np.maximum(np.where(fin, np.abs(x0), 0.0), 1.0)
    if key == "A":
        D[~np.any(x0 != 0.0, axis=1)] = 0.0
    if key in ("bu", "bl"):
        D[~fin | (qp["bu"] - qp["bl"] < 1e-4 * np.maximum(np.abs(x0), 1.0))] = 0.0
    return D, 1.0


def _golden_qp(name):
    g = load_golden(name)
    n = g["H"].shape[0]
    qp = dict(H=np.asarray(g["H"], float), f=np.asarray(g["f"], float).reshape(n), f_theta=np.asarray(g["f_theta"], float).reshape(n, -1),
              A=np.asarray(g["A"], float).reshape(-1, n), bu=np.asarray(g["bu"], float).reshape(-1), bl=np.asarray(g["bl"], float).reshape(-1))
    qp["W"] = np.asarray(g["W"], float).reshape(len(qp["bu"]), -1)
    kw = dict(senses=np.asarray(g["senses"], np.int32), nout=n)
    return qp, kw


def _random_qp():
    rng = np.random.default_rng(5)
    n, ms, mg, nth, nout, nx = 6, 4, 5, 3, 2, 2
    R = rng.standard_normal((n, n))
    A = rng.standard_normal((mg, n))
    A[3] = 0.0                                              # a zero-norm row: the transform leaves it unscaled
    qp = dict(H=R @ R.T + n * np.eye(n), f=rng.standard_normal(n), f_theta=rng.standard_normal((n, nth)), A=A,
              bu=rng.uniform(0.5, 2, ms + mg), bl=-rng.uniform(0.5, 2, ms + mg), W=rng.standard_normal((ms + mg, nth)))
    return qp, dict(senses=np.zeros(ms + mg, np.int32), nout=nout, K=rng.standard_normal((nout, nx)), nx=nx)


def lib_adjoint(lmpc):
    return lambda qp, kw, bars: lmpc.transform_vjp(*[qp[k] for k in QP_KEYS], bars, **kw)


def ref_adjoint(qp, kw, bars):
    return pr.transform_vjp(*[qp[k] for k in QP_KEYS], bars, nout=kw["nout"], K=kw.get("K"), nx=kw.get("nx", 0))


def _transform_problem(name):
    if name == "random":
        return _random_qp()
    qp, kw = _golden_qp(name)
    if name == "prestab":
        g = load_golden(name)
        assert "K" in g, "the prestab fixture carries its feedback"
        kw.update(K=np.asarray(g["K"], float), nx=int(np.asarray(g["K"]).shape[1]), nout=int(np.asarray(g["K"]).shape[0]))
    return qp, kw


def transform_fd_error(lmpc, qp, kw, seed, adjoint):
    rng = np.random.default_rng(seed)
    base = lmpc.transform(*[qp[k] for k in QP_KEYS], **kw)
    # (cotangents in proportion to 1 / max(|output|, 1): every output entry weighs the same in the inner product, so that
    # the rounding of the large ones -- mass_spring's Dth reaches 1e9 -- does not drown the difference)
    bars = {k: rng.standard_normal(np.shape(base[k])) / np.maximum(np.abs(base[k]), 1.0) for k in pc.NAMES}
    g = adjoint(qp, kw, bars)
    worst = 0.0
    keys = QP_KEYS + (("K",) if kw.get("K") is not None else ())
    for key in keys:
        x0 = kw["K"] if key == "K" else qp[key]
        if np.size(x0) == 0:
            continue
        D, scale = _direction(rng, qp, key, x0)
        h = 1e-6 * scale
        val = []
        for sgn in (1, -1):
            q2, k2 = dict(qp), dict(kw)
            if key == "K":
                k2["K"] = x0 + sgn * h * D
            else:
                q2[key] = x0 + sgn * h * D
            t = lmpc.transform(*[q2[k] for k in QP_KEYS], **k2)
            val.append(sum(float((bars[k] * t[k]).sum()) for k in pc.NAMES))
        fd = (val[0] - val[1]) / (2 * h)
        ad = float((g[key] * D).sum())
        worst = max(worst, abs(fd - ad) / max(float(np.abs(g[key] * D).sum()), 1e-300))
    assert np.array_equal(np.asarray(g["H"]), np.asarray(g["H"]).T)
    return worst


@pytest.mark.parametrize("name", ["pendulum", "mass_spring", "soft_doc", "prestab", "random"])
def test_transform_vjp_against_central_differences(lmpc, name):
    qp, kw = _transform_problem(name)
    e = max(transform_fd_error(lmpc, qp, kw, s, lib_adjoint(lmpc)) for s in TRANSFORM_SEEDS)
    print(f"{name}: relative difference {e:.3g}")
    assert e <= TRANSFORM_BOUND


def test_transform_vjp_fails_as_the_transform_fails(lmpc):
    qp, kw = _random_qp()
    bars = {}
    with pytest.raises(lmpc.LmpcError) as e:
        lmpc.transform_vjp(-qp["H"], *[qp[k] for k in QP_KEYS[1:]], bars, **kw)
    assert e.value.code == -5                                               # not positive definite
    H = qp["H"].copy()
    H[0, 1] += 1.0
    with pytest.raises(lmpc.LmpcError) as e:
        lmpc.transform_vjp(H, *[qp[k] for k in QP_KEYS[1:]], bars, **kw)
    assert e.value.code == -103
    g = lmpc.transform_vjp(*[qp[k] for k in QP_KEYS], bars, **kw)          # no cotangent: zero gradients
    assert all(np.all(g[k] == 0) for k in g)


# End to end from the QP data: <xbar, x(data + h D) - x(data - h D)> / 2h by the oracle (qp2ldp + solve_batch) against
# transform_vjp(pack gradient) contracted with D, over the points whose active set is the same at the point and at +-h.
# Relative to the terms of the second inner product, worst direction of the three problems.  Measured with the numpy
# reference in the place of the library (pack_grad_reference.pack_vjp and transform_vjp): E2E_MEASURED, the bound the
# next power of two at or above 8 x that.
E2E_MEASURED = 5.91e-8                                     # mass_spring_3in, A; pendulum 8.1e-11, mass_spring 1.8e-9
E2E_BOUND = st.next_pow2_bound(E2E_MEASURED)
assert E2E_BOUND == 2.0 ** -21


def ref_pack_grad(pack, th, act, ef, xbar):
    return pr.pack_vjp(pack, th, act, ef, xbar)


@pytest.mark.parametrize("name", ["pendulum", "mass_spring", "mass_spring_3in"])
def test_end_to_end_against_central_differences_of_the_oracle(lmpc, name):
    worst = e2e_error(lmpc, name, lmpc.pack_vjp_host, lib_adjoint(lmpc))
    assert worst <= E2E_BOUND


def e2e_error(lmpc, name, pack_grad, adjoint):
    import bench
    qp, kw = _golden_qp(name)
    N = 600
    th = bench.make_theta(name, N, 11, False)
    rng = np.random.default_rng(3)
    xbar = rng.standard_normal((N, qp["H"].shape[0]))

    def solve(q):
        L = oldp.qp2ldp(q["H"], q["f"], q["f_theta"], q["A"], q["bu"], q["bl"], q["W"], kw["senses"], nout=kw["nout"])
        X, ef, _, act = oldp.solve_batch(L, th)
        return L, X, ef, act

    L0, X0, ef0, a0 = solve(qp)
    pack = sc.pack_of(L0)
    worst, solved = 0.0, int((ef0 >= 1).sum())
    for key in ("H", "f_theta", "A", "bu", "W"):
        if qp[key].size == 0:
            continue
        D, scale = _direction(rng, qp, key, qp[key])
        h = 1e-6 * scale
        _, Xp, efp, ap = solve(dict(qp, **{key: qp[key] + h * D}))
        _, Xm, efm, am = solve(dict(qp, **{key: qp[key] - h * D}))
        use = (ef0 >= 1) & (efp >= 1) & (efm >= 1) & (ap == a0).all(axis=1) & (am == a0).all(axis=1)
        assert use.sum() >= 0.9 * solved, f"{name}/{key}: {use.sum()} usable points of {solved}"
        fd = float((xbar[use] * (Xp[use] - Xm[use])).sum() / (2 * h))
        g = pack_grad(pack, th[use], a0[use], ef0[use], xbar[use])
        assert (g["status"] == 1).all()
        d = adjoint(qp, kw, {k: g[k] for k in pc.NAMES})
        ad = float((d[key] * D).sum())
        rel = abs(fd - ad) / max(float(np.abs(d[key] * D).sum()), 1e-300)
        print(f"{name}/{key}: central difference {fd:.9g}, adjoint {ad:.9g}, relative to the terms {rel:.3g}, usable {use.sum()}/{solved}")
        worst = max(worst, rel)
    return worst
