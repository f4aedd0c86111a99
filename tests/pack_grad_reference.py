"""TEST INFRASTRUCTURE: the arithmetic contract of the gradient with respect to the pack (include/lmpc_hip.h, "Gradient
with respect to the pack") restated in numpy, one IEEE-754 operation at a time.  Nothing here calls the library, and
nothing but numpy is imported: the fused multiply-add is emulated in binary64 arrays (`fma`; tests/test_pack_grad_host.py
holds it to libm's on random and cancelling operands), the factor and the substitutions are those of sens_reference.py
restated with it.

A pack is a dict with n, m, nth, nout, M (m x n), du, dl (m), Dth (m x nth), Rout (nout x n), Xth (nout x nth), sense
(m), as `BatchedQP.ldp()` returns it.  Points are grouped by |A| and every operation is applied to a whole group at
once; the order of the operations on any one value is the contract's.  The sum over the batch is the balanced tree,
by repeated pairwise addition of neighbours.
"""
import numpy as np

from types import SimpleNamespace

NAMES = ("M", "du", "dl", "Dth", "Rout", "x0", "Xth")
LEAF_BYTES = 48 << 20           # the leaves of one tree are built for as many columns of M at a time as fit in this


sr = SimpleNamespace(SENSE_SOFT=8, MAX_SET=64, DONE=1, FAILED_POINT=0, SINGULAR=-1, TOO_MANY=-7)


def _two_sum(x, y):
    s = x + y
    b = s - x
    return s, (x - (s - b)) + (y - b)


def fma(a, b, c):
    """round(a * b + c) with ONE rounding, elementwise with broadcasting, in binary64: the product exactly as a pair
    (Veltkamp's split and Dekker's product), then the sum of three by Boldo and Melquiond's emulation (two exact sums, the
    low parts added with rounding to odd, one last rounded sum).  Exact while no intermediate overflows or is subnormal;
    the operands here are far from both."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (a, b, c)))
    with np.errstate(over="ignore", invalid="ignore"):
        t = 134217729.0 * a
        ah = t - (t - a)
        al = a - ah
        t = 134217729.0 * b
        bh = t - (t - b)
        bl = b - bh
        uh = a * b
        ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl
        th, tl = _two_sum(c, ul)
        vh, vl = _two_sum(uh, th)
        z, e = _two_sum(tl, vl)
        bits = np.ascontiguousarray(z).view(np.int64)
        fix = (e != 0.0) & ((bits & 1) == 0)
        step = np.where((e > 0.0) == (z > 0.0), 1, -1)
        z = np.where(fix, bits + step, bits).view(np.float64)
        return vh + z


def rows_of(active, m):
    """Boolean (N, m): row j is active if bit j (upper side) or bit m + j (lower side) is set."""
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    bits = np.unpackbits(a.view(np.uint8), axis=1, bitorder="little")[:, :2 * m].astype(bool)
    return bits[:, :m] | bits[:, m:2 * m]


def derived(pack):
    """(G = M M' in full, P = M Rout') by their chains from 0 over the n columns."""
    M, Rout = np.asarray(pack["M"], float), np.asarray(pack["Rout"], float)
    G, P = np.zeros((M.shape[0], M.shape[0])), np.zeros((M.shape[0], Rout.shape[0]))
    for k in range(M.shape[1]):
        G = fma(M[:, k][:, None], M[:, k][None, :], G)
        P = fma(M[:, k][:, None], Rout[:, k][None, :], P)
    return G, P


def factor(G, soft, idx, rho, zero_tol):
    """LDL' of K_A for a group: idx (g, k) ascending rows.  Returns (ok (g,), L (g, k, k) strictly lower, D, rD)."""
    g, k = idx.shape
    K = G[idx[:, :, None], idx[:, None, :]]
    d = np.arange(k)
    K[:, d, d] = np.where(soft[idx], K[:, d, d] + rho, K[:, d, d])
    L = np.zeros((g, k, k))
    D, rD = np.ones((g, k)), np.ones((g, k))
    ok = np.ones(g, bool)
    for j in range(k):
        v = K[:, j:, j].copy()
        for p in range(j):
            c = L[:, j, p] * D[:, p]
            v = fma(-L[:, j:, p], c[:, None], v)
        bad = v[:, 0] < zero_tol
        ok &= ~bad                                   # (a failed point's later columns are computed and thrown away)
        D[:, j] = np.where(bad, 1.0, v[:, 0])
        rD[:, j] = 1.0 / D[:, j]
        L[:, j + 1:, j] = v[:, 1:] * rD[:, j][:, None]
    return ok, L, D, rD


def substitute(L, rD, w):
    """Solutions of L D L' y = w for right-hand sides w (g, k, r): forward with columns ascending, the diagonal through
    the stored reciprocals, backward with columns descending."""
    z = w.copy()
    k = z.shape[1]
    for p in range(k - 1):
        z[:, p + 1:] = fma(-L[:, p + 1:, p][:, :, None], z[:, p][:, None, :], z[:, p + 1:])
    z = z * rD[:, :, None]
    for p in range(k - 1, 0, -1):
        z[:, :p] = fma(-L[:, p, :p][:, :, None], z[:, p][:, None, :], z[:, :p])
    return z


def tree_sum(leaves):
    """Root of the balanced binary tree over the first axis, padded with +0.0 to a power of two: node = left + right."""
    N = leaves.shape[0]
    P = 1
    while P < N:
        P *= 2
    a = np.zeros((P,) + leaves.shape[1:])
    a[:N] = leaves
    while a.shape[0] > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def upper_bits(active, m):
    """Boolean (N, m): the upper-side bit of row j (a row with both bits counts as upper)."""
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    return np.unpackbits(a.view(np.uint8), axis=1, bitorder="little")[:, :m].astype(bool)


def point_solve(pack, theta, active, exitflag, xbar, rho_soft=1e-6, zero_tol=1e-11, cache=None):
    """Stage 1 of the contract per point: status (N,), thbar (N, nth), and for the points of status 1 their rows idx
    (list of (sel, idx (g, k))), lam and y (N, 64; position i of the set)."""
    m, nth, nout = int(pack["m"]), int(pack["nth"]), int(pack["nout"])
    G, P = cache if cache is not None else derived(pack)
    Dth, Xth = np.asarray(pack["Dth"], float).reshape(m, nth), np.asarray(pack["Xth"], float).reshape(nout, nth)
    du, dl = np.asarray(pack["du"], float).reshape(m), np.asarray(pack["dl"], float).reshape(m)
    soft = (np.asarray(pack["sense"]) & sr.SENSE_SOFT) != 0
    rows = rows_of(active, m)
    up = upper_bits(active, m)
    N = len(rows)
    th, xb = np.asarray(theta, float).reshape(N, nth), np.asarray(xbar, float).reshape(N, nout)
    cnt = rows.sum(axis=1)
    ef = np.asarray(exitflag)
    status = np.where(ef < 1, sr.FAILED_POINT, np.where(cnt > sr.MAX_SET, sr.TOO_MANY, sr.DONE)).astype(np.int32)
    thbar = np.zeros((N, nth))
    lam, y = np.zeros((N, sr.MAX_SET)), np.zeros((N, sr.MAX_SET))
    groups = []
    live = np.nonzero(status == sr.DONE)[0]
    for k in np.unique(cnt[live]):
        sel = live[cnt[live] == k]
        g = len(sel)
        idx = np.nonzero(rows[sel])[1].reshape(g, k) if k else np.zeros((g, 0), int)
        acc = np.zeros((g, nth))
        for q in range(nout):
            acc = fma(Xth[q][None, :], xb[sel, q][:, None], acc)
        ok = np.ones(g, bool)
        if k:
            ok, L, D, rD = factor(G, soft, idx, rho_soft, zero_tol)
            w = np.zeros((g, k))
            for q in range(nout):
                w = fma(P[idx, q], xb[sel, q][:, None], w)
            u = up[sel[:, None], idx]
            d = np.where(u, du[idx], dl[idx])
            for t in range(nth):
                d = fma(Dth[idx, t], th[sel, t][:, None], d)
            sol = substitute(L, rD, np.stack([d, w], axis=2))
            for i in range(k):
                acc = fma(Dth[idx[:, i]], sol[:, i, 1][:, None], acc)
            lam[sel[ok], :k], y[sel[ok], :k] = sol[ok, :, 0], sol[ok, :, 1]
        status[sel[~ok]] = sr.SINGULAR
        thbar[sel[ok]] = acc[ok]
        if ok.any():
            groups.append((sel[ok], idx[ok]))
    return dict(status=status, thbar=thbar, lam=lam, y=y, groups=groups, upper=up)


def prefix(s, N):
    """point_solve's result restricted to the first N points of its batch (a point's values do not depend on the batch)."""
    groups = [(sel[sel < N], idx[sel < N]) for sel, idx in s["groups"]]
    return dict(status=s["status"][:N], thbar=s["thbar"][:N], lam=s["lam"][:N], y=s["y"][:N], upper=s["upper"][:N],
                groups=[(sel, idx) for sel, idx in groups if len(sel)])


def pack_vjp(pack, theta, active, exitflag, xbar, rho_soft=1e-6, zero_tol=1e-11, cache=None, solved=None):
    """The seven sums over the batch (dict M, du, dl, Dth, Rout, x0, Xth), thbar (N, nth) and status (N,).  solved: the
    result of point_solve on these points, where the caller has it."""
    n, m, nth, nout = (int(pack[k]) for k in ("n", "m", "nth", "nout"))
    M, Rout = np.asarray(pack["M"], float).reshape(m, n), np.asarray(pack["Rout"], float).reshape(nout, n)
    s = solved if solved is not None else point_solve(pack, theta, active, exitflag, xbar, rho_soft, zero_tol, cache)
    N = len(s["status"])
    th, xb = np.asarray(theta, float).reshape(N, nth), np.asarray(xbar, float).reshape(N, nout)
    lam, y = s["lam"], s["y"]
    done = s["status"] == sr.DONE
    # v, w, vbar, g per point and column
    v, w, vb = np.zeros((N, n)), np.zeros((N, n)), np.zeros((N, n))
    for sel, idx in s["groups"]:
        vv, ww = np.zeros((len(sel), n)), np.zeros((len(sel), n))
        for i in range(idx.shape[1]):
            vv = fma(M[idx[:, i]], lam[sel, i][:, None], vv)
            ww = fma(M[idx[:, i]], y[sel, i][:, None], ww)
        v[sel], w[sel] = vv, ww
    for q in range(nout):
        vb = fma(Rout[q][None, :], xb[:, q][:, None], vb)
    g = vb - w
    xq = np.where(done[:, None], xb, 0.0)
    out = {}
    out["x0"] = tree_sum(xq)
    out["Xth"] = tree_sum(np.where(done[:, None, None], xb[:, :, None] * th[:, None, :], 0.0))
    out["Rout"] = tree_sum(np.where(done[:, None, None], xb[:, :, None] * v[:, None, :], 0.0))
    leaf_u, leaf_l, leaf_d = np.zeros((N, m)), np.zeros((N, m)), np.zeros((N, m, nth))
    for sel, idx in s["groups"]:
        k = idx.shape[1]
        if k == 0:
            continue
        u = s["upper"][sel[:, None], idx]
        yy = y[sel, :k]
        leaf_u[sel[:, None], idx] = np.where(u, yy, 0.0)
        leaf_l[sel[:, None], idx] = np.where(u, 0.0, yy)
        leaf_d[sel[:, None], idx] = yy[:, :, None] * th[sel][:, None, :]
    out["du"], out["dl"], out["Dth"] = tree_sum(leaf_u), tree_sum(leaf_l), tree_sum(leaf_d)
    Mb = np.zeros((m, n))
    cb = max(1, LEAF_BYTES // (8 * max(1, m) * 2 * max(1, N)))
    for c0 in range(0, n, cb):
        c1 = min(n, c0 + cb)
        leaf = np.zeros((N, m, c1 - c0))
        for sel, idx in s["groups"]:
            k = idx.shape[1]
            if k == 0:
                continue
            prod = y[sel, :k][:, :, None] * v[sel, None, c0:c1]
            leaf[sel[:, None], idx] = fma(lam[sel, :k][:, :, None], g[sel, None, c0:c1], -prod)
        Mb[:, c0:c1] = tree_sum(leaf)
    out["M"] = Mb
    out["thbar"], out["status"] = s["thbar"], s["status"]
    return out


def transform_vjp(H, f, f_theta, A, bu, bl, W, bars, nout, K=None, nx=0):
    """The adjoint of the QP -> LDP transform in plain numpy binary64 (no bit contract; the formulas of DESIGN 3.9a): what
    the tolerance of the library's lmpc_transform_vjp is measured with.  bars: dict of row-major M, du, dl, Dth, Rout, x0,
    Xth (a missing one counts as zero).  Returns dict H, f, f_theta, A, bu, bl, W, K."""
    H, f, fth, A = np.asarray(H, float), np.asarray(f, float), np.asarray(f_theta, float), np.asarray(A, float)
    n, nth = fth.shape
    A = A.reshape(-1, n)
    m = len(bu)
    ms = m - A.shape[0]
    sym = lambda X: 0.5 * (X + X.T)
    C = np.linalg.inv(np.linalg.cholesky(sym(H)).T)             # H = R'R, C = R^-1 (upper)
    Z = C @ C.T
    E = np.vstack([np.eye(ms, n), A])
    M0 = E @ C
    s = np.sqrt((M0 * M0).sum(axis=1))
    sc = np.where(s > 0, s, 1.0)
    shp = dict(M=(m, n), du=(m,), dl=(m,), Dth=(m, nth), Rout=(nout, n), x0=(nout,), Xth=(nout, nth))
    b = {k: np.zeros(shp[k]) if bars.get(k) is None else np.asarray(bars[k], float).reshape(shp[k]) for k in NAMES}
    M, Dth = M0 / sc[:, None], (np.asarray(W, float).reshape(m, nth) + E @ Z @ fth) / sc[:, None]
    du, dl = (np.asarray(bu, float) + E @ Z @ f) / sc, (np.asarray(bl, float) + E @ Z @ f) / sc
    dot = np.where(s > 0, (b["M"] * M).sum(axis=1) + (b["Dth"] * Dth).sum(axis=1) + b["du"] * du + b["dl"] * dl, 0.0)
    M0b = (b["M"] - M * dot[:, None]) / sc[:, None]
    Wb, bub, blb = b["Dth"] / sc[:, None], b["du"] / sc, b["dl"] / sc
    shb = bub + blb
    pad = lambda X: np.vstack([X.reshape(nout, -1), np.zeros((n - nout, X.reshape(nout, -1).shape[1]))])
    Phi = E.T @ Wb - pad(b["Xth"])
    phi = E.T @ shb - pad(b["x0"])[:, 0]
    Cb = np.triu(E.T @ M0b + pad(b["Rout"]))
    T = C.T @ Cb
    U = np.triu(T, 1) + 0.5 * np.diag(np.diag(T))
    Hb = -Z @ sym(Phi @ fth.T + np.outer(phi, f)) @ Z - C @ sym(U) @ C.T
    Ab = M0b[ms:] @ C.T + Wb[ms:] @ (Z @ fth).T + np.outer(shb[ms:], Z @ f)
    return dict(H=sym(Hb), f=Z @ phi, f_theta=Z @ Phi, A=Ab, bu=bub, bl=blb, W=Wb,
                K=None if K is None else -b["Xth"][:, :nx])
