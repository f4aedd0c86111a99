"""TEST INFRASTRUCTURE: the arithmetic contract of the differentiable solve (include/lmpc_hip.h, "Differentiable solve")
restated in numpy, one IEEE-754 operation at a time, with `fma` of loop_reference.py.  Nothing here calls the library.

A pack is a dict with n, m, nth, nout, M (m x n), Dth (m x nth), Rout (nout x n), Xth (nout x nth), sense (m), as
`BatchedQP.ldp()` returns it.  Points are grouped by |A| and every operation is applied to a whole group at once; the
order of the operations on any one value is the contract's.
"""
import numpy as np

from loop_reference import fma

SENSE_SOFT = 8
MAX_SET = 64
DONE, FAILED_POINT, SINGULAR, TOO_MANY = 1, 0, -1, -7


def tri(a):
    return a * (a + 1) // 2


def gram(pack):
    """Full symmetric G = M M' with the chain acc = fma(M[a][k], M[b][k], acc) from 0 over k (the pack's triangle)."""
    M = np.asarray(pack["M"], float)
    m, n = M.shape
    G = np.zeros((m, m))
    for k in range(n):
        G = fma(M[:, k][:, None], M[:, k][None, :], G)
    return G


def derived(pack):
    """(G, P = M Rout') by their chains."""
    M, Rout = np.asarray(pack["M"], float), np.asarray(pack["Rout"], float)
    P = np.zeros((M.shape[0], Rout.shape[0]))
    for k in range(M.shape[1]):
        P = fma(M[:, k][:, None], Rout[:, k][None, :], P)
    return gram(pack), P


def rows_of(active, m):
    """Boolean (N, m): row j is active if bit j (upper side) or bit m + j (lower side) is set."""
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    bits = np.unpackbits(a.view(np.uint8), axis=1, bitorder="little")[:, :2 * m].astype(bool)
    return bits[:, :m] | bits[:, m:2 * m]


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
    """y of L D L' y = w for right-hand sides w (g, k, r): forward with columns ascending, the diagonal through the
    stored reciprocals, backward with columns descending."""
    z = w.copy()
    k = z.shape[1]
    for p in range(k - 1):
        z[:, p + 1:] = fma(-L[:, p + 1:, p][:, :, None], z[:, p][:, None, :], z[:, p + 1:])
    z = z * rD[:, :, None]
    for p in range(k - 1, 0, -1):
        z[:, :p] = fma(-L[:, p, :p][:, :, None], z[:, p][:, None, :], z[:, :p])
    return z


def sens(pack, active, exitflag, xbar=None, rho_soft=1e-6, zero_tol=1e-11, cache=None):
    """VJP (xbar (N, nout): returns thbar (N, nth)) or Jacobian (xbar None: J (N, nout, nth)), and status (N,)."""
    m, nth, nout = int(pack["m"]), int(pack["nth"]), int(pack["nout"])
    G, P = cache if cache is not None else derived(pack)
    Dth, Xth = np.asarray(pack["Dth"], float).reshape(m, nth), np.asarray(pack["Xth"], float).reshape(nout, nth)
    soft = (np.asarray(pack["sense"]) & SENSE_SOFT) != 0
    rows = rows_of(active, m)
    N = len(rows)
    cnt = rows.sum(axis=1)
    ef = np.asarray(exitflag)
    jac = xbar is None
    nr = nout if jac else 1
    out = np.zeros((N, nr, nth))
    status = np.where(ef < 1, FAILED_POINT, np.where(cnt > MAX_SET, TOO_MANY, DONE)).astype(np.int32)
    xb = None if jac else np.asarray(xbar, float).reshape(N, nout)
    live = np.nonzero(status == DONE)[0]
    if len(live) == 0:
        return (out if jac else out[:, 0, :]), status
    # the factor depends on the set alone (and so does the Jacobian): computed once per distinct set
    uniq, inv = np.unique(rows[live], axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    ucnt = uniq.sum(axis=1)
    for k in np.unique(ucnt):
        us = np.nonzero(ucnt == k)[0]                            # distinct sets of this size
        idx = np.nonzero(uniq[us])[1].reshape(len(us), k) if k else np.zeros((len(us), 0), int)
        local = np.full(len(uniq), -1)
        local[us] = np.arange(len(us))
        pts = np.nonzero(local[inv] >= 0)[0]                     # positions in `live` of the points with such a set
        sel, lu = live[pts], local[inv[pts]]
        if k:
            ok, L, D, rD = factor(G, soft, idx, rho_soft, zero_tol)
        else:
            ok = np.ones(len(us), bool)
        if jac:
            acc = np.broadcast_to(Xth[None, :, :], (len(us), nout, nth)).copy()
            if k:
                y = substitute(L, rD, P[idx])                    # (u, k, nout): w_i of e_r is P[a_i][r]
                for i in range(k):
                    acc = fma(Dth[idx[:, i]][:, None, :], y[:, i, :][:, :, None], acc)
            acc = acc[lu]
        else:
            acc = np.zeros((len(sel), 1, nth))
            for q in range(nout):
                acc = fma(Xth[q][None, None, :], xb[sel, q][:, None, None], acc)
            if k:
                pidx = idx[lu]
                w = np.zeros((len(sel), k, 1))
                for q in range(nout):
                    w = fma(P[pidx, q][:, :, None], xb[sel, q][:, None, None], w)
                y = substitute(L[lu], rD[lu], w)
                for i in range(k):
                    acc = fma(Dth[pidx[:, i]][:, None, :], y[:, i, :][:, :, None], acc)
        bad = ~ok[lu]
        acc[bad] = 0.0
        status[sel[bad]] = SINGULAR
        out[sel] = acc
    return (out if jac else out[:, 0, :]), status
