"""TEST INFRASTRUCTURE: the derivative of the solution map computed independently of the arithmetic contract -- the
formula J = Xth + Rout M_A' K_A^-1 Dth_A solved densely in extended precision (np.longdouble: Gaussian elimination with
partial pivoting on the binary64 pack), central differences of the oracle, and the error measure the tolerance tests
share.  numpy and the oracle only."""
import numpy as np

from oracle import ldp as oldp

SENSE_SOFT = 8
EPS = float(np.finfo(np.float64).eps)


def solve_ld(K, B):
    """K^-1 B in np.longdouble, Gaussian elimination with partial pivoting."""
    K = np.array(K, np.longdouble)
    B = np.array(B, np.longdouble)
    k = len(K)
    for j in range(k):
        p = j + int(np.argmax(np.abs(K[j:, j])))
        if p != j:
            K[[j, p]] = K[[p, j]]
            B[[j, p]] = B[[p, j]]
        f = K[j + 1:, j] / K[j, j]
        K[j + 1:] -= f[:, None] * K[j][None, :]
        B[j + 1:] -= f[:, None] * B[j][None, :]
    for j in range(k - 1, -1, -1):
        B[j] = (B[j] - K[j, j + 1:] @ B[j + 1:]) / K[j, j]
    return B


def dense_jacobian(pack, rows, rho_soft):
    """(J in longdouble, cond(K_A) in binary64) for the active rows `rows`."""
    ld = np.longdouble
    rows = np.asarray(rows, int)
    Xth = np.asarray(pack["Xth"], ld).reshape(pack["nout"], pack["nth"])
    if len(rows) == 0:
        return Xth, 1.0
    M = np.asarray(pack["M"], ld)[rows]
    soft = (np.asarray(pack["sense"])[rows] & SENSE_SOFT) != 0
    K = M @ M.T + np.diag(np.where(soft, ld(rho_soft), ld(0)))
    Y = solve_ld(K, np.asarray(pack["Dth"], ld).reshape(pack["m"], pack["nth"])[rows])
    J = Xth + (np.asarray(pack["Rout"], ld) @ M.T) @ Y
    return J, float(np.linalg.cond(K.astype(np.float64)))


def dense_terms(pack, rows, rho_soft):
    """|| |Xth| + |Rout M_A'| |K_A^-1 Dth_A| ||_inf: the size of the terms J is the sum of.  Where outputs are pinned by
    their own active bounds J is zero and the computed J is the rounding residue of terms of this size."""
    ld = np.longdouble
    rows = np.asarray(rows, int)
    T = np.abs(np.asarray(pack["Xth"], ld).reshape(pack["nout"], pack["nth"]))
    if len(rows):
        M = np.asarray(pack["M"], ld)[rows]
        soft = (np.asarray(pack["sense"])[rows] & SENSE_SOFT) != 0
        K = M @ M.T + np.diag(np.where(soft, ld(rho_soft), ld(0)))
        Y = solve_ld(K, np.asarray(pack["Dth"], ld).reshape(pack["m"], pack["nth"])[rows])
        T = T + np.abs(np.asarray(pack["Rout"], ld) @ M.T) @ np.abs(Y)
    return float(T.sum(axis=1).max())


CANCELLED = 1e-6        # ||J||_inf below this share of the terms' size: J is a cancellation residue


def scaled_errors(J, Jtrue, cond, terms):
    """(max |J - Jtrue| / (eps cond(K_A) ||Jtrue||_inf), the same with the terms' size for ||Jtrue||_inf).  The first is
    None where ||Jtrue||_inf is a cancellation residue (below CANCELLED x terms): the measure is undefined at J = 0."""
    err = float(np.abs(np.asarray(J, np.longdouble) - Jtrue).max())
    nrm = float(np.abs(Jtrue).sum(axis=1).max())
    return (err / (EPS * cond * nrm) if nrm > CANCELLED * terms else None), err / (EPS * cond * terms)


def next_pow2_bound(measured):
    """The next power of two at or above 8 x measured."""
    return 2.0 ** int(np.ceil(np.log2(8.0 * measured)))


def central_differences(ldp, theta, h=1e-6, settings=None):
    """(FD (N, nout, nth), keep (N, nth)): central differences of the oracle's x, and which columns are usable: the point
    and its two neighbours are solved (exit flag >= 1) on the same active set."""
    X0, ef0, _, a0 = oldp.solve_batch(ldp, theta, settings)
    N, nth = theta.shape
    FD = np.zeros((N, ldp.nout, nth))
    keep = np.zeros((N, nth), bool)
    for t in range(nth):
        e = np.zeros(nth)
        e[t] = h
        Xp, efp, _, ap = oldp.solve_batch(ldp, theta + e, settings)
        Xm, efm, _, am = oldp.solve_batch(ldp, theta - e, settings)
        FD[:, :, t] = (Xp - Xm) / (2 * h)
        keep[:, t] = (ef0 >= 1) & (efp >= 1) & (efm >= 1) & (ap == a0).all(axis=1) & (am == a0).all(axis=1)
    return FD, keep, ef0, a0
