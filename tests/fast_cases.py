"""Case table of the one-launch kernel's tests (tests/test_fast_cases_host.py, tests/test_gpu_fast.py): one boxed
problem per instantiated (n, nth) pair of lmpc_fast_inst.hip, the parameter batches that go with it, and the conditions
every batch of 1000 points or more has to meet ON THE ORACLE before a comparison with it counts as a test of the
kernel.  Numpy and the oracle only: nothing of the library is imported here.

The kernel finishes a point in one of three places: the streaming pass (the unconstrained optimum is feasible:
iters == 1), the straight-line tiers (rows are only ever added: iters == |active set| + 1) or the generic loop behind
them (fast_fallback: a row leaves the working set again, a pivot is singular or fval_bound is exceeded:
iters > |active set| + 1).  A batch that is to test all three has to hold points of all three kinds, and which kind a
point is depends on the Hessian and on how far theta pushes the optimum outside the box -- hence a Hessian family and
a per-point mix of theta scales per case, chosen on the CPU (KNOBS below).

n = 2: the oracle never removes a row on a two-variable boxed problem.  300 random problems (correlations up to
+-0.999, parameter spreads 0.3 ... 30, W on and off) x 1000 points: iters <= |active set| + 1 at every point, no point
fails.
The n = 2 cases are therefore held to every condition but the third (removing points).
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from oracle import ldp as oldp

K_FAST_PAY = 256            # kFastPay of lmpc_fast_kernel.hpp: queue positions whose shifts are handed over in LDS
N_COND = 2309               # 37 tiles, 5 workgroups of 8: the batch size the conditions apply to
SIZES = (1, 63, 64, 65, 513, 577, 641, 705, 2309)
# 513: the partial tile is a workgroup's only tile; 577 / 641 / 705: it lands on each of the three streaming roles
GUARD = 64                  # guard rows behind every output of the GPU tests
ITER_LIMIT_MIN = 7          # the smallest iteration limit fast_covers() accepts (LMPC_FAST_KMAX + 2)

# instantiated (n, nth) pairs of lmpc_fast_inst.hip
PAIRS = tuple((n, nth) for n in (2, 3, 4) for nth in range(1, 17)) + tuple((5, nth) for nth in range(1, 9))
# record paths, launch shapes, several batches: one pair per NT (the per-NT constants of the LDS-DMA path -- PIECES,
# LASTB, the last-piece guard, the counted waits -- are functions of NT alone)
NT_PAIRS = ((5, 1), (5, 2), (5, 3), (5, 7), (5, 8), (3, 9), (4, 15), (3, 16))


@dataclass(frozen=True)
class FastCase:
    n: int
    nth: int
    seed: int = 0
    family: str = "lowrank"         # "lowrank": Rm Rm' + ridge I, Rm of rank ceil(n/2); "equi": d ((1-c) I + c s s') d
    param: float = 0.0              # ridge / n ("lowrank"), c ("equi")
    scales: tuple = (1.0,)          # theta scale of point i: scales[i % len(scales)]
    use_w: bool = False             # parameter-dependent bounds (W != 0)
    nout: int = 1
    iter_limit: int = 0             # 0 = the default settings
    # generated controller's call: theta = [state; reference; disturbance; control[:nuprev]; parameter]
    layout: tuple = (0, 0, 0, 0, 0)     # (nx, nr, nd, nuprev, np)
    gather_nout: int = 1                # width of `control`
    null: tuple = ()                    # blocks of width > 0 passed as NULL (= zeros): "r", "d", "p"

    @property
    def name(self):
        return f"n{self.n}-nth{self.nth}"

    def with_nout(self, nout):
        return replace(self, nout=int(nout))


def problem(case):
    """(H, f, f_theta, bu, bl, W) of a case: a strictly convex QP with the n simple bounds as its only constraints."""
    n, nth = case.n, case.nth
    rng = np.random.default_rng(1000 * n + 10 * nth + 100_000 * case.seed)
    if case.family == "lowrank":
        Rm = rng.normal(size=(n, (n + 1) // 2))
        H = Rm @ Rm.T + case.param * n * np.eye(n)
    elif case.family == "equi":
        d = rng.uniform(0.7, 1.4, n)
        s = rng.choice([-1.0, 1.0], n)
        H = (d[:, None] * ((1.0 - case.param) * np.eye(n) + case.param * np.outer(s, s))) * d[None, :]
    else:
        raise ValueError(case.family)
    f_theta = rng.normal(size=(n, nth))
    f = np.zeros(n)
    bu = rng.uniform(0.2, 1.5, n)
    bl = -rng.uniform(0.2, 1.5, n)
    W = rng.normal(size=(n, nth)) * (0.2 if case.use_w else 0.0)
    return H, f, f_theta, bu, bl, W


def theta(case, N, batch=0):
    """Parameter batch number `batch` of a case, N points: point i is a standard normal vector times
    scales[i % len(scales)], so every tile holds the whole mix.  A smaller batch is a prefix of a larger one."""
    rng = np.random.default_rng(7 + 1000 * case.n + 10 * case.nth + 100_000 * case.seed + 1_000_003 * batch)
    full = max(int(N), N_COND)
    sc = np.asarray(case.scales, float)[np.arange(full) % len(case.scales)]
    return np.ascontiguousarray((rng.normal(size=(full, case.nth)) * sc[:, None])[:N])


def oracle_settings(case):
    s = oldp.default_settings()
    if case.iter_limit:
        s.iter_limit = case.iter_limit
    return s


def reference(case, th):
    """The oracle on the pack oracle.ldp.qp2ldp makes of the case: (x, exitflag, iters, active)."""
    H, f, f_theta, bu, bl, W = problem(case)
    L = oldp.qp2ldp(H, f, f_theta, np.zeros((0, case.n)), bu, bl, W, np.zeros(case.n, np.int32), case.nout)
    return oldp.solve_batch(L, th, oracle_settings(case))


def popcount(active):
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    out = np.zeros(len(a), np.int64)
    for w in range(a.shape[1]):
        v = a[:, w].copy()
        while v.any():
            out += (v & np.uint64(1)).astype(np.int64)
            v >>= np.uint64(1)
    return out


def removing(iters, active):
    """Points that finish in the generic loop: more iterations than rows added."""
    return np.asarray(iters) > popcount(active) + 1


def fast_stats(case, iters, active, exitflag):
    it, ef = np.asarray(iters), np.asarray(exitflag)
    nact = popcount(active)
    word = np.ascontiguousarray(active).view(np.uint64).reshape(len(it), -1)[:, 0]
    n = case.n
    queued = it != 1
    blocks = [int(queued[s:s + 512].sum()) for s in range(0, len(it), 512)]
    return dict(N=len(it), settled=int((it == 1).sum()), append_only=int(((it == nact + 1) & (it > 1) & (ef == 1)).sum()),
                removing=int((it > nact + 1).sum()), upper=int((word & np.uint64((1 << n) - 1) != 0).sum()),
                lower=int(((word >> np.uint64(n)) & np.uint64((1 << n) - 1) != 0).sum()), max_queued_in_block=max(blocks),
                failed=int((ef < 1).sum()))


def check_fast_conditions(case, iters, active, exitflag):
    """Conditions on the ORACLE's outputs for a batch of N >= 1000 points of `case` (nothing here is measured on the
    kernel): raises AssertionError naming the one that fails, returns the counts."""
    st = fast_stats(case, iters, active, exitflag)
    N = st["N"]
    assert N >= 1000, "the conditions apply to batches of 1000 points or more"
    assert st["settled"] >= 0.05 * N, (case.name, "settled by the screen", st)
    assert st["append_only"] >= 0.05 * N, (case.name, "append-only", st)
    if case.n >= 3:                                        # (n = 2: the oracle never removes a row, see above)
        assert st["removing"] >= 8, (case.name, "rows removed again", st)
    assert st["lower"] >= 1 and st["upper"] >= 1, (case.name, "a lower and an upper bound active", st)
    # more queued points in one workgroup's 8 tiles than positions that carry their shifts: the solving side takes
    # the handed-over AND the re-read record path
    assert st["max_queued_in_block"] > K_FAST_PAY, (case.name, "a 512-problem block with more than kFastPay queued", st)
    return st


# ---------------------------------------------------------------------------------------------------------------------
# Per-case knobs, chosen on the CPU so that the oracle alone meets the conditions at every pair:
# (seed, family, param, scales).  One setting did not serve all 56 pairs -- whether a row leaves again depends on the
# draw of f_theta as much as on H.
_A = (0.002, 0.05, 0.3, 2.0)
_B = (0.02, 0.5, 2.0, 6.0)
_C = (0.001, 0.02, 0.2, 1.0, 5.0)
_DEFAULT = {2: (0, "equi", 0.9, _A), 3: (0, "equi", 0.98, _A), 4: (0, "lowrank", 0.002, _A), 5: (0, "lowrank", 0.002, _A)}
KNOBS = {(2, 1): (0, "equi", 0.9, _B), (2, 2): (0, "equi", 0.9, _B), (2, 5): (0, "equi", 0.9, _B), (2, 7): (0, "equi", 0.9, _B),
         (3, 1): (0, "lowrank", 0.002, _A), (3, 5): (0, "equi", 0.98, _C),
         (4, 10): (0, "lowrank", 0.002, _C), (4, 12): (0, "lowrank", 0.002, _C), (4, 13): (0, "lowrank", 0.002, _C),
         (4, 15): (0, "lowrank", 0.002, _C), (4, 16): (0, "lowrank", 0.002, _C),
         (5, 1): (1, "lowrank", 0.002, _A)}


def _layout(k, n, nth):
    """Split of nth into (nx >= 1, nr, nd, nuprev, np), the control width and the NULL blocks of table entry k."""
    gnout = 1 if k % 2 == 0 else n
    nup = min((0, 1, gnout)[k % 3], nth - 1)
    rest = nth - 1 - nup
    want = ((1, 1, 1), (1, 0, 1), (0, 1, 0), (2, 1, 0), (0, 0, 2))[k % 5]
    w = []
    for v in want:
        v = min(v, rest)
        rest -= v
        w.append(v)
    nr, nd, npp = w
    nx = nth - nup - nr - nd - npp
    null = ((), ("r",), ("d", "p"), ("p",), ("r", "d"))[(k // 2) % 5]
    null = tuple(b for b in null if dict(r=nr, d=nd, p=npp)[b] > 0)
    return (nx, nr, nd, nup, npp), gnout, null


def _case(k, n, nth):
    seed, family, param, scales = KNOBS.get((n, nth), _DEFAULT[n])
    lay, gnout, null = _layout(k, n, nth)
    return FastCase(n, nth, seed, family, param, tuple(scales), use_w=(k % 2 == 1), layout=lay, gather_nout=gnout, null=null)


CASES = tuple(_case(k, n, nth) for k, (n, nth) in enumerate(PAIRS))
BY_PAIR = {(c.n, c.nth): c for c in CASES}
NT_CASES = tuple(BY_PAIR[p] for p in NT_PAIRS)
# the iteration limit in numbers: an n = 5 case on which the oracle, limited to ITER_LIMIT_MIN iterations, reports -4
LIMIT_CASE = replace(BY_PAIR[(5, 7)], iter_limit=ITER_LIMIT_MIN)


def instantiations():
    """The template arguments (NTHMAX, NT, N) the table claims for fast_kernel (plain and gather form) and
    fast_kernel_multi."""
    return {(8 if nth <= 8 else 16, nth, n) for n, nth in PAIRS}


def gather_blocks(case, th, nout=None):
    """theta of the generated controller's call split into its argument arrays: dict(control, state, reference,
    disturbance, parameter); a block of width 0 is None.  `control` is N x gather_nout with the previous control in
    its first nuprev columns and NaN (the sentinel) elsewhere."""
    nx, nr, nd, nup, npp = case.layout
    N = len(th)
    o1, o2, o3, o4 = nx, nx + nr, nx + nr + nd, nx + nr + nd + nup
    cut = lambda a, b: np.ascontiguousarray(th[:, a:b]) if b > a else None
    control = np.full((N, case.gather_nout if nout is None else nout), np.nan)
    control[:, :nup] = th[:, o3:o4]
    return dict(control=control, state=cut(0, o1), reference=cut(o1, o2), disturbance=cut(o2, o3), parameter=cut(o4, case.nth))


def null_theta(case, th):
    """theta as the kernel assembles it when the case's `null` blocks are passed as NULL: zeros there."""
    nx, nr, nd, nup, npp = case.layout
    o = dict(r=(nx, nx + nr), d=(nx + nr, nx + nr + nd), p=(nx + nr + nd + nup, case.nth))
    out = th.copy()
    for b in case.null:
        out[:, o[b][0]:o[b][1]] = 0.0
    return out
