"""Case table of the tiers pass's tests (tests/test_tiers_cases_host.py, tests/test_gpu_tiers.py): qp_tiers_kernel<N>
(lmpc_qp_tiers_kernel.hpp, launched by lmpc_qp_tiers.hip) at every instantiation N = 2 ... 12, the arithmetic of its
launch restated, the rule for what the pass must FINISH and what it must leave on the work list, and the conditions a
batch has to meet ON THE ORACLE before a comparison with it counts as a test of the kernel.  Numpy and the oracle only:
nothing of the library is imported here.

The pass and the kernel behind it give the same bits, so "x, flags, iteration counts and active sets equal the oracle's"
says nothing about WHICH of the two finished a point: a pass that queues everything passes such a test.  The GPU tests
therefore read the pass's work list (option "list_snapshot", lmpc_work_list_read) and hold it against must_finish()
below, point for point; the launch record (lmpc_front_pass_info) is held against the restated launch arithmetic.

What the pass finishes (the kernel's text, restated on the oracle's outputs): a point whose path only ever APPENDS rows
-- iters == popcount(active) + 1 -- and ends optimal (1), optimal with a SOFT row violated (2) or infeasible (-1) on a
working set of at most n + 1 rows.  Everything else is queued:
  * a blocking multiplier (a removal): iters > popcount(active) + 1;
  * a working set that outgrows the last tier: popcount(active) > n + 1 (SOFT rows only: n + 1 hard rows are singular);
  * the stall guard (progress_tol / cycle_tol) and a violated row of the working set: the oracle reports -2 for both.
fval_bound ends a point inside the pass: infeasible (-1), append-only, so the rule needs no clause for it.

Families.  "random": the parity test's family (H = Hh Hh' + n I, standard normal rows, bounds +-U(0.5, 2), W = 0.3 N(0, 1)
on the general rows), theta in four amplitude blocks 1, 3, 8, 20 interleaved point by point, so every tile of 64 holds
the whole mix.  On that family every append-only infeasible finish sits at n + 1 hard rows (the count rule): tiers k < N
never see a vanishing pivot.  The dependent-row cases put one there:
  "dup"   row b repeats row a with a lower bound ABOVE a's upper bound: whenever both are in the working set the pivot
          vanishes, nothing blocks the singular direction, the point is infeasible at that size;
  "sum"   row c = row a + row b with an upper bound they can jointly violate: the pivot vanishes and the direction IS
          blocked -- a removal, which the pass must queue;
  "tie"   row b repeats row a bounds and all: two rows violated by the same amount to the bit, the first one wins.
(Both SIDES of one row violated at once -- the kernel's "upper bound before lower" -- would take a row whose lower bound
lies above its upper bound, and lmpc_setup refuses such a problem: no case can reach that order through the library.)
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from oracle import ldp as oldp

K_SHARDS = 64               # kShards of lmpc_wave_layout.hpp: segments of the work list
N_COND = 4096               # points of a case's batch: 64 tiles, one per segment
GUARD = 64                  # guard rows behind every output of the GPU tests
SIZES = (1, 63, 64, 65)
AMPS = (1.0, 3.0, 8.0, 20.0)
NS = tuple(range(2, 13))    # the instantiations of lmpc_qp_tiers.hip
WIDTH_N = (2, 3, 7, 11)     # one N per QpRow width (4, 8, 12, 16 reals a row)
SENSE_SOFT, SENSE_IMMUTABLE, SENSE_EQUALITY, SENSE_BINARY = 8, 4, 5, 16


# ---------------------------------------------------------------------------------------------------------------------
# the launch arithmetic of lmpc_qp_tiers_kernel.hpp / lmpc_qp_tiers.hip, restated
def scan_row_reals(n):
    """qp_scan_row_reals: M_j (n), du0_j, dl0_j padded to 4, 8, 12 or 16 reals."""
    return 4 if n <= 2 else (8 if n <= 6 else (12 if n <= 10 else 16))


def lds_reals(n, m):
    """QpTiersLds<N>::reals(m): the scan pack, the packed Gram matrix (rounded up to an even count), four wavefronts'
    bound shifts b[m][64]."""
    oB = (m * scan_row_reals(n) + m * (m + 1) // 2 + 1) & ~1
    return oB + 4 * m * 64


def lds_bytes(n, m):
    return 8 * lds_reals(n, m)


def grid(nprob, cus):
    """Workgroups of four wavefronts: min(CUs, ceil(tiles / 4)), rounded up to a multiple of 16."""
    tiles = (nprob + 63) // 64
    g = min(cus, (tiles + 3) // 4)
    return (g + 15) // 16 * 16


def seg_cap(nprob):
    """Entries a segment of the work list holds (lane_seg_cap of lmpc_api.hip)."""
    return (((nprob + K_SHARDS - 1) // K_SHARDS + 64 * 32 + 256) + 255) & ~255


def tile_segment(t):
    """Tile t (points 64 t ... 64 t + 63) belongs to wavefront t % (4 grid); 4 grid is a multiple of 64, so its segment
    is t % 64 whatever the grid."""
    return t % K_SHARDS


def pack_active(upper, lower, m):
    """The kernel's two-word packing of an active set: bit j of word 0 = row j at its upper bound, bit m + j of the
    128-bit pair = at its lower bound.  upper / lower: Python ints (bit j = row j).  Returns (w0, w1)."""
    full = (1 << 64) - 1
    both = upper | (lower << m)
    return both & full, (both >> 64) & full


def words(m):
    return (2 * m + 63) // 64


# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class TiersCase:
    name: str
    n: int
    mg: int                         # general rows
    ms: int = -1                    # simple bounds in front of them: -1 = n, else 0
    nth: int = 4
    nout: int = 1
    seed: int = 0
    scale: float = 1.0              # factor on the bounds
    soft: tuple = ()                # rows flagged SOFT
    dep: tuple = ()                 # dependent rows: ("dup", a, b, gap) / ("sum", a, b, c, t) / ("tie", a, b)
    flags: tuple = ()               # (row, sense) pairs beyond SOFT: refusals
    fval_bound: float = 0.0         # 0 = the default settings
    progress_tol: float = 0.0
    iter_limit: int = 0
    amps: tuple = AMPS

    @property
    def nms(self):
        return self.n if self.ms < 0 else self.ms

    @property
    def m(self):
        return self.nms + self.mg

    @property
    def words(self):
        return words(self.m)


def problem(case):
    """(H, f, f_theta, A, bu, bl, W, sense) of a case.  Row indices in `soft`, `dep` and `flags` count all m rows, the
    simple bounds first."""
    n, mg, nth, ms = case.n, case.mg, case.nth, case.nms
    rng = np.random.default_rng(7919 * case.seed + 1000 * n + 10 * mg + nth)
    Hh = rng.standard_normal((n, n))
    H = Hh @ Hh.T + n * np.eye(n)
    A = rng.standard_normal((mg, n))
    m = ms + mg
    bu = case.scale * rng.uniform(0.5, 2.0, m)
    bl = -case.scale * rng.uniform(0.5, 2.0, m)
    W = 0.3 * rng.standard_normal((m, nth))
    W[:ms] = 0.0
    f_theta = rng.standard_normal((n, nth))
    sense = np.zeros(m, np.int32)
    for j in case.soft:
        sense[j] |= SENSE_SOFT
    for j, s in case.flags:
        sense[j] |= s
    g = lambda j: j - ms                                     # (dependent rows are general rows)
    if case.dep:
        kind = case.dep[0]
        if kind == "dup":
            _, a, b, gap = case.dep
            A[g(b)] = A[g(a)]; W[b] = W[a]
            bl[a] = -50.0 * case.scale; bu[b] = 50.0 * case.scale
            bl[b] = bu[a] + gap
        elif kind == "sum":
            _, a, b, c, t = case.dep
            A[g(c)] = A[g(a)] + A[g(b)]; W[c] = W[a] + W[b]
            bu[a] = bu[b] = t; bu[c] = 1.5 * t; bl[c] = -50.0 * case.scale
        elif kind == "tie":
            _, a, b = case.dep
            A[g(b)] = A[g(a)]; W[b] = W[a]; bu[b] = bu[a]; bl[b] = bl[a]
        else:
            raise ValueError(kind)
    return H, np.zeros(n), f_theta, A, bu, bl, W, sense


def theta(case, N, batch=0):
    """Parameter batch of a case: point i is uniform in the cube of half-width amps[i % 4].  A batch of up to N_COND
    points is a prefix of the condition batch; a larger one repeats it (tiled), so its reference is the same rows."""
    rng = np.random.default_rng(31 + 7919 * case.seed + 1000 * case.n + 10 * case.mg + case.nth + 1_000_003 * batch)
    amp = np.asarray(case.amps, float)[np.arange(N_COND) % len(case.amps)]
    base = rng.uniform(-1.0, 1.0, (N_COND, case.nth)) * amp[:, None]
    reps = (int(N) + N_COND - 1) // N_COND
    return np.ascontiguousarray(np.tile(base, (reps, 1))[:N])


def oracle_settings(case):
    s = oldp.default_settings()
    if case.fval_bound:
        s.fval_bound = case.fval_bound
    if case.progress_tol:
        s.progress_tol = case.progress_tol
    if case.iter_limit:
        s.iter_limit = case.iter_limit
    return s


def host_ldp(case, nout=None):
    H, f, f_theta, A, bu, bl, W, sense = problem(case)
    return oldp.qp2ldp(H, f, f_theta, A, bu, bl, W, sense, case.nout if nout is None else nout)


def reference(case, th, L=None):
    """The oracle on a pack (default: the one oracle.ldp.qp2ldp makes of the case): (x, exitflag, iters, active)."""
    return oldp.solve_batch(host_ldp(case) if L is None else L, th, oracle_settings(case))


# ---------------------------------------------------------------------------------------------------------------------
def popcount(active):
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    out = np.zeros(len(a), np.int64)
    for w in range(a.shape[1]):
        v = a[:, w].copy()
        while v.any():
            out += (v & np.uint64(1)).astype(np.int64)
            v >>= np.uint64(1)
    return out


def side_bits(active, m):
    """(upper, lower): N x m boolean arrays from the packed active sets."""
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    bit = lambda p: ((a[:, p >> 6] >> np.uint64(p & 63)) & np.uint64(1)).astype(bool)
    up = np.stack([bit(j) for j in range(m)], axis=1)
    lo = np.stack([bit(m + j) for j in range(m)], axis=1)
    return up, lo


def removing(iters, active):
    """Points on whose path a row left the working set again: more iterations than rows added."""
    return np.asarray(iters) > popcount(active) + 1


def must_finish(n, exitflag, iters, active):
    """The rule: the points the tiers pass has to finish itself (True) -- all others it has to queue."""
    ef, it = np.asarray(exitflag), np.asarray(iters)
    nact = popcount(active)
    return (it == nact + 1) & np.isin(ef, (1, 2, -1)) & (nact <= n + 1)


def expected_list(n, exitflag, iters, active):
    """What the pass leaves on the work list for a batch with these oracle outputs: per segment the sorted points, tile
    t in segment t % 64."""
    queued = np.flatnonzero(~must_finish(n, exitflag, iters, active))
    seg = (queued // 64) % K_SHARDS
    return [queued[seg == s] for s in range(K_SHARDS)]


def check_list(counts, lst, want, what=""):
    """The snapshot (counts[64], list[64][seg_cap]) against expected_list(): the same SET per segment -- a point queued
    where the rule says finished or the other way round is named --, and every tile's entries one contiguous ascending
    run (a wavefront appends its tile with one atomic: the order of the tiles in a segment is free, the order inside a
    tile is not)."""
    for s in range(K_SHARDS):
        got = np.asarray(lst[s][:counts[s]], np.int64)
        w = np.asarray(want[s], np.int64)
        if not np.array_equal(np.sort(got), w):
            extra, missing = np.setdiff1d(got, w), np.setdiff1d(w, got)
            raise AssertionError((what, f"segment {s}", f"{len(got)} entries, {len(w)} expected",
                                  "queued but the rule says finished", extra[:8].tolist(),
                                  "finished but the rule says queued", missing[:8].tolist()))
        if len(got):
            tile = got // 64
            start = np.flatnonzero(np.r_[True, tile[1:] != tile[:-1]])
            assert len(np.unique(tile[start])) == len(start), (what, f"segment {s}", "a tile's entries in two runs")
            inside = np.ones(len(got), bool); inside[start] = False
            assert (np.diff(got)[inside[1:]] > 0).all(), (what, f"segment {s}", "a tile's entries out of order")


def stats(case, exitflag, iters, active):
    ef, it = np.asarray(exitflag), np.asarray(iters)
    nact = popcount(active)
    up, lo = side_bits(active, case.m)
    app = it == nact + 1
    m = case.m
    lo_pos = [m + j for j in range(m)]
    return dict(N=len(it), settled=int((it == 1).sum()),
                opt_sizes=sorted(set(nact[app & (ef >= 1) & (it > 1)].tolist())),
                inf_sizes=sorted(set(nact[app & (ef == -1)].tolist())),
                removing=int((~app & (it > nact + 1)).sum()), upper=int(up.any(axis=1).sum()), lower=int(lo.any(axis=1).sum()),
                lower_word0=int(lo[:, [j for j in range(m) if lo_pos[j] < 64]].any(axis=1).sum()),
                lower_word1=int(lo[:, [j for j in range(m) if lo_pos[j] >= 64]].any(axis=1).sum()),
                first_row=int((up[:, 0] | lo[:, 0]).sum()), last_row=int((up[:, -1] | lo[:, -1]).sum()),
                flag2=int((ef == 2).sum()), flagm2=int((ef == -2).sum()), longer=int((nact > case.n + 1).sum()),
                finished=int(must_finish(case.n, ef, it, active).sum()))


def path_sets(case, th, kmax):
    """The working set of every point after 1, 2, ... kmax iterations: the oracle stopped by its iteration limit
    (exit flag -4 where the point wanted more).  What a final active set cannot show -- that a row entered and left
    again -- shows here.  Returns a list of (exitflag, active), entry k - 1 for limit k."""
    out = []
    L = host_ldp(case)
    for k in range(1, kmax + 1):
        s = oracle_settings(case)
        s.iter_limit = k
        x, ef, it, act = oldp.solve_batch(L, th, s)
        out.append((ef, act))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The table.  Seeds, SOFT rows and the gaps of the dependent rows were chosen on the CPU so that the oracle alone meets
# the conditions below (tests/test_tiers_cases_host.py asserts that they do).
SOFT_ROWS = (0, 63, 5, 17, 30, 41, 9, 22, 50, 58)            # rows 0 and m - 1 = 63: bits 0 and 63 of soft_mask
_SOFT_SEED = {4: 1, 9: 1, 12: 3}

HARD = tuple(TiersCase(f"hard-n{n}", n, 64 - n) for n in NS)                                 # m = 64, ms = n
SOFT = tuple(TiersCase(f"soft-n{n}", n, 64, ms=0, soft=SOFT_ROWS, seed=_SOFT_SEED.get(n, 0)) for n in NS)


def lds_line(n):
    """The largest m whose LDS stays within 48 KiB (beyond it the launcher has to raise the kernel's limit)."""
    m = 1
    while lds_bytes(n, m + 1) <= 48 * 1024:
        m += 1
    return m


EDGE_M = (1, 2, 31, 32, 33, 63, 64)
_NTHS = (1, 16, 5, 9, 2, 12, 3, 16, 1, 7, 4)


def _edge_cases():
    out = []
    for n in WIDTH_N:
        line = lds_line(n)
        ms_ = EDGE_M + (line - 1, line, line + 1, line + 2)          # one even and one odd m on each side of the line
        for k, m in enumerate(ms_):
            nth = _NTHS[k]
            nout = 1 if k % 2 == 0 else n
            out.append(TiersCase(f"edge-n{n}-m{m}-nth{nth}-nout{nout}", n, m, ms=0, nth=nth, nout=nout,
                                 seed=_EDGE_SEED.get((n, m), 0)))
    return tuple(out)


_EDGE_SEED = {(2, 1): 1, (2, 33): 4, (2, 22): 13, (2, 24): 1, (3, 22): 1}
EDGE = _edge_cases()

# dependent rows (general rows of an ms = n problem with 20 general rows)
DUP = tuple(TiersCase(f"dup-n{n}", n, 20, dep=("dup", n + 3, n + 9, 0.05)) for n in WIDTH_N)
SUM = TiersCase("sum-n7", 7, 20, dep=("sum", 8, 10, 12, 0.05))
TIE = tuple(TiersCase(f"tie-n{n}", n, 20, dep=("tie", n + 2, n + 7)) for n in (3, 11))
# settings that act
FVAL = TiersCase("fval-n7", 7, 57, fval_bound=3.0)
STALL = TiersCase("stall-n12", 12, 52, progress_tol=1e9)       # (11 stalled iterations: cycle_tol = 10)

CASES = HARD + SOFT + EDGE + DUP + (SUM,) + TIE + (FVAL, STALL)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Refusals: (case, what, the kernel name shows it).  The name tells what the HANDLE can do (lmpc_kernel_name knows
# nothing of a call's arguments or of the settings' iteration limit); the front-pass record tells what a call did.
REFUSED_SETUP = (
    (TiersCase("ref-nth17", 7, 57, nth=17), "nth = 17"),
    (TiersCase("ref-m65", 7, 58), "m = 65"),
    (TiersCase("ref-n13", 13, 40), "n = 13"),
    (TiersCase("ref-immutable", 7, 57, flags=((20, SENSE_IMMUTABLE),)), "an IMMUTABLE row"),
    (TiersCase("ref-equality", 7, 57, flags=((20, SENSE_EQUALITY),)), "an equality row"),
    (TiersCase("ref-binary", 7, 57, flags=((20, SENSE_BINARY),)), "a binary row"),
)
LIMIT_CASE = TiersCase("limit-n7", 7, 57)                   # iter_limit = n + 2 refuses, n + 3 takes the pass
WARM_CASE = HARD[5]
SCREEN0_CASE = HARD[5]

# Cells no family of the table reaches, with the reason; at most two per instantiation (none at present).  The cell
# "optimal at size N" the issue expected to stay open for n = 12 is reached by hard-n12's seed.
UNREACHED = {}


def instantiations():
    """The template arguments N the table claims for qp_tiers_kernel."""
    return {c.n for c in CASES}


# ---------------------------------------------------------------------------------------------------------------------
def check_hard_conditions(case, exitflag, iters, active):
    """Conditions on the ORACLE's outputs for the N_COND batch of a per-instantiation case (m = 64, hard rows)."""
    st = stats(case, exitflag, iters, active)
    n = case.n
    assert st["N"] >= N_COND, "the conditions apply to the N_COND batch"
    assert st["settled"] >= 1, (case.name, "a settled point", st)
    assert st["upper"] >= 1 and st["lower"] >= 1, (case.name, "an upper and a lower side active", st)
    missing = [k for k in range(1, n) if k not in st["opt_sizes"] and (n, f"optimal at size {k}") not in UNREACHED]
    assert not missing, (case.name, "an append-only optimal finish at every size 1 ... N - 1", missing, st)
    assert n + 1 in st["inf_sizes"], (case.name, "an infeasible finish at size N + 1 (count rule)", st)
    assert st["removing"] >= 1, (case.name, "a point with a removal", st)
    # (m = 64: bit m + j of a lower side is bit j of word 1 -- none can land in word 0; the edge cases at m = 33 and 63
    # have both)
    if case.m == 64:
        assert st["lower_word1"] >= 1, (case.name, "a lower side in word 1", st)
    return st


def check_soft_conditions(case, exitflag, iters, active):
    st = stats(case, exitflag, iters, active)
    n = case.n
    assert st["N"] >= N_COND, "the conditions apply to the N_COND batch"
    assert st["flag2"] >= 1, (case.name, "flag 2", st)
    assert n + 1 in st["opt_sizes"], (case.name, "an optimal finish at size N + 1", st)
    assert st["longer"] >= 1, (case.name, "a path longer than N + 1 rows", st)
    up, lo = side_bits(active, case.m)
    for j in (0, case.m - 1):
        assert j in case.soft and (up[:, j] | lo[:, j]).any(), (case.name, f"SOFT row {j} active", st)
    assert st["settled"] >= 1 and st["removing"] >= 1 and st["upper"] >= 1 and st["lower"] >= 1, (case.name, "settled, removal, both sides", st)
    return st


def check_edge_conditions(case, exitflag, iters, active):
    st = stats(case, exitflag, iters, active)
    m = case.m
    assert st["N"] >= N_COND, "the conditions apply to the N_COND batch"
    assert st["settled"] >= 1 and st["finished"] > st["settled"], (case.name, "settled points and points the tiers finish", st)
    assert st["upper"] >= 1 and st["lower"] >= 1, (case.name, "an upper and a lower side active", st)
    if m > 2:
        assert st["finished"] < st["N"], (case.name, "queued points", st)
    if m <= 32:
        assert st["lower_word0"] >= 1 and st["lower_word1"] == 0, (case.name, "lower sides in word 0 only", st)
    elif m < 64:
        assert st["lower_word0"] >= 1 and st["lower_word1"] >= 1, (case.name, "a lower side in word 0 and one in word 1", st)
    else:
        assert st["lower_word1"] >= 1, (case.name, "a lower side in word 1", st)
    assert st["first_row"] >= 1 and st["last_row"] >= 1, (case.name, "the first and the last row active", st)
    return st


def check_dup_conditions(case, exitflag, iters, active):
    """Every point infeasible; append-only infeasible finishes WITH BOTH ROWS OF THE PAIR in the working set at every
    size 2 ... N (the pivot rule: fewer than n + 1 hard rows) and at N + 1."""
    _, a, b, gap = case.dep
    ef, it = np.asarray(exitflag), np.asarray(iters)
    nact = popcount(active)
    up, lo = side_bits(active, case.m)
    pair = up[:, a] & lo[:, b]
    fin = must_finish(case.n, ef, it, active)
    assert (ef == -1).all(), (case.name, "every point infeasible")
    sizes = sorted(set(nact[pair & fin].tolist()))
    assert set(range(2, case.n + 1)) <= set(sizes), (case.name, "pivot-singular infeasible at every size 2 ... N", sizes)
    assert (~fin).any(), (case.name, "queued points")
    return dict(sizes=sizes, queued=int((~fin).sum()))


def check_sum_conditions(case, th, exitflag, iters, active):
    """Points whose working set held rows a, b and c = a + b at once (singular, and the direction blocked: one of them
    left again), found on the oracle's path; all of them removals, which the pass must queue."""
    _, a, b, c, t = case.dep
    seen = np.zeros(len(th), bool)
    for ef_k, act_k in path_sets(case, th, case.n + 4):
        up, lo = side_bits(act_k, case.m)
        seen |= up[:, a] & up[:, b] & up[:, c]
    rem = removing(iters, active)
    assert seen.sum() >= 1, (case.name, "a point whose working set held all three dependent rows")
    assert rem[seen].all(), (case.name, "the dependent set was left by a removal")
    assert not must_finish(case.n, exitflag, iters, active)[seen].any()
    return dict(blocked=int(seen.sum()))


def check_tie_conditions(case, exitflag, iters, active):
    _, a, b = case.dep
    up, lo = side_bits(active, case.m)
    fin = must_finish(case.n, exitflag, iters, active)
    first = (up[:, a] | lo[:, a]) & fin
    assert first.sum() >= 8 and up[first, a].any() and lo[first, a].any(), (case.name, "the first of the two equal rows chosen, either side")
    assert not (up[:, b] | lo[:, b]).any(), (case.name, "the second of two equal rows never wins")
    return dict(ties=int(first.sum()))


def check_fval_conditions(case, th, exitflag, iters, active):
    """fval_bound acts: points the default settings solve to an optimum end infeasible on it, append-only."""
    ef = np.asarray(exitflag)
    x0, ef0, it0, act0 = oldp.solve_batch(host_ldp(case), th)
    cut = (ef0 == 1) & (ef == -1)
    fin = must_finish(case.n, ef, iters, active)
    assert cut.sum() >= 8 and fin[cut].any(), (case.name, "points ended by fval_bound inside the tiers", int(cut.sum()))
    return dict(cut=int(cut.sum()), cut_finished=int((cut & fin).sum()))


def check_stall_conditions(case, exitflag, iters, active):
    ef = np.asarray(exitflag)
    assert (ef == -2).sum() >= 8, (case.name, "points the stall guard ends (-2)")
    fin = must_finish(case.n, ef, iters, active)
    assert fin.sum() > (np.asarray(iters) == 1).sum(), (case.name, "points the tiers still finish")
    return dict(stalled=int((ef == -2).sum()))


def check_case(case, th, exitflag, iters, active):
    """The conditions that belong to a case, by the group its name puts it in."""
    kind = case.name.split("-")[0]
    if kind in ("sum", "fval"):
        return dict(sum=check_sum_conditions, fval=check_fval_conditions)[kind](case, th, exitflag, iters, active)
    if kind in _CHECKS:
        return _CHECKS[kind](case, exitflag, iters, active)
    raise KeyError(case.name)


_CHECKS = dict(hard=check_hard_conditions, soft=check_soft_conditions, edge=check_edge_conditions, dup=check_dup_conditions,
               tie=check_tie_conditions, stall=check_stall_conditions)


def infeasible_tiers():
    """Per N of WIDTH_N: the working-set sizes with an append-only infeasible finish over the dup case (pivot rule) and
    the hard case (count rule) together -- the host test asserts sizes 2 ... N + 1, that is tiers k = 1 ... N."""
    out = {}
    for n in WIDTH_N:
        sizes = set()
        for c in (BY_NAME[f"dup-n{n}"], BY_NAME[f"hard-n{n}"]):
            x, ef, it, act = reference(c, theta(c, N_COND))
            sizes |= set(stats(c, ef, it, act)["inf_sizes"])
        out[n] = sizes
    return out
