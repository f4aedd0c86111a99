"""Case table of the two-kernel lane path's tests (tests/test_lane_cases_host.py, tests/test_gpu_lane.py): one problem per
instantiation of screen_kernel<NTHMAX, NT, MODE> and lane_kernel<N, MS, MA, SIM, MULTI> the dispatch (`launch` behind
api_launch, lmpc_api.hip) can reach, the parameter batches that go with it, and the conditions a batch has to meet ON
THE ORACLE before a comparison with it counts as a test of the kernels.  Numpy and the oracle only: nothing of the
library is imported here.

Where a point is finished.  The screening pass finishes a point whose unconstrained optimum violates no row
(iters == 1), and queues every other one for the lane kernel; there a boxed problem first runs the straight-line tiers
(N <= 6) or the generic loop at capacity 3 (N >= 4) and continues at full capacity when the working set outgrows it.
Which of these a point meets depends on the Hessian and on how far theta pushes the optimum out of the constraints --
hence a Hessian family and a per-point mix of theta scales per case, chosen on the CPU (the table below).

Two tiles of every condition batch are built: points 192 ... 255 are scaled by 1e-9 (an aligned run of 64 settled
points: the wavefront's ballot is zero and it appends nothing to the work list) and points 320 ... 383 are pushed out to
|theta_t| >= QUEUED_PUSH (an aligned run of 64 queued points).  Every other tile holds the whole scale mix.

Rows in front of the screening pass.  The pass takes the rows four at a time and the last m mod 4 of them in a branch
of its own; `tail` multiplies W of exactly those rows, so that at small theta a point violates one of them and nothing
else.  An IMMUTABLE row (sense 4) gets the same treatment (`imm`): a point that violates only that row is not queued.

n = 2 boxed: the oracle never removes a row there (tests/fast_cases.py), so those cases are held to every condition but
the removing points.  n = 1 (one bound and three general rows, which in one variable are bounds again, every row normalised to
+-1) is exempt from it too: the solver adds the MOST violated row, which is the tightest of its side, so no later row of
that side is violated and a row of the other side makes the point infeasible -- nothing is ever swapped out (0 removing
points among 2309 at every scale mix tried).  A boxed problem with an IMMUTABLE bound cannot hold that row: its full
working set is n - 1 rows.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

import fast_cases as fc
from oracle import ldp as oldp

N_COND = fc.N_COND          # 2309 points: 10 screening workgroups of 256 (the last one 5 points), 37 wavefronts
GUARD = fc.GUARD
SIZES = (1, 63, 64, 65, 255, 256, 257, N_COND)
K_SHARDS = 64               # kShards of lmpc_wave_layout.hpp: work-list segments; screening workgroup b -> b % K_SHARDS
SCREEN_BLOCK = 256          # the screening pass's workgroup
N_BIG = 3 * 16384 + 257     # the one large batch per launch-shape case
LANE_SIZES = (2, 3, 4, 5, 6, 8, 10, 12)     # kLaneSizes of lmpc_internal.hpp
LDS_MAX = 160 * 1024        # kLdsMax
SETTLED_TILE, QUEUED_TILE = 3, 5            # aligned runs of 64 points: 192 ... 255 and 320 ... 383
QUEUED_PUSH = 50.0
SENSE_ACTIVE, SENSE_IMMUTABLE = 1, 4
INF = 1e30                  # a bound the solver treats as absent


@dataclass(frozen=True)
class LaneCase:
    name: str
    n: int
    mg: int                         # general rows behind the n simple bounds (0: boxed)
    nth: int
    seed: int = 0
    family: str = "lowrank"         # boxed: fast_cases.problem's families; "general": R R' + 0.3 n I
    param: float = 0.02
    scales: tuple = (0.05, 0.3, 1.0, 3.0, 10.0)
    use_w: bool = True
    tail: float = 40.0              # factor on W of the screening pass's last, partial group of rows
    imm: int = -1                   # row flagged IMMUTABLE (its W times `imm_w`)
    imm_w: float = 1.0
    eq: int = -1                    # row flagged ACTIVE (an equality row: the batch is not screened)
    onesided: bool = False          # general rows ms + 1 / ms + 2 lose their lower / upper bound
    iter_limit: int = 0
    opts: tuple = ()                # lmpc_set_option pairs that put the case on the lane path
    screened: bool = True
    k: int = 0                      # index into the tables of layouts, output counts and plant sizes

    @property
    def m(self):
        return self.n + self.mg

    @property
    def lane_n(self):
        return next(s for s in LANE_SIZES if s >= self.n)

    @property
    def boxed(self):
        """The dispatch's `boxed`: the instantiation with the row scans unrolled and capacity N."""
        return self.mg == 0 and self.n == self.lane_n

    @property
    def only_bounds(self):
        return self.mg == 0

    @property
    def words(self):
        return (2 * self.m + 63) // 64


def problem(case):
    """(H, f, f_theta, A, bu, bl, W, sense) of a case."""
    n, nth, m = case.n, case.nth, case.m
    if case.family == "general":
        rng = np.random.default_rng(77_000 + 1000 * n + 10 * case.mg + nth + 100_000 * case.seed)
        Rm = rng.normal(size=(n, n))
        H = Rm @ Rm.T + 0.3 * n * np.eye(n)
        A = rng.normal(size=(case.mg, n))
        f_theta = rng.normal(size=(n, nth))
        bu, bl = rng.uniform(0.5, 2.0, m), -rng.uniform(0.5, 2.0, m)
        W = 0.3 * rng.normal(size=(m, nth))
        W[:n] = 0.0
    else:
        H, _, f_theta, bu, bl, W = fc.problem(fc.FastCase(n, max(nth, 1), case.seed, case.family, case.param, use_w=case.use_w))
        f_theta, W = f_theta[:, :nth], W[:, :nth]
        A = np.zeros((0, n))
    # f = H c with a small c: the unconstrained optimum at theta = 0 is -c, inside every bound, and the outputs'
    # offsets x0 = -c[:nout] differ from zero and from each other
    f = H @ np.random.default_rng(424_242 + 1000 * n + 10 * case.mg + nth).uniform(-0.004, 0.004, n)
    sense = np.zeros(m, np.int32)
    for j in tail_rows(m):
        W[j] *= case.tail
    if case.imm >= 0:
        sense[case.imm] = SENSE_IMMUTABLE
        W[case.imm] *= case.imm_w
    if case.eq >= 0:
        sense[case.eq] = SENSE_ACTIVE
    if case.onesided:
        assert case.mg >= 3
        bl[n + 1] = -INF
        bu[n + 2] = INF
    return H, f, f_theta, A, bu, bl, W, sense


def tail_rows(m):
    """Rows of the screening pass's last, partial group of four."""
    return range(m & ~3, m)


def theta(case, N, batch=0, scales=None):
    """Parameter batch number `batch` of a case, N points: point i is a standard normal vector times
    scales[i % len(scales)]; tiles SETTLED_TILE and QUEUED_TILE are built as the module text says.  A smaller batch is
    a prefix of a larger one."""
    rng = np.random.default_rng(11 + 1000 * case.n + 10 * case.nth + 7919 * case.mg + 100_000 * case.seed + 1_000_003 * batch)
    full = max(int(N), N_COND)
    mix = np.asarray(case.scales if scales is None else scales, float)
    sc = mix[np.arange(full) % len(mix)]
    z = rng.normal(size=(full, case.nth))
    th = z * sc[:, None]
    if scales is None:
        s0, q0 = 64 * SETTLED_TILE, 64 * QUEUED_TILE
        th[s0:s0 + 64] = z[s0:s0 + 64] * 1e-9
        th[q0:q0 + 64] = np.where(z[q0:q0 + 64] < 0, -1.0, 1.0) * (1.0 + np.abs(z[q0:q0 + 64])) * QUEUED_PUSH
    return np.ascontiguousarray(th[:N])


def big_theta(case):
    """The large batch: the smallest scale of the case's mix once and its three largest twice -- a seventh of the
    points settled, more than half queued."""
    return theta(case, N_BIG, batch=3, scales=case.scales[:1] + 2 * case.scales[-3:])


def oracle_settings(case):
    s = oldp.default_settings()
    if case.iter_limit:
        s.iter_limit = case.iter_limit
    return s


def host_ldp(case, nout=1):
    H, f, f_theta, A, bu, bl, W, sense = problem(case)
    return oldp.qp2ldp(H, f, f_theta, A, bu, bl, W, sense, nout)


def reference(case, th, warm=None, nout=1):
    """The oracle on the pack oracle.ldp.qp2ldp makes of the case: (x, exitflag, iters, active)."""
    return oldp.solve_batch(host_ldp(case, nout), th, oracle_settings(case), warm=warm)


# ---------------------------------------------------------------------------------------------------------------------
# conditions
popcount = fc.popcount


def side_bits(active, m):
    """(upper, lower): boolean (N, m) arrays from the oracle's active words (bit j: upper side of row j, bit m + j: lower)."""
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    bit = lambda p: ((a[:, p >> 6] >> np.uint64(p & 63)) & np.uint64(1)).astype(bool)
    up = np.stack([bit(j) for j in range(m)], axis=1)
    lo = np.stack([bit(m + j) for j in range(m)], axis=1)
    return up, lo


def _sides_at_zero(L, th):
    """(upper slack, lower slack, rounding allowance) of every row at u = 0, from the pack's Dth, du0 and dl0 with
    numpy alone.  The allowance is 1e-9 of the row's terms (an absent bound, +-1e30 before scaling, adds nothing to it):
    no summation order moves a slack by that much."""
    th = np.asarray(th, float)
    b = th @ L.Dth.T
    fin = lambda v: np.where(np.abs(v) < 1e20, np.abs(v), 0.0)
    tol = 1e-9 * (np.abs(th) @ np.abs(L.Dth.T) + fin(L.du0) + fin(L.dl0))
    return L.du0 + b, -(L.dl0 + b), tol


def violated_at_zero(L, th, primal_tol=1e-6):
    """Boolean (N, m): the rows the screening pass clearly finds violated at u = 0 (by ten times the solver's
    tolerance and the rounding allowance)."""
    su, sl, tol = _sides_at_zero(L, th)
    return (su < -(10 * primal_tol + tol)) | (sl < -(10 * primal_tol + tol))


def clearly_feasible_at_zero(L, th):
    su, sl, tol = _sides_at_zero(L, th)
    return (su > tol) & (sl > tol)


def only_row(L, th, j):
    """Points that clearly violate row j and clearly satisfy every other row at u = 0."""
    v, ok = violated_at_zero(L, th), clearly_feasible_at_zero(L, th)
    others = np.ones(L.m, bool)
    others[j] = False
    return v[:, j] & ok[:, others].all(axis=1)


def full_set(case):
    """Rows of a full working set: n, or n - 1 where one of the n simple bounds is IMMUTABLE and cannot enter it."""
    return case.n - (1 if case.only_bounds and case.imm >= 0 else 0)


def lane_stats(case, L, th, exitflag, iters, active):
    it, ef = np.asarray(iters), np.asarray(exitflag)
    m, n = case.m, case.n
    nact = popcount(active)
    up, lo = side_bits(active, m)
    queued = it != 1
    tiles = [queued[s:s + 64] for s in range(0, len(it) - 63, 64)]
    st = dict(N=len(it), settled=int(((it == 1) & (ef == 1)).sum()),
              append_only=int(((it == nact + 1) & (it > 1) & (ef == 1)).sum()), removing=int((it > nact + 1).sum()),
              upper=int(up.any(axis=1).sum()), lower=int(lo.any(axis=1).sum()),
              settled_tiles=[t for t, q in enumerate(tiles) if not q.any()],
              queued_tiles=[t for t, q in enumerate(tiles) if q.all()],
              rows4=int((nact >= 4).sum()), rows_n=int((nact >= full_set(case)).sum()), infeasible=int((ef == -1).sum()),
              general_upper=int(up[:, n:].any(axis=1).sum()), general_lower=int(lo[:, n:].any(axis=1).sum()),
              failed=int((ef < 1).sum()))
    if m % 4:
        st["tail_only"] = {j: int(only_row(L, th, j).sum()) for j in tail_rows(m)}
    if case.imm >= 0:
        st["imm_only_settled"] = int((only_row(L, th, case.imm) & (it == 1) & (ef == 1)).sum())
    return st


def check_lane_conditions(case, L, th, exitflag, iters, active):
    """Conditions on the ORACLE's outputs (and, for the rows in front of the screening pass, on the pack) for the
    condition batch of `case`: raises AssertionError naming every one that fails, returns the counts."""
    st = lane_stats(case, L, th, exitflag, iters, active)
    missed = []
    need = lambda ok, what: None if ok else missed.append(what)
    assert st["N"] == N_COND, "the conditions apply to the batch of N_COND points"
    need(st["settled"] >= 64, "settled by the screen")
    need(st["append_only"] >= 64, "append-only")
    if not ((case.only_bounds and case.n == 2) or case.n == 1):
        need(st["removing"] >= 8, "rows removed again")
    need(st["upper"] >= 8 and st["lower"] >= 8, "both bound sides active")
    need(st["settled_tiles"] == [SETTLED_TILE], "one aligned run of 64 settled points, every other tile mixed")
    need(st["queued_tiles"] == [QUEUED_TILE], "one aligned run of 64 queued points, every other tile mixed")
    if case.only_bounds and case.n >= 4:
        # the first tier at capacity 3 is outgrown; a full working set of n rows (n = 6: past LMPC_FAST_KMAX = 5)
        need(st["rows4"] >= 8, "final sets of four rows or more")
        need(st["rows_n"] >= 8, "full working sets of n rows")
    if not case.only_bounds:
        need(st["infeasible"] >= 8, "infeasible points")
        need(st["general_upper"] >= 8 and st["general_lower"] >= 8, "a general row active on either side")
        need(st["rows_n"] >= 8, "points with n active rows")
    if case.m % 4:
        need(min(st["tail_only"].values()) >= 4, "points that violate one row of the partial group alone")
    if case.imm >= 0:
        need(st["imm_only_settled"] >= 8, "points that violate the IMMUTABLE row alone, settled")
    assert not missed, (case.name, missed, st)
    return st


def check_big_batch(case, iters):
    """The large batch: more than half of it queued, and every work-list segment longer than the largest lane
    workgroup, so that a grid of one workgroup per segment ("lane_per" 1) makes several trips of its stride loop."""
    it = np.asarray(iters)
    assert len(it) == N_BIG
    queued = it != 1
    shard = (np.arange(N_BIG) // SCREEN_BLOCK) % K_SHARDS
    per = np.bincount(shard, weights=queued, minlength=K_SHARDS)
    assert queued.sum() > N_BIG // 2, (case.name, "more than half queued", int(queued.sum()))
    assert per.min() > 256, (case.name, "every segment longer than a workgroup", per.min())
    return int(queued.sum()), int(per.min())


# ---------------------------------------------------------------------------------------------------------------------
# The table.  Scale mixes, families and the factors on W were chosen on the CPU until the oracle alone met the
# conditions above (tests/test_lane_cases_host.py re-checks every one).
_S = (0.003, 0.05, 0.3, 1.0, 3.0, 10.0)
_SG = (0.02, 0.1, 0.4, 1.5, 6.0, 40.0)


def _b(name, n, nth, **kw):
    kw.setdefault("family", "lowrank")
    kw.setdefault("param", 0.02)
    kw.setdefault("scales", _S)
    return LaneCase(name, n, 0, nth, **kw)


def _g(name, n, mg, nth, **kw):
    kw.setdefault("scales", _SG)
    opts = tuple(kw.pop("opts", ()))
    if (n + mg) * n >= 600:
        opts += (("wave", 0),)                       # (finalize_handle: general rows from m n = 600 on default to the wavefront kernel)
    return LaneCase(name, n, mg, nth, family="general", param=0.0, opts=opts, **kw)


_TABLE = (
    # ---- boxed, one per lane size, kept off the one-launch kernel by nth (fast_covers: nth <= 16, n = 5: nth <= 8)
    _b("box2-nth17", 2, 17, family="equi", param=0.6, scales=(0.01, 0.05, 0.3, 1.0, 3.0)),
    _b("box3-nth31", 3, 31, family="equi", param=0.6, scales=(0.005, 0.03, 0.1, 0.3, 1.0, 3.0)),
    _b("box4-nth32", 4, 32, scales=(0.005, 0.03, 0.1, 0.3, 1.0, 3.0)),
    _b("box5-nth13", 5, 13),
    _b("box6-nth14", 6, 14),
    _b("box8-nth15", 8, 15),
    _b("box10-nth16", 10, 16),
    _b("box12-nth9", 12, 9),
    # ---- their twins at "fast" 0
    _b("box2-nth3-fast0", 2, 3, family="equi", param=0.6, opts=(("fast", 0),)),
    _b("box3-nth2-fast0", 3, 2, opts=(("fast", 0),), tail=15.0),
    _b("box4-nth1-fast0", 4, 1, param=0.002, opts=(("fast", 0),)),
    _b("box5-nth4-fast0", 5, 4, opts=(("fast", 0),)),
    # ---- boxed problems fast_covers() turns away: an IMMUTABLE row, a tight iteration limit
    _b("box6-nth6-imm", 6, 6, imm=2, imm_w=40.0),
    _b("box3-nth5-limit6", 3, 5, family="equi", param=0.6, iter_limit=6),
    # ---- boxed problems at padded sizes: the general instantiation of the next lane size
    _b("box7-nth7-pad", 7, 7),
    _b("box11-nth11-pad", 11, 11),
    # ---- general rows: every lane size, the padded sizes, m = 0 ... 3 (mod 4), m = 31, 32, 33, 63, 64
    _g("gen1-m4-nth3", 1, 3, 3),
    _g("gen2-m5-nth2", 2, 3, 2, onesided=True),
    _g("gen3-m64-nth3", 3, 61, 3, onesided=True),
    _g("gen4-m31-nth4", 4, 27, 4),
    _g("gen5-m14-nth5", 5, 9, 5, onesided=True),
    _g("gen6-m32-nth6", 6, 26, 6),
    _g("gen7-m33-nth8", 7, 26, 8),
    _g("gen8-m63-nth10", 8, 55, 10, onesided=True),
    _g("gen8-m14-nth12-imm", 8, 6, 12, imm=10, imm_w=40.0),
    _g("gen9-m19-nth9", 9, 10, 9, tail=15.0),
    _g("gen10-m64-nth10", 10, 54, 10),
    _g("gen11-m23-nth11", 11, 12, 11),
    _g("gen12-m64-nth12", 12, 52, 12),
    _g("gen6-m10-nth17", 6, 4, 17, scales=(0.01, 0.05, 0.2, 0.8, 3.0, 20.0)),
)
CASES = tuple(replace(c, k=k) for k, c in enumerate(_TABLE))
BY_NAME = {c.name: c for c in CASES}

# not screened: the lane kernel walks the whole batch (will_screen: "screen" 0, an ACTIVE-flagged row, nth outside 1 ... 32)
UNSCREENED = tuple(replace(c, k=k, screened=False) for k, c in enumerate((
    _b("box6-nth33", 6, 33, scales=(0.005, 0.03, 0.1, 0.3, 1.0, 3.0)),
    _b("box5-nth7-screen0", 5, 7, opts=(("screen", 0),)),
    _g("gen5-m14-nth5-eq", 5, 9, 5, eq=7),
    _b("box4-nth0", 4, 0),
)))

# launch shapes, the large batch and the call sequences: one boxed and one general case per lane size
SHAPE_CASES = tuple(BY_NAME[s] for s in (
    "box2-nth17", "box3-nth31", "box4-nth32", "box5-nth13", "box6-nth14", "box8-nth15", "box10-nth16", "box12-nth9",
    "gen1-m4-nth3", "gen3-m64-nth3", "gen4-m31-nth4", "gen5-m14-nth5", "gen6-m32-nth6", "gen8-m63-nth10", "gen10-m64-nth10",
    "gen12-m64-nth12"))

NOUTS = (2, 3, 5, 7)        # several outputs, next to nout = n


def nouts(case):
    return tuple(sorted({v for v in NOUTS + (case.n,) if 2 <= v <= case.n}))


def lane_lds_bytes(case, block):
    """lane_lds_bytes of lmpc_api.hip."""
    m, N = case.m, case.lane_n
    return 8 * (m * N + m * (m + 1) // 2 + 2 * m + m * block)


def lane_blocks(case):
    return tuple(b for b in (64, 128, 256) if lane_lds_bytes(case, b) <= LDS_MAX)


# ---------------------------------------------------------------------------------------------------------------------
# closed loop and generated controller: shapes per case
def sim_shape(case):
    """(nx, nr, nup, nu) of the case's lock-step closed loop: theta = [x; r; uprev]; nu = 1 ... 4 over the table."""
    nu = min(1 + case.k % 4, case.n, 4)
    nup = min((0, nu, 1)[case.k % 3], case.nth - 1)
    nr = min(case.k % 2, case.nth - 1 - nup)
    return case.nth - nr - nup, nr, nup, nu


def sim_data(case, S):
    """(F, G, x0, r, uprev) of the case's closed loop, S scenarios: a stable plant, states from the case's scale mix."""
    nx, nr, nup, nu = sim_shape(case)
    rng = np.random.default_rng(31_000 + case.k)
    F = 0.5 * rng.normal(size=(nx, nx)) / np.sqrt(nx)
    G = 0.01 * rng.normal(size=(nx, nu))          # (small: the outputs' offsets must not carry a settled scenario off)
    th = theta(case, max(S, 1), batch=5)[:S]
    r = np.ascontiguousarray(th[:, nx:nx + nr]) if nr else None
    up = np.ascontiguousarray(th[:, nx + nr:]) if nup else None
    return F, G, np.ascontiguousarray(th[:, :nx]), r, up


def check_loop_steps(case, flags, active):
    """Every step of a closed loop (flags, active: (T, S) and (T, S, words) from the host loop) has scenarios the
    screening pass finishes and scenarios it queues."""
    for k in range(len(flags)):
        nact = popcount(active[k])
        assert ((nact == 0) & (flags[k] == 1)).sum() >= 8 and (nact > 0).sum() >= 8, (case.name, "step", k)


def gather_layout(case):
    """((nx, nr, nd, nuprev, np), control width, NULL blocks): the block layouts fast_cases enumerates."""
    lay, gnout, null = fc._layout(case.k, case.n, case.nth)
    return lay, gnout, null


def gather_case(case):
    lay, gnout, null = gather_layout(case)
    return fc.FastCase(case.n, case.nth, layout=lay, gather_nout=gnout, null=null)


# ---------------------------------------------------------------------------------------------------------------------
# instantiations the table reaches, as `launch` chooses them
def screen_inst(case, mode):
    """(NTHMAX, NT, MODE) of LMPC_SCREEN_SWITCH; MODE 0 plain, 1 closed loop, 2 generated controller, 3 several outputs."""
    nt = case.nth if case.nth <= 16 else 32
    return (8 if nt <= 8 else 16 if nt <= 16 else 32, nt, mode)


def lane_inst(case, sim=False, nout=1):
    """(N, MS, MA, SIM, MULTI) of LMPC_CASE / LMPC_LN."""
    N = case.lane_n
    ms, ma = (N, N) if case.boxed else (0, N + 1)
    return (N, ms, ma, bool(sim), (not sim) and nout > 1 and N <= 6)


def instantiations():
    """(screen_kernel arguments, lane_kernel arguments) the GPU tests run: every case in the plain form, with several
    outputs, in the closed loop and through the generated controller's gather."""
    screen, lane = set(), set()
    for c in CASES:
        modes = [(0, False, 1), (1, True, sim_shape(c)[3]), (2, False, gather_layout(c)[1])]
        modes += [(3, False, k) for k in nouts(c)]
        for mode, sim, nout in modes:
            screen.add(screen_inst(c, mode))
            lane.add(lane_inst(c, sim, nout))
    for c in UNSCREENED:                                     # (plain form only, and no screening pass)
        lane.add(lane_inst(c))
    return screen, lane


# Instantiations the library holds and `launch` cannot reach: (kernel, template arguments) -> the line of `launch`
# that excludes it.  Empty: the switch of LMPC_SCREEN_SWITCH and LMPC_CASE x LMPC_LN instantiate exactly what they call.
UNREACHED = {}
