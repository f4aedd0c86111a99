"""Case table of the wavefront path's tests (tests/test_wave_cases_host.py, tests/test_gpu_wave.py): the problems, the
launch choices and the parameter batches that reach every instantiation of
    wave_kernel<R, MR, LDSC, BNB, PACKED, NU, GRAM = false, SIM>            (lmpc_wave_kernel.hpp)
the dispatch of launch_wave_inst (lmpc_wave_launch.hpp) can reach, big_kernel<R> behind it, and the conditions a batch
has to meet ON THE ORACLE before a comparison with it counts as a test of the kernels.  Numpy and the oracle only:
nothing of the library is imported here.

Which instantiation a launch runs.  MR follows from m (`wave_slots`), NU from n (two variable slots beyond 64), the real
type and BNB from the call and the problem; LDSC and PACKED are launch choices ("wave_level", "wave_packed") that the
launcher honours only where the shared copy fits the 160 KiB of LDS next to the per-wave factors -- otherwise it falls
back silently.  `fits` below restates that arithmetic so that the table only asks for what can run; what DID run is
read from the handle's launch record (lmpc_wave_launch_info) by every GPU test, and that record decides.  SIM: plain
binary64 solves run the translation unit built without the closed-loop machinery (SIM = false); the closed loop, every
binary32 call and every search run SIM = true.

Problems.  One random family: H = R R' + n I, n simple bounds in front of mg general rows A x, bounds drawn from
+-[0.5, 2] * `bs`, the general rows' bounds moved by W theta (W = `ws` * normal); flags as the case names them.  Every
batch mixes parameter scales point by point (`scales`), so that one batch holds points that settle at iteration 1,
append-only points, points that drop rows again and infeasible points.  Where m = 1 (mod 64) the LAST row -- alone in
its constraint slot -- gets bounds a quarter as wide, so that it is active at many points.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from oracle import ldp as oldp

LDS_MAX = 160 * 1024        # kLdsMax
WAVE_MAX_CAP = 64           # kWaveMaxCap
RUN_AHEAD_SLOTS = 6         # kWaveRunAheadSlots
K_SHARDS = 64               # kShards: work-list segments; screening workgroup b -> segment b % K_SHARDS
SCREEN_BLOCK = 256
GUARD = 8                   # sentinel rows behind every device output
N_COND = 400                # points of a condition batch
SENSE_IMMUTABLE, SENSE_SOFT, SENSE_BINARY = 4, 8, 16
INF = 1e30
MR_PLAIN = (1, 2, 3, 4, 5, 6, 8, 16)
MR_BNB = (1, 2, 4, 8, 16)
MR_FOUR_LEVELS = (1, 2, 4)  # LMPC_WV: levels 0 .. 3 square; everything else (LMPC_WVB) and packed: 0 and 1


@dataclass(frozen=True)
class WaveCase:
    name: str
    n: int
    mg: int
    nth: int
    nsoft: int = 0
    nbin: int = 0                   # leading simple bounds flagged BINARY
    seed: int = 0
    f32: bool = False
    bs: float = 2.0                 # factor on the bounds
    ws: float = 0.1                 # scale of W
    sb: float = 1.0                 # further factor on the n simple bounds
    fc: float = 0.004               # f = H c with c uniform in +-fc: the unconstrained optimum at theta = 0 is -c
    last: float = 0.25              # m = 1 (mod 64): factor on the bounds of the last row
    even: bool = True               # bounds from +-[0.9, 1.1] instead of +-[0.5, 2]: many rows on the feasible set's boundary
    scales: tuple = (0.02, 0.3, 1.0, 2.0, 4.0)
    onesided: bool = False          # general rows 1 / 2 lose their lower / upper bound
    imm: bool = False               # general row 3 is IMMUTABLE
    dup: bool = False               # the last but one general row repeats general row 0, the one before it opposes row 4
    iter_limit: int = 0
    sim: bool = True                # also run in the closed loop
    deep: bool = False              # held to the conditions on large working sets
    exempt: tuple = ()              # conditions the case is not held to (reasons: next to the table)

    @property
    def m(self):
        return self.n + self.mg

    @property
    def bnb(self):
        return self.nbin > 0

    @property
    def MR(self):
        return wave_slots(self.m, self.bnb)

    @property
    def NU(self):
        return 2 if self.n > 64 else 1

    @property
    def cap(self):
        """W.cap of finalize_handle."""
        return min(self.n + 1 + self.nsoft + (1 if self.bnb else 0), WAVE_MAX_CAP)

    @property
    def words(self):
        return (2 * self.m + 63) // 64

    @property
    def rs(self):
        return 4 if self.f32 else 8

    @property
    def dtype(self):
        return np.float32 if self.f32 else np.float64


def wave_slots(m, bnb):
    """wave_slots of lmpc_wave_launch.hpp."""
    need = (m + 63) // 64
    if need <= 2:
        return max(need, 1)
    if need == 3:
        return 4 if bnb else 3
    if need == 4:
        return 4
    if need <= 6:
        return 8 if bnb else need
    return 8 if need <= 8 else 16


def max_nwv(MR, bnb):
    """wave_launch_bound / 64 (lmpc_wave_kernel.hpp): wavefronts per workgroup the instantiation is built for."""
    return 4 if MR >= 7 else 8 if (MR >= 5 or bnb) else 8 if MR == 4 else 12 if MR == 3 else 16


def shared_bytes(case, level):
    """wave_shared_bytes: 1: M transposed, 2: + M, 3: + packed Gram."""
    nM, nG = case.m * case.n, case.m * (case.m + 1) // 2
    return case.rs * (2 * nM + nG if level >= 3 else 2 * nM if level == 2 else nM if level == 1 else 0)


def lds_bytes(case, level, packed, nwv, cap=None):
    cap = case.cap if cap is None else cap
    per = case.rs * ((cap * (cap - 1) // 2 if packed else cap * (cap | 1)) + 64)
    return per * nwv + shared_bytes(case, level)


def levels_built(case, packed):
    """Staging levels the dispatch macros instantiate at this case's slot counts."""
    if case.NU == 2:
        return (0,)
    if packed or case.MR not in MR_FOUR_LEVELS:
        return (0, 1)
    return (0, 1, 2, 3)


def fits(case, level, packed, nwv, cap=None):
    return nwv <= max_nwv(case.MR, case.bnb) and lds_bytes(case, level, packed, nwv, cap) <= LDS_MAX


def launches(case):
    """(level, packed, nwv) of every launch choice the case is run at: each level the dispatch builds at its slot
    counts, square and packed, wherever the shared copy fits; nwv rotates through 1, 2 and 4 (all of them allowed at
    every slot count), dropping to 1 where the larger workgroup does not fit."""
    out = []
    for packed in (False, True):
        for level in levels_built(case, packed):
            nwv = (2, 4, 1, 2)[level] if not packed else (4, 1)[level]
            if not fits(case, level, packed, nwv):
                nwv = 1
            if fits(case, level, packed, nwv):
                out.append((level, packed, nwv))
    return tuple(out)


def inst(case, level, packed, sim=False):
    """(sizeof(R), MR, LDSC, BNB, PACKED, NU, SIM) of the wave_kernel instantiation a launch runs."""
    return (case.rs, case.MR, level, case.bnb, bool(packed), case.NU, bool(sim or case.f32 or case.bnb))


def problem(case):
    """(H, f, f_theta, A, bu, bl, W, sense) of a case."""
    n, mg, nth, m = case.n, case.mg, case.nth, case.m
    rng = np.random.default_rng(91_000 + 1000 * n + 7 * mg + nth + 100_000 * case.seed)
    Rm = rng.standard_normal((n, n))
    H = Rm @ Rm.T + n * np.eye(n)
    A = rng.standard_normal((mg, n))
    lo, hi = (0.9, 1.1) if case.even else (0.5, 2.0)
    bu, bl = case.bs * rng.uniform(lo, hi, m), -case.bs * rng.uniform(lo, hi, m)
    bu[:n] *= case.sb
    bl[:n] *= case.sb
    W = case.ws * rng.standard_normal((m, nth))
    W[:n] = 0.0
    f_theta = rng.standard_normal((n, nth))
    f = H @ rng.uniform(-case.fc, case.fc, n)
    sense = np.zeros(m, np.int32)
    if case.nsoft:
        soft = n + rng.choice(mg, case.nsoft, replace=False)
        sense[soft] = SENSE_SOFT
        bu[soft] *= 0.4                                    # (tighter than the hard rows: they give way at many points)
        bl[soft] *= 0.4
    if case.dup:
        assert mg >= 8
        A[mg - 2] = A[0]
        A[mg - 3] = -A[4]
        W[n + mg - 3] = -W[n + 4]
    if case.onesided:
        bl[n + 1] = -INF
        bu[n + 2] = INF
    if case.imm:
        sense[n + 3] = SENSE_IMMUTABLE
    if case.nbin:
        sense[:case.nbin] |= SENSE_BINARY
        bu[:case.nbin], bl[:case.nbin] = 1.0, 0.0
    if m % 64 == 1 and mg:
        bu[m - 1] *= case.last
        bl[m - 1] *= case.last
        sense[m - 1] = 0
    return H, f, f_theta, A, bu, bl, W, sense


def theta(case, N=N_COND, batch=0, scales=None):
    """Parameter batch number `batch`: point i is a standard normal vector times scales[i % len(scales)].  A smaller
    batch is a prefix of a larger one.  (Binary32 cases: rounded to binary32.)"""
    rng = np.random.default_rng(17 + 1000 * case.n + 10 * case.nth + 7919 * case.mg + 100_000 * case.seed + 1_000_003 * batch)
    full = max(int(N), N_COND)
    mix = np.asarray(case.scales if scales is None else scales, float)
    th = rng.standard_normal((full, case.nth)) * mix[np.arange(full) % len(mix)][:, None]
    return np.ascontiguousarray(th[:N].astype(case.dtype))


def oracle_settings(case):
    s = oldp.default_settings_f32() if case.f32 else oldp.default_settings()
    if case.iter_limit:
        s.iter_limit = case.iter_limit
    return s


def host_ldp(case, nout=1):
    return oldp.qp2ldp(*problem(case), nout)


def reference(case, th, warm=None, nout=1, ldp=None):
    """The oracle (binary32 cases: its binary32 build) on `ldp`, or on the pack oracle.ldp.qp2ldp makes of the case."""
    L = host_ldp(case, nout) if ldp is None else ldp
    return oldp.solve_batch(L, th, oracle_settings(case), warm=warm, dtype=case.dtype)


def warm_masks(ef, active):
    """Warm starts that are not the points' own final sets: point i starts from the final set of point i + 1 where that
    one was solved, from nothing otherwise."""
    w = np.roll(np.array(active, copy=True), -1, axis=0)
    w[np.roll(np.asarray(ef), -1) < 1] = 0
    return w


# ---------------------------------------------------------------------------------------------------------------------
# conditions
def popcount(active):
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    return np.unpackbits(a.view(np.uint8), axis=1).sum(axis=1).astype(np.int64)


def side_bits(active, m):
    """(upper, lower): boolean (N, m) arrays (bit j: upper side of row j, bit m + j: lower side)."""
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    bits = np.unpackbits(a.view(np.uint8), axis=1, bitorder="little").astype(bool)
    return bits[:, :m], bits[:, m:2 * m]


FLOOR = 8


def wave_stats(case, ef, it, active):
    ef, it = np.asarray(ef), np.asarray(it)
    nact = popcount(active)
    up, lo = side_bits(active, case.m)
    slots = (case.m + 63) // 64
    st = dict(N=len(it), settled=int(((it == 1) & (ef == 1)).sum()),
              append_only=int(((it == nact + 1) & (it > 1) & (ef >= 1)).sum()), removing=int(((it > nact + 1) & (ef >= 1)).sum()),
              infeasible=int((ef == -1).sum()), soft_optimal=int((ef == 2).sum()), limit=int((ef == -4).sum()),
              slot_upper=[int(up[:, 64 * r:64 * r + 64].any(axis=1).sum()) for r in range(slots)],
              slot_lower=[int(lo[:, 64 * r:64 * r + 64].any(axis=1).sum()) for r in range(slots)],
              last_row=int((up[:, -1] | lo[:, -1]).sum()), beyond32=int((nact > 32).sum()),
              cap_less_one=int((nact == case.cap - 1).sum()), at_cap=int((nact >= case.cap).sum()),
              beyond64=int((nact > 64).sum()), max_rows=int(nact.max()))
    return st


def check_wave_conditions(case, ef, it, active):
    """Conditions on the ORACLE's outputs for the cold condition batch of `case`; raises AssertionError naming every one
    that fails, returns the counts.  `case.exempt` names the ones a case is not held to."""
    st = wave_stats(case, ef, it, active)
    missed = []

    def need(ok, what):
        if not ok and what not in case.exempt:
            missed.append(what)
    assert st["N"] == N_COND, "the conditions apply to the batch of N_COND points"
    if case.bnb:                                           # (a search: see check_search_conditions)
        assert not missed
        return st
    need(st["settled"] >= FLOOR, "settled at iteration 1")
    need(st["append_only"] >= FLOOR, "append-only")
    need(st["removing"] >= FLOOR, "rows removed again")
    need(st["infeasible"] >= FLOOR, "infeasible points")
    if case.nsoft:
        need(st["soft_optimal"] >= FLOOR, "exit flag 2")
    need(min(st["slot_upper"]) >= FLOOR, "an upper side active in every constraint slot")
    need(min(st["slot_lower"]) >= FLOOR, "a lower side active in every constraint slot")
    if case.m % 64 == 1:
        need(st["last_row"] >= FLOOR, "the last row, alone in its slot, active")
    if case.iter_limit:
        need(st["limit"] >= FLOOR, "iteration limit reached")
    if case.deep:
        need(st["beyond32"] >= FLOOR, "working sets beyond 32 rows")
        need(st["cap_less_one"] >= FLOOR, "working sets of capacity - 1 rows")
        need(st["at_cap"] >= FLOOR, "working sets that fill the capacity")
    assert not missed, (case.name, missed, st)
    return st


def check_warm_conditions(case, warm, ef, active):
    """Warm batch: points whose warm set is neither empty nor their final set."""
    w = np.ascontiguousarray(warm).view(np.uint64).reshape(len(warm), -1)
    a = np.ascontiguousarray(active).view(np.uint64).reshape(len(active), -1)
    differs = int(((w != a).any(axis=1) & (w != 0).any(axis=1)).sum())
    assert differs >= FLOOR, (case.name, "warm sets that are not the final sets", differs)
    return differs


def check_two_pass_share(case, active, cap1, kind):
    """Two passes at a first-pass capacity of cap1 rows: `kind` = "none" (no point's final set outgrows it), "all"
    (every point's does) or "mixed" (at least FLOOR on either side).  A final set of more than cap1 rows certainly
    outgrew the first pass; one of at most cap1 - 2 rows is taken as having stayed inside (a working set can pass
    through a larger size on its way -- the launch record and the equality of results do not depend on this count)."""
    nact = popcount(active)
    over, inside = int((nact > cap1).sum()), int((nact <= cap1 - 2).sum())
    ok = {"none": over == 0 and inside >= FLOOR, "all": over == len(nact), "mixed": over >= FLOOR and inside >= FLOOR}[kind]
    assert ok, (case.name, "two-pass share", kind, cap1, over, inside)
    return over, inside


def check_search_conditions(case, it, it_relaxed, ef):
    """Searches (the oracle reports no node counts): points whose summed iterations are well above one solve's -- more
    than twice the relaxation's plus two, i.e. at least three nodes' worth --, solved searches and pruned-to-infeasible
    ones."""
    it, itr, ef = np.asarray(it), np.asarray(it_relaxed), np.asarray(ef)
    deep = int((it > 2 * itr + 2).sum())
    assert deep >= FLOOR, (case.name, "searches of several nodes", deep)
    assert (ef >= 1).sum() >= FLOOR, (case.name, "solved searches", int((ef >= 1).sum()))
    return deep


def check_segments(it, kind):
    """Work-list mode behind the screening pass: the queued points (iters != 1) per segment.  "some-empty": at least
    one segment stays empty and at least one is filled; "all-filled": every one of the 64 holds FLOOR points."""
    it = np.asarray(it)
    shard = (np.arange(len(it)) // SCREEN_BLOCK) % K_SHARDS
    per = np.bincount(shard, weights=(it != 1), minlength=K_SHARDS)
    ok = (per.min() == 0 and per.max() >= FLOOR) if kind == "some-empty" else per.min() >= FLOOR
    assert ok, ("work-list segments", kind, int(per.min()), int(per.max()))
    return int(per.min()), int(per.max())


def check_loop_steps(case, flags, active):
    """Closed loop: every step has scenarios with an empty and scenarios with a non-empty final working set."""
    for k in range(len(flags)):
        nact = popcount(active[k])
        assert (nact == 0).sum() >= FLOOR and (nact > 0).sum() >= FLOOR, (case.name, "step", k)


# ---------------------------------------------------------------------------------------------------------------------
# The table.  Sizes, bound factors and scale mixes were chosen on the CPU until the oracle alone met the conditions
# (tests/test_wave_cases_host.py re-checks every one).
def _c(name, n, mg, nth, **kw):
    return WaveCase(name, n, mg, nth, **kw)


_MANY = dict(bs=2.0, ws=0.1)
# Exemptions.  A problem with n = 1 never removes a row (the solver adds the most violated row, which is the tightest
# of its side); a box with ONE general row (n = 63, m = 64) is feasible wherever that row meets the box and hardly ever
# swaps a row (3 points of 400); an infeasible exit of the n = 10 problem takes n + 2 = 12 iterations, which the limit
# case's limit of 12 ends first; the all-SOFT slow-path problem is never infeasible (soft rows always give way).
_TABLE = (
    # ---- one constraint slot: m small; n = 1, nth = 1 (nth = 0: NTH0 below)
    _c("mr1-n1-m6-nth1", 1, 5, 1, ws=1.0, exempt=("rows removed again",), sim=False),
    _c("mr1-n4-m40-nth7", 4, 36, 7, onesided=True, imm=True, dup=True),
    _c("mr1-n12-m64-nth8", 12, 52, 8, nsoft=6),
    _c("mr1-n63-m64-nth9", 63, 1, 9, sim=False, exempt=("infeasible points", "rows removed again"), sb=0.03, scales=(0.02, 0.3, 1.0, 3.0, 8.0)),
    # ---- two slots: m = 65 (the last row alone in slot 1), inside, 128
    _c("mr2-n3-m65-nth2", 3, 62, 2, last=0.1),
    _c("mr2-n8-m100-nth16", 8, 92, 16, nsoft=10, onesided=True, dup=True, sim=False),
    _c("mr2-n64-m128-nth17", 64, 64, 17, sim=False, sb=0.03, scales=(0.02, 0.3, 1.0, 3.0, 8.0)),
    # ---- three
    _c("mr3-n3-m129-nth3", 3, 126, 3),
    _c("mr3-n6-m160-nth4", 6, 154, 4, imm=True),
    _c("mr3-n10-m192-nth5", 10, 182, 5, nsoft=12),
    # ---- four: level 3 (packed Gram staged) fits the LDS at m = 193 only, with n <= 4
    _c("mr4-n3-m193-nth2", 3, 190, 2, last=0.1),
    _c("mr4-n7-m230-nth6", 7, 223, 6, dup=True),
    _c("mr4-n5-m256-nth4", 5, 251, 4, nsoft=8),
    # ---- five, six
    _c("mr5-n4-m257-nth3", 4, 253, 3),
    _c("mr5-n6-m300-nth5", 6, 294, 5),
    _c("mr5-n8-m320-nth4", 8, 312, 4, nsoft=10),
    _c("mr6-n4-m321-nth3", 4, 317, 3),
    _c("mr6-n6-m350-nth5", 6, 344, 5),
    _c("mr6-n8-m384-nth4", 8, 376, 4, nsoft=10),
    # ---- eight, sixteen (no run-ahead in the closed loop)
    _c("mr8-n4-m385-nth3", 4, 381, 3),
    _c("mr8-n6-m480-nth5", 6, 474, 5),
    _c("mr8-n8-m512-nth4", 8, 504, 4, nsoft=10),
    _c("mr16-n4-m513-nth3", 4, 509, 3),
    _c("mr16-n6-m800-nth5", 6, 794, 5),
    _c("mr16-n8-m1024-nth4", 8, 1016, 4, nsoft=10, seed=1),
    # ---- two variable slots (n = 65, 127), every slot count built for them
    _c("nu2-mr2-n65-m128-nth4", 65, 63, 4, sb=0.03, scales=(0.02, 0.3, 1.0, 3.0, 8.0)),
    _c("nu2-mr3-n65-m150-nth3", 65, 85, 3, sb=0.03, scales=(0.02, 0.3, 1.0, 3.0, 8.0)),
    _c("nu2-mr4-n127-m256-nth4", 127, 129, 4, sb=0.03, scales=(0.02, 0.3, 1.0, 3.0, 8.0)),
    _c("nu2-mr5-n65-m300-nth3", 65, 235, 3, sb=0.03, scales=(0.02, 0.3, 1.0, 3.0, 8.0)),
    _c("nu2-mr6-n65-m384-nth3", 65, 319, 3, sb=0.03, scales=(0.02, 0.3, 1.0, 3.0, 8.0)),
    _c("nu2-mr8-n65-m500-nth3", 65, 435, 3, sb=0.03, scales=(0.02, 0.3, 1.0, 3.0, 8.0)),
    _c("nu2-mr16-n65-m1024-nth3", 65, 959, 3, sb=0.03, scales=(0.02, 0.3, 1.0, 3.0, 8.0)),
    # ---- deep working sets: beyond 32 rows, capacity - 1, the capacity itself
    _c("deep-n40-m90-nth6", 40, 50, 6, deep=True, bs=4.0, ws=0.015, sb=0.02, scales=(0.02, 1.0, 5.0, 20.0, 60.0), sim=False),
    # ---- an iteration limit
    _c("limit-n10-m80-nth5", 10, 70, 5, iter_limit=12, sim=False, scales=(0.02, 0.5, 1.5, 3.0, 6.0), exempt=("infeasible points",)),
)
CASES = _TABLE
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# nth = 0: theta has no columns, every point of a batch is the same problem (below the eight-entry parameter fetch: nothing
# is fetched).  c is large, so that the one solution has active rows; the batch conditions cannot apply -- check_nth0 instead.
NTH0 = _c("mr1-n5-m9-nth0", 5, 4, 0, fc=3.0, sim=False)
NTH0_F32 = replace(NTH0, name=NTH0.name + "-f32", f32=True)


def check_nth0(case, ef, it, active):
    """Every point the same solved problem, with rows in its final set and more than one iteration."""
    ef, it = np.asarray(ef), np.asarray(it)
    nact = popcount(active)
    ok = (ef == ef[0]).all() and (it == it[0]).all() and ef[0] >= 1 and it[0] >= 2 and nact[0] >= 1 and (nact == nact[0]).all()
    assert ok, (case.name, "one solved problem with active rows", int(ef[0]), int(it[0]), int(nact[0]))
    return int(ef[0]), int(it[0]), int(nact[0])


# limits: a batch that is infeasible throughout and one that is feasible at iteration 1 throughout
LIMIT_BATCH_CASES = ("mr3-n6-m160-nth4", "mr16-n6-m800-nth5")


def limit_theta(case, kind, N=N_COND):
    return theta(case, N, batch=6, scales={"all-infeasible": (60.0, 90.0), "all-settled": (1e-4, 1e-3)}[kind])


def check_limit_batch(case, ef, it, active, kind):
    ef, it = np.asarray(ef), np.asarray(it)
    if kind == "all-infeasible":
        ok = (ef == -1).all() and (it >= 2).all()
    else:
        ok = (ef == 1).all() and (it == 1).all() and (popcount(active) == 0).all()
    assert ok, (case.name, "limit batch", kind, np.unique(ef).tolist(), int(it.min()), int(it.max()))


# binary32 twins: one problem per slot count and variable-slot count (the levels fit more easily at four bytes a real)
F32_CASES = tuple(replace(BY_NAME[s], name=BY_NAME[s].name + "-f32", f32=True, sim=False, nsoft=0) for s in (
    "mr1-n4-m40-nth7", "mr2-n8-m100-nth16", "mr3-n6-m160-nth4", "mr4-n3-m193-nth2", "mr5-n6-m300-nth5", "mr6-n6-m350-nth5",
    "mr8-n6-m480-nth5", "mr16-n6-m800-nth5", "nu2-mr2-n65-m128-nth4", "nu2-mr3-n65-m150-nth3", "nu2-mr4-n127-m256-nth4",
    "nu2-mr5-n65-m300-nth3", "nu2-mr6-n65-m384-nth3", "nu2-mr8-n65-m500-nth3", "nu2-mr16-n65-m1024-nth3"))

# searches: binaries next to general and SOFT rows at every slot count built for branch and bound, both real types
_BNB = (
    _c("bnb-mr1-n6-m11-nth3", 6, 5, 3, nbin=3, nsoft=1, scales=(0.3, 1.0)),
    _c("bnb-mr2-n6-m100-nth3", 6, 94, 3, nbin=4, nsoft=4, scales=(0.3, 1.0)),
    _c("bnb-mr4-n4-m193-nth3", 4, 189, 3, nbin=3, scales=(0.3, 1.0)),
    _c("bnb-mr8-n5-m300-nth3", 5, 295, 3, nbin=3, scales=(0.3, 1.0)),
    _c("bnb-mr16-n5-m600-nth3", 5, 595, 3, nbin=3, scales=(0.3, 1.0)),
)
BNB_CASES = tuple(replace(c, sim=False) for c in _BNB) + tuple(replace(c, name=c.name + "-f32", f32=True, sim=False) for c in _BNB)

# a search in two passes: n = 60 makes the factor of the full capacity (62 rows) so large that a first pass at 24 rows
# keeps more wavefronts resident, which is what bnb_first_pass_cap asks for; it also asks for 4096 points
BNB_TWO_PASS = _c("bnb-twopass-n60-m80-nth3", 60, 20, 3, nbin=4, scales=(0.3, 2.0, 6.0), sb=0.02, sim=False)
N_BNB_TWO_PASS = 4096

# the slow path: every general row SOFT, theta_0 >> 0 pushes all of them over their bounds -- working sets of up to
# n + 150 rows, far beyond the wavefront kernel's 64
SLOW = _c("slow-n6-m156-nth2", 6, 150, 2, nsoft=150, bs=1.0, ws=0.3, sim=False, exempt=("infeasible points",))
SLOW_F32 = replace(SLOW, name=SLOW.name + "-f32", f32=True)
# two passes: W.cap >= 40
TWO_PASS = _c("twopass-n48-m100-nth5", 48, 52, 5, bs=0.6, ws=0.3, sim=False)
CAP1 = (8, 24, 48)
# work-list mode and ticket queue: a small problem, batches of a few thousand points
QUEUE = BY_NAME["mr2-n3-m65-nth2"]
N_QUEUE = 9001              # > 2 * grid * nwv at a grid of one workgroup per CU and nwv = 1; 2 problems per ticket at 256 CUs
N_FILL = K_SHARDS * SCREEN_BLOCK + 300      # every work-list segment gets a screening workgroup


def slow_theta(case=SLOW, N=N_COND):
    """A quarter of the points with theta_0 in [30, 60]: every soft row violated."""
    rng = np.random.default_rng(5)
    th = rng.uniform(-1, 1, (N, case.nth))
    th[::4, 0] = rng.uniform(30, 60, len(th[::4]))
    return np.ascontiguousarray(th.astype(case.dtype))


def slow_problem(case=SLOW):
    H, f, f_theta, A, bu, bl, W, sense = problem(case)
    W[case.n:, 0] = np.abs(W[case.n:, 0]) + 0.5
    return H, f, f_theta, A, bu, bl, W, sense


def two_pass_theta(kind, N=N_COND):
    """TWO_PASS batches by the share of points that outgrow a first pass: small parameters (none does), large ones
    (every one does, at 8 rows) and the case's own mix."""
    sc = {"none": (0.01, 0.05), "all": (30.0, 50.0), "mixed": None}[kind]
    return theta(TWO_PASS, N, batch=2, scales=sc)


def batch_sizes(nwv):
    """1, nwv - 1, nwv, nwv + 1 and a ragged few hundred: a wavefront owns one problem, the workgroup width is the edge."""
    return tuple(sorted({1, max(nwv - 1, 1), nwv, nwv + 1, 333}))


def nouts(case):
    return tuple(sorted({1, max(case.n // 2, 1), case.n}))


# closed loop: theta = [x] (nx = nth <= 8, no reference, no previous control), nu = nout = min(n, 2).  With the
# screening pass in front ("screen_wave" 1) and nx <= 8 the lock-step loop fuses the plant step into the wavefront
# kernel: the SIM = true instantiations of the binary64 unit, walking a work list.
S_LOOP, T_LOOP = 300, 3
SIM_CASES = tuple(c for c in CASES if c.sim)
assert all(c.nth <= 8 for c in SIM_CASES)
# the execution modes of tests/test_gpu_loops.py at one small and one many-slot case
SIM_MODE_CASES = ("mr1-n4-m40-nth7", "mr8-n6-m480-nth5")


def sim_nu(case):
    return min(case.n, 2)


def sim_data(case, S=S_LOOP):
    """(F, G, x0): a slowly contracting plant, initial states from the case's own scale mix."""
    rng = np.random.default_rng(41_000 + case.n + 7 * case.mg)
    nx = case.nth
    F = 0.97 * np.linalg.qr(rng.standard_normal((nx, nx)))[0]        # (nearly norm-preserving: the states stay in the mix)
    G = 0.3 * rng.standard_normal((nx, sim_nu(case)))
    return F, G, np.ascontiguousarray(theta(case, S, batch=5).astype(np.float64))


def sim_launches(case):
    """Launch choices of a closed-loop run: as in the plain form."""
    return launches(case)


# ---------------------------------------------------------------------------------------------------------------------
# instantiations
def instantiations():
    """(wave_kernel template arguments (sizeof(R), MR, LDSC, BNB, PACKED, NU, SIM) the GPU tests run -- GRAM is false
    throughout --, big_kernel real sizes)."""
    wave = set()
    for c in CASES + F32_CASES + BNB_CASES + (SLOW, SLOW_F32, TWO_PASS, BNB_TWO_PASS, NTH0, NTH0_F32):
        for level, packed, nwv in launches(c):
            wave.add(inst(c, level, packed))
    for c in SIM_CASES:
        for level, packed, nwv in sim_launches(c):
            wave.add(inst(c, level, packed, sim=True))
    return wave, {8, 4}


def built_by_the_dispatch():
    """What the dispatch macros of launch_wave_inst instantiate in the five n-chain translation units: 3 x 52 + 2 x 26."""
    out = set()
    for rs, sims in ((8, (False, True)), (4, (True,))):
        for sim in sims:
            for MR in MR_PLAIN:
                for packed in (False, True):
                    for level in ((0, 1, 2, 3) if (MR in MR_FOUR_LEVELS and not packed) else (0, 1)):
                        out.add((rs, MR, level, False, packed, 1, sim))
                    if MR >= 2:
                        out.add((rs, MR, 0, False, packed, 2, sim))
        for MR in MR_BNB:
            for packed in (False, True):
                for level in ((0, 1, 2, 3) if (MR in MR_FOUR_LEVELS and not packed) else (0, 1)):
                    out.add((rs, MR, level, True, packed, 1, True))
    return out


# Instantiations the library holds and `launch_wave_inst` cannot reach: template arguments -> the line of the launcher
# that excludes it.  Filled in from the built library's metadata (tests/test_wave_cases_host.py compares).
# Empty: every one of the 208 n-chain instantiations is reached by a case above -- level 3 at four constraint slots only at
# m = 193 with n <= 4 (binary64; wave_config_for, `if (lds > kLdsMax) continue`), the closed loop also with two variable
# slots (lmpc_simulate_device takes n > 64).
UNREACHED = {}
