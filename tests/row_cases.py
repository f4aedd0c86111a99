"""Case table of the row path's tests (tests/test_row_cases_host.py, tests/test_gpu_row.py): the problems, the forced
modes and the parameter batches that reach every instantiation of
    row_kernel<R, S, NS, MS, CAPP, BNB>                                      (lmpc_row_kernel.hpp)
that launch_row / launch_row_bnb (lmpc_row_inst.hip) spell -- six plain and three search shapes, two real types --, and
the conditions a batch has to meet ON THE ORACLE before a comparison with it counts as a test of the kernel.  Numpy and
the oracle only: nothing of the library is imported here.

The launch arithmetic of lmpc_row_inst.hip / lmpc_row_kernel.hpp is restated below (`shape_covers`, `launch_for`,
`pass_cap`, `bnb_pass_cap`, `expected`) so that the table only asks for what can run; what DID run is read from the handle's launch
record (lmpc_row_launch_info) by every GPU test, and that record decides.

Problems: the family of tests/wave_cases.py (`problem`), with one extension -- the row kernel's constraint slots are 16
rows wide, so the last row's bounds are narrowed wherever m = 1 (mod 16), not only where m = 1 (mod 64).  The slot
conditions are per 16 rows here.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

import wave_cases as wc
from wave_cases import FLOOR, GUARD, N_COND, SENSE_BINARY, popcount, side_bits

LDS_MAX = 160 * 1024
K_SHARDS = wc.K_SHARDS

# ---------------------------------------------------------------------------------------------------------------------
# (a) the launch arithmetic restated
SHAPES = ((1, 1, 4, 16), (2, 2, 6, 31), (2, 2, 6, 32), (1, 4, 10, 16), (2, 4, 10, 31), (2, 4, 10, 32))     # kRowShapes
SHAPES_BNB = ((1, 1, 2, 16), (3, 4, 4, 44), (3, 4, 4, 48))                                                 # kRowShapesBnb


def rowp_cb(capp, t):
    return 4 * (t >> 2) * capp - 8 * (t >> 2) * ((t >> 2) - 1) + (t & 3) * (capp - 4 * (t >> 2))


def rowp_size(capp):
    return {48: 1291, 44: 1095, 16: 171}.get(capp, rowp_cb(capp, capp - 1))


def row_ps(capp, nwv):
    ps = rowp_size(capp)
    while (nwv * ps) % 32 != 16:
        ps += 1
    return ps


def row_copy16(capp, rs):
    return not (capp == 44 and rs == 4)


def row_ps4(capp, nwv):
    ps = (rowp_size(capp) + 3) & ~3
    for _ in range(16):
        if (nwv * ps) % 32 == 16:
            return ps
        ps += 4
    return -1


def row_mpad(ms, rs):
    return 16 * ms + (4 if (rs == 4 and ms % 4 == 0) else 2)


def _one_per_simd(ms, s, rs):
    return (ms > 6 and s >= 2) or (s >= 3 and rs == 8)


def row_launch_bound(ms, s, rs):
    return 256 if _one_per_simd(ms, s, rs) else 512


def row_waves_per_simd(s, ms, rs):
    return 1 if _one_per_simd(ms, s, rs) else (3 if (s == 1 and ms <= 6) else 2)


def row_bnb_depth_max(ms):
    return min(16 * ms, 48) - 1


def row_snap_reals(s, capp):
    return 64 * s + ((rowp_size(capp) + 3) & ~3)


def row_snap_ints(s):
    return 16 * s + 16


def shape_covers(sh, n, m, cap):
    S, NS, MS, CAPP = sh
    return n <= 16 * NS and m <= 16 * MS and cap <= CAPP and m <= 256


def aux_reals(n, m, nth, nout):
    """row_aux_reals: du, dl, Dth, Rout, x0, Xth of the constant pack."""
    return 2 * m + m * nth + nout * n + nout + nout * nth


def launch_for(n, m, nth, nout, cap, rs, bnb=False, nbin=0):
    """row_launch_for: dict(shape, nwv, blocks, ps, lds, aux) of the launch, or None where the launcher refuses."""
    for sh in (SHAPES_BNB if bnb else SHAPES):
        S, NS, MS, CAPP = sh
        if not shape_covers(sh, n, m, cap):
            continue
        if bnb and nbin > row_bnb_depth_max(MS):
            continue
        best, best_waves = None, 0
        mt = ((n + 3) & ~3) * row_mpad(MS, rs)
        for nwv in (8, 7, 6, 5, 4, 3, 2, 1):
            if 64 * nwv > row_launch_bound(MS, S, rs):
                continue
            ps = row_ps4(CAPP, nwv) if (bnb and row_copy16(CAPP, rs)) else row_ps(CAPP, nwv)
            if ps < 0:
                continue
            front = rs * (32 + mt + nwv * 4 * ps + 2) + 4 * (m + CAPP)
            lds, aux = front + 16, 0
            if lds > LDS_MAX:
                continue
            if MS >= 10:
                lds, aux = ((front + 15) & ~15) + rs * aux_reals(n, m, nth, nout) + 16, 1
                if lds > LDS_MAX:
                    continue
            blocks = LDS_MAX // lds
            maxw = 4 * row_waves_per_simd(S, MS, rs)
            if blocks * nwv > maxw:
                blocks = maxw // nwv
            if blocks < 1:
                continue
            if blocks * nwv > best_waves:
                best_waves, best = blocks * nwv, dict(shape=sh, nwv=nwv, blocks=blocks, ps=ps, lds=lds, aux=aux)
        return best
    return None


@dataclass(frozen=True)
class RowCase:
    """A problem of the wave family (`w`), the options that force the row kernel onto it, and what the restated
    arithmetic expects to launch.  mode: "full" = "row_kernel" 1 alone, "cap1" = + "wave_two_pass" 1, "wave_cap1" cap1,
    "default" (searches) = no option at all: the dispatch's own rule."""
    w: wc.WaveCase
    mode: str = "full"
    cap1: int = 0
    share: str = ""                 # two-pass share the condition batch must show at the launch's capacity: none / mixed / all
    nout: int = 1
    slow: bool = False              # SOFT rows: some sets go beyond 64 rows (row pass -> second pass -> big_kernel)
    mid: float = 0.0                # searches: the unconstrained optimum of the binaries moved by this much, into (0, 1)
    exempt: tuple = ()

    @property
    def name(self):
        return self.w.name

    @property
    def n(self):
        return self.w.n

    @property
    def m(self):
        return self.w.m

    @property
    def f32(self):
        return self.w.f32

    @property
    def rs(self):
        return self.w.rs

    @property
    def dtype(self):
        return self.w.dtype

    @property
    def bnb(self):
        return self.w.bnb

    @property
    def full(self):
        return self.w.cap

    @property
    def cap_full(self):
        """capFull of finalize_handle: n + 2 + #soft."""
        return self.w.n + 2 + self.w.nsoft

    @property
    def options(self):
        o = (("row_kernel", 1),)
        if self.mode == "cap1":
            o += (("wave_two_pass", 1), ("wave_cap1", self.cap1))
        return o


def pass_cap(case):
    """row_pass_cap for a cold plain batch on a FRESH handle with "row_kernel" 1 and the slow path on ("big_path" 1,
    the default), "wave_two_pass" -1 or 1: the capacity of the row launch, 0 = the row kernel does not take the batch.
    (The 16-row first pass the statistics can choose after 1000 problems -- `fits16` -- is kept out by the condition
    `beyond16_share`: more than 2 in 100 points with more than 16 rows.)"""
    w = case.w
    if w.bnb or (w.iter_limit and w.iter_limit < 2):
        return 0
    lf = lambda c: launch_for(w.n, w.m, w.nth, case.nout, c, w.rs)
    if case.mode == "cap1" and 0 < case.cap1 < case.full:
        return case.cap1 if lf(case.cap1) else 0
    if case.full <= 32:
        return case.full if lf(case.full) else 0
    return 31 if lf(31) else 0


def bnb_pass_cap(case):
    """row_bnb_pass_cap with "row_kernel" 1 (mode "full") or + "wave_two_pass" 1, "wave_cap1" c (mode "cap1");
    mode "default" = "row_kernel" -1, "wave_two_pass" -1: the default rule."""
    w = case.w
    if not w.bnb or (w.iter_limit and w.iter_limit < 2) or w.nbin > 47:
        return 0
    lf = lambda c: launch_for(w.n, w.m, w.nth, case.nout, c, w.rs, True, w.nbin)
    full = case.full
    if full <= 16:
        return full if lf(full) else 0
    if full <= 48 and case.mode != "default":
        return full if lf(full) else 0
    if case.mode == "cap1":
        c = min(case.cap1, 48)
        return c if lf(c) else 0
    if full <= 52:
        return 0
    c1 = 44 if w.nbin + 4 <= 44 else 48
    return c1 if lf(c1) else 0


def expected(case):
    """What a cold call on a fresh handle should launch: dict(inst, cap, pass, + launch_for's fields), or None.  Plain
    form: the only pass (0) where nothing lies behind the capacity -- with the slow path on there always is
    (capFull = n + 2 + #soft > W.cap), so a plain row launch is the first of two; a search's is the only one when the
    capacity is the problem's."""
    w = case.w
    cap = bnb_pass_cap(case) if w.bnb else pass_cap(case)
    if cap <= 0:
        return None
    L = launch_for(w.n, w.m, w.nth, case.nout, cap, w.rs, w.bnb, w.nbin)
    only = cap >= case.full and (w.bnb or not case.cap_full > case.full)
    return dict(L, inst=(w.rs,) + L["shape"] + (int(w.bnb),), cap=cap, **{"pass": 0 if only else 1})


def options_for(case):
    if case.mode == "default":
        return ()
    return case.options


# ---------------------------------------------------------------------------------------------------------------------
# problems, batches, the oracle
def problem(case):
    """wave_cases.problem, the last row narrowed also where m = 1 (mod 16) leaves it alone in a 16-row slot."""
    H, f, f_theta, A, bu, bl, W, sense = wc.problem(case.w)
    w = case.w
    if w.m % 16 == 1 and w.m % 64 != 1 and w.mg:
        bu[w.m - 1] *= w.last
        bl[w.m - 1] *= w.last
        sense[w.m - 1] = 0
    if case.slow:
        W[w.n:, 0] = np.abs(W[w.n:, 0]) + 0.5
    if case.mid:
        f = f - H[:, :w.nbin] @ np.full(w.nbin, case.mid)
    return H, f, f_theta, A, bu, bl, W, sense


def theta(case, N=N_COND, batch=0, scales=None):
    if case.slow:
        return np.ascontiguousarray(wc.slow_theta(case.w, max(int(N), N_COND))[:N])    # (a smaller batch: a prefix)
    return wc.theta(case.w, N, batch, scales)


def host_ldp(case):
    from oracle import ldp as oldp
    return oldp.qp2ldp(*problem(case), case.nout)


def reference(case, th, ldp=None):
    return wc.reference(case.w, th, nout=case.nout, ldp=host_ldp(case) if ldp is None else ldp)


def relaxed_iters(case, th, ldp=None):
    """Iterations of the relaxation (the BINARY flags dropped) -- what one node of a search costs."""
    L = host_ldp(case) if ldp is None else ldp
    Lr = replace(L, sense=(L.sense & ~SENSE_BINARY).astype(np.int32))
    return wc.reference(case.w, th, nout=case.nout, ldp=Lr)[2]


# ---------------------------------------------------------------------------------------------------------------------
# (c) conditions
def row_stats(case, ef, it, active):
    ef, it = np.asarray(ef), np.asarray(it)
    nact = popcount(active)
    up, lo = side_bits(active, case.m)
    slots = (case.m + 15) // 16
    return dict(N=len(it), settled=int(((it == 1) & (ef == 1)).sum()),
                append_only=int(((it == nact + 1) & (it > 1) & (ef >= 1)).sum()), removing=int(((it > nact + 1) & (ef >= 1)).sum()),
                infeasible=int((ef == -1).sum()), soft_optimal=int((ef == 2).sum()), limit=int((ef == -4).sum()),
                slot_upper=[int(up[:, 16 * r:16 * r + 16].any(axis=1).sum()) for r in range(slots)],
                slot_lower=[int(lo[:, 16 * r:16 * r + 16].any(axis=1).sum()) for r in range(slots)],
                last_row=int((up[:, -1] | lo[:, -1]).sum()), beyond16=int((nact > 16).sum()),
                cap_less_one=int((nact == case.full - 1).sum()), at_cap=int((nact == case.full).sum()),
                beyond_cap_full=int((nact > case.cap_full).sum()), beyond64=int((nact > 64).sum()), max_rows=int(nact.max()))


def check_row_conditions(case, ef, it, active):
    """Conditions on the ORACLE's outputs for the cold condition batch of a plain case; raises AssertionError naming
    every one that fails, returns the counts."""
    st = row_stats(case, ef, it, active)
    e = expected(case)
    missed = []

    def need(ok, what):
        if not ok and what not in case.exempt:
            missed.append(what)
    assert st["N"] == N_COND, "the conditions apply to the batch of N_COND points"
    assert not case.bnb
    w = case.w
    need(st["settled"] >= FLOOR, "settled at iteration 1")
    need(st["append_only"] >= FLOOR, "append-only")
    need(st["removing"] >= FLOOR, "rows removed again")
    need(st["infeasible"] >= FLOOR, "infeasible points")
    if w.nsoft:
        need(st["soft_optimal"] >= FLOOR, "exit flag 2")
    need(min(st["slot_upper"]) >= FLOOR, "an upper side active in every 16-row slot")
    need(min(st["slot_lower"]) >= FLOOR, "a lower side active in every 16-row slot")
    if case.m % 16 == 1:
        need(st["last_row"] >= FLOOR, "the last row, alone in its slot, active")
    if w.iter_limit:
        need(st["limit"] >= FLOOR, "iteration limit reached")
    if w.deep:
        need(st["cap_less_one"] >= FLOOR, "working sets of capacity - 1 rows")
        need(st["at_cap"] >= FLOOR, "working sets that fill the capacity")
    if e is not None and e["shape"][0] >= 2:
        need(st["beyond16"] >= FLOOR, "working sets beyond 16 rows")
    if e is not None and case.mode == "full" and case.full > 32:
        need(st["beyond16"] * 50 > st["N"], "beyond16_share")     # (keeps the statistics from choosing 16 rows)
    if case.slow:
        need(st["beyond64"] >= FLOOR, "working sets beyond 64 rows")
    else:
        # a set beyond capFull is beyond every kernel of the library (exit flag -7 against the oracle's own arrays)
        assert st["beyond_cap_full"] == 0, (case.name, "working sets beyond capFull", st)
    assert not missed, (case.name, missed, st)
    if case.share:
        check_share(case, active, e["cap"], case.share)
    return st


def check_search_conditions(case, ef, it, it_relaxed, active):
    """Searches: several nodes' worth of iterations (wave_cases.check_search_conditions), every binary row in the final
    set of every solved point, and binaries that change their side between points."""
    deep = wc.check_search_conditions(case.w, it, it_relaxed, ef)
    up, lo = side_bits(active, case.m)
    nb = case.w.nbin
    solved = np.asarray(ef) >= 1
    fixed = (up[:, :nb] ^ lo[:, :nb])[solved]
    assert fixed.all(), (case.name, "a solved search with a binary row outside its final set")
    u = up[:, :nb][solved]
    both = int((u.any(axis=0) & (~u).any(axis=0)).sum())
    assert both >= 1, (case.name, "no binary changes its side between points")
    nact = popcount(active)
    assert (nact <= case.cap_full).all()
    if case.share:
        check_share(case, active, expected(case)["cap"], case.share)
    return dict(deep=deep, solved=int(solved.sum()), sides_both=both, max_rows=int(nact.max()))


def check_share(case, active, cap, kind):
    """wave_cases.check_two_pass_share, plus kind "most": more than half of the points' final sets outgrow the first
    pass and at least FLOOR certainly stay inside it."""
    if kind != "most":
        return wc.check_two_pass_share(case.w, active, cap, kind)
    nact = popcount(active)
    over, inside = int((nact > cap).sum()), int((nact <= cap - 2).sum())
    assert 2 * over > len(nact) and inside >= FLOOR, (case.name, "two-pass share", kind, cap, over, inside)
    return over, inside


def check_segments(it, kind, block):
    """Work-list mode: the queued points (iters != 1) per segment; the pass in front assigns workgroup b of `block`
    points to segment b % K_SHARDS (wave_cases.check_segments is the screening pass's, block = 256)."""
    it = np.asarray(it)
    queued = it if it.dtype == bool else (it != 1)            # (a boolean array: the points certainly queued, as they are)
    shard = (np.arange(len(it)) // block) % K_SHARDS
    per = np.bincount(shard, weights=queued, minlength=K_SHARDS)
    ok = (per.min() == 0 and per.max() >= FLOOR) if kind == "some-empty" else per.min() >= FLOOR
    assert ok, ("work-list segments", kind, int(per.min()), int(per.max()))
    return int(per.min()), int(per.max())


# ---------------------------------------------------------------------------------------------------------------------
# (b) the table.  Sizes, bound factors and scale mixes were chosen on the CPU until the oracle alone met the conditions
# (tests/test_row_cases_host.py re-checks every one).
_WIDE = (0.02, 0.3, 1.0, 3.0, 8.0)
_DEEP = dict(deep=True, bs=4.0, ws=0.015, sb=0.02, scales=(0.02, 1.0, 5.0, 20.0, 60.0))


def _w(name, n, m, nth, **kw):
    kw.setdefault("sim", False)
    return wc.WaveCase(name, n, m - n, nth, **kw)


def _r(name, n, m, nth, mode="full", cap1=0, share="", nout=1, slow=False, exempt=(), mid=0.0, **kw):
    return RowCase(_w(name, n, m, nth, **kw), mode, cap1, share, nout, slow, mid, tuple(exempt))


_MOST = (0.02, 1.0, 3.0, 8.0, 8.0)      # (first passes of 8 rows: more than half of the points outgrow them)
_S = dict(sb=0.03, scales=_WIDE)        # tight simple bounds: the low constraint slots (the n simple bounds) are active too
# Exemptions.  n = 1 and n = 2: the solver adds the most violated row, which is the tightest of its side, so a row is
# (almost) never removed again -- 0 and 1 of 400 points.  The limit case: an infeasible exit of the n = 10 problem takes
# n + 2 = 12 iterations, which the limit of 12 ends first.  The all-SOFT slow-path problem is never infeasible.
PLAIN = (
    # ---- {1, 1, 4, 16}: n <= 15 (16 rows hold n + 1), m <= 64: m = 49 (row 48 alone in slot 3), 56, 64
    _r("s1-n1-m17-nth1", 1, 17, 1, ws=0.2, bs=2.0, scales=(0.02, 1, 3, 8, 20), exempt=("rows removed again",)),
    _r("s1-n2-m33-nth2", 2, 33, 2, ws=0.2, bs=2.0, scales=(0.02, 1, 3, 8, 20), exempt=("rows removed again",)),
    _r("s1-n10-m49-nth5", 10, 49, 5, **_S),
    _r("s1-n12-m56-nth16", 12, 56, 16, **_S),
    _r("s1-n12-m60-nth8-soft", 12, 60, 8, nsoft=3, onesided=True, imm=True, dup=True, **_S),
    _r("s1-n10-m63-nth5-limit", 10, 63, 5, iter_limit=12, sb=0.3, scales=(0.02, 0.5, 1.5, 3.0, 6.0), exempt=("infeasible points",)),
    _r("s1-n15-m64-nth6-deep", 15, 64, 6, **_DEEP),
    # (the tiers-list case: 60 of 400 points remove a row again, which the tiers pass in front certainly leaves to the list)
    _r("s1-n10-m49-nth5-deep", 10, 49, 5, **_DEEP),
    # (n = 16, the slot's full width: 17 rows are the capacity, so the one-slot shape takes it as a first pass of 16)
    _r("s1-n16-m64-nth5-c16", 16, 64, 5, mode="cap1", cap1=16, share="mixed", **_S),
    # ---- {2, 2, 6, 31}: n = 16, 17 .. 30, m <= 96: m = 81 (row 80 alone in slot 5), 90, 96
    _r("s2-n16-m81-nth17", 16, 81, 17, **_S),
    _r("s2-n17-m90-nth4", 17, 90, 4, **_S),
    _r("s2-n20-m90-nth17-soft", 20, 90, 17, nsoft=6, onesided=True, imm=True, dup=True, **_S),
    _r("s2-n30-m96-nth6-deep", 30, 96, 6, **_DEEP),
    # (n = 32, both slots full: capacity 33, first of two passes at 31 rows)
    _r("s2-n32-m96-nth5", 32, 96, 5, share="mixed", seed=1, **_S),
    # ---- {2, 2, 6, 32}: n = 31
    _r("s2-n31-m81-nth3", 31, 81, 3, **_S),
    _r("s2-n31-m96-nth6-deep", 31, 96, 6, **_DEEP),
    _r("s2-n32-m81-nth5-c32", 32, 81, 5, mode="cap1", cap1=32, share="mixed", seed=1, **_S),       # (n = 32 through "wave_cap1" 32)
    # ---- {1, 4, 10, 16}: n <= 15 with m = 145 (row 144 alone in slot 9), 150, 160 -- and as a first pass below
    _r("t1-n8-m145-nth33", 8, 145, 33, **_S),
    _r("t1-n15-m160-nth5", 15, 160, 5, **_S),
    # ---- {2, 4, 10, 31}: n = 30 with m > 96 as the only capacity; n = 32, 33, 48, 49, 64 as the first of two passes at 31 rows
    _r("t2-n30-m145-nth5", 30, 145, 5, **_S),
    _r("t2-n32-m160-nth5", 32, 160, 5, share="mixed", **_S),
    _r("t2-n33-m150-nth5", 33, 150, 5, share="mixed", **_S),
    _r("t2-n48-m160-nth5", 48, 160, 5, share="mixed", **_S),
    _r("t2-n49-m145-nth5", 49, 145, 5, share="mixed", **_S),
    _r("t2-n64-m160-nth5", 64, 160, 5, share="mixed", **_S),
    _r("t2-n40-m160-nth16-soft", 40, 160, 16, nsoft=10, share="mixed", **_S),
    # (wide theta: the per-problem constants leave room for three wavefronts' factors instead of four)
    _r("t2-n48-m160-nth33-aux", 48, 160, 33, ws=0.04, share="mixed", **_S),
    # ---- {2, 4, 10, 32}: n = 31 with m > 96; n > 32 through "wave_cap1" 32
    _r("t2-n31-m160-nth5", 31, 160, 5, **_S),
    _r("t2-n33-m150-nth5-c32", 33, 150, 5, mode="cap1", cap1=32, share="mixed", **_S),
    _r("t2-n48-m160-nth5-c32", 48, 160, 5, mode="cap1", cap1=32, share="mixed", **_S),
    _r("t2-n49-m145-nth5-c32", 49, 145, 5, mode="cap1", cap1=32, share="mixed", **_S),
    _r("t2-n64-m160-nth5-c32", 64, 160, 5, mode="cap1", cap1=32, share="mixed", **_S),
    # ---- first passes of 16 rows on {1, 4, 10, 16} ("wave_two_pass" 1, "wave_cap1" 16)
    _r("t1-n33-m150-nth5-c16", 33, 150, 5, mode="cap1", cap1=16, share="mixed", **_S),
    _r("t1-n48-m97-nth5-c16", 48, 97, 5, mode="cap1", cap1=16, share="mixed", **_S),
    _r("t1-n49-m145-nth5-c16", 49, 145, 5, mode="cap1", cap1=16, share="mixed", **_S),
    _r("t1-n64-m160-nth5-c16", 64, 160, 5, mode="cap1", cap1=16, share="mixed", **_S),
    # ---- first passes of 8 rows on the one- and two-slot shapes
    _r("s1-n12-m56-nth16-c8", 12, 56, 16, mode="cap1", cap1=8, share="most", sb=0.03, scales=_MOST),
    _r("s2-n24-m96-nth4-c8", 24, 96, 4, mode="cap1", cap1=8, share="most", sb=0.03, scales=_MOST),
    # ---- row pass -> wavefront second pass -> big_kernel: SOFT rows, sets beyond 64 rows
    _r("t2-n40-m100-nth2-slow", 40, 100, 2, nsoft=60, bs=1.0, ws=0.3, slow=True, share="mixed", exempt=("infeasible points",)),
)
PLAIN_F32 = tuple(replace(c, w=replace(c.w, name=c.w.name + "-f32", f32=True)) for c in PLAIN)

# two-pass shares "none" and "all" (mixed: the cases' own batches): (case, scales)
SHARE_CASES = ("t1-n33-m150-nth5-c16", "t2-n48-m160-nth5", "t2-n49-m145-nth5-c32", "s1-n12-m56-nth16-c8", "s2-n24-m96-nth4-c8")
SHARE_SCALES = {"none": (1e-3, 5e-3), "all": (30.0, 50.0)}

# several outputs: nout = n / 2 and n
NOUT_CASES = ("s1-n12-m56-nth16", "s2-n17-m90-nth4", "t1-n15-m160-nth5", "t2-n33-m150-nth5")

# nth = 0: every point the same problem (wave_cases.check_nth0); nth = 1, 16, 17, 33 are in the table
NTH0 = _r("t1-n12-m150-nth0", 12, 150, 0, fc=3.0)
NTH0_F32 = replace(NTH0, w=replace(NTH0.w, name=NTH0.w.name + "-f32", f32=True))

# a batch that is infeasible throughout / settled at iteration 1 throughout (wave_cases.limit_theta)
LIMIT_BATCH_CASES = ("s1-n10-m49-nth5", "s2-n17-m90-nth4", "t2-n33-m150-nth5")

# searches.  Binaries: the leading simple bounds, 0 <= x <= 1; f shifts the unconstrained optimum to +-0.6 so that they
# take both sides.  One pass: {1, 1, 2, 16} at m = 17 and 32; {3, 4, 4, 44} (capacity <= 44) and {3, 4, 4, 48} (45 .. 48) at
# m = 49 and 64, with 8, 17 and 34 binaries (stack entries in register slots 0, 1, 2).  First passes: the default rule
# (capacity > 52: 44 rows where the binaries + 4 fit, else 48) and "wave_cap1" 20, which lists most searches.
_B = dict(scales=(1.0, 4.0), fc=0.6)
_B2 = dict(scales=(0.3, 4.0, 12.0), fc=0.15, sb=0.03)
_BNB = (
    _r("bnb-n6-m17-b3", 6, 17, 3, nbin=3, nsoft=1, **_B),
    _r("bnb-n14-m32-b5", 14, 32, 3, nbin=5, **_B),
    _r("bnb-n20-m49-b17", 20, 49, 3, nbin=17, **_B),
    _r("bnb-n42-m64-b8", 42, 64, 3, nbin=8, **_B),
    _r("bnb-n46-m64-b34", 46, 64, 3, nbin=34, **_B),
    _r("bnb-n52-m64-b8-default", 52, 64, 3, nbin=8, mode="default", share="mixed", **_B2),
    _r("bnb-n52-m64-b41-default", 52, 64, 3, nbin=41, mode="default", share="mixed", **_B2),
    _r("bnb-n52-m64-b8-c20", 52, 64, 3, nbin=8, mode="cap1", cap1=20, share="most", **_B2),
)
BNB = _BNB + tuple(replace(c, w=replace(c.w, name=c.w.name + "-f32", f32=True)) for c in _BNB)

ALL = PLAIN + PLAIN_F32 + BNB + (NTH0, NTH0_F32)
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)

# work-list mode: behind the tiers pass (n <= 12, m <= 64) and behind the screening pass (the ten-slot class)
LIST_TIERS = BY_NAME["s1-n10-m49-nth5-deep"]
TIERS_BLOCK = 64        # lmpc_qp_tiers_kernel.hpp: wavefront gw takes the tiles gw, gw + nw, ... (nw % 64 == 0), segment gw % 64
LIST_SCREEN = BY_NAME["t1-n15-m160-nth5"]
# ticket queue: the narrowest shape, "row_blocks" 1
QUEUE = BY_NAME["s1-n10-m49-nth5"]

# refusals: "row_kernel" 1 is asked for and no row launch may show.  (name, case, how the GPU test sets it up)
REFUSE_WIDE = _r("refuse-n64-m160-nth40-nout64", 64, 160, 40, nout=64, ws=0.04, **_S)     # no LDS size fits
REFUSE_M = _r("refuse-n10-m170-nth3", 10, 170, 3, **_S)                                    # no covering shape
REFUSE_BIN = _r("refuse-n50-m64-b48", 50, 64, 3, nbin=48, **_B)                            # more binaries than the depth


def batch_sizes(nwv):
    """A wavefront carries four problems, a workgroup 4 nwv."""
    return tuple(sorted({1, 2, 3, 4, 5, 4 * nwv - 1, 4 * nwv, 4 * nwv + 1, 333}))


def instantiations():
    """(sizeof(R), S, NS, MS, CAPP, BNB) of every instantiation the table expects to launch."""
    return {expected(c)["inst"] for c in ALL if expected(c) is not None}


def built():
    """What launch_row / launch_row_bnb spell: every shape in both real types."""
    return {(rs,) + sh + (0,) for rs in (8, 4) for sh in SHAPES} | {(rs,) + sh + (1,) for rs in (8, 4) for sh in SHAPES_BNB}


# Instantiations the dispatch cannot reach: none.
UNREACHED = {}


# The search stack's third register slot (depths 32 ... 47).  A node branches on the lowest binary row OUTSIDE its working
# set, and with the optimum of the relaxation spread over +-0.6 half of the binaries sit on a bound at the root: the
# searches above reach depth ~ nbin / 2, i.e. slots 0 and 1 only.  Here the binaries' unconstrained optimum is moved to
# 0.5 +- 0.45, inside (0, 1): the relaxation at the root leaves (nearly) all 34 binaries free, so a leaf lies 33 or 34
# levels deep, and both sides are tried first.  Such a search costs the oracle ~2e5 iterations, so the batch is 8 points,
# not N_COND; the condition (on the oracle: the root relaxation's free binaries) is held by at least half of them.
N_DEEP_STACK = 8
DEEP_STACK = _r("bnb-n46-m64-b34-mid", 46, 64, 3, nbin=34, mid=0.5, scales=(1.0, 4.0), fc=0.45)
DEEP_STACK_F32 = replace(DEEP_STACK, w=replace(DEEP_STACK.w, name=DEEP_STACK.w.name + "-f32", f32=True))


def check_deep_stack(case, ef, active, active_relaxed):
    """Every search solved with every binary fixed; at least half of the points leave 33 or more binaries outside the
    root relaxation's final set (the depth a leaf then has is NOT witnessed by the oracle: see DESIGN)."""
    nb = case.w.nbin
    up, lo = side_bits(active, case.m)
    assert (np.asarray(ef) >= 1).all() and (up[:, :nb] ^ lo[:, :nb]).all(), (case.name, "solved searches")
    ur, lr_ = side_bits(active_relaxed, case.m)
    free = (~(ur[:, :nb] | lr_[:, :nb])).sum(axis=1)
    assert (free >= 33).sum() * 2 >= len(free), (case.name, "binaries free at the root", free.tolist())
    return dict(free_min=int(free.min()), free_max=int(free.max()), upper_among_last=int(up[:, 32:nb].sum()), lower_among_last=int(lo[:, 32:nb].sum()))


def relaxed_active(case, th, ldp=None):
    L = host_ldp(case) if ldp is None else ldp
    Lr = replace(L, sense=(L.sense & ~SENSE_BINARY).astype(np.int32))
    return wc.reference(case.w, th, nout=case.nout, ldp=Lr)[3]
