"""Host side of the lane path's tests (no GPU): every case of tests/lane_cases.py meets the conditions that keep
tests/test_gpu_lane.py from passing emptily -- on the oracle alone, with the pack oracle.ldp.qp2ldp makes --, the
condition checker rejects batches that miss one, and the case table reaches exactly the screen_kernel / lane_kernel
instantiations the built library holds (kernel NAMES from the AMDGPU metadata notes; no code is read)."""
import os
import re
from dataclasses import replace

import numpy as np
import pytest

import lane_cases as lc
from test_fast_fallback import LIB, _kernel_vgprs

_REF = {}


def _cond(case):
    if case not in _REF:
        th = lc.theta(case, lc.N_COND)
        _REF[case] = (lc.host_ldp(case), th) + tuple(lc.reference(case, th)[1:])
    return _REF[case]


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_case_meets_the_conditions_on_the_oracle(case):
    L, th, ef, it, act = _cond(case)
    st = lc.check_lane_conditions(case, L, th, ef, it, act)
    if case.only_bounds and not case.iter_limit:
        assert st["failed"] == 0, st
    if case.iter_limit:
        assert (ef == -4).sum() >= 1 and (it[ef == -4] == case.iter_limit).all(), st
    # the smaller batches are prefixes of this one; the further batches differ from it
    for N in lc.SIZES:
        assert np.array_equal(lc.theta(case, N), th[:N])
    assert not np.array_equal(lc.theta(case, 65, batch=1), th[:65])


@pytest.mark.parametrize("case", lc.SHAPE_CASES, ids=lambda c: c.name)
def test_large_batch_fills_every_segment(case):
    th = lc.big_theta(case)
    x, ef, it, act = lc.reference(case, th)
    queued, shortest = lc.check_big_batch(case, it)
    assert (it == 1).sum() >= 64, "the large batch keeps settled points"
    with pytest.raises(AssertionError, match="half"):
        lc.check_big_batch(case, np.where(np.arange(lc.N_BIG) % 2 == 0, 1, it))


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_closed_loop_and_gather_shapes(case):
    nx, nr, nup, nu = lc.sim_shape(case)
    assert nx >= 1 and nr >= 0 and 0 <= nup <= nu and 1 <= nu <= min(4, case.n) and nx + nr + nup == case.nth <= 32
    F, G, x0, r, up = lc.sim_data(case, 321)
    assert F.shape == (nx, nx) and G.shape == (nx, nu) and x0.shape == (321, nx)
    import loop_reference as lr
    S = 321                                                  # (S_LOOP of tests/test_gpu_lane.py)
    for warm in (False, True):
        ref = lr.simulate_reference(lc.host_ldp(case, nu), x0, 3, F, G, r=r, uprev=up, warm=warm, settings=lc.oracle_settings(case))
        lc.check_loop_steps(case, ref["flags"], ref["active"])
    with pytest.raises(AssertionError, match="step"):
        lc.check_loop_steps(case, ref["flags"], np.zeros_like(ref["active"]))
    lay, gnout, null = lc.gather_layout(case)
    assert sum(lay) == case.nth and lay[0] >= 1 and lay[3] <= gnout <= case.n


def test_tables_cover_what_the_issue_lists():
    box = {c.n for c in lc.CASES if c.boxed and not c.opts and c.imm < 0 and not c.iter_limit}
    assert box == set(lc.LANE_SIZES)
    assert {c.n for c in lc.CASES if c.opts == (("fast", 0),)} == {2, 3, 4, 5}
    gen = [c for c in lc.CASES if c.mg]
    assert {c.lane_n for c in gen} == set(lc.LANE_SIZES) and {1, 7, 9, 11} <= {c.n for c in gen}
    assert {7, 11} <= {c.n for c in lc.CASES if c.only_bounds and not c.boxed}
    assert {c.m % 4 for c in gen} == {0, 1, 2, 3} and {31, 32, 33, 63, 64} <= {c.m for c in gen}
    assert {c.nth for c in lc.CASES} >= set(range(1, 18)) | {31, 32}
    assert {lc.sim_shape(c)[3] for c in lc.CASES} == {1, 2, 3, 4}
    assert any(c.imm >= 0 and c.boxed for c in lc.CASES) and any(c.imm >= c.n for c in lc.CASES)
    assert any(c.onesided for c in lc.CASES)
    assert {c.nth for c in lc.UNSCREENED} >= {0, 33} and any(c.eq >= 0 for c in lc.UNSCREENED)
    assert {c.lane_n for c in lc.SHAPE_CASES if c.boxed} == set(lc.LANE_SIZES) == {c.lane_n for c in lc.SHAPE_CASES if c.mg}
    # the m = 64, n = 12 case: its LDS copy exceeds 48 KiB at every block size, and still fits at every one
    big = lc.BY_NAME["gen12-m64-nth12"]
    assert lc.lane_blocks(big) == (64, 128, 256) and lc.lane_lds_bytes(big, 64) > 48 * 1024
    # several outputs: 2, 3, 5, 7 and n, on MULTI (N <= 6, nth <= 16) and on the generic epilogue (N >= 8, nth >= 17)
    assert {k for c in lc.CASES for k in lc.nouts(c)} >= {2, 3, 5, 7, 12}
    assert any(c.lane_n <= 6 and c.nth >= 17 and lc.nouts(c) for c in lc.CASES)
    states = {b: set() for b in "rdp"}
    for c in lc.CASES:
        (nx, nr, nd, nup, npp), gnout, null = lc.gather_layout(c)
        for b, w in zip("rdp", (nr, nd, npp)):
            states[b].add("absent" if w == 0 else ("null" if b in null else "present"))
    assert all(s == {"absent", "present", "null"} for s in states.values()), states


def test_conditions_reject_batches_that_miss_one():
    case = lc.BY_NAME["gen7-m33-nth8"]
    L, th, ef, it, act = _cond(case)
    lc.check_lane_conditions(case, L, th, ef, it, act)
    nact = lc.popcount(act)
    pick = lambda keep: np.resize(np.flatnonzero(keep), len(it))

    def rejects(idx, what, c=case, LL=L):
        with pytest.raises(AssertionError, match=what):
            lc.check_lane_conditions(c, LL, th[idx], ef[idx], it[idx], act[idx])

    def keep_tiles(drop):
        """The batch with the points `drop` replaced by others of the same kind (settled / queued), tile for tile."""
        idx = np.arange(len(it))
        for kind in (it == 1, it != 1):
            bad = np.flatnonzero(drop & kind)
            good = np.flatnonzero(~drop & kind)
            idx[bad] = np.resize(good, len(bad))
        return idx

    rejects(keep_tiles(it > nact + 1), "removed")
    rejects(keep_tiles(ef == -1), "infeasible")
    up, lo = lc.side_bits(act, case.m)
    rejects(keep_tiles(lo[:, case.n:].any(axis=1)), "either side")
    rejects(keep_tiles((nact >= case.n)), "n active rows")
    rejects(keep_tiles(lc.only_row(L, th, 32)), "partial group")
    rejects(pick(it != 1), "settled")
    rejects(keep_tiles((it == nact + 1) & (it > 1) & (ef == 1)), "append-only")
    # the built tiles: without the settled run, without the queued run, and with a second settled run
    idx = np.arange(len(it))
    s0, q0 = 64 * lc.SETTLED_TILE, 64 * lc.QUEUED_TILE
    swap = idx.copy(); swap[s0] = q0
    rejects(swap, "settled points, every other tile mixed")
    swap = idx.copy(); swap[q0] = s0
    rejects(swap, "queued points, every other tile mixed")
    swap = idx.copy(); swap[0:64] = idx[s0:s0 + 64]
    rejects(swap, "settled points, every other tile mixed")
    with pytest.raises(AssertionError, match="N_COND"):
        lc.check_lane_conditions(case, L, th[:65], ef[:65], it[:65], act[:65])
    # boxed: the first tier at capacity 3 outgrown, a full set; IMMUTABLE: points that violate that row alone
    cb = lc.BY_NAME["box6-nth14"]
    Lb, thb, efb, itb, actb = _cond(cb)
    nb = lc.popcount(actb)
    for drop, what in ((nb >= 4, "four rows"), (nb >= 6, "full working sets")):
        idx = np.arange(len(itb))
        bad = np.flatnonzero(drop)
        idx[bad] = np.resize(np.flatnonzero(~drop & (itb != 1)), len(bad))
        with pytest.raises(AssertionError, match=what):
            lc.check_lane_conditions(cb, Lb, thb[idx], efb[idx], itb[idx], actb[idx])
    ci = lc.BY_NAME["box6-nth6-imm"]
    Li, thi, efi, iti, acti = _cond(ci)
    idx = np.arange(len(iti))
    bad = np.flatnonzero(lc.only_row(Li, thi, ci.imm))
    idx[bad] = np.resize(np.flatnonzero(~lc.only_row(Li, thi, ci.imm) & (iti == 1)), len(bad))
    with pytest.raises(AssertionError, match="IMMUTABLE"):
        lc.check_lane_conditions(ci, Li, thi[idx], efi[idx], iti[idx], acti[idx])
    # the same problem without the flag: the points that violate only that row are queued, so none of them is settled
    plain = replace(ci, imm=-1)
    Hs = list(lc.problem(ci))
    Hs[7] = np.zeros(ci.m, np.int32)
    from oracle import ldp as oldp
    Lp = oldp.qp2ldp(*Hs, 1)
    xp, efp, itp, actp = oldp.solve_batch(Lp, thi)
    assert (lc.only_row(Lp, thi, ci.imm) & (itp == 1)).sum() == 0 and plain.imm == -1


def _names(pattern):
    assert os.path.exists(LIB), "build the library first"
    return _kernel_vgprs(LIB, pattern)


def test_case_table_reaches_every_instantiation_of_the_library():
    screen, lane = set(), set()
    for k in _names(r"13screen_kernelILi\d+E"):
        m = re.search(r"13screen_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", k)
        assert m, k
        screen.add(tuple(int(g) for g in m.groups()))
    for k in _names(r"4lmpc11lane_kernelILi\d+E"):
        m = re.search(r"11lane_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])EE", k)
        assert m, k
        lane.add((int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4) == "1", m.group(5) == "1"))
    assert len(screen) == 17 * 4 and len(lane) == 8 * 2 * 2 + 5 * 2, (len(screen), len(lane))
    want_screen, want_lane = lc.instantiations()
    listed_screen = {a for (kern, a) in lc.UNREACHED if kern == "screen_kernel"}
    listed_lane = {a for (kern, a) in lc.UNREACHED if kern == "lane_kernel"}
    assert not (want_screen & listed_screen) and not (want_lane & listed_lane)
    assert want_screen | listed_screen == screen, sorted(screen ^ (want_screen | listed_screen))
    assert want_lane | listed_lane == lane, sorted(lane ^ (want_lane | listed_lane))
    assert all(isinstance(v, str) and "lmpc_api.hip" in v for v in lc.UNREACHED.values())


def test_lane_cases_imports_nothing_of_the_library():
    import ast
    tree = ast.parse(open(lc.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert not names & {"linearmpc_jl_amd", "torch", "ctypes"}, names
