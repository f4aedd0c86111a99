"""Host side of the wavefront path's tests (no GPU): every case of tests/wave_cases.py meets the conditions that keep
tests/test_gpu_wave.py from passing emptily -- on the oracle alone, with the pack oracle.ldp.qp2ldp makes --, the
condition checkers reject batches that miss one, and the case table reaches exactly the wave_kernel / big_kernel
instantiations the built library holds (kernel NAMES from the AMDGPU metadata notes; no code is read).

The conditions, each a floor of wave_cases.FLOOR = 8 points of the 400-point cold batch unless the table exempts a case
(reasons next to the table): points settled at iteration 1; append-only points; points that remove a row again;
infeasible points; exit flag 2 where rows are SOFT; for EVERY constraint slot r < (m + 63) / 64 final active sets that
hold a row j with j >> 6 == r, upper and lower side counted apart (where m = 1 (mod 64) that slot IS the last row); the
iteration limit where one is set; on the deep case final sets beyond 32 rows, of capacity - 1 rows and of the whole
capacity; warm batches: points whose warm set is neither empty nor their final set; two passes: the shares of points
whose final set outgrows the first pass (none, all, mixed); searches: points whose summed iterations exceed twice the
relaxation's plus two, the oracle reporting no node counts; work-list mode: empty and filled segments; closed loop:
every step with empty and non-empty working sets."""
import os
import re
from dataclasses import replace

import numpy as np
import pytest

import wave_cases as wc
from oracle import ldp as oldp
from test_fast_fallback import LIB, _kernel_vgprs

_REF = {}
ids = lambda c: c.name


def _cold(case):
    if case not in _REF:
        th = wc.theta(case)
        _REF[case] = (th,) + tuple(wc.reference(case, th))
    return _REF[case]


@pytest.mark.parametrize("case", wc.CASES + wc.F32_CASES, ids=ids)
def test_case_meets_the_conditions_on_the_oracle(case):
    th, x, ef, it, act = _cold(case)
    st = wc.check_wave_conditions(case, ef, it, act)
    if case.iter_limit:
        assert (it[ef == -4] == case.iter_limit).all(), st
    w = wc.warm_masks(ef, act)
    xw, efw, itw, actw = wc.reference(case, th, warm=w)
    wc.check_warm_conditions(case, w, efw, actw)
    # the smaller batches are prefixes of this one; the further batches differ from it
    for N in wc.batch_sizes(4):
        assert np.array_equal(wc.theta(case, N), th[:N])
    assert not np.array_equal(wc.theta(case, 65, batch=1), th[:65])
    assert wc.launches(case), "no launch choice fits the LDS"


def _relaxed(case, L):
    Lr = replace(L, sense=(L.sense & ~wc.SENSE_BINARY).astype(np.int32))
    return Lr


@pytest.mark.parametrize("case", wc.BNB_CASES + (wc.BNB_TWO_PASS,), ids=ids)
def test_searches_visit_several_nodes(case):
    N = wc.N_BNB_TWO_PASS if case is wc.BNB_TWO_PASS else wc.N_COND
    th = wc.theta(case, N)
    L = wc.host_ldp(case)
    x, ef, it, act = wc.reference(case, th, ldp=L)
    itr = wc.reference(case, th, ldp=_relaxed(case, L))[2]
    wc.check_search_conditions(case, it, itr, ef)
    with pytest.raises(AssertionError, match="several nodes"):
        wc.check_search_conditions(case, itr, itr, ef)          # the relaxation itself: one node
    with pytest.raises(AssertionError, match="solved"):
        wc.check_search_conditions(case, it, itr, np.full_like(ef, -1))


def test_problem_without_parameters_is_one_solved_problem():
    for case in (wc.NTH0, wc.NTH0_F32):
        th = wc.theta(case)
        assert th.shape == (wc.N_COND, 0) and wc.launches(case)
        x, ef, it, act = wc.reference(case, th)
        wc.check_nth0(case, ef, it, act)
        with pytest.raises(AssertionError, match="one solved problem"):
            wc.check_nth0(case, ef, np.ones_like(it), np.zeros_like(act))      # settled at iteration 1: nothing active
        with pytest.raises(AssertionError, match="one solved problem"):
            wc.check_nth0(case, np.where(np.arange(len(ef)) == 7, -1, ef), it, act)


@pytest.mark.parametrize("name", wc.LIMIT_BATCH_CASES)
def test_limit_batches_are_infeasible_and_settled_throughout(name):
    case = wc.BY_NAME[name]
    out = {kind: wc.reference(case, wc.limit_theta(case, kind)) for kind in ("all-infeasible", "all-settled")}
    for kind, (x, ef, it, act) in out.items():
        wc.check_limit_batch(case, ef, it, act, kind)
    th, x, ef, it, act = _cold(case)                         # the mixed condition batch is neither
    for kind in out:
        with pytest.raises(AssertionError, match="limit batch"):
            wc.check_limit_batch(case, ef, it, act, kind)
    # one point of the other kind among 400 is enough to reject
    xi, efi, iti, acti = (np.array(a, copy=True) for a in out["all-infeasible"])
    efi[3], iti[3], acti[3] = 1, 1, 0
    with pytest.raises(AssertionError, match="limit batch"):
        wc.check_limit_batch(case, efi, iti, acti, "all-infeasible")
    xs, efs, its, acts = (np.array(a, copy=True) for a in out["all-settled"])
    its[5] = 2
    with pytest.raises(AssertionError, match="limit batch"):
        wc.check_limit_batch(case, efs, its, acts, "all-settled")


def test_slow_path_batches_outgrow_the_64_rows():
    for case in (wc.SLOW, wc.SLOW_F32):
        L = oldp.qp2ldp(*wc.slow_problem(case), 1)
        x, ef, it, act = wc.reference(case, wc.slow_theta(case), ldp=L)
        st = wc.check_wave_conditions(case, ef, it, act)
        assert st["beyond64"] >= wc.FLOOR and st["max_rows"] <= 256 and st["soft_optimal"] >= wc.FLOOR, st
        assert (wc.popcount(act) <= 24 - 2).sum() >= wc.FLOOR, "points a first pass at 24 rows finishes"
    # the long-horizon cases reach it too: an infeasible exit there holds n + 1 or n + 2 > 64 rows
    for name in ("mr2-n64-m128-nth17", "nu2-mr2-n65-m128-nth4", "nu2-mr16-n65-m1024-nth3"):
        th, x, ef, it, act = _cold(wc.BY_NAME[name])
        assert (wc.popcount(act) > 64).sum() >= wc.FLOOR, name


def test_two_pass_batches_split_as_named():
    case = wc.TWO_PASS
    assert case.cap >= 40
    acts = {kind: wc.reference(case, wc.two_pass_theta(kind))[3] for kind in ("none", "all", "mixed")}
    for c1 in wc.CAP1:
        for kind in ("none", "all", "mixed"):
            wc.check_two_pass_share(case, acts[kind], c1, kind)
        for kind, other in (("none", "mixed"), ("all", "mixed"), ("mixed", "none"), ("mixed", "all")):
            with pytest.raises(AssertionError, match="two-pass share"):
                wc.check_two_pass_share(case, acts[other], c1, kind)


def test_work_list_and_queue_batches():
    case = wc.QUEUE
    it_small = wc.reference(case, wc.theta(case, 2309, batch=3))[2]
    wc.check_segments(it_small, "some-empty")
    it_fill = wc.reference(case, wc.theta(case, wc.N_FILL, batch=3))[2]
    wc.check_segments(it_fill, "all-filled")
    with pytest.raises(AssertionError, match="segments"):
        wc.check_segments(it_small, "all-filled")
    with pytest.raises(AssertionError, match="segments"):
        wc.check_segments(it_fill, "some-empty")
    with pytest.raises(AssertionError, match="segments"):
        wc.check_segments(np.ones_like(it_small), "some-empty")     # nothing queued at all
    it_q = wc.reference(case, wc.theta(case, wc.N_QUEUE, batch=4))[2]
    assert (it_q != 1).sum() >= 1000 and (it_q == 1).sum() >= 1000
    # more than two problems per resident wavefront at one single-wavefront workgroup per CU, two per ticket
    assert wc.N_QUEUE > 2 * 256 and wc.N_QUEUE // (16 * 256) == 2


@pytest.mark.parametrize("case", wc.SIM_CASES, ids=ids)
def test_closed_loop_steps_have_both_kinds_of_scenario(case):
    import loop_reference as lr
    nu = wc.sim_nu(case)
    F, G, x0 = wc.sim_data(case)
    assert F.shape == (case.nth, case.nth) and G.shape == (case.nth, nu) and x0.shape == (wc.S_LOOP, case.nth) and case.nth <= 32
    L = wc.host_ldp(case, nu)
    for warm in (False, True):
        ref = lr.simulate_reference(L, x0, wc.T_LOOP, F, G, warm=warm, settings=wc.oracle_settings(case))
        wc.check_loop_steps(case, ref["flags"], ref["active"])
    with pytest.raises(AssertionError, match="step"):
        wc.check_loop_steps(case, ref["flags"], np.zeros_like(ref["active"]))


def test_conditions_reject_batches_that_miss_one():
    case = wc.BY_NAME["mr3-n10-m192-nth5"]
    th, x, ef, it, act = _cold(case)
    wc.check_wave_conditions(case, ef, it, act)
    nact = wc.popcount(act)
    up, lo = wc.side_bits(act, case.m)

    def rejects(drop, what, c=case, EF=ef, IT=it, ACT=act):
        """The batch with the points `drop` replaced by settled ones."""
        idx = np.arange(len(IT))
        idx[np.flatnonzero(drop)] = np.flatnonzero((IT == 1) & (EF == 1) & ~drop)[0]
        with pytest.raises(AssertionError, match=what):
            wc.check_wave_conditions(c, EF[idx], IT[idx], ACT[idx])

    rejects((it == nact + 1) & (it > 1) & (ef >= 1), "append-only")
    rejects((it > nact + 1) & (ef >= 1), "removed")
    rejects(ef == -1, "infeasible")
    rejects(ef == 2, "exit flag 2")
    for r in range(3):
        rejects(up[:, 64 * r:64 * r + 64].any(axis=1), "upper side")
        rejects(lo[:, 64 * r:64 * r + 64].any(axis=1), "lower side")
    idx = np.resize(np.flatnonzero(it != 1), len(it))
    with pytest.raises(AssertionError, match="settled"):
        wc.check_wave_conditions(case, ef[idx], it[idx], act[idx])
    with pytest.raises(AssertionError, match="N_COND"):
        wc.check_wave_conditions(case, ef[:65], it[:65], act[:65])
    # m = 1 (mod 64): the last row
    c1 = wc.BY_NAME["mr4-n3-m193-nth2"]
    th1, x1, ef1, it1, act1 = _cold(c1)
    u1, l1 = wc.side_bits(act1, c1.m)
    rejects(u1[:, -1] | l1[:, -1], "last row", c1, ef1, it1, act1)
    # the iteration limit, the deep working sets
    cl = wc.BY_NAME["limit-n10-m80-nth5"]
    thl, xl, efl, itl, actl = _cold(cl)
    rejects(efl == -4, "iteration limit", cl, efl, itl, actl)
    cd = wc.BY_NAME["deep-n40-m90-nth6"]
    thd, xd, efd, itd, actd = _cold(cd)
    nd = wc.popcount(actd)
    rejects(nd > 32, "beyond 32", cd, efd, itd, actd)
    rejects(nd == cd.cap - 1, "capacity - 1", cd, efd, itd, actd)
    rejects(nd >= cd.cap, "fill the capacity", cd, efd, itd, actd)
    # warm batches
    w = wc.warm_masks(ef, act)
    with pytest.raises(AssertionError, match="warm sets"):
        wc.check_warm_conditions(case, act, ef, act)            # every point started from its own final set
    with pytest.raises(AssertionError, match="warm sets"):
        wc.check_warm_conditions(case, np.zeros_like(act), ef, act)
    assert wc.check_warm_conditions(case, w, *wc.reference(case, th, warm=w)[1::2]) >= wc.FLOOR


def test_tables_cover_what_the_issue_lists():
    plain = [c for c in wc.CASES if not c.deep and not c.iter_limit]
    for MR in wc.MR_PLAIN:
        ms = {c.m for c in plain if c.MR == MR and c.NU == 1}
        if MR == 1:
            assert min(ms) <= 8 and 64 in ms
        else:
            lo = {2: 65, 3: 129, 4: 193, 5: 257, 6: 321, 8: 385, 16: 513}[MR]
            hi = {2: 128, 3: 192, 4: 256, 5: 320, 6: 384, 8: 512, 16: 1024}[MR]
            assert lo in ms and hi in ms and any(lo < v < hi for v in ms), (MR, sorted(ms))
    assert {c.n for c in wc.CASES if c.NU == 1} >= {1, 63, 64} and {c.n for c in wc.CASES if c.NU == 2} == {65, 127}
    assert {c.MR for c in wc.CASES if c.NU == 2} == {2, 3, 4, 5, 6, 8, 16}
    assert {c.nth for c in wc.CASES + (wc.NTH0,)} >= {0, 1, 7, 8, 9, 16, 17}
    assert any(c.onesided for c in wc.CASES) and any(c.imm for c in wc.CASES) and any(c.dup for c in wc.CASES)
    assert {c.MR for c in wc.CASES if c.nsoft} >= {1, 2, 3, 4, 5, 6, 8, 16}
    assert {c.MR for c in wc.SIM_CASES} == set(wc.MR_PLAIN) and {c.NU for c in wc.SIM_CASES} == {1, 2}
    assert {(c.MR, c.f32) for c in wc.BNB_CASES} == {(MR, f) for MR in wc.MR_BNB for f in (False, True)}
    assert all(c.nsoft or c.MR > 2 for c in wc.BNB_CASES) and all(c.mg for c in wc.BNB_CASES)
    assert {c.MR for c in wc.F32_CASES if c.NU == 1} == set(wc.MR_PLAIN)
    for c in wc.CASES + wc.F32_CASES + wc.BNB_CASES:
        for level, packed, nwv in wc.launches(c):
            assert wc.fits(c, level, packed, nwv) and level in wc.levels_built(c, packed)
    # m = 1024 only where sixteen slots demand it, with n <= 8 (two variable slots: n = 65)
    assert all(c.n <= 8 or c.NU == 2 for c in wc.CASES if c.m > 512)
    # every level the dispatch builds per slot count, square and packed, is asked for by some case that fits it
    for MR in wc.MR_PLAIN:
        got = {(lv, pk) for c in wc.CASES if c.MR == MR and c.NU == 1 for lv, pk, _ in wc.launches(c)}
        want = {(lv, pk) for pk in (False, True) for lv in ((0, 1, 2, 3) if (MR in wc.MR_FOUR_LEVELS and not pk) else (0, 1))}
        assert got == want, (MR, sorted(want - got))
    # level 3 at four slots: fits at m = 193 with n = 3, not at m = 256
    assert (3, False) in {(lv, pk) for lv, pk, _ in wc.launches(wc.BY_NAME["mr4-n3-m193-nth2"])}
    assert (3, False) not in {(lv, pk) for lv, pk, _ in wc.launches(wc.BY_NAME["mr4-n5-m256-nth4"])}
    assert wc.TWO_PASS.cap >= 40 and wc.SLOW.cap == 64 and wc.BNB_TWO_PASS.cap >= 24 + 4


def _built():
    assert os.path.exists(LIB), "build the library first"
    wave, big = set(), set()
    for k in _kernel_vgprs(LIB, r"4lmpc1[01](wave|big)_kernelI[df]"):
        if "big_kernel" in k:
            m = re.search(r"10big_kernelI([df])E", k)
            assert m, k
            big.add(8 if m.group(1) == "d" else 4)
            continue
        m = re.search(r"11wave_kernelI([df])Li(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)ELb([01])ELb([01])EE", k)
        assert m, k
        R, MR, LV, B, P, NU, G, S = m.groups()
        if G == "1":                                         # the Gram-scan units: tests/test_gpu_gram.py, not this table
            continue
        wave.add((8 if R == "d" else 4, int(MR), int(LV), B == "1", P == "1", int(NU), S == "1"))
    return wave, big


def test_case_table_reaches_every_instantiation_of_the_library():
    wave, big = _built()
    assert len(wave) == 3 * 52 + 2 * 26 and wave == wc.built_by_the_dispatch(), (len(wave), sorted(wave ^ wc.built_by_the_dispatch())[:8])
    want_wave, want_big = wc.instantiations()
    listed = set(wc.UNREACHED)
    assert not (want_wave & listed)
    assert want_wave | listed == wave, sorted(wave ^ (want_wave | listed))
    assert want_big == big, (want_big, big)
    assert all(isinstance(v, str) and "lmpc_wave_launch.hpp" in v for v in wc.UNREACHED.values())


def test_launch_record_entry_point_is_exported_and_refuses_bad_arguments():
    import ctypes
    import linearmpc_jl_amd as lmpc
    L = lmpc.lib()
    assert "lmpc_wave_launch_info" in lmpc.SYMBOLS and hasattr(L, "lmpc_wave_launch_info")
    out = (ctypes.c_int32 * 80)()
    assert L.lmpc_wave_launch_info(None, out, 4) == -100 and len(lmpc.BatchedQP.WAVE_LAUNCH_FIELDS) == 20
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    header = open(os.path.join(root, "include", "lmpc_hip.h")).read()
    assert "#define LMPC_WAVE_INFO_WORDS 20" in header and "int lmpc_wave_launch_info(const lmpc_handle *h, int32_t *out, int max);" in header


def test_wave_cases_imports_nothing_of_the_library():
    import ast
    tree = ast.parse(open(wc.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert not names & {"linearmpc_jl_amd", "torch", "ctypes"}, names
