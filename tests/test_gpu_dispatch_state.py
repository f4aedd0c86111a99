"""No form of the batched-solve dispatch leaves anything behind in the handle: pass, work list, first-pass capacity and
the second pass's level / workgroup preference are arguments of a launch, so a call's launch records and results depend
on the handle's options and the call's arguments alone -- never on which form ran before it.

ONE wavefront-kernel handle (wave_cases.TWO_PASS: n = 48, m = 100, nth = 5, capacity 49) runs 300 points in turn as one
pass, behind the screening pass, in two passes at 24 rows, behind the row kernel, in binary32, warm-started, with
profiling on, and as one pass again.  The layout is pinned to the square factor; staging level and workgroup width are
left to the launcher, so that the row path's second-pass preference (small workgroups, highest level) is in play.  Every
step's launch records are asserted first -- the words the launcher does not choose against the case, the chosen
(level, nwv) against the arithmetic of tests/wave_cases.py (instantiation, LDS bytes) and, for the row path, of
tests/row_cases.py -- then the results against the oracle, bit for bit.  The last step's records (all words but `seq`)
and outputs equal the first step's.  The same on one lane-kernel handle, which keeps no launch record: screened,
one-launch kernel, screened, warm, screened."""
from dataclasses import replace

import numpy as np
import pytest

import lane_cases as lc
import row_cases as rc
import test_gpu_lane as tl
import test_gpu_wave as tw
import wave_cases as wc

pytestmark = pytest.mark.gpu

N = 300


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _words(recs):
    return [{k: v for k, v in r.items() if k != "seq"} for r in recs]


def _expect(recs, case, passes, caps, worklist, what):
    """One record per pass; square layout; (level, nwv) as recorded must be a launch the case's LDS arithmetic allows,
    and everything that follows from them -- instantiation, LDS bytes -- as tests/wave_cases.py restates it."""
    assert [r["pass"] for r in recs] == list(passes), (what, recs)
    for r, cap in zip(recs, caps):
        level, nwv = r["level"], r["nwv"]
        assert level in wc.levels_built(case, False) and wc.fits(case, level, False, nwv, cap), (what, "launch configuration", r)
        rs, MR, LDSC, BNB, PACKED, NU, SIM = wc.inst(case, level, False)
        got = (r["real_bytes"], r["MR"], r["LDSC"], r["BNB"], r["PACKED"], r["NU"], r["GRAM"], r["SIM"])
        assert got == (rs, MR, LDSC, int(BNB), 0, NU, 0, int(SIM)), (what, "instantiation", r)
        assert r["cap"] == cap and r["lds"] == wc.lds_bytes(case, level, False, nwv, cap), (what, "capacity / LDS bytes", r)
        assert r["big"] == (0 if r["pass"] == 1 else 1), (what, "slow path", r)
        want_list = 1 if (worklist or r["pass"] == 2) else 0
        assert (r["worklist"], r["queue"], r["qchunk"]) == (want_list, want_list, 1), (what, "work list / tickets", r)
        assert r["nprob"] == N and 1 <= r["grid"] <= -(-N // nwv), (what, "grid", r)
    assert [r["seq"] for r in recs] == list(range(recs[0]["seq"], recs[0]["seq"] + len(recs)))


def test_wavefront_handle_forms_in_turn(lmpc):
    case = wc.TWO_PASS
    case32 = replace(case, name=case.name + "-f32", f32=True)
    qp = tw._handle(lmpc, case)
    qp.set_option("wave_packed", 0)
    th = wc.two_pass_theta("mixed")[:N]
    ref = tw._cached((case, "state", "cold"), lambda: tw._oracle(qp, case, th))
    ref32 = tw._cached((case32, "state", "cold"), lambda: tw._oracle(qp, case32, th.astype(np.float32)))
    warm = wc.warm_masks(ref[1], ref[3])
    refw = tw._cached((case, "state", "warm"), lambda: tw._oracle(qp, case, th, warm=warm))
    print(wc.check_two_pass_share(case, ref[3], 24, "mixed"))

    def opts(**kw):
        for k, v in {**dict(screen_wave=0, wave_two_pass=0, wave_cap1=24, row_kernel=0), **kw}.items():
            qp.set_option(k, v)

    # 1: one pass
    opts()
    first, recs1 = tw._solve(qp, case, th)
    _expect(recs1, case, (0,), (case.cap,), False, "1: one pass")
    tw._same(first, ref, N, "1: one pass")
    # 2: behind the screening pass
    opts(screen_wave=1)
    got, recs = tw._solve(qp, case, th)
    _expect(recs, case, (0,), (case.cap,), True, "2: screening pass")
    tw._same(got, ref, N, "2: screening pass")
    # 3: two passes, the first at 24 rows
    opts(wave_two_pass=1)
    got, recs = tw._solve(qp, case, th)
    _expect(recs, case, (1, 2), (24, case.cap), False, "3: two passes")
    tw._same(got, ref, N, "3: two passes")
    # 4: the row kernel as the first of two passes; the second pass at the preferred configuration -- two wavefronts per
    # workgroup at the highest staging level that fits them ("wave_two_pass" 0 would rule a first pass out)
    opts(row_kernel=1, wave_two_pass=-1)
    rcase = rc.RowCase(case)
    e = rc.expected(rcase)
    assert e is not None and (e["pass"], e["cap"]) == (1, 31), e
    rseq = (qp.row_launch_info() or [dict(seq=0)])[-1]["seq"]
    got, recs = tw._solve(qp, case, th)
    rrecs = qp.row_launch_info(rseq)
    assert len(rrecs) == 1, rrecs
    r = rrecs[0]
    assert (r["real_bytes"], r["S"], r["NS"], r["MS"], r["CAPP"], r["BNB"]) == e["inst"], (r, e)
    assert (r["pass"], r["cap"], r["nwv"], r["blocks"], r["ps"], r["lds"], r["aux"]) == \
        (1, 31, e["nwv"], e["blocks"], e["ps"], e["lds"], e["aux"]), (r, e)
    assert (r["worklist"], r["queue"], r["qchunk"], r["nprob"], r["snap_bytes"]) == (0, 0, 1, N, 0), r
    assert 1 <= r["grid"] <= -(-N // (4 * r["nwv"])), r
    _expect(recs, case, (2,), (case.cap,), False, "4: row kernel")
    level = next(lv for lv in (3, 2, 1) if wc.fits(case, lv, False, 2))
    assert (recs[0]["level"], recs[0]["nwv"]) == (level, 2), ("4: the second pass's preference", recs)
    tw._same(got, ref, N, "4: row kernel")
    # 5: the binary32 entry point
    opts()
    got, recs = tw._solve(qp, case32, th)
    _expect(recs, case32, (0,), (case.cap,), False, "5: binary32")
    tw._same(got, ref32, N, "5: binary32")
    # 6: warm-started
    got, recs = tw._solve(qp, case, th, warm=warm)
    _expect(recs, case, (0,), (case.cap,), False, "6: warm")
    assert _words(recs) == _words(recs1), ("6: warm", recs, recs1)
    tw._same(got, refw, N, "6: warm")
    # 7: profiling on
    qp.profile(True)
    try:
        got, recs = tw._solve(qp, case, th)
    finally:
        qp.profile(False)
    assert qp.profile_read()[0] == 1
    _expect(recs, case, (0,), (case.cap,), False, "7: profiling")
    assert _words(recs) == _words(recs1), ("7: profiling", recs, recs1)
    tw._same(got, ref, N, "7: profiling")
    # 8: as step 1
    opts()
    last, recs8 = tw._solve(qp, case, th)
    _expect(recs8, case, (0,), (case.cap,), False, "8: one pass again")
    assert _words(recs8) == _words(recs1), ("8: the records of step 1", recs8, recs1)
    tw._same(last, ref, N, "8: one pass again")
    for a, b in zip(last, first):
        assert np.array_equal(a, b)
    qp.check()


def test_lane_handle_forms_in_turn(lmpc):
    case = lc.BY_NAME["box5-nth4-fast0"]
    qp = tl._handle(lmpc, case)                               # ("fast" 0: screening pass + lane kernel)
    ref, refw = tl._ref(case, qp), tl._ref_warm(case, qp)
    th = lc.theta(case, lc.N_COND)[:N]
    warm = np.ascontiguousarray(ref[3][:N])
    first = tl._solve(qp, th)
    tl._same(first, ref, N, "screened")
    qp.set_option("fast", 1)
    assert qp.kernel_name.startswith("fast<"), qp.kernel_name
    tl._same(tl._solve(qp, th), ref, N, "one-launch kernel")
    qp.set_option("fast", 0)
    tl._same(tl._solve(qp, th), ref, N, "screened after the one-launch kernel")
    tl._same(tl._solve(qp, th, warm=warm), refw, N, "warm")
    last = tl._solve(qp, th)
    tl._same(last, ref, N, "screened again")
    for a, b in zip(last, first):
        assert np.array_equal(a, b)
    qp.check()
