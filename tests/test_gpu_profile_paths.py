"""lmpc_profile / lmpc_profile_read on every form of the batched-solve dispatch that brackets its launches with timing
events: the wavefront kernel alone, behind the screening pass, behind the tiers pass, behind the row kernel, in its own
two passes, a search, the lane path behind the screening pass, and an is_avi handle.  (The one-launch kernel's bracket:
tests/test_gpu_fast.py, test_profile_shows_one_launch.)

Per form: one warm-up call, profiling on, three calls, one read -- three timed calls with a positive total, both parts
inside it, and both parts positive where a front pass runs before the iterating kernel; a second read is empty; with
profiling off three further calls leave nothing to read.  Every call's results are compared with the oracle on the
handle's own pack, bit for bit, as the tests of the paths themselves do.  Cases: tests/wave_cases.py,
tests/row_cases.py, tests/lane_cases.py and the game_kat fixture."""
import numpy as np
import pytest

import lane_cases as lc
import row_cases as rc
import test_gpu_lane as tl
import test_gpu_row as tr
import test_gpu_wave as tw
import wave_cases as wc
from conftest import load_golden

pytestmark = pytest.mark.gpu

N = 300


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _profiled(qp, call, front, what):
    """`call` solves one batch and compares it with the oracle."""
    call()                                                   # (first call on the handle: allocations, code load)
    qp.profile(True)
    try:
        for _ in range(3):
            call()
        cnt, total, screen, iterate = qp.profile_read()
        print(what, cnt, total, screen, iterate)
        assert cnt == 3 and total > 0.0, (what, cnt, total)
        assert 0.0 <= screen <= total and 0.0 <= iterate <= total, (what, total, screen, iterate)
        if front:
            assert screen > 0.0 and iterate > 0.0, (what, screen, iterate)
        assert qp.profile_read()[0] == 0, (what, "a second read")
    finally:
        qp.profile(False)
    for _ in range(3):
        call()
    assert qp.profile_read()[0] == 0, (what, "calls with profiling off")
    qp.check()


def _wave_form(lmpc, case, options, th, front, what, records):
    qp = tw._handle(lmpc, case)
    for k, v in options:
        qp.set_option(k, v)
    ref = tw._cached((case, what), lambda: tw._oracle(qp, case, th))

    def call():
        got, recs = tw._solve(qp, case, th)
        records(recs)
        tw._same(got, ref, len(th), what)
    _profiled(qp, call, front, what)


def test_wavefront_kernel_alone(lmpc):
    case = wc.QUEUE

    def records(recs):
        assert [(r["pass"], r["worklist"]) for r in recs] == [(0, 0)], recs
    _wave_form(lmpc, case, (), wc.theta(case, N), False, "wavefront kernel alone", records)


def test_screening_pass_and_wavefront_kernel(lmpc):
    case = wc.QUEUE

    def records(recs):
        assert [(r["pass"], r["worklist"]) for r in recs] == [(0, 1)], recs
    _wave_form(lmpc, case, (("screen_wave", 1),), wc.theta(case, N), True, "screening pass + wavefront kernel", records)


def test_wavefront_kernel_in_two_passes(lmpc):
    case = wc.TWO_PASS

    def records(recs):
        assert [(r["pass"], r["cap"]) for r in recs] == [(1, 24), (2, case.cap)], recs
    _wave_form(lmpc, case, (("wave_two_pass", 1), ("wave_cap1", 24)), wc.two_pass_theta("mixed")[:N], False,
               "wavefront kernel in two passes", records)


def test_search(lmpc):
    case = wc.BNB_CASES[0]

    def records(recs):
        assert [(r["pass"], r["BNB"]) for r in recs] == [(0, 1)], recs
    _wave_form(lmpc, case, (), wc.theta(case, N), False, "branch and bound", records)


def _row_form(lmpc, case, options, front, what, records, front_record=None):
    qp = tr._handle(lmpc, case, options=options)
    th = rc.theta(case)[:N]
    ref = tr._ref(case, qp)

    def call():
        seq = (qp.front_pass_info() or [dict(seq=0)])[-1]["seq"]
        got, rr, wr = tr._solve(qp, case, th)
        records(rr, wr)
        if front_record is not None:
            front_record(qp, qp.front_pass_info(seq))
        tr._same(got, ref, N, what)
    _profiled(qp, call, front, what)


def test_tiers_pass_and_wavefront_kernel(lmpc):
    case = rc.LIST_TIERS

    def records(rr, wr):
        assert not rr and [(r["pass"], r["worklist"]) for r in wr] == [(0, 1)], (rr, wr)

    def front_record(qp, recs):                              # (lmpc_front_pass_info: ONE tiers launch, the wavefront kernel behind it)
        assert [(r["kind"], r["N"], r["nprob"], r["walker"]) for r in recs] == [(qp.FRONT_TIERS, case.n, N, qp.WALK_WAVE)], recs
    qp_opts = (("row_kernel", 0), ("qp_tiers", 2))
    _row_form(lmpc, case, qp_opts, True, "tiers pass + wavefront kernel", records, front_record)


def test_row_kernel_as_the_first_of_two_passes(lmpc):
    case = rc.BY_NAME["s2-n32-m96-nth5"]
    assert rc.expected(case)["pass"] == 1

    def records(rr, wr):
        tr._expect(rr, wr, case, N, "row kernel, first of two passes")
    _row_form(lmpc, case, None, False, "row kernel + wavefront kernel", records)


def test_lane_path_behind_the_screening_pass(lmpc):
    case = lc.BY_NAME["box5-nth4-fast0"]
    assert ("fast", 0) in case.opts
    qp = tl._handle(lmpc, case)
    ref = tl._ref(case, qp)
    th = lc.theta(case, lc.N_COND)[:N]
    _profiled(qp, lambda: tl._same(tl._solve(qp, th), ref, N, "lane path"), True, "screening pass + lane kernel")


def test_avi_handle(lmpc):
    import torch
    from oracle import avi as oavi
    from test_gpu_parity import _avi_oracle_pack, _qp_from_golden
    g = load_golden("game_kat")
    qp = _qp_from_golden(lmpc, g)
    assert qp.is_avi
    th = np.ascontiguousarray(g["theta"][:N])
    ref = oavi.solve_batch(_avi_oracle_pack(qp), th)
    th_d = torch.from_numpy(th).cuda()

    def call():
        it = torch.empty(len(th), dtype=torch.int32, device="cuda:0")
        act = torch.zeros((len(th), qp.words), dtype=torch.int64, device="cuda:0")
        x, ef = qp.solve_device(th_d, iters=it, active=act)
        torch.cuda.synchronize()
        got = (x.cpu().numpy(), ef.cpu().numpy(), it.cpu().numpy(), act.cpu().numpy().view(np.uint64))
        for a, r in zip(got, ref):
            assert np.array_equal(a, r)
    _profiled(qp, call, False, "avi")
