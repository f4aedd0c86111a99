"""The row path -- row_kernel<R, S, NS, MS, CAPP, BNB> (lmpc_row_kernel.hpp), launched by launch_row / launch_row_bnb
(lmpc_row_inst.hip): four problems per wavefront -- at every one of its 18 instantiations, against the oracle on the
handle's own pack, bit for bit: np.array_equal on x, exitflag, iters and active, on every point of every batch.  The
reference is the oracle (binary64, and its binary32 build), never the wavefront kernel.  Cases and the conditions that
keep a comparison from passing emptily: tests/row_cases.py (checked on the host in tests/test_row_cases_host.py,
re-asserted here on the oracle's outputs for the handle's pack).

Every test first reads the handle's launch records and asserts them against the case: lmpc_row_launch_info must show
exactly one row-kernel launch per call, of the instantiation, pass, capacity and launch shape the table expects; where
that launch is the first of two passes, lmpc_wave_launch_info must show exactly one wavefront-kernel launch behind it:
pass 2, walking a work list, at the problem's capacity.  "row_kernel" 1 is a request -- a call the dispatch does not
hand to the row kernel would compare the wavefront kernel with the oracle and pass; the record turns that into a
failure.  The refusals the dispatch documents are pinned the other way round: no row launch may show.

Every output of a device call is allocated with GUARD rows behind row N and pre-filled with sentinels; the guard rows
must come back untouched and no sentinel may survive in rows 0 ... N - 1."""
import re
from dataclasses import replace

import numpy as np
import pytest

import loop_reference as lr
import row_cases as rc
import wave_cases as wc
from conftest import oracle_ldp_from
from test_gpu_wave import _Guarded, _cached, _oset, _same

pytestmark = pytest.mark.gpu

ids = lambda c: c.name
PINS = (("qp_tiers", 0), ("screen_wave", 0), ("wave_probe", 0))
SEEN = set()                               # instantiations the records of this module showed (the coverage test reads it)


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _settings(lmpc, case, iter_limit=None):
    s = lmpc.default_settings_f32() if case.f32 else lmpc.default_settings()
    if case.w.iter_limit or iter_limit:
        s.iter_limit = iter_limit or case.w.iter_limit
    return s


def _handle(lmpc, case, prob=None, options=None, iter_limit=None):
    H, f, f_theta, A, bu, bl, W, sense = rc.problem(case) if prob is None else prob
    s = _settings(lmpc, case, iter_limit)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, senses=sense, nout=case.nout, settings=s)
    qp.set_option("wave", 1)
    for k, v in PINS + (rc.options_for(case) if options is None else tuple(options)):
        qp.set_option(k, v)
    assert (qp.n, qp.m, qp.nth, qp.nout) == (case.n, case.m, case.w.nth, case.nout)
    qp._oset = _oset(s)
    return qp


def _seqs(qp):
    r, w = qp.row_launch_info(), qp.wave_launch_info()
    return (r[-1]["seq"] if r else 0), (w[-1]["seq"] if w else 0)


def _solve(qp, case, th, warm=None):
    """One lmpc_solve_batch[_f32]_device call on guarded outputs: ((x, exitflag, iters, active), row records, wave records)."""
    import torch
    N = len(th)
    rs, ws = _seqs(qp)
    th_d = torch.from_numpy(np.ascontiguousarray(th, dtype=case.dtype)).cuda()
    g = _Guarded(N, qp.nout, qp.words, case.f32)
    w_d = None if warm is None else torch.from_numpy(np.array(warm).view(np.int64)).cuda()
    qp.solve_device(th_d, x=g.x[:N], exitflag=g.ef[:N], iters=g.it[:N], active=g.act[:N], warm=w_d)
    torch.cuda.synchronize()
    return g.read(), qp.row_launch_info(rs), qp.wave_launch_info(ws)


def _expect(rrecs, wrecs, case, N, what="", blocks=None, worklist=0, e=None):
    """The records of one call against the table: ONE row launch of the expected instantiation, pass, capacity and launch
    shape; behind a first pass ONE wavefront-kernel launch, pass 2 on the overflow list at the problem's capacity."""
    e = rc.expected(case) if e is None else e
    assert e is not None, (what, "the table expects no row launch")
    assert len(rrecs) == 1, (what, "row launches of the call", rrecs, wrecs)
    r = rrecs[0]
    got = (r["real_bytes"], r["S"], r["NS"], r["MS"], r["CAPP"], r["BNB"])
    assert got == e["inst"], (what, "instantiation", got, e["inst"], r)
    SEEN.add(got)
    assert (r["pass"], r["cap"]) == (e["pass"], e["cap"]), (what, "pass / capacity", r, e)
    assert (r["nwv"], r["ps"], r["lds"], r["aux"]) == (e["nwv"], e["ps"], e["lds"], e["aux"]), (what, "launch shape", r, e)
    assert r["blocks"] == (e["blocks"] if blocks is None else blocks), (what, "workgroups per CU", r, e)
    need = -(-N // (4 * r["nwv"]))
    assert r["nprob"] == N and 1 <= r["grid"] <= need and (r["grid"] == need or r["grid"] % r["blocks"] == 0), (what, r)
    assert r["worklist"] == worklist and r["qchunk"] >= 1, (what, r)
    if case.bnb:
        S, CAPP = e["shape"][0], e["shape"][3]
        per = case.w.nbin * (case.rs * rc.row_snap_reals(S, CAPP) + 4 * rc.row_snap_ints(S))
        assert r["snap_bytes"] >= per * r["grid"] * r["nwv"] * 4, (what, "snapshot scratch", r, per)
    else:
        assert r["snap_bytes"] == 0
    if e["pass"] == 1:
        assert len(wrecs) == 1, (what, "a second pass on the wavefront kernel", wrecs)
        w = wrecs[0]
        assert (w["pass"], w["worklist"], w["cap"], w["BNB"], w["real_bytes"], w["nprob"]) == \
            (2, 1, case.full, int(case.bnb), case.rs, N), (what, "second pass", w)
        assert w["big"] == (0 if case.bnb else 1), (what, "slow path behind the second pass", w)
    else:
        assert not wrecs, (what, "the only pass", wrecs)
    return r


def _no_row(rrecs, wrecs, what):
    assert not rrecs, (what, "a row launch where the dispatch documents a refusal", rrecs)
    assert wrecs, (what, "the wavefront kernel takes the batch")


def _ldp(qp):
    return oracle_ldp_from(qp.ldp())


def _oracle(qp, case, th, warm=None):
    from oracle import ldp as oldp
    return oldp.solve_batch(_ldp(qp), th, qp._oset, warm=warm, dtype=case.dtype)


def _ref(case, qp):
    """The oracle on the handle's pack for the case's condition batch, computed once and never written to; a smaller
    batch is a prefix of it.  The conditions are asserted on what it returns."""
    def make():
        th = rc.theta(case)
        out = _oracle(qp, case, th)
        if case.bnb:
            Lr = replace(_ldp(qp), sense=(_ldp(qp).sense & ~wc.SENSE_BINARY).astype(np.int32))
            from oracle import ldp as oldp
            itr = oldp.solve_batch(Lr, th, qp._oset, dtype=case.dtype)[2]
            print(case.name, rc.check_search_conditions(case, out[1], out[2], itr, out[3]))
        elif case.w.nth == 0:
            print(case.name, wc.check_nth0(case.w, out[1], out[2], out[3]))
        else:
            print(case.name, rc.check_row_conditions(case, out[1], out[2], out[3]))
        return out
    return _cached((case, "row-cold"), make)


# ------------------------------------------------------------------ plain form
@pytest.mark.parametrize("case", rc.PLAIN + rc.PLAIN_F32 + (rc.NTH0, rc.NTH0_F32), ids=ids)
def test_plain_form_condition_batch(lmpc, case):
    """Every plain case and its binary32 twin on the condition batch: the record first, then the oracle, twice on the
    handle (the counter sets alternate)."""
    qp = _handle(lmpc, case)
    ref = _ref(case, qp)
    th = rc.theta(case)
    for k in range(2):
        got, rr, wr = _solve(qp, case, th)
        _expect(rr, wr, case, wc.N_COND, (case.name, k))
        _same(got, ref, wc.N_COND, (case.name, k))
    qp.check()


@pytest.mark.parametrize("case", rc.PLAIN + rc.PLAIN_F32, ids=ids)
def test_plain_form_batch_sizes(lmpc, case):
    """1 ... 5 problems (rows of a wavefront without a problem), a workgroup less one, full, plus one, and a ragged 333:
    nwv from the record; all prefixes of the cached reference."""
    qp = _handle(lmpc, case)
    ref = _ref(case, qp)
    th = rc.theta(case)
    got, rr, wr = _solve(qp, case, th[:1])
    nwv = _expect(rr, wr, case, 1, (case.name, 1))["nwv"]
    _same(got, ref, 1, (case.name, 1))
    for N in rc.batch_sizes(nwv)[1:]:
        got, rr, wr = _solve(qp, case, th[:N])
        _expect(rr, wr, case, N, (case.name, N))
        _same(got, ref, N, (case.name, N))
    qp.check()


@pytest.mark.parametrize("name", rc.NOUT_CASES)
def test_several_outputs(lmpc, name):
    """nout = n / 2 and n, both real types: outputs beyond the first go through the affine map per output."""
    for base in (rc.BY_NAME[name], rc.BY_NAME[name + "-f32"]):
        for nout in (base.n // 2, base.n):
            case = replace(base, nout=nout)
            qp = _handle(lmpc, case)
            ref = _ref(case, qp)
            assert ref[0].shape == (wc.N_COND, nout)
            got, rr, wr = _solve(qp, case, rc.theta(case)[:333])
            _expect(rr, wr, case, 333, (case.name, nout))
            _same(got, ref, 333, (case.name, nout))
            qp.check()


@pytest.mark.parametrize("kind", ["all-infeasible", "all-settled"])
@pytest.mark.parametrize("name", rc.LIMIT_BATCH_CASES)
def test_limit_batches(lmpc, name, kind):
    """A batch that is infeasible throughout and one settled at iteration 1 throughout, both real types."""
    for case in (rc.BY_NAME[name], rc.BY_NAME[name + "-f32"]):
        qp = _handle(lmpc, case)
        th = wc.limit_theta(case.w, kind)
        ref = _cached((case, kind), lambda: _oracle(qp, case, th))
        wc.check_limit_batch(case.w, ref[1], ref[2], ref[3], kind)
        got, rr, wr = _solve(qp, case, th)
        _expect(rr, wr, case, wc.N_COND, (case.name, kind))
        _same(got, ref, wc.N_COND, (case.name, kind))
        qp.check()


# ------------------------------------------------------------------ two passes
@pytest.mark.parametrize("kind", ["none", "all"])
@pytest.mark.parametrize("name", rc.SHARE_CASES)
def test_first_pass_none_and_all_outgrow_it(lmpc, name, kind):
    """The first-pass cases (16 rows on {1, 4, 10, 16}, 31 on {2, 4, 10, 31}, 32 on {2, 4, 10, 32}, 8 on the one- and
    two-slot shapes) with batches of which no point / every point outgrows the first pass (mixed: the condition batches
    of test_plain_form_condition_batch): pass 1 at the intended capacity, a listed second pass behind it."""
    for case in (rc.BY_NAME[name], rc.BY_NAME[name + "-f32"]):
        qp = _handle(lmpc, case)
        th = rc.theta(case, batch=2, scales=rc.SHARE_SCALES[kind])
        ref = _cached((case, "share", kind), lambda: _oracle(qp, case, th))
        e = rc.expected(case)
        print(case.name, kind, rc.check_share(case, ref[3], e["cap"], kind))
        assert e["pass"] == 1
        got, rr, wr = _solve(qp, case, th)
        _expect(rr, wr, case, wc.N_COND, (case.name, kind))
        _same(got, ref, wc.N_COND, (case.name, kind))
        qp.check()


# ------------------------------------------------------------------ work-list mode, ticket queue
def _tiled(ref, N):
    reps = -(-N // wc.N_COND)
    return tuple(np.ascontiguousarray(np.concatenate([a] * reps)[:N]) for a in ref)


def test_work_list_mode_behind_the_tiers_pass(lmpc):
    """ "qp_tiers" 1 (n <= 12, m <= 64, binary64): the row kernel walks the list of what the tiers pass left -- the shape
    {1, 1, 4, 16}.  That pass sends tile t (64 points) to segment t % 64 and certainly leaves the points that remove a
    row again: at N_COND the segments 7 ... 63 stay empty and one holds FLOOR such points, at 64 x 256 + 300 points
    every segment does (row_cases.check_segments on the oracle's outputs, as behind the screening pass)."""
    case = rc.LIST_TIERS
    qp = _handle(lmpc, case, options=(("row_kernel", 1), ("qp_tiers", 1)))
    assert qp.kernel_name.startswith("qp_tiers<"), qp.kernel_name
    ref = _ref(case, qp)
    for N, kind in ((wc.N_COND, "some-empty"), (wc.N_FILL, "all-filled")):
        th = np.ascontiguousarray(np.concatenate([rc.theta(case)] * (-(-N // wc.N_COND)))[:N])
        want = _tiled(ref, N)
        removing = (want[2] > wc.popcount(want[3]) + 1) & (want[1] >= 1)
        print(kind, rc.check_segments(removing, kind, rc.TIERS_BLOCK))
        if kind == "some-empty":
            assert not np.bincount((np.arange(N) // 64) % 64, weights=removing, minlength=64)[7:].any()
        got, rr, wr = _solve(qp, case, th)
        r = _expect(rr, wr, case, N, (case.name, N), worklist=1)
        assert r["queue"] == 1 and r["qchunk"] == 1, r
        _same(got, _tiled(ref, N), N, (case.name, N))
    qp.check()


def test_work_list_mode_behind_the_screening_pass(lmpc):
    """ "screen_wave" 1 on the ten-slot class: the row kernel walks the 64 segments the screening pass filled -- a batch
    that leaves segments empty and one that fills every segment (wave_cases.check_segments)."""
    case = rc.LIST_SCREEN
    qp = _handle(lmpc, case, options=(("row_kernel", 1), ("screen_wave", 1)))
    ref = _ref(case, qp)
    for N, kind in ((2309, "some-empty"), (wc.N_FILL, "all-filled")):
        th = np.ascontiguousarray(np.concatenate([rc.theta(case)] * (-(-N // wc.N_COND)))[:N])
        want = _tiled(ref, N)
        print(kind, rc.check_segments(want[2], kind, wc.SCREEN_BLOCK))
        got, rr, wr = _solve(qp, case, th)
        r = _expect(rr, wr, case, N, (case.name, kind), worklist=1)
        assert r["queue"] == 1 and r["qchunk"] == 1, r
        _same(got, want, N, (case.name, kind))
    qp.check()


def test_ticket_queue_against_the_static_split(lmpc):
    """ "row_blocks" 1 on the narrowest shape: the smallest batch at which the record reports the ticket queue in use
    (more than two problems per row of the grid), the batch one smaller (static split), and one at which a ticket hands
    out two problems; "wave_queue" 0 splits the same batches statically.  The batch is the condition batch tiled."""
    import torch
    case = rc.QUEUE
    qp = _handle(lmpc, case, options=(("row_kernel", 1), ("row_blocks", 1)))
    ref = _ref(case, qp)
    e = rc.expected(case)
    rows = torch.cuda.get_device_properties(0).multi_processor_count * e["nwv"] * 4
    for N, queue, qchunk in ((2 * rows, 0, 1), (2 * rows + 1, 1, 1), (64 * rows, 1, 2)):
        th = np.ascontiguousarray(np.concatenate([rc.theta(case)] * (-(-N // wc.N_COND)))[:N])
        want = _tiled(ref, N)
        for on in (1, 0):
            qp.set_option("wave_queue", on)
            got, rr, wr = _solve(qp, case, th)
            r = _expect(rr, wr, case, N, (case.name, N, on), blocks=1)
            assert r["grid"] * r["nwv"] * 4 == rows and (r["queue"], r["qchunk"]) == ((queue, qchunk) if on else (0, 1)), (N, on, r)
            _same(got, want, N, (case.name, N, on))
    qp.check()


# ------------------------------------------------------------------ searches
@pytest.mark.parametrize("case", rc.BNB, ids=ids)
def test_searches(lmpc, case):
    """Every search case in both real types at 1, 3, 4 nwv + 1 and N_COND searches on ONE handle, smallest first: the
    snapshot scratch is regrown with the grid (the record's snap_bytes).  One pass on {1, 1, 2, 16}, {3, 4, 4, 44} and
    {3, 4, 4, 48}; first passes by the default rule (44 / 48 rows) and at "wave_cap1" 20, which lists most searches for
    the wavefront kernel's second pass."""
    qp = _handle(lmpc, case)
    ref = _ref(case, qp)
    th = rc.theta(case)
    nwv = rc.expected(case)["nwv"]
    snap = []
    for N in (1, 3, 4 * nwv + 1, wc.N_COND):
        got, rr, wr = _solve(qp, case, th[:N])
        r = _expect(rr, wr, case, N, (case.name, N))
        snap.append(r["snap_bytes"])
        _same(got, ref, N, (case.name, N))
    assert snap == sorted(snap) and snap[-1] > snap[0], ("the snapshot scratch grows with the grid", snap)
    qp.release_scratch()
    got, rr, wr = _solve(qp, case, th[:3])
    r = _expect(rr, wr, case, 3, (case.name, "after release_scratch"))
    assert r["snap_bytes"] == snap[1], (r, snap)
    _same(got, ref, 3, (case.name, "after release_scratch"))
    qp.check()


@pytest.mark.parametrize("case", [rc.DEEP_STACK, rc.DEEP_STACK_F32], ids=ids)
def test_search_stack_beyond_32_levels(lmpc, case):
    """34 binaries whose relaxation leaves (nearly) all of them free at the root: leaves 33 and 34 levels deep, stack
    entries in the third register slot, both sides tried first there.  8 searches of ~1e5 iterations each."""
    from oracle import ldp as oldp
    qp = _handle(lmpc, case)
    th = rc.theta(case, rc.N_DEEP_STACK)

    def make():
        out = _oracle(qp, case, th)
        Lr = replace(_ldp(qp), sense=(_ldp(qp).sense & ~wc.SENSE_BINARY).astype(np.int32))
        rel = oldp.solve_batch(Lr, th, qp._oset, dtype=case.dtype)[3]
        print(case.name, rc.check_deep_stack(case, out[1], out[3], rel))
        return out
    ref = _cached((case, "deep-stack"), make)
    got, rr, wr = _solve(qp, case, th)
    _expect(rr, wr, case, rc.N_DEEP_STACK, case.name)
    _same(got, ref, rc.N_DEEP_STACK, case.name)
    qp.check()


# ------------------------------------------------------------------ sequences on one handle
def test_cold_row_off_cold_again(lmpc):
    """cold -> "row_kernel" 0 -> cold again, lmpc_release_scratch in between: the record shows the row launch, none,
    the row launch."""
    for case in (rc.BY_NAME["s2-n17-m90-nth4"], rc.BY_NAME["t2-n33-m150-nth5-f32"]):
        qp = _handle(lmpc, case)
        ref = _ref(case, qp)
        th = rc.theta(case)
        for k, on in enumerate((1, 0, 1, 1, 0, 1)):
            qp.set_option("row_kernel", on)
            N = (wc.N_COND, 333, 65, wc.N_COND, 5, 333)[k]
            got, rr, wr = _solve(qp, case, th[:N])
            if on:
                _expect(rr, wr, case, N, (case.name, k))
            else:
                _no_row(rr, wr, (case.name, k))
            _same(got, ref, N, (case.name, k))
            if k == 2:
                qp.release_scratch()
        qp.check()


def test_first_passes_of_different_capacities_alternate(lmpc):
    """A first pass of 8 rows that most points outgrow between calls at the problem's capacity, and the only-pass form
    ("big_path" 0: nothing lies behind the capacity, pass 0) in between: the overflow counter sets alternate per call and
    every call clears the next one's."""
    base = rc.BY_NAME["s2-n24-m96-nth4-c8"]
    full = replace(base, mode="full", cap1=0, share="")
    qp = _handle(lmpc, full)
    th = rc.theta(base)
    ref = _ref(base, qp)
    assert (wc.popcount(ref[3]) <= base.full).all()
    e_only = dict(rc.expected(full), **{"pass": 0})
    for k, mode in enumerate(("full", "c8", "full", "only", "c8", "c8", "only", "full", "c8", "only")):
        qp.set_option("big_path", 0 if mode == "only" else 1)
        qp.set_option("wave_two_pass", 1 if mode == "c8" else -1)
        qp.set_option("wave_cap1", 8)
        got, rr, wr = _solve(qp, base, th)
        if mode == "only":
            _expect(rr, wr, full, wc.N_COND, (k, mode), e=e_only)
        else:
            _expect(rr, wr, base if mode == "c8" else full, wc.N_COND, (k, mode))
        _same(got, ref, wc.N_COND, (k, mode))
    qp.check()


def test_binary64_and_binary32_handles_interleaved(lmpc):
    c64 = rc.BY_NAME["t2-n48-m160-nth5"]
    c32 = rc.BY_NAME["t2-n48-m160-nth5-f32"]
    q64, q32 = _handle(lmpc, c64), _handle(lmpc, c32)
    r64, r32 = _ref(c64, q64), _ref(c32, q32)
    for k in range(4):
        for qp, case, ref in ((q64, c64, r64), (q32, c32, r32))[::(1 if k % 2 == 0 else -1)]:
            N = (wc.N_COND, 65, 333, 1)[k]
            got, rr, wr = _solve(qp, case, rc.theta(case, N))
            _expect(rr, wr, case, N, (case.name, k))
            _same(got, ref, N, (case.name, k))
        if k == 1:
            q64.release_scratch()
            q32.release_scratch()
    q64.check()
    q32.check()


# ------------------------------------------------------------------ refusals
def test_refusals_are_visible(lmpc):
    """Every reason for which row_pass_cap / row_bnb_pass_cap / row_launch_for hand a batch back to the wavefront
    kernel although "row_kernel" 1 asks for the row kernel: the record shows NO row launch, the result is the oracle's.
    (A change of the dispatch's boundary shows here.)"""
    case = rc.BY_NAME["s2-n17-m90-nth4"]
    th = rc.theta(case)
    qp = _handle(lmpc, case)
    ref = _ref(case, qp)
    got, rr, wr = _solve(qp, case, th)
    _expect(rr, wr, case, wc.N_COND, "the case itself runs on the row kernel")
    # a warm call
    w = wc.warm_masks(ref[1], ref[3])
    got, rr, wr = _solve(qp, case, th, warm=w)
    _no_row(rr, wr, "warm")
    _same(got, _oracle(qp, case, th, warm=w), wc.N_COND, "warm")
    # the Gram form
    qp.set_option("gram_scan", 1)
    got, rr, wr = _solve(qp, case, th)
    _no_row(rr, wr, "gram_scan")
    assert all(r["GRAM"] == 1 for r in wr), wr
    from oracle import ldp as oldp
    so = _oset(_settings(lmpc, case))
    so.mode = 1                                              # (the oracle's Gram form: tests/test_gpu_gram.py)
    _same(got, oldp.solve_batch(_ldp(qp), th, so, dtype=case.dtype), wc.N_COND, "gram_scan")
    qp.set_option("gram_scan", 0)
    # "row_kernel" 0
    qp.set_option("row_kernel", 0)
    got, rr, wr = _solve(qp, case, th)
    _no_row(rr, wr, "row_kernel 0")
    _same(got, ref, wc.N_COND, "row_kernel 0")
    qp.set_option("row_kernel", 1)
    got, rr, wr = _solve(qp, case, th)
    _expect(rr, wr, case, wc.N_COND, "the row kernel again")
    qp.check()
    # a closed loop (kept factor, fused plant step): lmpc_simulate on a handle the row kernel covers
    cl = rc.BY_NAME["s1-n10-m49-nth5"]
    ql = _handle(lmpc, replace(cl, nout=2), options=(("row_kernel", 1), ("screen_wave", 1)))
    F, G, x0 = wc.sim_data(cl.w)
    for warm in (False, True):
        rs, ws = _seqs(ql)
        out = ql.simulate(x0, wc.T_LOOP, F, G, warm=warm)
        _no_row(ql.row_launch_info(rs), ql.wave_launch_info(ws), ("closed loop", warm))
        # (warm on the kept factorisation: the oracle's warm == 2)
        want = oldp.simulate(_ldp(ql), x0, wc.T_LOOP, F, G, settings=ql._oset, warm=2) if warm else \
            lr.simulate_reference(_ldp(ql), x0, wc.T_LOOP, F, G, warm=False, settings=ql._oset)
        for key in ("U", "X", "x", "flag_min"):
            assert np.array_equal(out[key], want[key]), ("closed loop", warm, key)
    ql.check()
    # an ACTIVE row (an equality)
    H, f, f_theta, A, bu, bl, W, sense = rc.problem(case)
    bu[case.n + 5] = bl[case.n + 5] = 0.1
    sense[case.n + 5] = 5
    qa = _handle(lmpc, case, prob=(H, f, f_theta, A, bu, bl, W, sense))
    got, rr, wr = _solve(qa, case, th)
    _no_row(rr, wr, "ACTIVE row")
    _same(got, _oracle(qa, case, th), wc.N_COND, "ACTIVE row")
    # an iteration limit below 2
    q1 = _handle(lmpc, case, iter_limit=1)
    got, rr, wr = _solve(q1, case, th)
    _no_row(rr, wr, "iter_limit 1")
    _same(got, _oracle(q1, case, th), wc.N_COND, "iter_limit 1")
    # capacity beyond 32 rows without the slow path, and with "wave_two_pass" 0
    big = rc.BY_NAME["t2-n48-m160-nth5"]
    for opt in (("big_path", 0), ("wave_two_pass", 0)):
        qb = _handle(lmpc, big, options=(("row_kernel", 1), opt))
        got, rr, wr = _solve(qb, big, rc.theta(big))
        _no_row(rr, wr, opt)
        _same(got, _ref(big, qb), wc.N_COND, opt)
    # no covering shape (m > 160); no LDS size that fits (n = 64, m = 160, 40 parameters, 64 outputs)
    for c in (rc.REFUSE_M, rc.REFUSE_WIDE):
        assert rc.expected(c) is None
        qc = _handle(lmpc, c)
        got, rr, wr = _solve(qc, c, rc.theta(c))
        _no_row(rr, wr, c.name)
        _same(got, _oracle(qc, c, rc.theta(c)), wc.N_COND, c.name)
    # more binaries than the search's depth on the row kernel (48 > 47); 16 searches
    c = rc.REFUSE_BIN
    qc = _handle(lmpc, c)
    thb = rc.theta(c, 16)
    got, rr, wr = _solve(qc, c, thb)
    _no_row(rr, wr, c.name)
    assert all(r["BNB"] == 1 for r in wr)
    _same(got, _oracle(qc, c, thb), 16, c.name)


# ------------------------------------------------------------------ coverage (runs last in the file)
def test_every_instantiation_of_the_library_was_launched():
    """The union of the instantiations the records of this module showed = the 18 the table claims = the row_kernel
    instantiations named by the built library's symbol table (names only).  It reads what the tests above recorded: it
    holds only when the whole module has run, in file order, in one process (not under -k, not spread over workers)."""
    assert len(rc.built()) == 18 and SEEN == rc.built(), ("instantiations never launched", sorted(rc.built() - SEEN),
                                                          "launched and not in the table", sorted(SEEN - rc.built()))
    from test_fast_fallback import LIB, _kernel_vgprs
    built = set()
    for k in _kernel_vgprs(LIB, r"4lmpc10row_kernelI[df]"):
        m = re.search(r"10row_kernelI([df])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE", k)
        assert m, k
        R, S, NS, MS, CAPP, B = m.groups()
        built.add((8 if R == "d" else 4, int(S), int(NS), int(MS), int(CAPP), int(B)))
    assert len(built) == 18 and built == rc.built(), sorted(built ^ rc.built())
    assert SEEN == built, ("instantiations never launched", sorted(built - SEEN), "launched and not built", sorted(SEEN - built))
