"""The tiers pass -- qp_tiers_kernel<N> (lmpc_qp_tiers_kernel.hpp), N = 2 ... 12 -- at every instantiation, against
the oracle on the handle's own pack, bit for bit: np.array_equal on x (failed points too), exitflag, iters and active.
Cases, the restated launch arithmetic, the rule for what the pass must finish and the conditions that keep a comparison
from passing emptily: tests/tiers_cases.py (checked on the host in tests/test_tiers_cases_host.py, re-asserted here on
the oracle's outputs for the handle's pack).

The kernel behind the pass solves whatever is queued from scratch to the same bits, so equal outputs do not show that
the pass did anything.  Every test therefore
  1. reads the handle's front-pass record (lmpc_front_pass_info) FIRST and asserts kind, N, LDS bytes, workgroups (the
     restated arithmetic with the device's CU count) and the kernel that walks the list;
  2. compares the bits;
  3. reads the snapshot of the pass's work list ("list_snapshot" 1, lmpc_work_list_read) and asserts that, segment by
     segment, it holds exactly the points tiers_cases.must_finish() says the pass cannot finish: no tolerance on a count.

Every output of a device call is allocated with GUARD rows behind row N and pre-filled with sentinels; the guard rows
must come back untouched and no sentinel may survive in rows 0 ... N - 1."""
import warnings

import numpy as np
import pytest

import row_cases as rc
import tiers_cases as tc
from conftest import oracle_ldp_from

pytestmark = pytest.mark.gpu

SENT = 12345
ACT_SENT = 0x5A5A5A5A5A5A5A5A              # (32 bits set in a word: more rows than a working set of n + 1 + soft holds)
# ("row_kernel" 0: by default the row kernel walks the list of a large batch; it has its own tests below)
PINS = (("qp_tiers", 2), ("list_snapshot", 1), ("wave_probe", 0), ("row_kernel", 0))
ids = lambda c: c.name


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _settings(lmpc, case):
    s = lmpc.default_settings()
    if case.fval_bound:
        s.fval_bound = case.fval_bound
    if case.progress_tol:
        s.progress_tol = case.progress_tol
    if case.iter_limit:
        s.iter_limit = case.iter_limit
    return s


def _handle(lmpc, case, wave=1, options=PINS, nout=None):
    H, f, f_theta, A, bu, bl, W, sense = tc.problem(case)
    nout = case.nout if nout is None else nout
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, senses=sense, nout=nout, settings=_settings(lmpc, case))
    qp.set_option("wave", wave)
    for k, v in options:
        qp.set_option(k, v)
    assert (qp.n, qp.m, qp.ms, qp.nth, qp.nout, qp.words) == (case.n, case.m, case.nms, case.nth, nout, case.words)
    return qp


_REF = {}


def _ref(case, qp, check=True):
    """The oracle on the handle's pack for the case's condition batch, computed once and never written to; a smaller
    batch is a prefix of it, a larger one repeats it.  The case's conditions are asserted on what it returns."""
    from oracle import ldp as oldp
    key = (case, qp.nout)
    if key not in _REF:
        th = tc.theta(case, tc.N_COND)
        out = oldp.solve_batch(oracle_ldp_from(qp.ldp()), th, tc.oracle_settings(case))
        if check:
            print(case.name, tc.check_case(case, th, out[1], out[2], out[3]))
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _tiled(ref, N):
    reps = -(-N // tc.N_COND)
    return tuple(np.ascontiguousarray(np.concatenate([a] * reps)[:N]) for a in ref)


class _Guarded:
    """Outputs of one device call with GUARD sentinel rows behind them."""

    def __init__(self, N, nout, words, iters=True, active=True):
        import torch
        G, dev = tc.GUARD, "cuda:0"
        self.N = N
        self.x = torch.full((N + G, nout), float("nan"), dtype=torch.float64, device=dev)
        self.ef = torch.full((N + G,), SENT, dtype=torch.int32, device=dev)
        self.it = torch.full((N + G,), SENT, dtype=torch.int32, device=dev) if iters else None
        self.act = torch.full((N + G, words), ACT_SENT, dtype=torch.int64, device=dev) if active else None

    def read(self):
        N = self.N
        x, ef = self.x.cpu().numpy(), self.ef.cpu().numpy()
        assert np.isnan(x[N:]).all() and (ef[N:] == SENT).all(), "a store behind the batch"
        assert not np.isnan(x[:N]).any() and not (ef[:N] == SENT).any(), \
            ("rows the kernels never wrote", np.flatnonzero(np.isnan(x[:N]).any(axis=1))[:8])
        out = [x[:N], ef[:N], None, None]
        if self.it is not None:
            it = self.it.cpu().numpy()
            assert (it[N:] == SENT).all() and not (it[:N] == SENT).any(), "iters: a store behind the batch or a row never written"
            out[2] = it[:N]
        if self.act is not None:
            act = self.act.cpu().numpy()
            assert (act[N:] == ACT_SENT).all() and not (act[:N] == ACT_SENT).any(), "active: a store behind the batch or a row never written"
            out[3] = act[:N].view(np.uint64)
        return tuple(out)


def _seqs(qp):
    f, w, r = qp.front_pass_info(), qp.wave_launch_info(), qp.row_launch_info()
    return tuple(v[-1]["seq"] if v else 0 for v in (f, w, r))


def _solve(qp, th, iters=True, active=True, warm=None):
    """One lmpc_solve_batch_device call on guarded outputs: ((x, exitflag, iters, active), front / wave / row records of
    the call)."""
    import torch
    N = len(th)
    fs, ws, rs = _seqs(qp)
    th_d = torch.from_numpy(np.ascontiguousarray(th)).cuda()
    g = _Guarded(N, qp.nout, qp.words, iters, active)
    w_d = None if warm is None else torch.from_numpy(np.array(warm).view(np.int64)).cuda()
    qp.solve_device(th_d, x=g.x[:N], exitflag=g.ef[:N], iters=None if g.it is None else g.it[:N],
                    active=None if g.act is None else g.act[:N], warm=w_d)
    torch.cuda.synchronize()
    return g.read(), qp.front_pass_info(fs), qp.wave_launch_info(ws), qp.row_launch_info(rs)


def _expect_tiers(Q, front, n, m, N, cus, walker, what):
    """The front-pass record of one call: ONE launch, the tiers pass at template argument n, in the restated shape."""
    assert len(front) == 1, (what, "front-pass launches of the call", front)
    r = front[0]
    assert r["kind"] == Q.FRONT_TIERS and r["N"] == n, (what, "kind / N", r)
    assert r["lds"] == tc.lds_bytes(n, m), (what, "LDS bytes", r, tc.lds_bytes(n, m))
    assert r["grid"] == tc.grid(N, cus), (what, "workgroups", r, tc.grid(N, cus), cus)
    assert r["nprob"] == N and r["seg_cap"] == tc.seg_cap(N), (what, "batch / seg_cap", r)
    assert r["walker"] == walker, (what, "the kernel that walks the list", r)
    return r


def _same(got, ref, N, what):
    names = ("x", "exitflag", "iters", "active")
    for k, a in enumerate(got):
        if a is None:
            continue
        r = ref[k][:N]
        assert a.shape == r.shape, (what, names[k], a.shape, r.shape)
        if not np.array_equal(a, r):
            bad = np.flatnonzero((a != r).reshape(N, -1).any(axis=1))
            raise AssertionError((what, names[k], f"{len(bad)} of {N} rows differ", bad[:8].tolist(),
                                  a[bad[:3]].tolist(), r[bad[:3]].tolist()))


def _list(qp, n, ref, N, what):
    """The snapshot of the call's work list against the rule, on the oracle's outputs for the same N points."""
    snap = qp.work_list_read()
    assert snap is not None, (what, "no snapshot")
    counts, lst = snap
    assert lst.shape == (tc.K_SHARDS, tc.seg_cap(N)), (what, lst.shape)
    tc.check_list(counts, lst, tc.expected_list(n, ref[1][:N], ref[2][:N], ref[3][:N]), what)
    return int(counts.sum())


def _run(lmpc, qp, case, ref, N, cus, walker, what, **kw):
    """Record first, then the bits, then the list."""
    th = tc.theta(case, N)
    got, front, wave, row = _solve(qp, th, **kw)
    _expect_tiers(lmpc.BatchedQP, front, case.n, case.m, N, cus, walker, what)
    if walker == lmpc.BatchedQP.WALK_WAVE:
        assert len(wave) == 1 and wave[0]["worklist"] == 1 and not row, (what, wave, row)
    elif walker == lmpc.BatchedQP.WALK_LANE:
        assert not wave and not row, (what, wave, row)
    want = ref if N <= tc.N_COND else _tiled(ref, N)
    _same(got, want, N, what)
    return _list(qp, case.n, want, N, what)


# ------------------------------------------------------------------ every case behind the wavefront kernel
@pytest.mark.parametrize("case", tc.CASES, ids=ids)
def test_in_front_of_the_wavefront_kernel(lmpc, cus, case):
    """qp_tiers_kernel<n> + wave_kernel on the list: the condition batch (64 tiles, one per segment), then the batch
    sizes 1, 63, 64 and 65 as prefixes of it."""
    qp = _handle(lmpc, case)
    assert qp.kernel_name == "qp_tiers<%d>|wave" % case.n, qp.kernel_name
    ref = _ref(case, qp)
    queued = _run(lmpc, qp, case, ref, tc.N_COND, cus, qp.WALK_WAVE, (case.name, tc.N_COND))
    assert queued == int((~tc.must_finish(case.n, ref[1], ref[2], ref[3])).sum())
    for N in tc.SIZES:
        _run(lmpc, qp, case, ref, N, cus, qp.WALK_WAVE, (case.name, N))
    qp.check()
    qp.close()


# ------------------------------------------------------------------ behind the lane kernel
LANE_CASES = tuple(c for c in tc.HARD + tc.EDGE + tc.DUP + tc.TIE + (tc.SUM, tc.FVAL)
                   if c.m * c.n < 600 and c.mg > 0 and (c.n >= 7 or c in tc.HARD or c in tc.DUP))


def test_lane_cases_hold_the_padded_sizes():
    assert {7, 9, 11} <= {c.n for c in LANE_CASES} and {2, 3, 4, 5, 6, 8} <= {c.n for c in LANE_CASES}
    assert any(c.nout > 1 for c in LANE_CASES) and {31, 32, 33, 63, 64} <= {c.m for c in LANE_CASES}


@pytest.mark.parametrize("case", LANE_CASES, ids=ids)
def test_in_front_of_the_lane_kernel(lmpc, cus, case):
    """ "wave" 0 (m n < 600): the same pass fills the list the lane kernel walks -- n = 7, 9, 11 run on the lane
    kernel of the next even size."""
    qp = _handle(lmpc, case, wave=0)
    ref = _ref(case, qp)
    for N in (tc.N_COND, 65):
        _run(lmpc, qp, case, ref, N, cus, qp.WALK_LANE, (case.name, "lane", N))
    qp.check()
    qp.close()


# ------------------------------------------------------------------ behind the row kernel
def test_in_front_of_the_row_kernel(lmpc, cus):
    """row_cases.LIST_TIERS: "row_kernel" 1 behind the pass -- the record names the row kernel as the one that walks the
    list, and the list holds what the rule says."""
    from oracle import ldp as oldp
    case = rc.LIST_TIERS
    H, f, f_theta, A, bu, bl, W, sense = rc.problem(case)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, senses=sense, nout=case.nout)
    qp.set_option("wave", 1)
    for k, v in PINS[:3] + (("row_kernel", 1),):
        qp.set_option(k, v)
    th = np.ascontiguousarray(rc.theta(case))
    N = len(th)
    ref = oldp.solve_batch(oracle_ldp_from(qp.ldp()), th)
    fin = tc.must_finish(case.n, ref[1], ref[2], ref[3])
    assert fin.any() and not fin.all()
    got, front, wave, row = _solve(qp, th)
    _expect_tiers(qp, front, case.n, case.m, N, cus, qp.WALK_ROW, case.name)
    assert len(row) == 1 and row[0]["worklist"] == 1, (row, wave)
    _same(got, ref, N, case.name)
    assert _list(qp, case.n, ref, N, case.name) == int((~fin).sum())
    qp.check()
    qp.close()


# ------------------------------------------------------------------ outputs the caller does not want
NULL_FORMS = ((tc.HARD[1], 1), (tc.HARD[1], 0), (tc.HARD[9], 1), (tc.SOFT[5], 1), (tc.BY_NAME["dup-n7"], 1), (tc.BY_NAME["dup-n7"], 0))


@pytest.mark.parametrize("case,wave", NULL_FORMS, ids=lambda v: v.name if isinstance(v, tc.TiersCase) else f"wave{v}")
def test_iters_and_active_null(lmpc, cus, case, wave):
    qp = _handle(lmpc, case, wave=wave)
    ref = _ref(case, qp)
    walker = qp.WALK_WAVE if wave else qp.WALK_LANE
    for iters, active in ((False, False), (True, False), (False, True)):
        _run(lmpc, qp, case, ref, tc.N_COND, cus, walker, (case.name, wave, iters, active), iters=iters, active=active)
    qp.check()
    qp.close()


# ------------------------------------------------------------------ large batches
def test_stride_loop_takes_a_second_trip(lmpc, cus):
    """One tile more than 4 x 64 x the largest grid holds in one trip: the first wavefront goes round its loop a second
    time (the 4096 checked points repeated)."""
    case = tc.BY_NAME["hard-n10"]
    full = tc.grid(1 << 40, cus)
    N = 4 * 64 * full + 65
    assert tc.grid(N, cus) == full and (N + 63) // 64 > 4 * full
    qp = _handle(lmpc, case)
    ref = _ref(case, qp)
    queued = _run(lmpc, qp, case, ref, N, cus, qp.WALK_WAVE, (case.name, N))
    assert queued > 0
    qp.check()
    qp.close()


@pytest.mark.parametrize("case", (tc.HARD[10], tc.SOFT[0]), ids=ids)
@pytest.mark.parametrize("row", (0, 1), ids=("wave", "row"))
def test_sixty_five_thousand_points_with_the_pass_forced(lmpc, cus, case, row):
    """65 536 points at "qp_tiers" 2: the size from which the default mode starts to measure -- the wavefront kernel
    behind the pass, and the row kernel ("row_kernel" 1; for a batch this large it is the default)."""
    qp = _handle(lmpc, case, options=PINS + (("row_kernel", row),))
    ref = _ref(case, qp)
    got, front, wave, rrec = _solve(qp, tc.theta(case, 65536))
    _expect_tiers(qp, front, case.n, case.m, 65536, cus, qp.WALK_ROW if row else qp.WALK_WAVE, (case.name, row))
    if row:         # (the row kernel walks the list; what outgrows its slots goes on to the wavefront kernel as a second pass)
        assert len(rrec) == 1 and rrec[0]["worklist"] == 1 and all(w["pass"] == 2 for w in wave), (rrec, wave)
    else:
        assert not rrec and len(wave) == 1 and wave[0]["worklist"] == 1, (rrec, wave)
    want = _tiled(ref, 65536)
    _same(got, want, 65536, (case.name, row))
    _list(qp, case.n, want, 65536, (case.name, row))
    qp.check()
    qp.close()


# ------------------------------------------------------------------ call sequences on one handle
def test_call_sequences_on_one_handle(lmpc, cus):
    """tiers -> screening -> tiers (both counter sets), a warm call in between, a growing batch (the lists are allocated
    again), lmpc_release_scratch (lists and snapshot buffer go and come back)."""
    from oracle import ldp as oldp
    case = tc.BY_NAME["hard-n10"]
    qp = _handle(lmpc, case)
    Q = lmpc.BatchedQP
    ref = _ref(case, qp)
    warm_ref = oldp.solve_batch(oracle_ldp_from(qp.ldp()), tc.theta(case, 65), tc.oracle_settings(case), warm=ref[3][:65])

    def tiers(N, what):
        _run(lmpc, qp, case, ref, N, cus, Q.WALK_WAVE, (case.name, what, N))

    def screening(N, what):
        qp.set_option("qp_tiers", 0)
        got, front, wave, row = _solve(qp, tc.theta(case, N))
        qp.set_option("qp_tiers", 2)
        assert len(front) == 1 and front[0]["kind"] == Q.FRONT_SCREEN and front[0]["N"] == 0 and front[0]["nprob"] == N, (what, front)
        assert front[0]["walker"] == Q.WALK_WAVE and front[0]["seg_cap"] == tc.seg_cap(N), (what, front)
        _same(got, ref if N <= tc.N_COND else _tiled(ref, N), N, (what, N))
        # the screening pass finishes exactly the settled points (iteration 1): what it queued is everything else
        counts, lst = qp.work_list_read()
        want = ref if N <= tc.N_COND else _tiled(ref, N)
        queued = np.sort(np.concatenate([lst[s][:counts[s]] for s in range(tc.K_SHARDS)]))
        assert np.array_equal(queued, np.flatnonzero(want[2][:N] != 1)), what

    tiers(65, "first")                                       # counter set 0
    screening(65, "screening")                               # set 1
    tiers(65, "again")                                       # set 0 again, cleared by the call before
    tiers(65, "and again")                                   # set 1
    got, front, wave, row = _solve(qp, tc.theta(case, 65), warm=ref[3][:65])
    assert not [r for r in front if r["kind"] == Q.FRONT_TIERS], ("a warm call takes no tiers pass", front)
    _same(got, warm_ref, 65, "warm")
    tiers(65, "after the warm call")
    tiers(tc.N_COND, "grown")                                # same seg_cap, more tiles
    tiers(70_000, "grown past the lists' capacity")          # ensure_lists allocates again: counter sets start over
    screening(70_000, "screening, large")
    tiers(tc.N_COND, "smaller again")
    qp.release_scratch()
    assert qp.work_list_read() is None, "the snapshot buffer went with the scratch"
    tiers(tc.N_COND, "after release_scratch")
    tiers(65, "after release_scratch, again")
    qp.check()
    qp.close()


def test_default_mode_measures_by_itself(lmpc, cus):
    """ "qp_tiers" 1 at 65 536 points and more: the handle times calls with and without the pass.  Every call's record is
    the screening pass or the tiers pass (both occur: the first six calls alternate), and the results never differ.  The
    order is not asserted beyond that: it depends on event timing."""
    case = tc.BY_NAME["hard-n10"]
    qp = _handle(lmpc, case, options=(("qp_tiers", 1), ("list_snapshot", 1), ("wave_probe", 0), ("row_kernel", 0)))
    Q = lmpc.BatchedQP
    ref = _ref(case, qp)
    N = 65536 + 64
    want = _tiled(ref, N)
    kinds = []
    for call in range(8):
        got, front, wave, row = _solve(qp, tc.theta(case, N))
        assert len(front) == 1 and front[0]["kind"] in (Q.FRONT_SCREEN, Q.FRONT_TIERS) and front[0]["nprob"] == N, (call, front)
        kinds.append(front[0]["kind"])
        _same(got, want, N, (case.name, "default mode", call))
        counts, lst = qp.work_list_read()
        if front[0]["kind"] == Q.FRONT_TIERS:
            tc.check_list(counts, lst, tc.expected_list(case.n, want[1], want[2], want[3]), ("default mode", call))
        else:
            assert int(counts.sum()) == int((want[2] != 1).sum()), ("default mode", call)
    assert set(kinds) == {Q.FRONT_SCREEN, Q.FRONT_TIERS}, kinds
    qp.check()
    qp.close()


# ------------------------------------------------------------------ refusals
def _no_tiers(qp, th, oracle_settings, what, warm=None):
    """A call that must not take the tiers pass: no kind-2 entry in the record, and still the oracle's bits."""
    from oracle import ldp as oldp
    ref = oldp.solve_batch(oracle_ldp_from(qp.ldp()), th, oracle_settings, warm=warm)
    got, front, wave, row = _solve(qp, th, warm=warm)
    assert not [r for r in front if r["kind"] == qp.FRONT_TIERS], (what, "a tiers pass ran", front)
    _same(got, ref, len(th), what)
    return front


@pytest.mark.parametrize("case,what", tc.REFUSED_SETUP, ids=lambda v: v.name if isinstance(v, tc.TiersCase) else None)
def test_problems_the_pass_does_not_cover(lmpc, case, what):
    qp = _handle(lmpc, case)
    assert "qp_tiers" not in qp.kernel_name, (what, qp.kernel_name)
    _no_tiers(qp, tc.theta(case, 1000), tc.oracle_settings(case), what)
    qp.check()
    qp.close()


def test_calls_and_settings_the_pass_does_not_cover(lmpc, cus):
    from oracle import ldp as oldp
    case = tc.LIMIT_CASE
    n = case.n
    th = tc.theta(case, 1000)
    for wave in (1, 0):
        qp = _handle(lmpc, case, wave=wave)
        walker = qp.WALK_WAVE if wave else qp.WALK_LANE
        s, so = lmpc.default_settings(), oldp.default_settings()
        s.iter_limit = so.iter_limit = n + 2                 # inside the reach of the tiers: refused
        qp.set_settings(s)
        _no_tiers(qp, th, so, ("iter_limit n + 2", wave))
        s.iter_limit = so.iter_limit = n + 3                 # the smallest limit the pass takes
        qp.set_settings(s)
        ref = oldp.solve_batch(oracle_ldp_from(qp.ldp()), th, so)
        assert (ref[1] == -4).any(), "the limit acts"
        got, front, wave_r, row = _solve(qp, th)
        _expect_tiers(qp, front, n, case.m, len(th), cus, walker, ("iter_limit n + 3", wave))
        _same(got, ref, len(th), ("iter_limit n + 3", wave))
        # (a point stopped by the limit took a removal on its way: n + 3 iterations without one end in the tiers)
        _list(qp, n, ref, len(th), ("iter_limit n + 3", wave))
        qp.set_settings(lmpc.default_settings())
        cold = oldp.solve_batch(oracle_ldp_from(qp.ldp()), th)
        _no_tiers(qp, th, None, ("warm start", wave), warm=cold[3])
        qp.set_option("screen", 0)
        front = _no_tiers(qp, th, None, ('"screen" 0', wave))
        assert not front, front
        qp.set_option("screen", 1)
        got, front, wave_r, row = _solve(qp, th)
        _expect_tiers(qp, front, n, case.m, len(th), cus, walker, ("back", wave))
        qp.check()
        qp.close()


# ------------------------------------------------------------------ the snapshot option itself
def test_snapshot_off_changes_no_call_and_on_refuses_a_capture(lmpc, cus):
    """With "list_snapshot" 0 (the default) a call enqueues what it always did: one front pass, one wavefront-kernel
    launch, no snapshot buffer; the profile counts the same calls either way.  With 1, a call inside a stream capture is
    refused before it enqueues anything."""
    import torch
    case = tc.BY_NAME["hard-n10"]
    qp = _handle(lmpc, case, options=(("qp_tiers", 2), ("wave_probe", 0), ("row_kernel", 0)))
    ref = _ref(case, qp)
    th = tc.theta(case, tc.N_COND)
    qp.profile(True)
    for call in range(3):
        got, front, wave, row = _solve(qp, th)
        _expect_tiers(qp, front, case.n, case.m, tc.N_COND, cus, qp.WALK_WAVE, ("off", call))
        assert len(wave) == 1 and not row, (wave, row)
        _same(got, ref, tc.N_COND, ("off", call))
        assert qp.work_list_read() is None, "a snapshot with the option off"
    cnt, ms, ms_front, ms_behind = qp.profile_read()
    assert cnt == 3 and ms_front > 0 and ms_behind > 0, (cnt, ms, ms_front, ms_behind)
    qp.set_option("list_snapshot", 1)
    for call in range(3):
        got, front, wave, row = _solve(qp, th)
        assert len(front) == 1 and len(wave) == 1 and not row
        _same(got, ref, tc.N_COND, ("on", call))
        _list(qp, case.n, ref, tc.N_COND, ("on", call))
    cnt, ms, ms_front, ms_behind = qp.profile_read()
    assert cnt == 3, cnt
    qp.profile(False)
    # inside a capture: refused, nothing recorded, nothing enqueued; the handle works on afterwards
    th_d = torch.from_numpy(th).cuda()
    x = torch.zeros((tc.N_COND, qp.nout), dtype=torch.float64, device="cuda")
    ef = torch.zeros(tc.N_COND, dtype=torch.int32, device="cuda")
    seq = _seqs(qp)
    st = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # (torch remarks that the captured graph is empty: it must be)
        with torch.cuda.stream(st):
            with torch.cuda.graph(graph, stream=st):
                with pytest.raises(lmpc.LmpcError, match="stream capture"):
                    qp.solve_device(th_d, x=x, exitflag=ef, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert _seqs(qp) == seq
    got, front, wave, row = _solve(qp, th)
    _same(got, ref, tc.N_COND, "after the refused capture")
    qp.check()
    qp.close()
