"""The one-launch kernel (lmpc_fast_kernel.hpp) at every instantiation and on every record path, against the oracle on
the handle's own pack, bit for bit: np.array_equal on x, exitflag, iters and active where the call returns them, on
x and exitflag elsewhere.  Cases and the conditions that keep a comparison from passing emptily: tests/fast_cases.py
(checked on the host in tests/test_fast_cases_host.py, re-asserted here on the oracle's outputs for the handle's pack).

Every output is allocated with GUARD rows behind row N and pre-filled with sentinels (NaN for x, 12345 for exitflag
and iters, a bit pattern no active set can be for active): the guard rows must come back untouched -- the batch's
partial tile is where a stray store would land -- and no sentinel may survive in rows 0 ... N - 1."""
import numpy as np
import pytest

import fast_cases as fc
from conftest import oracle_ldp_from

pytestmark = pytest.mark.gpu

SENT = 12345
ACT_SENT = 0x5A5A5A5A5A5A5A5A              # (an active word of these problems has bits 0 ... 2 n - 1 <= 9 only)


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _handle(lmpc, case):
    H, f, f_theta, bu, bl, W = fc.problem(case)
    s = None
    if case.iter_limit:
        s = lmpc.default_settings()
        s.iter_limit = case.iter_limit
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, np.zeros((0, case.n)), bu, bl, W, nout=case.nout, settings=s)
    assert qp.kernel_name.startswith(f"fast<{case.n}>|"), qp.kernel_name
    assert qp.words == 1
    return qp


_REF = {}


def _ref(case, qp, batch=0, nulls=False):
    """The oracle on the handle's pack for the case's batch of N_COND points, computed once and never written to; a
    smaller batch is a prefix of it (fast_cases.theta), so its reference is the same rows."""
    from oracle import ldp as oldp
    key = (case, batch, nulls)
    if key not in _REF:
        th = fc.theta(case, fc.N_COND, batch)
        if nulls:
            th = fc.null_theta(case, th)
        out = oldp.solve_batch(oracle_ldp_from(qp.ldp()), th, fc.oracle_settings(case))
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _assert_conditions(case, ref):
    x, ef, it, act = ref
    st = fc.check_fast_conditions(case, it, act, ef)
    print(case.name, st)
    return st


class _Guarded:
    """Outputs of one device call with GUARD sentinel rows behind them."""

    def __init__(self, N, nout, words=1, optional=True):
        import torch
        G, dev = fc.GUARD, "cuda:0"
        self.N = N
        self.x = torch.full((N + G, nout), float("nan"), dtype=torch.float64, device=dev)
        self.ef = torch.full((N + G,), SENT, dtype=torch.int32, device=dev)
        self.it = torch.full((N + G,), SENT, dtype=torch.int32, device=dev) if optional else None
        self.act = torch.full((N + G, words), ACT_SENT, dtype=torch.int64, device=dev) if optional else None

    def read(self, x_may_keep_nan=False):
        """(x, exitflag[, iters, active]) of rows 0 ... N - 1 as numpy arrays, after the checks on both parts."""
        N = self.N
        x, ef = self.x.cpu().numpy(), self.ef.cpu().numpy()
        assert np.isnan(x[N:]).all() and (ef[N:] == SENT).all(), "a store behind the batch (x / exitflag)"
        assert not np.isnan(x[:N]).any() and not (ef[:N] == SENT).any(), \
            ("rows the kernel never wrote", np.flatnonzero(np.isnan(x[:N]).any(axis=1))[:8], np.flatnonzero(ef[:N] == SENT)[:8])
        if self.it is None:
            return x[:N], ef[:N]
        it, act = self.it.cpu().numpy(), self.act.cpu().numpy()
        assert (it[N:] == SENT).all() and (act[N:] == ACT_SENT).all(), "a store behind the batch (iters / active)"
        assert not (it[:N] == SENT).any() and not (act[:N] == ACT_SENT).any(), "rows the kernel never wrote (iters / active)"
        return x[:N], ef[:N], it[:N], act[:N].view(np.uint64)


def _solve_guarded(qp, th_d, optional=True):
    import torch
    N = int(th_d.shape[0])
    g = _Guarded(N, qp.nout, qp.words, optional)
    qp.solve_device(th_d, x=g.x[:N], exitflag=g.ef[:N], iters=g.it[:N] if optional else None,
                    active=g.act[:N] if optional else None)
    torch.cuda.synchronize()
    return g.read()


def _same(got, ref, N, what):
    names = ("x", "exitflag", "iters", "active")
    for k, a in enumerate(got):
        r = ref[k][:N]
        if not np.array_equal(a, r):
            bad = np.flatnonzero((a != r).reshape(N, -1).any(axis=1))
            raise AssertionError((what, names[k], f"{len(bad)} of {N} rows differ", bad[:8].tolist(),
                                  a[bad[:3]].tolist(), r[bad[:3]].tolist()))


# ------------------------------------------------------------------ plain form: all 56 pairs, one and n outputs
@pytest.mark.parametrize("nout", ["one", "n"])
@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_plain_form_every_instantiation(lmpc, case, nout):
    """fast_kernel<NTHMAX, NT, N, false> against the oracle, the two-kernel form ("fast" 0) and the device call
    without the optional outputs, at N_COND points (37 tiles, 5 workgroups, a partial tile) and at 65."""
    import torch
    case = case.with_nout(1 if nout == "one" else case.n)
    qp = _handle(lmpc, case)
    ref = _ref(case, qp)
    _assert_conditions(case, ref)
    rem = fc.removing(ref[2], ref[3])
    for N in (fc.N_COND, 65):
        th = fc.theta(case, N)
        th_d = torch.from_numpy(th).cuda()
        got = _solve_guarded(qp, th_d)
        _same(got, ref, N, (case.name, N, "one launch"))
        _same(_solve_guarded(qp, th_d, optional=False), ref, N, (case.name, N, "one launch, x and flags only"))
        qp.set_option("fast", 0)
        two = qp.solve(th)
        qp.set_option("fast", 1)
        _same(two, ref, N, (case.name, N, "two kernels"))
        if case.n >= 3 and N == fc.N_COND:
            # the generic loop behind the tiers (fast_fallback<N>) in numbers: the points that removed a row again
            assert rem.sum() >= 8
            for a, r in zip(got, ref):
                assert np.array_equal(a[rem], r[rem])
    qp.check()


def test_iteration_limit_in_the_fallback(lmpc):
    """iter_limit = 7, the smallest fast_covers() accepts: the tiers cannot meet it, the generic loop behind them
    does -- the oracle, limited alike, reports -4 on some points of this n = 5 case, and so must the kernel."""
    import torch
    case = fc.LIMIT_CASE
    qp = _handle(lmpc, case)
    ref = _ref(case, qp)
    assert (ref[1] == -4).sum() >= 8 and (ref[2][ref[1] == -4] == fc.ITER_LIMIT_MIN).all()
    th_d = torch.from_numpy(fc.theta(case, fc.N_COND)).cuda()
    got = _solve_guarded(qp, th_d)
    _same(got, ref, fc.N_COND, (case.name, "iter_limit 7"))
    assert (got[1] == -4).sum() == (ref[1] == -4).sum()
    qp.check()


# ------------------------------------------------------------------ record paths and launch shapes, one pair per NT
RECORD_OPTS = {
    "dma0": {"fast_dma": 0}, "dma2": {"fast_dma": 2}, "dma3": {"fast_dma": 3},
    "nstr1": {"fast_nstr": 1}, "nstr2": {"fast_nstr": 2}, "nstr3": {"fast_nstr": 3}, "nstr4": {"fast_nstr": 4},
    "in_flight3": {"in_flight": 3},
    # R >= 12 switches the dynamic tail on: at N_COND the last 5 tiles, the partial one included, go through tickets
    "dyn-dma0": {"fast_tiles": 12, "fast_dyn": 4, "fast_dma": 0}, "dyn-dma3": {"fast_tiles": 12, "fast_dyn": 4, "fast_dma": 3},
    "dyn-dma2": {"fast_tiles": 12, "fast_dyn": 4, "fast_dma": 2},
    "unaligned": {},
}


def _nt_nout(case):
    return case.n if case.nth % 2 == 0 else 1


@pytest.mark.parametrize("opts", list(RECORD_OPTS), ids=list(RECORD_OPTS))
@pytest.mark.parametrize("case", fc.NT_CASES, ids=lambda c: c.name)
def test_record_paths_and_launch_shapes(lmpc, case, opts):
    """Records through registers, by LDS-DMA into rings of two and three tiles, one to four streaming wavefronts, the
    batches-in-flight shape, the dynamic tail and a batch 8 bytes off a 16-byte boundary, at every batch size of
    fast_cases.SIZES: the execution order changes, the bits do not."""
    import torch
    case = case.with_nout(_nt_nout(case))
    qp = _handle(lmpc, case)
    for k, v in RECORD_OPTS[opts].items():
        qp.set_option(k, v)
    ref = _ref(case, qp)
    _assert_conditions(case, ref)
    dyn = "fast_dyn" in RECORD_OPTS[opts]
    for N in fc.SIZES:
        th = fc.theta(case, N)
        if opts == "unaligned":
            flat = torch.zeros(N * case.nth + 1, dtype=torch.float64, device="cuda:0")
            flat[1:] = torch.from_numpy(th.reshape(-1)).cuda()
            th_d = flat[1:].view(N, case.nth)
            assert th_d.data_ptr() % 16 == 8
        else:
            th_d = torch.from_numpy(th).cuda()
            assert th_d.data_ptr() % 16 == 0
        for rep in range(2 if dyn else 1):                   # (the ticket counters' two sets alternate from call to call)
            _same(_solve_guarded(qp, th_d), ref, N, (case.name, opts, N, rep))
    qp.check()


# ------------------------------------------------------------------ gather form: all 56 pairs
def _gather_call(qp, case, th, nulls, fused):
    """One lmpc_compute_control_device call on guarded buffers: (control, exitflag) of rows 0 ... N - 1."""
    import torch
    N = len(th)
    G = fc.GUARD
    b = fc.gather_blocks(case, th, qp.nout)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    skip = case.null if nulls else ()
    control = torch.full((N + G, qp.nout), float("nan"), dtype=torch.float64, device="cuda:0")
    control[:N] = torch.from_numpy(b["control"]).cuda()       # previous control in, u* out; NaN wherever nothing is read
    ef = torch.full((N + G,), SENT, dtype=torch.int32, device="cuda:0")
    qp.set_option("cc_fused", fused)
    qp.compute_control_device(control[:N], dev(b["state"]), None if "r" in skip else dev(b["reference"]),
                              None if "d" in skip else dev(b["disturbance"]), None if "p" in skip else dev(b["parameter"]),
                              exitflag=ef[:N])
    torch.cuda.synchronize()
    c, e = control.cpu().numpy(), ef.cpu().numpy()
    assert np.isnan(c[N:]).all() and (e[N:] == SENT).all(), "a store behind the batch"
    assert not np.isnan(c[:N]).any() and not (e[:N] == SENT).any(), "rows the kernel never wrote"
    return c[:N], e[:N]


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_gather_form_every_instantiation(lmpc, case):
    """fast_kernel<NTHMAX, NT, N, true>: set_parameter_layout + compute_control on the boxed problem, theta assembled
    by the kernel from the argument arrays (`control` read in place and overwritten), with every block given and
    with the case's NULL blocks; "cc_fused" 1 against "cc_fused" 0, solve(theta) of the assembled theta and the oracle."""
    case = case.with_nout(case.gather_nout)
    qp = _handle(lmpc, case)
    qp.set_parameter_layout(*case.layout)
    for nulls in ((False, True) if case.null else (False,)):
        ref = _ref(case, qp, nulls=nulls)
        if not nulls:
            _assert_conditions(case, ref)
        for N in (fc.N_COND, 65):
            th = fc.theta(case, N)
            fused = _gather_call(qp, case, th, nulls, 1)
            _same(fused, ref, N, (case.name, N, nulls, "fused"))
            _same(_gather_call(qp, case, th, nulls, 0), ref, N, (case.name, N, nulls, "unfused"))
            _same(qp.solve(fc.null_theta(case, th) if nulls else th)[:2], ref, N, (case.name, N, nulls, "solve(theta)"))
    qp.check()


# ------------------------------------------------------------------ several batches in one launch
@pytest.mark.parametrize("nout", ["one", "n"])
@pytest.mark.parametrize("case", fc.NT_CASES, ids=lambda c: c.name)
def test_several_batches_every_nt(lmpc, case, nout):
    """fast_kernel_multi<NTHMAX, NT, N> (lmpc_solve_batches_device): 2, 8 and 9 = 8 + 1 batches of N_COND and of 65
    points, every batch against the oracle in full, and one launch in which one batch starts 8 bytes off a 16-byte
    boundary (which takes the whole launch off the LDS-DMA path).

    The several-batches launch is taken when (lmpc_solve_batches_device): the handle is one the one-launch kernel
    covers, no closed loop or generated-controller call has lent it anything, MORE THAN ONE batch is left to enqueue,
    and profiling is OFF -- under lmpc_profile the batches go one launch each, so the profile cannot show this form."""
    import torch
    case = case.with_nout(1 if nout == "one" else case.n)
    qp = _handle(lmpc, case)
    refs = [_ref(case, qp, batch=b) for b in range(9)]
    _assert_conditions(case, refs[0])

    def run(th_d, N):
        gs = [_Guarded(N, qp.nout, optional=False) for _ in th_d]
        qp.solve_batches_device(th_d, [g.x[:N] for g in gs], [g.ef[:N] for g in gs])
        torch.cuda.synchronize()
        qp.check()
        for b, g in enumerate(gs):
            _same(g.read(), refs[b], N, (case.name, N, len(th_d), "batch", b))

    for N in (fc.N_COND, 65):
        th_d = [torch.from_numpy(fc.theta(case, N, b)).cuda() for b in range(9)]
        for nb in (2, 8, 9):
            run(th_d[:nb], N)
        if N == fc.N_COND:
            flat = torch.zeros(N * case.nth + 1, dtype=torch.float64, device="cuda:0")
            flat[1:] = th_d[1].reshape(-1)
            view = flat[1:].view(N, case.nth)
            assert view.data_ptr() % 16 == 8 and th_d[0].data_ptr() % 16 == 0
            run([th_d[0], view, th_d[2]], N)


# ------------------------------------------------------------------ the call really is the one-launch kernel
@pytest.mark.parametrize("form", ["plain", "gather"])
def test_profile_shows_one_launch(lmpc, form):
    """lmpc_profile_read reports an iterating-kernel time of exactly 0.0 and a screening time equal to the total for
    a call that recorded no middle event, which is what the one-launch branch of the dispatch does (it hands the
    middle event back to the pool); the two-kernel form ("fast" 0) records one and reports both parts."""
    import torch
    case = fc.BY_PAIR[(5, 7)]
    case = case.with_nout(case.gather_nout if form == "gather" else 1)
    qp = _handle(lmpc, case)
    ref = _ref(case, qp)
    N = 705
    th = fc.theta(case, N)
    th_d = torch.from_numpy(th).cuda()
    if form == "gather":
        qp.set_parameter_layout(*case.layout)
        call = lambda: _same(_gather_call(qp, case, th, False, 1), ref, N, "gather")
    else:
        call = lambda: _same(_solve_guarded(qp, th_d), ref, N, "plain")
    call()                                                   # (first call on the handle: allocations, code load)
    qp.profile(True)
    try:
        call()
        cnt, total, screen, iterate = qp.profile_read()
        print(form, "one launch:", cnt, total, screen, iterate)
        assert cnt == 1 and iterate == 0.0 and screen == total and total > 0.0
        qp.set_option("fast", 0)
        call()
        cnt, total, screen, iterate = qp.profile_read()
        print(form, "two kernels:", cnt, total, screen, iterate)
        assert cnt == 1 and iterate > 0.0 and 0.0 < screen < total
    finally:
        qp.set_option("fast", 1)
        qp.profile(False)
    qp.check()
