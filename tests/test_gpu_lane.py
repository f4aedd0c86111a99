"""The two-kernel lane path -- screen_kernel<NTHMAX, NT, MODE> (lmpc_screen_kernel.hpp), then lane_kernel<N, MS, MA, SIM,
MULTI> (lmpc_lane_kernel.hpp) -- at every instantiation the dispatch reaches, against the oracle on the handle's own
pack, bit for bit: np.array_equal on x, exitflag, iters and active where the call returns them; the closed loop against
tests/loop_reference.py, which is bitwise too.  Cases and the conditions that keep a comparison from passing emptily:
tests/lane_cases.py (checked on the host in tests/test_lane_cases_host.py, re-asserted here on the oracle's outputs for
the handle's pack).  No point of a batch is left out of a comparison.

Every output of a device call is allocated with GUARD rows behind row N and pre-filled with sentinels (NaN for x, 12345
for exitflag and iters, a bit pattern no active set can be for active): the guard rows must come back untouched and no
sentinel may survive in rows 0 ... N - 1.  (lmpc_simulate takes host arrays and keeps its device buffers to itself:
there the whole of every returned array is compared.)

General rows: with "qp_tiers" at its default a cold plain call below 65536 points takes the tiers pass instead of the
screening pass, so every such case is pinned to the screening pass with "qp_tiers" 0 and run once more at the default,
for the same bits."""
import numpy as np
import pytest

import lane_cases as lc
import loop_reference as lr
from conftest import oracle_ldp_from

pytestmark = pytest.mark.gpu

SENT = 12345
ACT_SENT = 0x5A5A5A5A5A5A5A5A              # (32 bits set in a word: more rows than a working set of n + 1 <= 13 holds)
case_ids = lambda c: c.name


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _handle(lmpc, case, nout=1, pin=True):
    H, f, f_theta, A, bu, bl, W, sense = lc.problem(case)
    s = None
    if case.iter_limit:
        s = lmpc.default_settings()
        s.iter_limit = case.iter_limit
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, senses=sense, nout=nout, settings=s)
    for k, v in case.opts:
        qp.set_option(k, v)
    if pin and case.mg:
        qp.set_option("qp_tiers", 0)
    name = f"screen+lane<{case.lane_n}>"                      # (neither the one-launch kernel nor the wavefront kernel)
    assert qp.kernel_name == name or (("screen", 0) in case.opts and qp.kernel_name.endswith("|" + name)), qp.kernel_name
    assert (qp.n, qp.m, qp.ms, qp.nth, qp.nout, qp.words) == (case.n, case.m, case.n, case.nth, nout, case.words)
    return qp


_REF = {}


def _cached(key, make):
    if key not in _REF:
        out = make()
        for a in (out.values() if isinstance(out, dict) else out):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _ldp(qp):
    return oracle_ldp_from(qp.ldp())


def _ref(case, qp, nout=1):
    """The oracle on the handle's pack for the case's condition batch, computed once and never written to; a smaller
    batch is a prefix of it, so its reference is the same rows.  The conditions are asserted on what it returns."""
    from oracle import ldp as oldp

    def make():
        th = lc.theta(case, lc.N_COND)
        L = _ldp(qp)
        out = oldp.solve_batch(L, th, lc.oracle_settings(case))
        if case.screened:
            print(case.name, lc.check_lane_conditions(case, L, th, out[1], out[2], out[3]))
        return out
    return _cached((case, nout, "cold"), make)


def _ref_warm(case, qp, nout=1):
    from oracle import ldp as oldp
    cold = _ref(case, qp, nout)
    return _cached((case, nout, "warm"), lambda: oldp.solve_batch(_ldp(qp), lc.theta(case, lc.N_COND), lc.oracle_settings(case),
                                                                  warm=cold[3]))


class _Guarded:
    """Outputs of one device call with GUARD sentinel rows behind them."""

    def __init__(self, N, nout, words, warm=None):
        import torch
        G, dev = lc.GUARD, "cuda:0"
        self.N = N
        self.x = torch.full((N + G, nout), float("nan"), dtype=torch.float64, device=dev)
        self.ef = torch.full((N + G,), SENT, dtype=torch.int32, device=dev)
        self.it = torch.full((N + G,), SENT, dtype=torch.int32, device=dev)
        self.act = torch.full((N + G, words), ACT_SENT, dtype=torch.int64, device=dev)
        if warm is not None:                                 # in place: the masks are read from the buffer they are written to
            self.act[:N] = torch.from_numpy(np.array(warm).view(np.int64)).to(dev)

    def read(self):
        N = self.N
        x, ef, it, act = (t.cpu().numpy() for t in (self.x, self.ef, self.it, self.act))
        assert np.isnan(x[N:]).all() and (ef[N:] == SENT).all() and (it[N:] == SENT).all() and (act[N:] == ACT_SENT).all(), \
            "a store behind the batch"
        assert not np.isnan(x[:N]).any() and not (ef[:N] == SENT).any() and not (it[:N] == SENT).any() and \
            not (act[:N] == ACT_SENT).any(), ("rows the kernels never wrote", np.flatnonzero(np.isnan(x[:N]).any(axis=1))[:8])
        return x[:N], ef[:N], it[:N], act[:N].view(np.uint64)


def _solve(qp, th, warm=None, inplace=False):
    """One lmpc_solve_batch_device call on guarded outputs.  warm: (N, words) masks -- in a buffer of their own, or
    (inplace) in the very buffer `active` is written to."""
    import torch
    N = len(th)
    th_d = torch.from_numpy(np.ascontiguousarray(th)).cuda()
    g = _Guarded(N, qp.nout, qp.words, warm if inplace else None)
    w_d = None
    if warm is not None:
        w_d = g.act[:N] if inplace else torch.from_numpy(np.array(warm).view(np.int64)).cuda()
    qp.solve_device(th_d, x=g.x[:N], exitflag=g.ef[:N], iters=g.it[:N], active=g.act[:N], warm=w_d)
    torch.cuda.synchronize()
    if warm is not None and not inplace:
        assert np.array_equal(w_d.cpu().numpy().view(np.uint64), warm), "the warm masks were written to"
    return g.read()


def _same(got, ref, N, what):
    names = ("x", "exitflag", "iters", "active")
    for k, a in enumerate(got):
        r = ref[k][:N]
        assert a.shape == r.shape, (what, names[k], a.shape, r.shape)
        if not np.array_equal(a, r):
            bad = np.flatnonzero((a != r).reshape(N, -1).any(axis=1))
            raise AssertionError((what, names[k], f"{len(bad)} of {N} rows differ", bad[:8].tolist(),
                                  a[bad[:3]].tolist(), r[bad[:3]].tolist()))


# ------------------------------------------------------------------ every case: plain form, cold and warm
@pytest.mark.parametrize("case", lc.CASES + lc.UNSCREENED, ids=case_ids)
def test_plain_form_cold_and_warm(lmpc, case):
    """screen_kernel<., NT, 0> + lane_kernel<N, MS, MA, false, false> at every batch size of lane_cases.SIZES: cold,
    then warm from the final sets -- masks in a buffer of their own, and in the buffer `active` is written to."""
    qp = _handle(lmpc, case)
    ref, refw = _ref(case, qp), _ref_warm(case, qp)
    th = lc.theta(case, lc.N_COND)
    for N in lc.SIZES:
        _same(_solve(qp, th[:N]), ref, N, (case.name, N, "cold"))
        _same(_solve(qp, th[:N], warm=ref[3][:N]), refw, N, (case.name, N, "warm, two buffers"))
        _same(_solve(qp, th[:N], warm=ref[3][:N], inplace=True), refw, N, (case.name, N, "warm, in place"))
    if case.mg:
        # the same cold calls with "qp_tiers" at its default (the handle's own choice of the first pass)
        qd = _handle(lmpc, case, pin=False)
        for N in lc.SIZES:
            _same(_solve(qd, th[:N]), ref, N, (case.name, N, "cold, qp_tiers at its default"))
        qd.check()
    qp.check()


# ------------------------------------------------------------------ several outputs
@pytest.mark.parametrize("case", [c for c in lc.CASES if lc.nouts(c)], ids=case_ids)
def test_several_outputs(lmpc, case):
    """screen_kernel<., NT, 3> (the wave-private transpose of the outputs) and the lane kernel's several-outputs
    epilogue -- MULTI for N <= 6 and nth <= 16, the generic one beyond --, nout = 2, 3, 5, 7 and n, at batch sizes
    that leave the last wavefront 1, 37, 63 and 5 points wide; cold and warm."""
    th = lc.theta(case, lc.N_COND)
    for nout in lc.nouts(case):
        qp = _handle(lmpc, case, nout)
        ref, refw = _ref(case, qp, nout), _ref_warm(case, qp, nout)
        assert ref[0].shape == (lc.N_COND, nout)
        for N in (256 + 1, 256 + 37, 256 + 63, lc.N_COND):
            _same(_solve(qp, th[:N]), ref, N, (case.name, nout, N, "cold"))
        _same(_solve(qp, th[:293], warm=ref[3][:293], inplace=True), refw, 293, (case.name, nout, "warm"))
        if case.mg:
            qp.set_option("qp_tiers", 1)
            _same(_solve(qp, th), ref, lc.N_COND, (case.name, nout, "cold, qp_tiers at its default"))
        qp.check()


# ------------------------------------------------------------------ generated controller: the gather form
def _gather_call(qp, fcase, th, nulls, prev=None):
    """One lmpc_compute_control_device call with warm = 1 on guarded buffers: (control, exitflag) of rows 0 ... N - 1.
    prev: the control array the call before left (u* in every column); else the previous control from theta."""
    import torch
    N, G = len(th), lc.GUARD
    b = lc.fc.gather_blocks(fcase, th, qp.nout)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    skip = fcase.null if nulls else ()
    control = torch.full((N + G, qp.nout), float("nan"), dtype=torch.float64, device="cuda:0")
    control[:N] = torch.from_numpy(b["control"] if prev is None else prev).cuda()
    ef = torch.full((N + G,), SENT, dtype=torch.int32, device="cuda:0")
    qp.compute_control_device(control[:N], dev(b["state"]), None if "r" in skip else dev(b["reference"]),
                              None if "d" in skip else dev(b["disturbance"]), None if "p" in skip else dev(b["parameter"]),
                              exitflag=ef[:N], warm=True)
    torch.cuda.synchronize()
    c, e = control.cpu().numpy(), ef.cpu().numpy()
    assert np.isnan(c[N:]).all() and (e[N:] == SENT).all(), "a store behind the batch"
    assert not np.isnan(c[:N]).any() and not (e[:N] == SENT).any(), "rows the kernels never wrote"
    return c[:N], e[:N]


@pytest.mark.parametrize("case", lc.CASES, ids=case_ids)
def test_gather_form_with_a_warm_mask(lmpc, case):
    """screen_kernel<., NT, 2>: set_parameter_layout + compute_control_device with warm = 1 -- the first call is given
    `active` (which alone keeps a small boxed problem off the one-launch kernel), the second starts from the first
    one's final sets and reads the first one's u* as its previous control; every block given, and with the layout's
    NULL blocks."""
    from oracle import ldp as oldp
    lay, gnout, null = lc.gather_layout(case)
    fcase = lc.gather_case(case)
    qp = _handle(lmpc, case, gnout)
    qp.set_option("cc_fused", 1)
    qp.set_parameter_layout(*lay)
    L, s = _ldp(qp), lc.oracle_settings(case)
    nx, nr, nd, nup, npp = lay
    o3 = nx + nr + nd
    for nulls in ((False, True) if null else (False,)):
        th = lc.theta(case, lc.N_COND)
        if nulls:
            th = lc.fc.null_theta(fcase, th)
            ref1 = oldp.solve_batch(L, th, s)
        else:
            ref1 = _ref(case, qp, gnout)
        th2 = th.copy()
        th2[:, o3:o3 + nup] = ref1[0][:, :nup]
        ref2 = oldp.solve_batch(L, th2, s, warm=ref1[3])
        for N in (lc.N_COND, 65):
            qp.set_parameter_layout(*lay)                    # (forgets the masks of a batch of another size)
            c1, e1 = _gather_call(qp, fcase, th[:N], nulls)
            _same((c1, e1), ref1, N, (case.name, N, nulls, "first call"))
            _same(_gather_call(qp, fcase, th[:N], nulls, prev=c1), ref2, N, (case.name, N, nulls, "second call, warm"))
    qp.check()


# ------------------------------------------------------------------ lock-step fused closed loop
S_LOOP = 321                # two screening workgroups, five full wavefronts and one lane


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("case", lc.CASES, ids=case_ids)
def test_lock_step_closed_loop(lmpc, case, warm):
    """screen_kernel<., NT, 1> + lane_kernel<N, MS, MA, true, false>: lmpc_simulate with "sim_async" 0, T = 3,
    nu = 1 ... 4 over the table, against the host loop of tests/loop_reference.py."""
    nx, nr, nup, nu = lc.sim_shape(case)
    F, G, x0, r, up = lc.sim_data(case, S_LOOP)
    qp = _handle(lmpc, case, nu)
    qp.set_option("sim_async", 0)
    ref = _cached((case, "loop", warm), lambda: lr.simulate_reference(_ldp(qp), x0, 3, F, G, r=r, uprev=up, warm=warm,
                                                                      settings=lc.oracle_settings(case)))
    lc.check_loop_steps(case, ref["flags"], ref["active"])
    got = qp.simulate(x0, 3, F, G, r=r, uprev=up, warm=warm)
    for key in ("U", "X", "x", "flag_min") + (("uprev",) if nup else ()):
        a, b = got[key], ref[key]
        assert a.shape == b.shape and np.array_equal(a, b), (case.name, key, np.argwhere(a != b)[:4].tolist())
    qp.check()


# ------------------------------------------------------------------ launch shapes
@pytest.mark.parametrize("case", lc.SHAPE_CASES, ids=case_ids)
def test_launch_shapes(lmpc, case):
    """ "lane_block" 64 / 128 / 256 wherever the LDS copy fits; on boxed cases "lane_tier" 0 / 1 x "lane_straight"
    0 / 1: another order of execution, the same bits."""
    qp = _handle(lmpc, case)
    ref = _ref(case, qp)
    th = lc.theta(case, lc.N_COND)
    blocks = lc.lane_blocks(case)
    assert blocks, case
    for B in blocks:
        qp.set_option("lane_block", B)
        for N in (lc.N_COND, 65):
            _same(_solve(qp, th[:N]), ref, N, (case.name, "lane_block", B, N))
    qp.set_option("lane_block", 0)
    if case.boxed:
        for tier in (0, 1):
            for straight in (0, 1):
                qp.set_option("lane_tier", tier)
                qp.set_option("lane_straight", straight)
                _same(_solve(qp, th), ref, lc.N_COND, (case.name, "lane_tier", tier, "lane_straight", straight))
    qp.check()


@pytest.mark.parametrize("case", lc.SHAPE_CASES, ids=case_ids)
def test_large_batch_and_stride_loop(lmpc, case):
    """3 * 16384 + 257 points, more than half of them queued: at "lane_per" 1 (one lane workgroup per work-list
    segment) every workgroup makes several trips of its stride loop; then the same batch at the default grid."""
    from oracle import ldp as oldp
    qp = _handle(lmpc, case)
    th = lc.big_theta(case)
    ref = _cached((case, "big"), lambda: oldp.solve_batch(_ldp(qp), th, lc.oracle_settings(case)))
    print(case.name, lc.check_big_batch(case, ref[2]))
    for B in (lc.lane_blocks(case)[0], 0):
        qp.set_option("lane_block", B)
        qp.set_option("lane_per", 1)
        _same(_solve(qp, th), ref, lc.N_BIG, (case.name, "lane_per 1, lane_block", B))
    qp.set_option("lane_per", 0)
    _same(_solve(qp, th), ref, lc.N_BIG, (case.name, "default grid"))
    qp.check()


# ------------------------------------------------------------------ call sequences on one handle
SEQ_CASES = tuple(lc.BY_NAME[s] for s in ("box6-nth14", "box12-nth9", "gen5-m14-nth5", "gen12-m64-nth12"))


def _batches(case):
    """(name, theta) of the sequence's calls: large and mostly queued, small and all settled, middle and all queued,
    then larger than any before (the work list is regrown)."""
    big = lc.theta(case, 6000, batch=7, scales=case.scales[:1] + 2 * case.scales[-3:])
    z = lc.theta(case, 641, batch=8, scales=(1.0,))
    pushed = np.where(z < 0, -1.0, 1.0) * (1.0 + np.abs(z)) * lc.QUEUED_PUSH
    return (("large, mostly queued", big[:lc.N_COND]), ("small, all settled", z[:65] * 1e-9), ("middle, all queued", pushed),
            ("larger than any before", big))


@pytest.mark.parametrize("case", SEQ_CASES, ids=case_ids)
def test_call_sequence_of_different_sizes(lmpc, case):
    """The two counter sets alternate from call to call, and the lane kernel of call k clears the set of call k + 1:
    calls of different sizes and queue lengths on one handle, each against the oracle; the whole sequence twice."""
    from oracle import ldp as oldp
    qp = _handle(lmpc, case)
    L, s = _ldp(qp), lc.oracle_settings(case)
    calls = [(name, th, oldp.solve_batch(L, th, s)) for name, th in _batches(case)]
    q = [float((r[2] != 1).mean()) for _, _, r in calls]
    assert 0.5 < q[0] < 1.0 and q[1] == 0.0 and q[2] == 1.0 and 0.5 < q[3] < 1.0, q
    for rep in range(2):
        for name, th, ref in calls:
            _same(_solve(qp, th), ref, len(th), (case.name, rep, name))
    qp.check()


@pytest.mark.parametrize("case", SEQ_CASES, ids=case_ids)
def test_cold_warm_cold_and_solve_simulate_solve(lmpc, case):
    from oracle import ldp as oldp
    qp = _handle(lmpc, case)
    ref, refw = _ref(case, qp), _ref_warm(case, qp)
    th = lc.theta(case, lc.N_COND)
    N = 641
    _same(_solve(qp, th[:N]), ref, N, (case.name, "cold"))
    _same(_solve(qp, th[:N], warm=ref[3][:N]), refw, N, (case.name, "warm"))
    _same(_solve(qp, th[:N]), ref, N, (case.name, "cold again"))
    # a closed loop in between (nu = 1: the handle's one output), cold and warm
    qp.set_option("sim_async", 0)
    rng = np.random.default_rng(5)
    nx = case.nth
    F, G = 0.8 * rng.normal(size=(nx, nx)) / np.sqrt(nx), 0.3 * rng.normal(size=(nx, 1))
    x0 = np.ascontiguousarray(lc.theta(case, S_LOOP, batch=5))
    for warm in (False, True):
        want = lr.simulate_reference(_ldp(qp), x0, 3, F, G, warm=warm, settings=lc.oracle_settings(case))
        got = qp.simulate(x0, 3, F, G, warm=warm)
        for key in ("U", "X", "x", "flag_min"):
            assert np.array_equal(got[key], want[key]), (case.name, "simulate", warm, key)
        _same(_solve(qp, th[:N]), ref, N, (case.name, "solve after simulate", warm))
        _same(_solve(qp, th[:N], warm=ref[3][:N], inplace=True), refw, N, (case.name, "warm solve after simulate", warm))
    qp.check()


def test_two_handles_interleaved(lmpc):
    """Two handles of different cases, their calls interleaved on one stream: the work lists and counters are the
    handles' own."""
    from oracle import ldp as oldp
    pairs = []
    for case in (lc.BY_NAME["box8-nth15"], lc.BY_NAME["gen3-m64-nth3"]):
        qp = _handle(lmpc, case)
        L, s = _ldp(qp), lc.oracle_settings(case)
        pairs.append((case, qp, [(name, th, oldp.solve_batch(L, th, s)) for name, th in _batches(case)]))
    for k in range(4):
        for case, qp, calls in pairs[::(1 if k % 2 == 0 else -1)]:
            name, th, ref = calls[(k + (1 if case.mg else 0)) % 4]
            _same(_solve(qp, th), ref, len(th), (case.name, k, name))
    for case, qp, calls in pairs:
        qp.check()
