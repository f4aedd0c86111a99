"""The wavefront path -- wave_kernel<R, MR, LDSC, BNB, PACKED, NU, GRAM = false, SIM> (lmpc_wave_kernel.hpp), launched by
launch_wave_inst (lmpc_wave_launch.hpp), and big_kernel<R> (lmpc_big_kernel.hpp) behind it -- at every instantiation of
the n-chain form, against the oracle on the handle's own pack, bit for bit: np.array_equal on x, exitflag, iters and
active; the closed loop against tests/loop_reference.py, which is bitwise too.  Cases and the conditions that keep a
comparison from passing emptily: tests/wave_cases.py (checked on the host in tests/test_wave_cases_host.py, re-asserted
here on the oracle's outputs for the handle's pack).  No point of a batch is left out of a comparison.

Every test first reads the handle's launch record (lmpc_wave_launch_info) and asserts it against the case: the
instantiation that ran, its staging level, layout, workgroup width, pass and capacity.  A launch choice the launcher
could not honour would run another instantiation and pass every comparison; the record turns that into a failure.

Every output of a device call is allocated with GUARD rows behind row N and pre-filled with sentinels (NaN for x, 12345
for exitflag and iters, a bit pattern no active set can be for active): the guard rows must come back untouched and no
sentinel may survive in rows 0 ... N - 1."""
import ctypes

import numpy as np
import pytest

import loop_reference as lr
import wave_cases as wc
from conftest import oracle_ldp_from

pytestmark = pytest.mark.gpu

SENT = 12345
ACT_SENT = 0x5A5A5A5A5A5A5A5A              # (a row active on both sides in every word: no working set looks like this)
ids = lambda c: c.name
PINS = (("row_kernel", 0), ("qp_tiers", 0), ("screen_wave", 0), ("wave_probe", 0), ("wave_two_pass", 0))


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _settings(lmpc, case):
    s = lmpc.default_settings_f32() if case.f32 else lmpc.default_settings()
    if case.iter_limit:
        s.iter_limit = case.iter_limit
    return s


def _oset(s):
    from oracle import ldp as oldp
    so = oldp.Settings()
    for f, _ in so._fields_:
        setattr(so, f, getattr(s, f, 0))
    return so


def _handle(lmpc, case, nout=1, prob=None):
    H, f, f_theta, A, bu, bl, W, sense = wc.problem(case) if prob is None else prob
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, senses=sense, nout=nout, settings=_settings(lmpc, case))
    qp.set_option("wave", 1)
    for k, v in PINS:
        qp.set_option(k, v)
    assert qp.kernel_name == "wave", qp.kernel_name
    assert (qp.n, qp.m, qp.nth, qp.nout, qp.words) == (case.n, case.m, case.nth, nout, case.words)
    qp._oset = _oset(_settings(lmpc, case))
    return qp


def _pin(qp, level, packed, nwv):
    qp.set_option("wave_level", level)
    qp.set_option("wave_packed", int(packed))
    qp.set_option("wave_nwv", nwv)


def _seq(qp):
    r = qp.wave_launch_info()
    return r[-1]["seq"] if r else 0


def _expect(recs, case, level, packed, nwv, sim=False, passes=(0,), caps=None, worklist=None, what=""):
    """The launch record of one call against the case: one entry per pass, the instantiation wave_cases.inst names."""
    assert [r["pass"] for r in recs] == list(passes), (what, recs)
    rs, MR, LDSC, BNB, PACKED, NU, SIM = wc.inst(case, level, packed, sim)
    for k, r in enumerate(recs):
        got = (r["real_bytes"], r["MR"], r["LDSC"], r["BNB"], r["PACKED"], r["NU"], r["GRAM"], r["SIM"])
        assert got == (rs, MR, LDSC, int(BNB), int(PACKED), NU, 0, int(SIM)), (what, "instantiation", got, r)
        assert (r["level"], r["nwv"]) == (level, nwv), (what, "launch configuration", r)
        cap = case.cap if caps is None else caps[k]
        assert r["cap"] == cap, (what, "capacity", r)
        assert r["big"] == (0 if (case.bnb or r["pass"] == 1) else 1), (what, "slow path", r)
        assert r["lds"] == wc.lds_bytes(case, level, packed, nwv, cap), (what, "LDS bytes", r)
        if worklist is not None:
            assert r["worklist"] == (1 if (worklist or r["pass"] == 2) else 0), (what, "work list", r)
        assert r["grid"] >= 1 and r["qchunk"] >= 1
    assert [r["seq"] for r in recs] == list(range(recs[0]["seq"], recs[0]["seq"] + len(recs)))


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


def _oracle(qp, case, th, warm=None):
    from oracle import ldp as oldp
    return oldp.solve_batch(_ldp(qp), th, qp._oset, warm=warm, dtype=case.dtype)


def _ref(case, qp, nout=1):
    """The oracle on the handle's pack for the case's condition batch, computed once and never written to; a smaller
    batch is a prefix of it.  The conditions are asserted on what it returns."""
    def make():
        out = _oracle(qp, case, wc.theta(case))
        print(case.name, wc.check_wave_conditions(case, out[1], out[2], out[3]))
        return out
    return _cached((case, nout, "cold"), make)


def _ref_warm(case, qp, nout=1):
    cold = _ref(case, qp, nout)

    def make():
        w = wc.warm_masks(cold[1], cold[3])
        out = _oracle(qp, case, wc.theta(case), warm=w)
        wc.check_warm_conditions(case, w, out[1], out[3])
        return (w,) + tuple(out)
    return _cached((case, nout, "warm"), make)


class _Guarded:
    """Outputs of one device call with GUARD sentinel rows behind them."""

    def __init__(self, N, nout, words, f32, warm=None):
        import torch
        G, dev = wc.GUARD, "cuda:0"
        self.N = N
        self.x = torch.full((N + G, nout), float("nan"), dtype=torch.float32 if f32 else torch.float64, device=dev)
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


def _solve(qp, case, th, warm=None, inplace=False):
    """One lmpc_solve_batch[_f32]_device call on guarded outputs: ((x, exitflag, iters, active), its launch records)."""
    import torch
    N = len(th)
    since = _seq(qp)
    th_d = torch.from_numpy(np.ascontiguousarray(th, dtype=case.dtype)).cuda()
    g = _Guarded(N, qp.nout, qp.words, case.f32, warm if inplace else None)
    w_d = None
    if warm is not None:
        w_d = g.act[:N] if inplace else torch.from_numpy(np.array(warm).view(np.int64)).cuda()
    qp.solve_device(th_d, x=g.x[:N], exitflag=g.ef[:N], iters=g.it[:N], active=g.act[:N], warm=w_d)
    torch.cuda.synchronize()
    if warm is not None and not inplace:
        assert np.array_equal(w_d.cpu().numpy().view(np.uint64), warm), "the warm masks were written to"
    return g.read(), qp.wave_launch_info(since)


def _same(got, ref, N, what):
    names = ("x", "exitflag", "iters", "active")
    for k, a in enumerate(got):
        r = ref[k][:N]
        assert a.shape == r.shape and a.dtype == r.dtype, (what, names[k], a.shape, r.shape, a.dtype, r.dtype)
        if not np.array_equal(a, r):
            bad = np.flatnonzero((a != r).reshape(N, -1).any(axis=1))
            raise AssertionError((what, names[k], f"{len(bad)} of {N} rows differ", bad[:8].tolist(),
                                  a[bad[:3]].tolist(), r[bad[:3]].tolist()))


# ------------------------------------------------------------------ plain form: every case at every launch choice
@pytest.mark.parametrize("case", wc.CASES + wc.F32_CASES, ids=ids)
def test_plain_form_every_launch_choice(lmpc, case):
    """Every (level, layout, nwv) the dispatch builds at the case's slot counts and the LDS holds: cold and warm (masks
    in a buffer of their own) on the condition batch -- all of them the oracle's bits, hence each other's."""
    qp = _handle(lmpc, case)
    ref, (w, *refw) = _ref(case, qp), _ref_warm(case, qp)
    th = wc.theta(case)
    choices = wc.launches(case)
    assert choices
    for level, packed, nwv in choices:
        _pin(qp, level, packed, nwv)
        what = (case.name, level, packed, nwv)
        got, recs = _solve(qp, case, th)
        _expect(recs, case, level, packed, nwv, worklist=False, what=what)
        _same(got, ref, wc.N_COND, what + ("cold",))
        got, recs = _solve(qp, case, th, warm=w)
        _expect(recs, case, level, packed, nwv, worklist=False, what=what)
        _same(got, refw, wc.N_COND, what + ("warm",))
    qp.check()


@pytest.mark.parametrize("case", wc.CASES + wc.F32_CASES, ids=ids)
def test_plain_form_batch_sizes(lmpc, case):
    """At the first and the last launch choice of a case the batch sizes 1, nwv - 1, nwv, nwv + 1 and 333: cold, warm in
    two buffers and warm in place (the references are the rows of the test above's, computed once)."""
    qp = _handle(lmpc, case)
    ref, (w, *refw) = _ref(case, qp), _ref_warm(case, qp)
    th = wc.theta(case)
    choices = wc.launches(case)
    for level, packed, nwv in (choices[0], choices[-1]):
        _pin(qp, level, packed, nwv)
        what = (case.name, level, packed, nwv)
        for N in wc.batch_sizes(nwv):
            got, recs = _solve(qp, case, th[:N])
            _expect(recs, case, level, packed, nwv, worklist=False, what=what + (N,))
            assert recs[0]["nprob"] == N and recs[0]["grid"] == min(recs[0]["grid"], -(-N // nwv))
            _same(got, ref, N, what + (N, "cold"))
            got, recs = _solve(qp, case, th[:N], warm=w[:N])
            _expect(recs, case, level, packed, nwv, what=what + (N, "warm"))
            _same(got, refw, N, what + (N, "warm, two buffers"))
            got, recs = _solve(qp, case, th[:N], warm=w[:N], inplace=True)
            _expect(recs, case, level, packed, nwv, what=what + (N, "warm in place"))
            _same(got, refw, N, what + (N, "warm, in place"))
    qp.check()


@pytest.mark.parametrize("case", [wc.NTH0, wc.NTH0_F32], ids=ids)
def test_problem_without_parameters(lmpc, case):
    """nth = 0: theta has no columns and nothing is fetched; every point is the same problem.  Every launch choice, the
    batch sizes at the first one."""
    qp = _handle(lmpc, case)
    th = wc.theta(case)
    ref = _cached((case, "nth0"), lambda: _oracle(qp, case, th))
    print(case.name, wc.check_nth0(case, ref[1], ref[2], ref[3]))
    for k, (level, packed, nwv) in enumerate(wc.launches(case)):
        _pin(qp, level, packed, nwv)
        for N in (wc.batch_sizes(nwv) + (wc.N_COND,) if k == 0 else (wc.N_COND,)):
            got, recs = _solve(qp, case, th[:N])
            _expect(recs, case, level, packed, nwv, worklist=False, what=(case.name, level, packed, nwv, N))
            _same(got, ref, N, (case.name, level, packed, nwv, N))
    qp.check()


@pytest.mark.parametrize("kind", ["all-infeasible", "all-settled"])
@pytest.mark.parametrize("name", wc.LIMIT_BATCH_CASES)
def test_limit_batches(lmpc, name, kind):
    """A batch that is infeasible throughout and one that is feasible at iteration 1 throughout, cold and -- from the
    mixed batch's final sets -- warm, at every launch choice."""
    case = wc.BY_NAME[name]
    qp = _handle(lmpc, case)
    th = wc.limit_theta(case, kind)
    ref = _cached((case, kind), lambda: _oracle(qp, case, th))
    wc.check_limit_batch(case, ref[1], ref[2], ref[3], kind)
    w = wc.warm_masks(*_ref(case, qp)[1::2])
    refw = _cached((case, kind, "warm"), lambda: _oracle(qp, case, th, warm=w))
    for level, packed, nwv in wc.launches(case):
        _pin(qp, level, packed, nwv)
        got, recs = _solve(qp, case, th)
        _expect(recs, case, level, packed, nwv, worklist=False, what=(name, kind, level, packed, nwv))
        _same(got, ref, wc.N_COND, (name, kind, level, packed, nwv, "cold"))
        got, recs = _solve(qp, case, th, warm=w)
        _expect(recs, case, level, packed, nwv, what=(name, kind, level, packed, nwv))
        _same(got, refw, wc.N_COND, (name, kind, level, packed, nwv, "warm"))
    qp.check()


SEVERAL = tuple(c for c in wc.CASES if c.n > 1) + tuple(c for c in wc.F32_CASES if c.name.startswith(("nu2-mr2", "mr3")))


@pytest.mark.parametrize("case", SEVERAL, ids=ids)
def test_several_outputs(lmpc, case):
    """nout = a middle value and n (nout = 1: the tests above), at one launch choice per case, rotating through them;
    the long-horizon cases (n = 64, 65, 127; binary32: n = 65) bring working sets beyond 64 rows, i.e. big_kernel<double>
    and <float> with 32 and more outputs."""
    th = wc.theta(case)
    choices = wc.launches(case)
    for j, nout in enumerate(v for v in wc.nouts(case) if v > 1):
        level, packed, nwv = choices[(j + case.n) % len(choices)]
        qp = _handle(lmpc, case, nout)
        _pin(qp, level, packed, nwv)
        ref, (w, *refw) = _ref(case, qp, nout), _ref_warm(case, qp, nout)
        assert ref[0].shape == (wc.N_COND, nout)
        if case.n >= 64:
            assert (wc.popcount(ref[3][:333]) > 64).sum() >= wc.FLOOR, "points the slow path solves"
        got, recs = _solve(qp, case, th[:333])
        _expect(recs, case, level, packed, nwv, what=(case.name, nout))
        _same(got, ref, 333, (case.name, nout, "cold"))
        got, recs = _solve(qp, case, th[:333], warm=w[:333], inplace=True)
        _expect(recs, case, level, packed, nwv, what=(case.name, nout, "warm"))
        _same(got, refw, 333, (case.name, nout, "warm, in place"))
        qp.check()


# ------------------------------------------------------------------ searches
def _search_handle(lmpc, case):
    qp = _handle(lmpc, case)
    N = wc.N_BNB_TWO_PASS if case is wc.BNB_TWO_PASS else wc.N_COND
    th = wc.theta(case, N)

    def make():
        from dataclasses import replace
        from oracle import ldp as oldp
        out = _oracle(qp, case, th)
        L = _ldp(qp)
        Lr = replace(L, sense=(L.sense & ~wc.SENSE_BINARY).astype(np.int32))
        itr = oldp.solve_batch(Lr, th, qp._oset, dtype=case.dtype)[2]
        print(case.name, "searches of several nodes:", wc.check_search_conditions(case, out[2], itr, out[1]))
        return out
    return qp, th, _cached((case, "search"), make)


@pytest.mark.parametrize("case", wc.BNB_CASES, ids=ids)
def test_searches_every_launch_choice(lmpc, case):
    """wave_kernel<R, MR, LDSC, true, PACKED>: MR 1, 2, 4, 8, 16 in both real types, binaries next to general and SOFT
    rows, one pass; where a row-kernel shape exists (m <= 64) "row_kernel" 1 gives the same bits."""
    qp, th, ref = _search_handle(lmpc, case)
    for level, packed, nwv in wc.launches(case):
        _pin(qp, level, packed, nwv)
        got, recs = _solve(qp, case, th)
        _expect(recs, case, level, packed, nwv, worklist=False, what=(case.name, level, packed, nwv))
        _same(got, ref, wc.N_COND, (case.name, level, packed, nwv))
    level, packed, nwv = wc.launches(case)[1]
    _pin(qp, level, packed, nwv)
    for N in wc.batch_sizes(nwv):
        got, recs = _solve(qp, case, th[:N])
        _expect(recs, case, level, packed, nwv, worklist=False, what=(case.name, N))
        _same(got, ref, N, (case.name, level, packed, nwv, N))
    if case.m <= 64:
        qp.set_option("row_kernel", 1)
        got, recs = _solve(qp, case, th)
        # (the row kernel's own pass; the wavefront kernel at most as the second pass behind it)
        assert all(r["pass"] == 2 and r["BNB"] == 1 for r in recs), recs
        _same(got, ref, wc.N_COND, (case.name, "row_kernel 1"))
        qp.set_option("row_kernel", 0)
    qp.check()


def test_search_in_two_passes(lmpc):
    """bnb_first_pass_cap: 4096 searches of a problem whose full factor (62 rows) keeps fewer wavefronts resident than
    one of 24 rows -- first pass at "wave_cap1" 24, the points that outgrow it searched again from scratch at the full
    capacity; the same bits as the one-pass run and the oracle."""
    case = wc.BNB_TWO_PASS
    qp, th, ref = _search_handle(lmpc, case)
    level, packed, nwv = 0, False, 2
    _pin(qp, level, packed, nwv)
    one, recs = _solve(qp, case, th)
    _expect(recs, case, level, packed, nwv, what="one pass")
    _same(one, ref, len(th), "one pass")
    qp.set_option("wave_two_pass", 1)
    qp.set_option("wave_cap1", 24)
    two, recs = _solve(qp, case, th)
    _expect(recs, case, level, packed, nwv, passes=(1, 2), caps=(24, case.cap), what="two passes")
    _same(two, ref, len(th), "two passes")
    assert (wc.popcount(ref[3]) > 24).sum() >= wc.FLOOR, "searches whose final set outgrows the first pass"
    qp.check()


# ------------------------------------------------------------------ two passes, slow path
@pytest.mark.parametrize("kind", ["none", "all", "mixed"])
def test_two_passes_equal_one(lmpc, kind):
    """ "wave_two_pass" 1 at "wave_cap1" 8, 24 and 48 on a problem of capacity 49: batches of which no point, every
    point, and a part outgrow the first pass; records show pass 1 at the smaller capacity, then pass 2 at the full one
    walking the first one's overflow list with the slow path behind it."""
    case = wc.TWO_PASS
    qp = _handle(lmpc, case)
    th = wc.two_pass_theta(kind)
    ref = _cached((case, kind), lambda: _oracle(qp, case, th))
    for k, c1 in enumerate(wc.CAP1):
        level, packed, nwv = wc.launches(case)[k]
        _pin(qp, level, packed, nwv)
        print(kind, c1, wc.check_two_pass_share(case, ref[3], c1, kind))
        qp.set_option("wave_two_pass", 0)
        one, recs = _solve(qp, case, th)
        _expect(recs, case, level, packed, nwv, what=(kind, c1, "one pass"))
        qp.set_option("wave_two_pass", 1)
        qp.set_option("wave_cap1", c1)
        two, recs = _solve(qp, case, th)
        _expect(recs, case, level, packed, nwv, passes=(1, 2), caps=(c1, case.cap), worklist=False, what=(kind, c1, "two passes"))
        _same(one, ref, wc.N_COND, (kind, c1, "one pass"))
        _same(two, ref, wc.N_COND, (kind, c1, "two passes"))
        w = wc.warm_masks(ref[1], ref[3])
        refw = _cached((case, kind, "warm"), lambda: _oracle(qp, case, th, warm=w))
        got, recs = _solve(qp, case, th, warm=w)
        _expect(recs, case, level, packed, nwv, passes=(1, 2), caps=(c1, case.cap), what=(kind, c1, "two passes, warm"))
        _same(got, refw, wc.N_COND, (kind, c1, "two passes, warm"))
    qp.check()


@pytest.mark.parametrize("case", [wc.SLOW, wc.SLOW_F32], ids=ids)
def test_slow_path_behind_one_and_two_passes(lmpc, case):
    """big_kernel<double> and <float>: working sets of up to 150 rows behind the wavefront kernel's 64, behind one pass
    and as the third stage behind two; "big_path" 0 shows the wavefront kernel's own flag -7 on exactly those points."""
    qp = _handle(lmpc, case, prob=wc.slow_problem(case))
    th = wc.slow_theta(case)
    ref = _cached((case, "slow"), lambda: _oracle(qp, case, th))
    st = wc.check_wave_conditions(case, ref[1], ref[2], ref[3])
    assert st["beyond64"] >= wc.FLOOR, st
    level, packed, nwv = wc.launches(case)[1]
    _pin(qp, level, packed, nwv)
    got, recs = _solve(qp, case, th)
    _expect(recs, case, level, packed, nwv, what=(case.name, "one pass"))
    _same(got, ref, wc.N_COND, (case.name, "one pass"))
    qp.set_option("wave_two_pass", 1)
    qp.set_option("wave_cap1", 24)
    got, recs = _solve(qp, case, th)
    _expect(recs, case, level, packed, nwv, passes=(1, 2), caps=(24, case.cap), what=(case.name, "two passes"))
    _same(got, ref, wc.N_COND, (case.name, "third stage behind two passes"))
    qp.set_option("wave_two_pass", 0)
    w = wc.warm_masks(ref[1], ref[3])
    got, recs = _solve(qp, case, th, warm=w)
    _expect(recs, case, level, packed, nwv, what=(case.name, "warm"))
    _same(got, _oracle(qp, case, th, warm=w), wc.N_COND, (case.name, "warm"))
    qp.set_option("big_path", 0)
    (x, ef, it, act), recs = _solve(qp, case, th)
    assert recs[0]["big"] == 0
    over = ef == -7
    assert over.sum() >= wc.FLOOR and (wc.popcount(ref[3])[over] >= 60).all()
    assert np.array_equal(ef[~over], ref[1][~over]) and np.array_equal(x[~over], ref[0][~over])
    qp.check()


# ------------------------------------------------------------------ work-list mode, ticket queue
def test_work_list_mode_behind_the_screening_pass(lmpc):
    """ "screen_wave" 1: the wavefront kernel walks the 64 segments the screening pass filled -- a batch that leaves
    segments empty (the prefix sum over empty segments) and one that fills every segment."""
    case = wc.QUEUE
    qp = _handle(lmpc, case)
    qp.set_option("screen_wave", 1)
    for N, kind in ((2309, "some-empty"), (wc.N_FILL, "all-filled")):
        th = wc.theta(case, N, batch=3)
        ref = _cached((case, "list", N), lambda: _oracle(qp, case, th))
        print(kind, wc.check_segments(ref[2], kind))
        for level, packed, nwv in wc.launches(case)[::2]:
            _pin(qp, level, packed, nwv)
            got, recs = _solve(qp, case, th)
            _expect(recs, case, level, packed, nwv, worklist=True, what=(kind, level, packed, nwv))
            assert recs[0]["queue"] == 1 and recs[0]["qchunk"] == 1
            _same(got, ref, N, (kind, level, packed, nwv))
        qp.set_option("wave_queue", 0)
        got, recs = _solve(qp, case, th)
        assert recs[0]["queue"] == 0 and recs[0]["worklist"] == 1
        _same(got, ref, N, (kind, "static split of the list"))
        qp.set_option("wave_queue", 1)
    qp.check()


def test_ticket_queue_against_the_static_split(lmpc):
    """A grid of one single-wavefront workgroup per CU ("wave_waves" 1, "wave_nwv" 1) and 9001 points: more than two per
    resident wavefront, so the problems are handed out through the ticket counter, several per ticket; "wave_queue" 0
    splits the batch statically.  Also at a many-slot case."""
    for case in (wc.QUEUE, wc.BY_NAME["mr8-n6-m480-nth5"]):
        qp = _handle(lmpc, case)
        qp.set_option("wave_waves", 1)
        th = wc.theta(case, wc.N_QUEUE, batch=4)
        ref = _cached((case, "queue"), lambda: _oracle(qp, case, th))
        assert (ref[2] != 1).sum() >= 1000
        for packed in (False, True):
            _pin(qp, 1, packed, 1)
            for queue in (1, 0):
                qp.set_option("wave_queue", queue)
                got, recs = _solve(qp, case, th)
                _expect(recs, case, 1, packed, 1, worklist=False, what=(case.name, packed, queue))
                r = recs[0]
                assert r["queue"] == queue and wc.N_QUEUE > 2 * r["grid"] * r["nwv"], r
                want = max(1, min(64, wc.N_QUEUE // (16 * r["grid"] * r["nwv"]))) if queue else 1
                assert r["qchunk"] == want and (not queue or want >= 2), r
                _same(got, ref, wc.N_QUEUE, (case.name, packed, queue))
        qp.check()


# ------------------------------------------------------------------ closed loop
def _sim_handle(lmpc, case):
    qp = _handle(lmpc, case, wc.sim_nu(case))
    qp.set_option("screen_wave", 1)
    return qp


def _loop_ref(case, qp, warm):
    F, G, x0 = wc.sim_data(case)

    def make():
        ref = lr.simulate_reference(_ldp(qp), x0, wc.T_LOOP, F, G, warm=warm, settings=qp._oset)
        wc.check_loop_steps(case, ref["flags"], ref["active"])
        return ref
    return _cached((case, "loop", warm), make)


def _expect_loop(recs, case, level, packed, nwv, sim, what):
    """Launch records of a closed loop (the ring keeps the last four): the instantiation and the launch configuration."""
    assert recs, what
    for r in recs:
        got = (r["real_bytes"], r["MR"], r["LDSC"], r["BNB"], r["PACKED"], r["NU"], r["GRAM"], r["SIM"])
        assert got == (8, case.MR, level, 0, int(packed), case.NU, 0, int(sim)), (what, r)
        assert (r["level"], r["nwv"], r["pass"], r["cap"], r["big"]) == (level, nwv, 0, case.cap, 1), (what, r)


def _same_loop(got, want, what):
    for key in ("U", "X", "x", "flag_min"):
        a, b = got[key], want[key]
        assert a.shape == b.shape and np.array_equal(a, b), (what, key, np.argwhere(a != b)[:4].tolist())


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("case", wc.SIM_CASES, ids=ids)
def test_closed_loop_every_launch_choice(lmpc, case, warm):
    """lmpc_simulate, lock-step with the plant step fused into the wavefront kernel ("sim_async" 0; warm: from the
    previous step's masks, "sim_keep_factor" 0): T = 3, 300 scenarios, every launch choice -- the SIM = true
    instantiations of the binary64 unit, one or two variable slots, MR 1 ... 6 (built with run-ahead) and 8, 16."""
    qp = _sim_handle(lmpc, case)
    qp.set_option("sim_async", 0)
    qp.set_option("sim_keep_factor", 0)
    F, G, x0 = wc.sim_data(case)
    ref = _loop_ref(case, qp, warm)
    for level, packed, nwv in wc.sim_launches(case):
        _pin(qp, level, packed, nwv)
        since = _seq(qp)
        got = qp.simulate(x0, wc.T_LOOP, F, G, warm=warm)
        recs = qp.wave_launch_info(since)
        assert len(recs) == wc.T_LOOP, recs
        _expect(recs, case, level, packed, nwv, sim=True, passes=(0,) * wc.T_LOOP, worklist=True,
                what=(case.name, level, packed, nwv, warm))
        _same_loop(got, ref, (case.name, level, packed, nwv, warm))
    qp.check()


@pytest.mark.parametrize("name", wc.SIM_MODE_CASES)
def test_closed_loop_scenario_counts(lmpc, name):
    """1, nwv - 1, nwv, nwv + 1 scenarios (scenarios are independent: the references are the leading rows of the
    300-scenario run's), lock-step fused loop, cold and warm."""
    case = wc.BY_NAME[name]
    qp = _sim_handle(lmpc, case)
    qp.set_option("sim_async", 0)
    qp.set_option("sim_keep_factor", 0)
    F, G, x0 = wc.sim_data(case)
    level, packed, nwv = wc.sim_launches(case)[1]
    _pin(qp, level, packed, nwv)
    for warm in (False, True):
        ref = _loop_ref(case, qp, warm)
        for S in (v for v in wc.batch_sizes(nwv) if v < 300):
            since = _seq(qp)
            got = qp.simulate(x0[:S], wc.T_LOOP, F, G, warm=warm)
            _expect_loop(qp.wave_launch_info(since), case, level, packed, nwv, True, (name, S, warm))
            want = dict(U=ref["U"][:, :S], X=ref["X"][:, :S], x=ref["x"][:S], flag_min=ref["flag_min"][:S])
            _same_loop(got, want, (name, S, warm))
    qp.check()


def _simulate_device(lmpc, qp, x0, T, F, G, warm):
    """lmpc_simulate_device on guarded device buffers."""
    import torch
    from linearmpc_jl_amd._cabi import check, lib
    S, nx, nu, Gd = len(x0), x0.shape[1], qp.nout, wc.GUARD
    full = lambda n, v, dt: torch.full((n + Gd,), v, dtype=dt, device="cuda:0")
    x = full(S * nx, float("nan"), torch.float64)
    x[:S * nx] = torch.from_numpy(np.ascontiguousarray(x0)).cuda().reshape(-1)
    U, X = full(T * S * nu, float("nan"), torch.float64), full((T + 1) * S * nx, float("nan"), torch.float64)
    fm = full(S, SENT, torch.int32)
    Fh, Gh = np.ascontiguousarray(F, dtype=np.float64), np.ascontiguousarray(G, dtype=np.float64)
    vp = ctypes.c_void_p
    st = torch.cuda.current_stream().cuda_stream
    check(lib().lmpc_simulate_device(qp._h, S, T, nx, 0, 0, vp(Fh.ctypes.data), vp(Gh.ctypes.data), vp(x.data_ptr()), None, None,
                                     vp(U.data_ptr()), vp(X.data_ptr()), vp(fm.data_ptr()), int(warm), vp(st)), qp._h)
    torch.cuda.synchronize()
    xs, Us, Xs, fms = (t.cpu().numpy() for t in (x, U, X, fm))
    assert np.isnan(xs[S * nx:]).all() and np.isnan(Us[T * S * nu:]).all() and np.isnan(Xs[(T + 1) * S * nx:]).all() and \
        (fms[S:] == SENT).all(), "a store behind the buffers"
    return dict(x=xs[:S * nx].reshape(S, nx), U=Us[:T * S * nu].reshape(T, S, nu), X=Xs[:(T + 1) * S * nx].reshape(T + 1, S, nx),
                flag_min=fms[:S])


@pytest.mark.parametrize("name", wc.SIM_MODE_CASES)
def test_closed_loop_execution_modes(lmpc, name):
    """ "sim_keep_factor" 0 / 1 x "sim_fused" 0 / 1 x "sim_async" 0 / 1 / 2 at one small and one many-slot case, cold and
    warm, through lmpc_simulate_device on guarded buffers: the rounds with run-ahead (MR <= 6), the rounds without
    (MR = 8), the fused and the plain lock-step loop.  A warm loop on the kept factorisation is the oracle's warm == 2;
    the rounds without run-ahead start every step from the masks whatever "sim_keep_factor" says (the oracle's warm == 1)."""
    from oracle import ldp as oldp
    case = wc.BY_NAME[name]
    F, G, x0 = wc.sim_data(case)
    qp = _sim_handle(lmpc, case)
    level, packed, nwv = wc.sim_launches(case)[1]
    _pin(qp, level, packed, nwv)
    slots = (case.m + 63) // 64
    for warm in (False, True):
        ref = _loop_ref(case, qp, warm)
        kept = oldp.simulate(_ldp(qp), x0, wc.T_LOOP, F, G, settings=qp._oset, warm=2) if warm else None
        for keep in (0, 1):
            for fused in (0, 1):
                for asyn in (0, 1, 2):
                    for k, v in (("sim_keep_factor", keep), ("sim_fused", fused), ("sim_async", asyn)):
                        qp.set_option(k, v)
                    what = (name, "warm" if warm else "cold", keep, fused, asyn)
                    since = _seq(qp)
                    got = _simulate_device(lmpc, qp, x0, wc.T_LOOP, F, G, warm)
                    recs = qp.wave_launch_info(since)
                    # (mirrors lmpc_simulate_device, lmpc_api_loop.hip: `runAhead`, `waveAsync`, the ensure_keep call in
                    # front of the lock-step loops, and launch_wave_t's choice of the SIM instantiation in lmpc_api.hip;
                    # RUN_AHEAD_SLOTS is kWaveRunAheadSlots of lmpc_wave_layout.hpp -- a change there changes this)
                    run_ahead = (not warm or keep == 1) and slots <= wc.RUN_AHEAD_SLOTS
                    rounds = asyn == 2 or (asyn == 1 and run_ahead)
                    sim = rounds or fused == 1 or (warm and keep == 1)
                    # (the factor is kept between steps by run-ahead inside the rounds, or by the lock-step loops; rounds
                    # without run-ahead -- eight slots and more -- start every step from the masks)
                    on_factor = warm and keep == 1 and (run_ahead or not rounds)
                    _expect_loop(recs, case, level, packed, nwv, sim, what)
                    _same_loop(got, kept if on_factor else ref, what)
    qp.check()


# ------------------------------------------------------------------ sequences on one handle
SEQ_CASES = tuple(wc.BY_NAME[s] for s in ("mr2-n3-m65-nth2", "mr6-n6-m350-nth5"))


def test_one_pass_two_passes_one_pass(lmpc):
    """The overflow counters alternate per call and every call clears the set of the next one -- a one-pass call too
    (lmpc_wave_kernel.hpp names the past defect): one and two passes in every order on one handle, with batches whose
    first pass overflows nothing, everything and a part."""
    case = wc.TWO_PASS
    qp = _handle(lmpc, case)
    level, packed, nwv = wc.launches(case)[0]
    _pin(qp, level, packed, nwv)
    qp.set_option("wave_cap1", 24)
    batches = {kind: wc.two_pass_theta(kind) for kind in ("mixed", "all", "none")}
    refs = {kind: _cached((case, kind), lambda: _oracle(qp, case, batches[kind])) for kind in batches}
    for j, tp in enumerate((0, 1, 0, 0, 1, 1, 0, 1, 1, 0)):
        kind = ("mixed", "all", "none")[j % 3]
        qp.set_option("wave_two_pass", tp)
        got, recs = _solve(qp, case, batches[kind])
        _expect(recs, case, level, packed, nwv, passes=(1, 2) if tp else (0,), caps=(24, case.cap) if tp else None, what=(j, tp, kind))
        _same(got, refs[kind], wc.N_COND, (j, tp, kind))
    qp.check()


@pytest.mark.parametrize("case", SEQ_CASES, ids=ids)
def test_cold_warm_cold_and_solve_simulate_solve(lmpc, case):
    """cold, warm, cold; a closed loop (cold and warm) between plain solves; lmpc_release_scratch in between."""
    qp = _sim_handle(lmpc, case)
    nu = wc.sim_nu(case)
    ref, (w, *refw) = _ref(case, qp, nu), _ref_warm(case, qp, nu)
    th = wc.theta(case)
    level, packed, nwv = wc.launches(case)[1]
    _pin(qp, level, packed, nwv)
    N = 333
    F, G, x0 = wc.sim_data(case)

    def plain(tag):
        got, recs = _solve(qp, case, th[:N])
        _expect(recs, case, level, packed, nwv, worklist=True, what=(case.name, tag))
        _same(got, ref, N, (case.name, tag, "cold"))
        got, recs = _solve(qp, case, th[:N], warm=w[:N])
        _expect(recs, case, level, packed, nwv, worklist=True, what=(case.name, tag, "warm"))
        _same(got, refw, N, (case.name, tag, "warm"))
        got, recs = _solve(qp, case, th[:N])
        _expect(recs, case, level, packed, nwv, worklist=True, what=(case.name, tag, "cold again"))
        _same(got, ref, N, (case.name, tag, "cold again"))

    def loop(warm, want, tag):
        # (the handle's default loop: the rounds with run-ahead, MR <= 6 -- the SIM = true instantiation)
        since = _seq(qp)
        got = qp.simulate(x0, wc.T_LOOP, F, G, warm=warm)
        _expect_loop(qp.wave_launch_info(since), case, level, packed, nwv, True, (case.name, tag))
        _same_loop(got, want, (case.name, tag))
    plain("first")
    from oracle import ldp as oldp
    for warm in (False, True):
        # (warm on the kept factorisation: the oracle's warm == 2)
        want = oldp.simulate(_ldp(qp), x0, wc.T_LOOP, F, G, settings=qp._oset, warm=2) if warm else _loop_ref(case, qp, False)
        loop(warm, want, ("simulate", warm))
        plain(("after simulate", warm))
    qp.release_scratch()
    plain("after release_scratch")
    loop(False, _loop_ref(case, qp, False), "simulate after release_scratch")
    qp.check()


def test_binary64_and_binary32_handles_interleaved(lmpc):
    """Handles of the same problem in both real types, their calls interleaved on one stream: the counters, lists and
    the binary32 copy of the pack are each handle's own."""
    c64 = wc.BY_NAME["mr3-n6-m160-nth4"]
    c32 = next(c for c in wc.F32_CASES if c.name == c64.name + "-f32")
    q64, q32 = _handle(lmpc, c64), _handle(lmpc, c32)
    r64, r32 = _ref(c64, q64), _ref(c32, q32)
    lv64, lv32 = wc.launches(c64)[1], wc.launches(c32)[2]
    _pin(q64, *lv64)
    _pin(q32, *lv32)
    for k in range(4):
        for qp, case, ref, lv in ((q64, c64, r64, lv64), (q32, c32, r32, lv32))[::(1 if k % 2 == 0 else -1)]:
            N = (wc.N_COND, 65, 333, 1)[k]
            got, recs = _solve(qp, case, wc.theta(case, N))
            _expect(recs, case, *lv, what=(case.name, k))
            _same(got, ref, N, (case.name, k))
        if k == 1:
            q64.release_scratch()
            q32.release_scratch()
    q64.check()
    q32.check()
