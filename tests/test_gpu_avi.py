"""The variational chain -- avi_tiers_kernel<N, K, false>, avi_lane_kernel<N, LIST>, avi_kernel<LDSC, PROX>
(lmpc_avi.hip::launch_avi) -- at every one of its 38 instantiations, against the oracle on the handle's own pack, bit for
bit: np.array_equal on x, exitflag, iters and active.  Cases, the restated launch arithmetic, the rules for which kernel
finishes which point and the conditions that keep a comparison from passing emptily: tests/avi_cases.py (checked on the
host in tests/test_avi_cases_host.py, re-asserted here on the oracle's trace for the handle's pack).

All three kernels give the same bits from scratch, so equal outputs do not show which kernel finished a point.  Every
test therefore
  1. reads the handle's launch record (lmpc_avi_launch_info) FIRST and asserts stage, N, K, LIST, LDSC, PROX, LDS bytes,
     workgroups (the restated arithmetic with the device's CU count and the recorded occupancy), nprob and seg_cap;
  2. compares the bits;
  3. reads the snapshots of both work lists ("list_snapshot" 1, lmpc_avi_list_read) and asserts that, segment by
     segment, they hold exactly the points avi_cases.expected_lists() names: no tolerance on a count.

Every output of a device call is allocated with GUARD rows behind row N and pre-filled with sentinels; the guard rows
must come back untouched and no sentinel may survive in rows 0 ... N - 1."""
import warnings

import numpy as np
import pytest

import avi_cases as ac

pytestmark = pytest.mark.gpu

SENT = 12345
ACT_SENT = 0x5A5A5A5A5A5A5A5A              # (32 bits set in a word: more rows than any working set here holds)
_SEEN = set()                              # instantiations asserted in some record, for the last test of the file
_RAN = {"chain": 0, "slab": 0}             # ... and how many of the tests that collect them have passed


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


def _settings(lmpc, iter_limit=0, eps_prox=0.0):
    s = lmpc.default_settings()
    if iter_limit:
        s.iter_limit = iter_limit
    if eps_prox:
        s.eps_prox, s.eta_prox = eps_prox, ac.ETA_PROX
    return s


def _handle(lmpc, case, kfirst=-1, iter_limit=0, options=()):
    H, f, f_theta, A, bu, bl, W, sense = ac.problem(case)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, senses=sense, nout=case.nout,
                                  settings=_settings(lmpc, iter_limit), is_avi=True)
    assert qp.is_avi and qp.kernel_name == "avi_tiers<%d>|avi" % case.n, qp.kernel_name
    assert (qp.n, qp.m, qp.ms, qp.nth, qp.nout, qp.words) == (case.n, case.n, case.n, case.nth, case.nout, 1)
    qp.set_option("list_snapshot", 1)
    qp.set_option("avi_tiers_first", kfirst)
    for k, v in options:
        qp.set_option(k, v)
    return qp


def _oracle_pack(qp):
    from oracle import avi as oavi
    pk = qp.avi_pack()
    return oavi.AVI(pk["n"], pk["m"], pk["ms"], pk["nth"], pk["nout"], pk["ML"], pk["MR"], pk["G"], pk["du"], pk["dl"],
                    pk["Dth"], pk["Rout"], pk["x0"], pk["Xth"], pk["sense"], np.ones(pk["m"])).contiguous()


_REF = {}


def _ref(case, qp, iter_limit=0):
    """The oracle with its trace on the handle's pack for the case's condition batch, computed once per (case, limit) and
    never written to (the pack depends on the problem alone); a smaller batch is a prefix of it, a larger one repeats it."""
    key = (case, iter_limit)
    if key not in _REF:
        out = ac.reference(case, ac.theta(case, ac.N_COND), P=_oracle_pack(qp), iter_limit=iter_limit)
        for a in out[:4]:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _sized(ref, N):
    if N <= ac.N_COND:
        return tuple(a[:N] for a in ref[:4]) + (ac._head(ref[4], N),)
    reps = -(-N // ac.N_COND)
    return tuple(np.ascontiguousarray(np.concatenate([a] * reps)[:N]) for a in ref[:4]) + (ac.tiled_trace(ref[4], N),)


class _Guarded:
    """Outputs of one device call with GUARD sentinel rows behind them."""

    def __init__(self, N, nout, words):
        import torch
        G, dev = ac.GUARD, "cuda:0"
        self.N = N
        self.x = torch.full((N + G, nout), float("nan"), dtype=torch.float64, device=dev)
        self.ef = torch.full((N + G,), SENT, dtype=torch.int32, device=dev)
        self.it = torch.full((N + G,), SENT, dtype=torch.int32, device=dev)
        self.act = torch.full((N + G, words), ACT_SENT, dtype=torch.int64, device=dev)

    def read(self):
        N = self.N
        x, ef, it, act = self.x.cpu().numpy(), self.ef.cpu().numpy(), self.it.cpu().numpy(), self.act.cpu().numpy()
        assert np.isnan(x[N:]).all() and (ef[N:] == SENT).all() and (it[N:] == SENT).all() and (act[N:] == ACT_SENT).all(), \
            "a store behind the batch"
        assert not np.isnan(x[:N]).any() and not (ef[:N] == SENT).any() and not (it[:N] == SENT).any() and \
            not (act[:N] == ACT_SENT).any(), ("rows the kernels never wrote", np.flatnonzero(ef[:N] == SENT)[:8])
        return x[:N], ef[:N], it[:N], act[:N].view(np.uint64)


def _seq(qp):
    r = qp.avi_launch_info()
    return r[-1]["seq"] if r else 0


def _solve(qp, th, warm=None):
    """One lmpc_solve_batch_device call on guarded outputs: ((x, exitflag, iters, active), the call's launch records)."""
    import torch
    N = len(th)
    seq = _seq(qp)
    th_d = torch.from_numpy(np.ascontiguousarray(th)).cuda()
    g = _Guarded(N, qp.nout, qp.words)
    w_d = None if warm is None else torch.from_numpy(np.array(warm).view(np.int64)).cuda()
    qp.solve_device(th_d, x=g.x[:N], exitflag=g.ef[:N], iters=g.it[:N], active=g.act[:N], warm=w_d)
    torch.cuda.synchronize()
    recs = qp.avi_launch_info(seq)
    assert [r["seq"] for r in recs] == list(range(seq + 1, seq + 1 + len(recs))), recs
    return g.read(), recs


def _expect_chain(Q, recs, n, nout, kfirst, N, cus, what, cap=0, seg_n=None, waves=0):
    """The records of one call that runs the chain: three launches in the restated shapes."""
    assert len(recs) == 3, (what, "launches of the call", recs)
    a, b, c = recs
    seg = ac.seg_cap(N if seg_n is None else seg_n)
    kf = ac.default_kfirst(n) if kfirst < 0 else kfirst
    if kf == 0:
        want = dict(stage=Q.AVI_LANE, N=n, K=0, LIST=0, LDSC=0, PROX=0, lds=ac.lane_lds_bytes(n))
    else:
        want = dict(stage=Q.AVI_TIERS, N=n, K=ac.tiers_k(n, kf), LIST=0, LDSC=0, PROX=0, lds=ac.tiers_lds_bytes(n, nout))
    assert {k: a[k] for k in want} == want, (what, "first launch", a, want)
    want = dict(stage=Q.AVI_LANE, N=n, K=0, LIST=1, LDSC=0, PROX=0, lds=ac.lane_lds_bytes(n))
    assert {k: b[k] for k in want} == want, (what, "second launch", b, want)
    for r in (a, b):
        assert 1 <= r["occ"] <= 8 and r["grid"] == ac.chain_grid(N, cus, r["occ"], cap), (what, "workgroups", r, cus)
        assert r["nprob"] == N and r["seg_cap"] == seg, (what, "batch / seg_cap", r, seg)
    want = dict(stage=Q.AVI_SLAB, N=0, K=0, LIST=1, LDSC=1, PROX=0, lds=ac.pack_bytes(n, n, _NTH[what[0]], nout),
                grid=ac.slab_grid(N, cus, n, n, 0, True, waves, cap), occ=waves or 16, nprob=N, seg_cap=seg)
    assert {k: c[k] for k in want} == want, (what, "third launch", c, want)
    _SEEN.add(("tiers", n, a["K"], False) if a["stage"] == Q.AVI_TIERS else ("lane", n, False))
    _SEEN.add(("lane", n, True))
    _SEEN.add(("slab", True, False))
    return a, b, c


_NTH = {c.name: c.nth for c in ac.BY_NAME.values()}


def _same(got, ref, what):
    for name, a, r in zip(("x", "exitflag", "iters", "active"), got, ref):
        assert a.shape == r.shape, (what, name, a.shape, r.shape)
        if not np.array_equal(a, r):
            bad = np.flatnonzero((a != r).reshape(len(a), -1).any(axis=1))
            raise AssertionError((what, name, f"{len(bad)} of {len(a)} rows differ", bad[:8].tolist(),
                                  a[bad[:3]].tolist(), r[bad[:3]].tolist()))


def _lists(qp, n, kfirst, ref, N, what, seg_n=None):
    """Both snapshots of the call against the rules, on the oracle's outputs and trace for the same N points.  Returns
    (entries of list 0, entries of list 1)."""
    kf = ac.default_kfirst(n) if kfirst < 0 else kfirst
    want = ac.expected_lists(n, kf, ref[1], ref[4])
    out = []
    for which in (0, 1):
        snap = qp.avi_list_read(which)
        assert snap is not None, (what, "no snapshot of list", which)
        counts, lst = snap
        assert lst.shape == (ac.K_SHARDS, ac.seg_cap(N if seg_n is None else seg_n)), (what, lst.shape)
        ac.check_list(counts, lst, want[which], what + ("list", which), runs=which == 0)
        out.append(int(counts.sum()))
    return tuple(out)


def _run(lmpc, qp, case, kfirst, ref, N, cus, cap=0, seg_n=None, tag=""):
    """Records first, then the bits, then the lists."""
    what = (case.name, kfirst, N, tag)
    got, recs = _solve(qp, ac.theta(case, N))
    _expect_chain(lmpc.BatchedQP, recs, case.n, case.nout, kfirst, N, cus, what, cap, seg_n)
    r = _sized(ref, N)
    _same(got, r, what)
    return _lists(qp, case.n, kfirst, r, N, what, seg_n)


# ------------------------------------------------------------------ every tiers and lane instantiation
_SHARES = {}


@pytest.mark.parametrize("kfirst", ac.KFIRSTS, ids=lambda k: f"first{k}")
@pytest.mark.parametrize("n", ac.NS, ids=lambda n: f"n{n}")
def test_every_tiers_and_lane_instantiation(lmpc, cus, n, kfirst):
    """For N = 2 ... 8 and "avi_tiers_first" 1, 2, 3 (avi_tiers_kernel<N, min(K, N)> + avi_lane_kernel<N, true>) and 0
    (avi_lane_kernel<N, false> over the whole batch): the condition batch of every family, then the base family at 1, 63,
    64 and 65 points.  The conditions are re-asserted on the oracle's trace for the handles' own packs."""
    results = []
    for case in ac.census_cases(n):
        qp = _handle(lmpc, case, kfirst)
        ref = _ref(case, qp)
        results.append((case,) + tuple(ref[1:]))
        q0, q1 = _run(lmpc, qp, case, kfirst, ref, ac.N_COND, cus)
        assert q0 == int((~ac.first_finish(n, kfirst, ref[1], ref[4])).sum()) and q1 == 0
        _SHARES[(case.name, kfirst)] = (ac.N_COND - q0, q0 - q1, q1)
        if case.family == "base":
            for N in ac.SIZES:
                _run(lmpc, qp, case, kfirst, ref, N, cus)
        qp.check()
        qp.close()
    ac.check_n_conditions(n, results)
    _RAN["chain"] += 1
    print(f"n = {n}, avi_tiers_first {kfirst}: points finished by (first launch, lane kernel, slab kernel):",
          {c.name: _SHARES[(c.name, kfirst)] for c in ac.census_cases(n)})


# ------------------------------------------------------------------ the second trip of the tile loops
@pytest.mark.parametrize("kfirst", (3, 1, 0), ids=lambda k: f"first{k}")
@pytest.mark.parametrize("n", (2, 4, 6, 7, 8), ids=lambda n: f"n{n}")
def test_second_trip_of_the_register_kernels(lmpc, cus, n, kfirst):
    """ "avi_chain_groups" at its minimum: 16 workgroups, 64 wavefronts, one tile of the first 64 each.  With 4096 + 65
    points wavefronts 0 and 1 run a second tile, the last one ragged (one point); with 2 x 4096 + 65 every wavefront runs
    a second tile and two a third.  The deferred push is carried across tiles, the parking areas and the register state
    are reused, and both snapshots still hold exactly the ruled points.  The lists behind are walked at a stride, too:
    a segment of list 0 holds more than 64 entries."""
    case = ac.BY_NAME[f"wide-n{n}"]
    qp = _handle(lmpc, case, kfirst, options=(("avi_chain_groups", 1),))
    ref = _ref(case, qp)
    for N in (ac.N_COND + 65, 2 * ac.N_COND + 65):
        assert ac.chain_grid(N, cus, 1, 1) == 16 and ac.tiles(N) > 64
        q0, q1 = _run(lmpc, qp, case, kfirst, ref, N, cus, cap=1)
        assert q1 == 0 and (q0 > 0 or kfirst != 1), (q0, q1)
    if kfirst == 1:
        r = _sized(ref, 2 * ac.N_COND + 65)
        assert max(len(s) for s in ac.expected_lists(n, 1, r[1], r[4])[0]) > 64, "the lane kernel strides its list, too"
    # the cap changes no bit and no list: the same batch at the default grid
    qp.set_option("avi_chain_groups", 0)
    _run(lmpc, qp, case, kfirst, ref, 2 * ac.N_COND + 65, cus)
    qp.check()
    qp.close()


# ------------------------------------------------------------------ call sequences on one handle
def test_two_calls_in_a_row_and_an_empty_first_list(lmpc, cus):
    """A large batch, then a small one, on one handle: seg_cap stays the larger batch's, both calls' lists are exact (the
    counters were cleared: cnt1 by the next call's first kernel, cnt0 by the slab kernel), and the record keeps both
    calls' six launches.  Then a batch whose first list is empty (every point ends at iteration 1): both later launches
    are still recorded, both lists are empty."""
    case = ac.BY_NAME["wide-n6"]
    qp = _handle(lmpc, case, 2, iter_limit=case.n + 2)
    ref = _ref(case, qp, case.n + 2)
    big = 2 * ac.N_COND + 65
    assert (ref[1] == -4).sum() >= 64, "list 1 is not empty: the limit acts"
    q = _run(lmpc, qp, case, 2, ref, big, cus, tag="large")
    q2 = _run(lmpc, qp, case, 2, ref, 65, cus, seg_n=big, tag="small after large")
    assert q[1] > q2[1] > 0 and q[0] > q2[0]
    recs = qp.avi_launch_info()
    assert len(recs) == 6 and [r["nprob"] for r in recs] == [big] * 3 + [65] * 3 and len({r["seg_cap"] for r in recs}) == 1
    _run(lmpc, qp, case, 2, ref, big, cus, tag="large again")
    _run(lmpc, qp, case, 2, ref, ac.N_COND, cus, seg_n=big, tag="and the condition batch")
    qp.release_scratch()
    assert qp.avi_list_read(0) is None and qp.avi_list_read(1) is None, "the snapshots went with the scratch"
    _run(lmpc, qp, case, 2, ref, 65, cus, tag="after release_scratch")          # (the lists are allocated again: 65 points)
    qp.check()
    qp.close()
    calm = ac.CALM
    for kfirst in (3, 0):
        qp = _handle(lmpc, calm, kfirst)
        ref = _ref(calm, qp)
        assert (ref[2] == 1).all()
        for N in (ac.N_COND, 65):
            assert _run(lmpc, qp, calm, kfirst, ref, N, cus, seg_n=ac.N_COND) == (0, 0)
        qp.check()
        qp.close()


# ------------------------------------------------------------------ iteration limits, warm starts, the option
@pytest.mark.parametrize("n", ac.NS, ids=lambda n: f"n{n}")
def test_iteration_limit_fills_the_second_list(lmpc, cus, n):
    """iter_limit = N + 2, the smallest the chain takes: list 1 is exactly the points the oracle stops at the limit, and
    the slab kernel writes them with the oracle's flag and count.  iter_limit = N + 1, a warm start and "avi_tiers" 0: no
    chain, ONE slab launch over the whole batch, no list."""
    case = ac.BY_NAME[f"wide-n{n}"] if n > 2 else ac.BY_NAME["base-n2"]
    Q = lmpc.BatchedQP
    qp = _handle(lmpc, case, iter_limit=n + 2)
    ref = _ref(case, qp, n + 2)
    stopped = int((ref[1] == -4).sum())
    assert stopped >= 8 and (ref[2][ref[1] == -4] == n + 2).all(), "the limit acts"
    for kfirst in (-1, 0):
        qp.set_option("avi_tiers_first", kfirst)
        q0, q1 = _run(lmpc, qp, case, kfirst, ref, ac.N_COND, cus)
        assert q1 == stopped
    # no chain: one launch, no list
    th = ac.theta(case, ac.N_COND)

    def alone(what, want, warm=None):
        got, recs = _solve(qp, th, warm=warm)
        assert len(recs) == 1, (what, recs)
        r = recs[0]
        exp = dict(stage=Q.AVI_SLAB, N=0, K=0, LIST=0, LDSC=1, PROX=0, lds=ac.pack_bytes(n, n, case.nth, case.nout),
                   grid=ac.slab_grid(ac.N_COND, cus, n, n, 0, False), occ=16, nprob=ac.N_COND, seg_cap=0)
        assert {k: r[k] for k in exp} == exp, (what, r, exp)
        _same(got, want, what)
        assert qp.avi_list_read(0) is None and qp.avi_list_read(1) is None, (what, "a list where no chain ran")

    from oracle import avi as oavi
    P = _oracle_pack(qp)
    qp.set_settings(_settings(lmpc, n + 1))
    assert not ac.uses_chain(n, n + 1)
    alone("iter_limit N + 1", oavi.solve_batch(P, th, ac.settings(n + 1)))
    qp.set_settings(_settings(lmpc))
    cold = _ref(case, qp)
    alone("warm start", oavi.solve_batch(P, th, warm=cold[3]), warm=cold[3])
    qp.set_option("avi_tiers", 0)
    alone('"avi_tiers" 0', cold[:4])
    qp.set_option("avi_tiers", 1)
    _run(lmpc, qp, case, 0, cold, ac.N_COND, cus, tag="back")
    qp.check()
    qp.close()


# ------------------------------------------------------------------ singular pivots
@pytest.mark.parametrize("case", ac.NEAR, ids=lambda c: c.name)
def test_singular_pivots_are_handed_down(lmpc, cus, case):
    """The near-singular family at the default settings: list 1 is exactly the points where the oracle met a pivot below
    zero_tol -- the lane kernel's hand-down that is not the iteration limit."""
    for kfirst in (-1, 0):
        qp = _handle(lmpc, case, kfirst)
        ref = _ref(case, qp)
        print(case.name, ac.check_near_conditions(case, ref[1], ref[4]))
        q0, q1 = _run(lmpc, qp, case, kfirst, ref, ac.N_COND, cus)
        assert q1 == int(ref[4].singular.sum()) > 0
        _run(lmpc, qp, case, kfirst, ref, 65, cus, seg_n=ac.N_COND)
        qp.check()
        qp.close()


# ------------------------------------------------------------------ the slab kernel's four instantiations
def _slab_handle(lmpc, case):
    H, f, f_theta, A, bu, bl, W, sense = ac.slab_problem(case)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, senses=sense, nout=case.nout,
                                  settings=_settings(lmpc, eps_prox=ac.EPS_PROX if case.prox else 0.0))
    assert qp.is_avi and qp.kernel_name == ("avi+prox" if case.prox else "avi"), qp.kernel_name
    assert (qp.n, qp.m, qp.ms, qp.nth, qp.nout, qp.words) == (case.n, case.m, case.ms, case.nth, case.nout, case.words)
    qp.set_option("list_snapshot", 1)
    return qp


@pytest.mark.parametrize("case", ac.SLAB_CASES, ids=lambda c: c.name)
def test_slab_kernel_instantiations_and_reused_slabs(lmpc, cus, case):
    """General and SOFT rows (outside the small case), the pack just under and just over the 64 KiB line, with and
    without eps_prox: LDSC and PROX from the record, LDS bytes = the pack's or 0, bits = the oracle's.  Then the same
    points under "avi_chain_groups" 1 and 2: one and two workgroups walk a batch of more than grid x 64 points, so every
    slab is initialised again for a second and a third problem."""
    from oracle import avi as oavi
    Q = lmpc.BatchedQP
    qp = _slab_handle(lmpc, case)
    P = _oracle_pack(qp)
    N = 256
    th = ac.slab_theta(case, N)
    if case.prox:
        ref = oavi.prox_solve_batch(P, qp.prox_pack(), th, ac.EPS_PROX, ac.ETA_PROX)
    else:
        ref = oavi.solve_batch(P, th)
    assert (ref[1] >= 1).sum() >= N // 4 and len(np.unique(ref[3], axis=0)) >= 8, "solved points, several active sets"
    pb = ac.pack_bytes(case.n, case.m, case.nth, case.nout, case.prox)
    ldsc = int(pb <= ac.LDS_PACK_LINE)
    assert ldsc == int(case in (ac.SLAB_UNDER, ac.SLAB_UNDER_PROX))
    for cap, n_pts in ((0, N), (0, 65), (1, N), (2, 193), (1, 65)):
        qp.set_option("avi_chain_groups", cap)
        got, recs = _solve(qp, th[:n_pts])
        assert len(recs) == 1, recs
        r = recs[0]
        exp = dict(stage=Q.AVI_SLAB, N=0, K=0, LIST=0, LDSC=ldsc, PROX=int(case.prox), lds=pb if ldsc else 0,
                   grid=ac.slab_grid(n_pts, cus, case.n, case.m, len(case.soft), False, 0, cap), occ=16, nprob=n_pts, seg_cap=0)
        assert {k: r[k] for k in exp} == exp, (case.name, cap, r, exp)
        if cap:
            assert r["grid"] == cap and n_pts > 64 * cap, "more points than grid x 64: slabs are reused"
        _same(got, tuple(a[:n_pts] for a in ref), (case.name, cap, n_pts))
        _SEEN.add(("slab", bool(ldsc), case.prox))
        assert qp.avi_list_read(0) is None
    _RAN["slab"] += 1
    qp.check()
    qp.close()


def test_slab_kernel_second_trip_behind_a_list(lmpc, cus):
    """Behind a list the slab kernel's grid is 64 workgroups at least, one per segment; at iter_limit = N + 2 the wide
    family leaves so many points at the limit that a segment of list 1 holds more than 64 of them at 4 x 4096 points:
    with "avi_chain_groups" 1 workgroup s walks segment s in several trips and its slab is initialised again each time."""
    case = ac.BY_NAME["wide-n8"]
    n = case.n
    qp = _handle(lmpc, case, iter_limit=n + 2, options=(("avi_chain_groups", 1),))
    ref = _ref(case, qp, n + 2)
    N = 4 * ac.N_COND
    r = _sized(ref, N)
    l1 = ac.expected_lists(n, ac.default_kfirst(n), r[1], r[4])[1]
    assert min(len(s) for s in l1) > 64, "every workgroup of the slab kernel takes a second trip"
    assert ac.slab_grid(N, cus, n, n, 0, True, 0, 1) == 64
    q0, q1 = _run(lmpc, qp, case, -1, ref, N, cus, cap=1)
    assert q1 == int((r[1] == -4).sum())
    qp.check()
    qp.close()


# ------------------------------------------------------------------ the options themselves
def test_snapshot_off_changes_no_call_and_on_refuses_a_capture(lmpc, cus):
    """With "list_snapshot" 0 (the default) a call records the same three launches and leaves no snapshot; with 1, a
    call inside a stream capture is refused before it enqueues anything.  "avi_chain_groups" defaults to off."""
    import torch
    case = ac.BY_NAME["base-n6"]
    qp = _handle(lmpc, case)
    qp.set_option("list_snapshot", 0)
    ref = _ref(case, qp)
    th = ac.theta(case, ac.N_COND)
    for call in range(2):
        got, recs = _solve(qp, th)
        _expect_chain(qp, recs, case.n, case.nout, -1, ac.N_COND, cus, (case.name, "off", call))
        _same(got, ref[:4], ("off", call))
        assert qp.avi_list_read(0) is None and qp.avi_list_read(1) is None, "a snapshot with the option off"
    qp.set_option("list_snapshot", 1)
    _run(lmpc, qp, case, -1, ref, ac.N_COND, cus, tag="on")
    th_d = torch.from_numpy(th).cuda()
    x = torch.zeros((ac.N_COND, qp.nout), dtype=torch.float64, device="cuda")
    ef = torch.zeros(ac.N_COND, dtype=torch.int32, device="cuda")
    seq = _seq(qp)
    st = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # (torch remarks that the captured graph is empty: it must be)
        with torch.cuda.stream(st):
            with torch.cuda.graph(graph, stream=st):
                with pytest.raises(lmpc.LmpcError, match="stream capture"):
                    qp.solve_device(th_d, x=x, exitflag=ef, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert _seq(qp) == seq
    _run(lmpc, qp, case, -1, ref, ac.N_COND, cus, tag="after the refused capture")
    qp.check()
    qp.close()


def test_every_instantiation_appears_in_an_asserted_record():
    """The tests above assert a record for each of the 38 instantiations: by their parameters (every (N, first) of
    test_every_tiers_and_lane_instantiation asserts the first launch's and the second's template arguments, every case of
    test_slab_kernel_instantiations_and_reused_slabs LDSC and PROX), and -- when the whole file has run in this process,
    as it does in the suite -- by the records they actually saw."""
    inst = ac.instantiations()
    want = {("tiers",) + t for t in inst["tiers"]} | {("lane",) + t for t in inst["lane"]} | {("slab",) + t for t in inst["slab"]}
    by_params = {("tiers", n, ac.tiers_k(n, kf), False) for n in ac.NS for kf in ac.KFIRSTS if kf} | \
                {("lane", n, False) for n in ac.NS if 0 in ac.KFIRSTS} | {("lane", n, True) for n in ac.NS} | \
                {("slab", ac.pack_bytes(c.n, c.m, c.nth, c.nout, c.prox) <= ac.LDS_PACK_LINE, c.prox) for c in ac.SLAB_CASES}
    assert len(want) == 38 and by_params == want, sorted(want ^ by_params, key=str)
    assert _SEEN <= want, sorted(_SEEN - want, key=str)
    if _RAN["chain"] == len(ac.NS) * len(ac.KFIRSTS) and _RAN["slab"] == len(ac.SLAB_CASES):
        assert _SEEN == want, sorted(want - _SEEN, key=str)
