"""The one-launch kernel's staged write-out (lmpc_fast_kernel.hpp, fast_staged_kernel): a call that returns x and the exit flags
alone keeps both in LDS and stores a workgroup's range once, as whole lines, at the workgroup's end.  Only where and
when bytes are stored changes, so every comparison is np.array_equal with the oracle on the handle's own pack
(tests/fast_cases.py, as tests/test_gpu_fast.py), and which path ran is READ from the handle's launch record
(lmpc_fast_launch_info), never inferred.  By default the launcher stages only under the hint "in_flight" >= 2 (a call
issued alone has the write-out on its critical path); "fast_stage" 1 asks for it wherever it applies, which is how the
other launch shapes are reached here.

Outputs carry GUARD sentinel rows behind row N (and, for the offset views, the elements in front of row 0): they must
come back untouched, and no sentinel may survive in rows 0 ... N - 1 -- the write-out's range ends at
min(last tile of the workgroup, N), which is where a stray store would land."""
import numpy as np
import pytest

import fast_cases as fc
from conftest import oracle_ldp_from

pytestmark = pytest.mark.gpu

SENT = 12345
ACT_SENT = 0x5A5A5A5A5A5A5A5A
PAIRS = ((5, 7), (2, 1), (3, 9), (4, 16))
SIZES = (1, 63, 64, 65, 705, 2309)     # one tile and a partial one, one workgroup and several (2309: 37 tiles)


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _handle(lmpc, case):
    H, f, f_theta, bu, bl, W = fc.problem(case)
    qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, np.zeros((0, case.n)), bu, bl, W, nout=case.nout)
    assert qp.kernel_name.startswith(f"fast<{case.n}>|"), qp.kernel_name
    return qp


_REF = {}


def _oracle(case, qp, th):
    from oracle import ldp as oldp
    out = oldp.solve_batch(oracle_ldp_from(qp.ldp()), th, fc.oracle_settings(case))
    for a in out:
        a.setflags(write=False)
    return out


def _ref(case, qp, batch=0):
    """(theta, oracle outputs) of the case's batch of N_COND points, computed once; a smaller batch is a prefix."""
    key = (case, batch)
    if key not in _REF:
        th = fc.theta(case, fc.N_COND, batch)
        th.setflags(write=False)
        _REF[key] = (th, _oracle(case, qp, th))
    return _REF[key]


def _same(got, ref, N, what):
    names = ("x", "exitflag", "iters", "active")
    for k, a in enumerate(got):
        r = ref[k][:N]
        if not np.array_equal(a, r):
            bad = np.flatnonzero((a != r).reshape(N, -1).any(axis=1))
            raise AssertionError((what, names[k], f"{len(bad)} of {N} rows differ", bad[:8].tolist(),
                                  a[bad[:3]].tolist(), r[bad[:3]].tolist()))


class _Out:
    """x and exitflag of one call between sentinels: `off` elements in front (off = 1 double / 2 flags puts both views
    8 bytes off a 16-byte boundary), GUARD rows behind."""

    def __init__(self, N, nout=1, off=False):
        import torch
        G, dev = fc.GUARD, "cuda:0"
        self.N, self.nout = N, nout
        self.ox, self.oe = (1, 2) if off else (0, 0)
        self.xbuf = torch.full((self.ox + (N + G) * nout,), float("nan"), dtype=torch.float64, device=dev)
        self.ebuf = torch.full((self.oe + N + G,), SENT, dtype=torch.int32, device=dev)
        self.x = self.xbuf[self.ox:self.ox + N * nout].view(N, nout)
        self.ef = self.ebuf[self.oe:self.oe + N]
        if off:
            assert self.x.data_ptr() % 16 == 8 and self.ef.data_ptr() % 16 == 8

    def read(self):
        N, nout = self.N, self.nout
        xb, eb = self.xbuf.cpu().numpy(), self.ebuf.cpu().numpy()
        x, ef = xb[self.ox:self.ox + N * nout].reshape(N, nout), eb[self.oe:self.oe + N]
        assert np.isnan(xb[:self.ox]).all() and (eb[:self.oe] == SENT).all(), "a store in front of the batch"
        assert np.isnan(xb[self.ox + N * nout:]).all() and (eb[self.oe + N:] == SENT).all(), "a store behind the batch"
        assert not np.isnan(x).any() and not (ef == SENT).any(), \
            ("rows the kernel never wrote", np.flatnonzero(np.isnan(x).any(axis=1))[:8], np.flatnonzero(ef == SENT)[:8])
        return x, ef


def _dev(th, off=False):
    """theta on the device; off: a view 8 bytes off a 16-byte boundary."""
    import torch
    N, nth = th.shape
    if not off:
        t = torch.from_numpy(np.array(th, order="C")).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    flat = torch.zeros(N * nth + 1, dtype=torch.float64, device="cuda:0")
    flat[1:] = torch.from_numpy(th.reshape(-1).copy()).cuda()
    t = flat[1:].view(N, nth)
    assert t.data_ptr() % 16 == 8
    return t


def _call(qp, th, off=False):
    """One lmpc_solve_batch_device call for x and the exit flags alone: ((x, exitflag), the launch record)."""
    import torch
    o = _Out(len(th), qp.nout, off)
    qp.solve_device(_dev(th, off), x=o.x, exitflag=o.ef)
    torch.cuda.synchronize()
    return o.read(), qp.fast_launch_info()


# ------------------------------------------------------------------ staged: launch shapes, record paths, sizes
SHAPES = {
    "default": {}, "tiles8": {"fast_tiles": 8}, "tiles12": {"fast_tiles": 12}, "in_flight3": {"in_flight": 3},
    "nstr1": {"fast_nstr": 1}, "nstr2": {"fast_nstr": 2}, "nstr3": {"fast_nstr": 3}, "nstr4": {"fast_nstr": 4},
    "dma0": {"fast_dma": 0}, "dma2": {"fast_dma": 2}, "dma3": {"fast_dma": 3},
    "offset8": {},
}


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"n{p[0]}-nth{p[1]}")
def test_staged_write_out_shapes_and_sizes(lmpc, pair, shape):
    """x and exitflag alone, one output: the staged path at every launch shape and record path, at sizes with one
    tile, a partial last tile, one workgroup and several, and on views 8 bytes off a 16-byte boundary.  The case's
    batch has a 512-problem block (a workgroup's 8 tiles at the default shape) with more than kFastPay queued points:
    the solving side takes the handed-over shifts and the re-read record, and the x shift from the slot in both."""
    case = fc.BY_PAIR[pair].with_nout(1)
    qp = _handle(lmpc, case)
    for k, v in SHAPES[shape].items():
        qp.set_option(k, v)
    if shape != "in_flight3":                                # (the hint switches staging on by itself)
        qp.set_option("fast_stage", 1)
    th, ref = _ref(case, qp)
    st = fc.check_fast_conditions(case, ref[2], ref[3], ref[1])
    assert st["max_queued_in_block"] > fc.K_FAST_PAY
    for N in SIZES:
        got, rec = _call(qp, th[:N], off=(shape == "offset8"))
        assert rec is not None and rec["form"] == qp.FAST_PLAIN and rec["dyn"] == 0, rec
        # The launcher declines staging where its 9 bytes per problem cost the shape a workgroup per CU: n = 3, nth = 9
        # with three rings of three 4608-byte tiles is 52,480 bytes unstaged (three per 160 KB) and would be 55,040 staged
        # (two) once a workgroup has its full 8 tiles.  The record must say so; the results are checked all the same.
        declined = (pair, shape) == ((3, 9), "dma3") and rec["tiles"] == 8
        assert rec["staged"] == (0 if declined else 1), rec
        if (pair, shape) == ((3, 9), "dma3"):
            # (constants 8 (22 + 72) bytes, hand-over 256 x 8 (n + 1) unstaged / 256 x 8 n staged, queue 256 + staging 576
            # bytes per tile, 16 bytes of control words, nine ring slots)
            assert rec["lds"] == (52480 if declined else 752 + 6144 + 832 * rec["tiles"] + 16 + 9 * 4608), rec
        if shape == "in_flight3":
            assert rec["nstr"] == 4 and rec["tiles"] == min(28, (N + 63) // 64), rec
        if shape in ("tiles8", "tiles12"):
            assert rec["tiles"] == min(int(shape[5:]), (N + 63) // 64), rec
        if shape in ("dma0", "offset8"):
            assert rec["dma"] == 0, rec
        _same(got, ref, N, (case.name, shape, N))
    qp.check()


def _scaled_batch(case, qp, scale, want_hard, N):
    """N points of the case's batches times `scale` that the ORACLE all settles in one iteration (want_hard False) or
    all iterates on (True): (theta, oracle outputs)."""
    th = np.vstack([fc.theta(case, fc.N_COND, b) for b in (0, 1)]) * scale
    out = _oracle(case, qp, th)
    keep = (out[2] > 1) if want_hard else (out[2] == 1)
    assert keep.sum() >= N, (case.name, scale, int(keep.sum()))
    idx = np.flatnonzero(keep)[:N]
    return np.ascontiguousarray(th[idx]), tuple(a[idx] for a in out)


@pytest.mark.parametrize("kind", ["no_hard_point", "every_point_hard"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"n{p[0]}-nth{p[1]}")
def test_staged_no_hard_point_and_every_point_hard(lmpc, pair, kind):
    """A batch the streaming wavefronts finish alone (empty queue: the write-out stores what they left) and one in
    which every slot is rewritten by a solving lane (queue of 64 per tile: most positions beyond kFastPay)."""
    case = fc.BY_PAIR[pair].with_nout(1)
    qp = _handle(lmpc, case)
    qp.set_option("fast_stage", 1)
    hard = kind == "every_point_hard"
    th, ref = _scaled_batch(case, qp, 30.0 if hard else 1e-4, hard, 1100)
    assert ((ref[2] > 1) if hard else (ref[2] == 1)).all()
    for N in (1100, 65):
        got, rec = _call(qp, th[:N])
        assert rec["staged"] == 1, rec
        _same(got, ref, N, (case.name, kind, N))
    qp.check()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"n{p[0]}-nth{p[1]}")
def test_staged_several_batches_in_one_launch(lmpc, pair):
    """fast_kernel_multi through lmpc_solve_batches_device: 2 and 8 batches of 65 and 2309 points, staged."""
    import torch
    case = fc.BY_PAIR[pair].with_nout(1)
    qp = _handle(lmpc, case)
    qp.set_option("fast_stage", 1)
    refs = [_ref(case, qp, batch=b) for b in range(8)]
    for N in (65, fc.N_COND):
        for nb in (2, 8):
            outs = [_Out(N, off=(b == 1)) for b in range(nb)]                 # (batch 1: views 8 bytes off a 16-byte boundary)
            qp.solve_batches_device([_dev(refs[b][0][:N], off=(b == 1)) for b in range(nb)], [o.x for o in outs],
                                    [o.ef for o in outs])
            torch.cuda.synchronize()
            rec = qp.fast_launch_info()
            assert rec["form"] == qp.FAST_MULTI and rec["batches"] == nb and rec["staged"] == 1, rec
            for b, o in enumerate(outs):
                _same(o.read(), refs[b][1], N, (case.name, N, nb, "batch", b))
    qp.check()


# ------------------------------------------------------------------ unstaged: the calls that keep today's stores
@pytest.mark.parametrize("why", ["nout_n", "iters_active", "iters_only", "active_only", "fast_dyn", "gather", "fast_stage_0", "alone"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"n{p[0]}-nth{p[1]}")
def test_staging_is_off_where_it_does_not_apply(lmpc, pair, why):
    """n outputs, iters and / or active requested (both, and each alone: the staged kernel writes neither, so a launcher
    that looked at one of the two only would leave sentinels in the other), the dynamic tail, the gather form -- each with "fast_stage" 1 --, "fast_stage"
    0 under "in_flight" 3 and the default of a call issued alone: the launch record shows the unstaged path, and the
    results still equal the oracle's."""
    import torch
    case = fc.BY_PAIR[pair]
    case = case.with_nout(case.n if why == "nout_n" else (case.gather_nout if why == "gather" else 1))
    qp = _handle(lmpc, case)
    th, ref = _ref(case, qp)
    if why == "fast_stage_0":
        qp.set_option("in_flight", 3)
    elif why != "alone":
        qp.set_option("fast_stage", 1)
    seq0 = 0
    for N in (65, fc.N_COND):
        if why in ("iters_active", "iters_only", "active_only"):
            G = fc.GUARD
            o = _Out(N)
            it = torch.full((N + G,), SENT, dtype=torch.int32, device="cuda:0")
            act = torch.full((N + G, qp.words), ACT_SENT, dtype=torch.int64, device="cuda:0")
            qp.solve_device(_dev(th[:N]), x=o.x, exitflag=o.ef, iters=None if why == "active_only" else it[:N],
                            active=None if why == "iters_only" else act[:N])
            torch.cuda.synchronize()
            it, act = it.cpu().numpy(), act.cpu().numpy()
            assert (it[N:] == SENT).all() and (act[N:] == ACT_SENT).all()
            got = o.read()
            if why == "active_only":
                assert (it == SENT).all()
                assert not (act[:N] == ACT_SENT).any() and np.array_equal(act[:N].view(np.uint64), ref[3][:N]), (case.name, why, N)
            else:
                got = got + (it[:N],)
            if why == "iters_only":
                assert (act == ACT_SENT).all()
            if why == "iters_active":
                got = got + (act[:N].view(np.uint64),)
        elif why == "gather":
            if N == 65:
                qp.set_parameter_layout(*case.layout)
            b = fc.gather_blocks(case, th[:N], qp.nout)
            dev = lambda a: None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()
            o = _Out(N, qp.nout)
            o.x[:] = torch.from_numpy(b["control"]).cuda()
            qp.compute_control_device(o.x, dev(b["state"]), dev(b["reference"]), dev(b["disturbance"]), dev(b["parameter"]),
                                      exitflag=o.ef)
            torch.cuda.synchronize()
            got = o.read()
        else:
            if why == "fast_dyn":
                qp.set_option("fast_tiles", 12)
                qp.set_option("fast_dyn", 4)
            if why == "fast_stage_0":
                qp.set_option("fast_stage", 0)
            got, _ = _call(qp, th[:N])
        rec = qp.fast_launch_info()
        assert rec is not None and rec["seq"] > seq0, rec
        seq0 = rec["seq"]
        assert rec["form"] == (qp.FAST_GATHER if why == "gather" else qp.FAST_PLAIN), rec
        if why == "fast_dyn":
            # (two tiles are a static split whatever "fast_dyn" asks for: staged; 37 tiles in workgroups of 12 have the tail)
            assert (rec["dyn"], rec["staged"]) == ((4, 0) if N == fc.N_COND else (0, 1)), rec
        else:
            assert rec["staged"] == 0, rec
        _same(got, ref, N, (case.name, why, N))
    if why in ("fast_stage_0", "alone"):
        qp.set_option("fast_stage", -1 if why == "fast_stage_0" else 1)
        got, rec = _call(qp, th)
        assert rec["staged"] == 1, rec
        _same(got, ref, fc.N_COND, (case.name, "staged again"))
    qp.check()
