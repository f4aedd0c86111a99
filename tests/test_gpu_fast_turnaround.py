"""The staged kernels' register path (lmpc_fast_kernel.hpp, fast_body): a streaming wavefront asks for its NEXT tile's
record between screen() and publish() of the current one, into the registers the screened record just left, from a
running address clamped to the batch's last record; publish() announces a queued problem with a relaxed LDS store
behind an LDS wait.  Only the order of requests and stores changes, so every comparison is np.array_equal -- with the
two-launch form ("fast" 0) on the same handle and with the oracle on the handle's own pack (tests/fast_cases.py) -- and
which kernel and record path ran is READ from the launch record (lmpc_fast_launch_info).

Batch sizes, in tiles of 64 with four streaming wavefronts and one workgroup: 1, 63, 64, 65 (one tile and a second,
partial one: no early request, or none that is used); 3 x 64 (one wavefront has no tile); 4 x 64 + 1 (one wavefront
asks early for a tile of one point); 8 x 64 (two tiles per wavefront: exactly one early request each); 9 x 64 - 1 (a
partial last tile behind an early request: its idle lane re-reads the batch's last record).  With fewer streaming
wavefronts the same sizes chain up to eight early requests; "fast_tiles" 2 and 3 give several workgroups and a short
last one.  Outputs lie between sentinels (tests/test_gpu_fast_lines.py): nothing is stored outside rows 0 ... N - 1."""
import numpy as np
import pytest

import fast_cases as fc
from test_gpu_fast_lines import _call, _handle, _ref, _same, _scaled_batch

pytestmark = pytest.mark.gpu

PAIRS = ((2, 1), (3, 9), (4, 16), (5, 7), (5, 8))
SIZES = (1, 63, 64, 65, 3 * 64, 4 * 64 + 1, 8 * 64, 9 * 64 - 1)
ONE_WORKGROUP = 28                          # tiles per workgroup of the in-flight shape: every size above is one workgroup
TILES = (ONE_WORKGROUP, 2, 3)
MODES = ("in_flight3", "fast_stage1")


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def _staged(qp, mode):
    """The staged kernel, either way the launcher offers it; the shape options are set after the hint, which resets them."""
    if mode == "in_flight3":
        qp.set_option("in_flight", 3)
    else:
        qp.set_option("fast_stage", 1)


_TWO = {}


def _two_launch(qp, case, th, N):
    """x and exit flags of the two-launch form for the first N points of the case's batch, computed once."""
    if (case, N) not in _TWO:
        qp.set_option("fast", 0)
        try:
            out = qp.solve(np.ascontiguousarray(th[:N]))[:2]
        finally:
            qp.set_option("fast", 1)
        for a in out:
            a.setflags(write=False)
        _TWO[(case, N)] = out
    return _TWO[(case, N)]


@pytest.mark.parametrize("nstr", (1, 2, 3, 4))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"n{p[0]}-nth{p[1]}")
def test_early_request_every_size_and_shape(lmpc, pair, mode, nstr):
    case = fc.BY_PAIR[pair].with_nout(1)
    qp = _handle(lmpc, case)
    _staged(qp, mode)
    qp.set_option("fast_nstr", nstr)
    th, ref = _ref(case, qp)
    for dma in (0, -1):
        qp.set_option("fast_dma", dma)
        for tiles in TILES:
            qp.set_option("fast_tiles", tiles)
            for N in SIZES:
                got, rec = _call(qp, th[:N])
                ntiles = (N + 63) // 64
                what = (case.name, mode, nstr, dma, tiles, N)
                assert rec["form"] == qp.FAST_PLAIN and rec["dyn"] == 0 and rec["nstr"] == nstr, (what, rec)
                assert rec["tiles"] == min(tiles, ntiles) and rec["grid"] == (ntiles + tiles - 1) // tiles, (what, rec)
                # records through registers -- the loop under test -- when asked for and, by default, with four streaming
                # wavefronts (the in-flight shape); rings of two tiles otherwise, which publish through the same code
                # (a batch of fewer than 16 bytes has no 16-byte piece to move: registers)
                rings = dma != 0 and nstr <= 3 and N * case.nth * 8 >= 16
                assert rec["dma"] == (2 if rings else 0), (what, rec)
                # (with rings the launcher may decline staging where its 9 bytes per problem cost a workgroup per CU --
                # tests/test_gpu_fast_lines.py has that rule; without them every shape here fits)
                assert rings or rec["staged"] == 1, (what, rec)
                _same(got, ref, N, what + ("against the oracle",))
                two = _two_launch(qp, case, th, N)
                _same(two, ref, N, what + ("two launches against the oracle",))
                for a, t in zip(got, two):
                    assert np.array_equal(a, t), what + ("one launch against two",)
    qp.check()


def test_in_flight_hint_alone_takes_the_register_path(lmpc):
    """The headline's options and nothing else: staged, four streaming wavefronts, 28 tiles, no rings."""
    case = fc.BY_PAIR[(5, 7)].with_nout(1)
    qp = _handle(lmpc, case)
    qp.set_option("in_flight", 3)
    th, ref = _ref(case, qp)
    got, rec = _call(qp, th)
    assert (rec["staged"], rec["nstr"], rec["tiles"], rec["dma"], rec["grid"]) == (1, 4, 28, 0, 2), rec
    _same(got, ref, fc.N_COND, (case.name, "in_flight 3"))
    qp.check()


@pytest.mark.parametrize("kind", ["no_hard_point", "every_point_hard"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"n{p[0]}-nth{p[1]}")
def test_empty_ballot_and_full_queue(lmpc, pair, kind):
    """A batch the screen settles entirely -- publish() finds an empty ballot on every tile, reserves nothing and the
    early requests are all that is in flight -- and one in which every point is queued: 1100 in one workgroup, so most
    queue positions lie beyond the kFastPay that carry their shifts, and every tile's ring store follows a request."""
    case = fc.BY_PAIR[pair].with_nout(1)
    qp = _handle(lmpc, case)
    qp.set_option("in_flight", 3)
    hard = kind == "every_point_hard"
    th, ref = _scaled_batch(case, qp, 30.0 if hard else 1e-4, hard, 1100)
    assert ((ref[2] > 1) if hard else (ref[2] == 1)).all()
    assert not hard or 1100 > fc.K_FAST_PAY
    for nstr in (4, 1):
        qp.set_option("fast_nstr", nstr)
        qp.set_option("fast_dma", 0)
        for N in (1100, 9 * 64 - 1):
            got, rec = _call(qp, th[:N])
            assert (rec["staged"], rec["dma"], rec["nstr"], rec["grid"]) == (1, 0, nstr, 1), rec
            _same(got, ref, N, (case.name, kind, nstr, N))
    qp.check()
