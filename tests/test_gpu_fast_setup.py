"""The one-launch kernel's set-up (lmpc_fast_kernel.hpp, fast_body).  The staged kernels take their constants from ONE
contiguous image in the handle's pack -- 16 bytes per thread, one LDS store --, the other kernels section by section;
the record stride of every kernel that reads theta from a buffer is the template argument NT.  The image holds copies, so
every form of the kernel must give the bits it gave before: here each form, at the problem sizes where the image's shape
changes, against the two-launch form ("fast" 0) on the same handle and against the oracle on the handle's pack,
np.array_equal on everything the call returns.

Sizes: (n, nth) with n in 2 ... 5 and nth in 1, 7, 8, 9, 16 (n = 5: up to 8).  n = 2 and 3 have an odd count of
M / G / du / dl doubles, so a padding double sits between the image's two halves; nth = 9 and 16 take NTHMAX = 16, the
longer image (62 pieces at n = 4 -- no instantiated size reaches the 64 at which a second wavefront would load: that
takes n = 5 with NTHMAX = 16, which the kernel is not built for).  Batches of 1, 63, 64, 65 and 64 * 8 + 1 points under
"fast_tiles" 8: one workgroup, and two with a partial tile.

No entry point writes the pack again after setup (the closed loops write F and G only, in front of the image), so
there is no re-upload to test.  The pack on the device cannot be read back through the library's interface, so the
image is not compared with its sections on the host; what the kernel computes from it is compared instead."""
import numpy as np
import pytest

import fast_cases as fc
from test_gpu_fast import _Guarded, _gather_call, _handle, _ref, _same, _solve_guarded

pytestmark = pytest.mark.gpu

TILES = 8
SIZES = (1, 63, 64, 65, 64 * TILES + 1)
PAIRS = tuple((n, nth) for n in (2, 3, 4) for nth in (1, 7, 8, 9, 16)) + tuple((5, nth) for nth in (1, 7, 8))
CASES = tuple(fc.BY_PAIR[p] for p in PAIRS)
FORMS = ("plain", "staged", "two-batches", "two-batches-staged", "gather", "iters-active")


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


def test_sizes_cover_the_image_shapes():
    """The list above holds what its docstring claims (the arithmetic of fast_image_doubles, restated)."""
    pieces = {}
    for n, nth in PAIRS:
        nthmax = 8 if nth <= 8 else 16
        nconst = n * n + n * (n + 1) // 2 + 2 * n
        pieces[(n, nth)] = (((nconst + 1) & ~1) + ((n * nthmax + 2 * n + nthmax + 2) & ~1)) // 2
    assert all((n * n + n * (n + 1) // 2 + 2 * n) % 2 == 1 for n in (2, 3)) and all((n * n + n * (n + 1) // 2) % 2 == 0 for n in (4, 5))
    assert pieces[(2, 1)] == 21 and pieces[(5, 8)] == 55 and pieces[(4, 16)] == 62 == max(pieces.values())


def _fast0(qp, call):
    qp.set_option("fast", 0)
    try:
        return call()
    finally:
        qp.set_option("fast", 1)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_form_after_the_one_round_trip_setup(lmpc, case, form):
    import torch
    gather = form == "gather"
    case = case.with_nout(case.gather_nout if gather else 1)
    qp = _handle(lmpc, case)
    qp.set_option("fast_tiles", TILES)
    if "staged" in form:
        qp.set_option("fast_stage", 1)
    if gather:
        qp.set_parameter_layout(*case.layout)
    multi = form.startswith("two-batches")
    refs = [_ref(case, qp, batch=b) for b in range(2 if multi else 1)]
    want_form = qp.FAST_GATHER if gather else qp.FAST_MULTI if multi else qp.FAST_PLAIN
    for N in SIZES:
        ths = [fc.theta(case, N, b) for b in range(len(refs))]
        ths_d = [torch.from_numpy(t).cuda() for t in ths]
        seq = (qp.fast_launch_info() or {"seq": 0})["seq"]
        if gather:
            got = [_gather_call(qp, case, ths[0], False, 1)]
            two = [_fast0(qp, lambda: _gather_call(qp, case, ths[0], False, 1))]
        elif multi:
            gs = [_Guarded(N, qp.nout, optional=False) for _ in ths_d]
            qp.solve_batches_device(ths_d, [g.x[:N] for g in gs], [g.ef[:N] for g in gs])
            torch.cuda.synchronize()
            got = [g.read() for g in gs]
            two = [_fast0(qp, lambda t=t: qp.solve(t))[:2] for t in ths]
        else:
            optional = form == "iters-active"
            got = [_solve_guarded(qp, ths_d[0], optional=optional)]
            two = [_fast0(qp, lambda: qp.solve(ths[0]))[:4 if optional else 2]]
        rec = qp.fast_launch_info()
        # the call under test was the kernel form it is named after, on the shape asked for
        assert rec["seq"] == seq + 1 and rec["form"] == want_form and rec["staged"] == (1 if "staged" in form else 0), rec
        assert rec["tiles"] == min(TILES, (N + 63) // 64) and rec["grid"] == ((N + 63) // 64 + TILES - 1) // TILES, rec
        for b, ref in enumerate(refs):
            _same(got[b], ref, N, (case.name, form, N, b, "one launch against the oracle"))
            _same(two[b], ref, N, (case.name, form, N, b, "two launches against the oracle"))
            for a, t in zip(got[b], two[b]):
                assert np.array_equal(a, t), (case.name, form, N, b, "one launch against two")
    qp.check()
