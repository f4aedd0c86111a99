"""The region reduction (csrc/lmpc_regions.hip: distinct_masks_kernel, distinct_masks_local_kernel,
distinct_masks_w1_kernel + publish_w1_kernel, publish_sets_kernel) against np.unique, exactly: every comparison is
np.array_equal of (masks, counts, first index) with tests/region_cases.reference -- there is no tolerance anywhere.
Cases, and the proof that they reach the kernel and the branch they are meant for: tests/region_cases.py, checked on
the host in tests/test_region_cases_host.py.

Inputs are views into larger tensors whose other rows hold a sentinel mask (and exit flag 1): a read before row 0 or
past row N - 1 adds a set and changes the answer.  Outputs of the direct calls have sentinel rows behind `capacity`
that must come back untouched.

The overflow word.  `lmpc_distinct_active_sets_overflowed` after a call tells about THAT call: 0 when its sets fitted,
whatever an earlier call on the handle did.  This was not so for a lock-free call (words == 1, N >= 65536) that
followed an overflowed, un-retried call of one of the ballot kernels on a handle whose lock-free tables already had
the size wanted: the lock-free path does not clear word 0 before it runs, publish_w1_kernel read the older call's 1 and
reported an overflow that had not happened (the sets it wrote were right; the Python wrapper answered with a needless
retry at four times the capacity).  test_overflow_then_a_call_that_fits[local-w1] showed it -- (n_sets, overflow) =
(6, 1) for (6, 0) --, [global-w1] is the same sequence behind the one-level kernel; the library now clears the word on the host's say-so (lmpc_regions.hip, `regOvStale`)."""
import ctypes

import numpy as np
import pytest

import region_cases as rc
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def lmpc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as mod
    return mod


_HANDLES = {}


def _handle(lmpc, words, lockfree=1, blocks=0, fresh=False):
    """The handle whose masks have `words` words (one per module, or a new one), with the two tuning options set."""
    if fresh or words not in _HANDLES:
        H, f, f_theta, A, bu, bl, W, sense = rc.problem(words)
        qp = lmpc.BatchedQP.from_mpqp(H, f, f_theta, A, bu, bl, W, sense, nout=1)
        assert qp.words == words and qp.m == sum(rc.SHAPES[words])
        if fresh:
            _HANDLES.pop(words, None)
        _HANDLES[words] = qp
    qp = _HANDLES[words]
    qp.set_option("region_lockfree", lockfree)
    qp.set_option("region_blocks", blocks)
    return qp


def _upload(act, ef):
    """(active, exitflag) on the device as views into sentinel-filled tensors with GUARD rows on either side."""
    import torch
    N, words = act.shape
    G = rc.GUARD
    big = torch.full((N + 2 * G, words), int(rc.SENT), dtype=torch.int64, device=DEV)
    big[G:G + N] = torch.from_numpy(np.array(act)).to(DEV)           # (a copy: the case arrays are read-only)
    a = big[G:G + N]
    assert a.is_contiguous() and a.data_ptr() == big.data_ptr() + 8 * G * words
    if ef is None:
        return a, None
    bigf = torch.ones(N + 2 * G, dtype=torch.int32, device=DEV)
    bigf[G:G + N] = torch.from_numpy(np.array(ef)).to(DEV)
    return a, bigf[G:G + N]


def _case_inputs(case):
    act, ef, _ = rc.build(case)
    return _upload(act, ef)


def _equal(got, want, what=""):
    for g, w, name in zip(got, want, ("masks", "counts", "first")):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name)


def _direct(lmpc, qp, act, ef, capacity):
    """One call of the C entry, no retry: (n_sets, overflow word, sorted (masks, counts, first) of the stored sets)."""
    import torch
    vp = ctypes.c_void_p
    G, S = rc.GUARD, int(rc.SENT)
    masks = torch.full((capacity + G, qp.words), S, dtype=torch.int64, device=DEV)
    counts = torch.full((capacity + G,), S, dtype=torch.int64, device=DEV)
    first = torch.full((capacity + G,), S, dtype=torch.int64, device=DEV)
    nset = torch.full((1 + G,), 12345, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    L = lmpc.lib()
    rcode = L.lmpc_distinct_active_sets_device(qp._h, int(act.shape[0]), vp(act.data_ptr()), vp(ef.data_ptr()) if ef is not None else None,
                                               int(capacity), vp(masks.data_ptr()), vp(counts.data_ptr()), vp(first.data_ptr()),
                                               vp(nset.data_ptr()), None)
    assert rcode == 1, rcode                             # (LMPC_OK)
    over = L.lmpc_distinct_active_sets_overflowed(qp._h, None)
    torch.cuda.synchronize()
    n = int(nset[0].item())
    assert (nset[1:] == 12345).all()
    stored = min(n, capacity)
    m, c, f = masks.cpu().numpy(), counts.cpu().numpy(), first.cpu().numpy()
    assert (m[capacity:] == S).all() and (c[capacity:] == S).all() and (f[capacity:] == S).all(), "store behind capacity"
    if over == 0:
        assert (m[stored:] == S).all() and (c[stored:] == S).all() and (f[stored:] == S).all(), "store behind n_sets"
    order = np.lexsort((f[:stored], -c[:stored]))
    return n, over, (m[:stored].view(np.uint64)[order], c[:stored][order], f[:stored][order])


# ------------------------------------------------------------------------------------------------ every case of the table
_RUNS = [(c, lf, b) for c in rc.CASES for lf, b in rc.variants(c)]


@pytest.mark.parametrize("case,lockfree,blocks", _RUNS, ids=[f"{c.name}-lf{lf}-rb{b}" for c, lf, b in _RUNS])
def test_case(lmpc, case, lockfree, blocks):
    qp = _handle(lmpc, case.words, lockfree, blocks)
    act, ef = _case_inputs(case)
    got = qp.distinct_active_sets_device(act, ef)
    _equal(got, rc.expected(case), (case.name, rc.path_of(case.words, case.N, bool(lockfree))))


@pytest.mark.parametrize("lockfree", [1, 0])
def test_deep_share(lmpc, lockfree):
    """More distinct keys in one workgroup's share than its LDS table holds (lock-free form: 1280 for 1024 slots; the
    two-level form: 1280 for 192), with the wrapper's default capacity -- smaller than the number of sets, so the
    call overflows (lock-free: more keys than global slots) and is repeated -- and with room for all of them."""
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    case = rc.deep_share_case(cu)
    assert rc.share(case.N, cu, 1, "w1" if lockfree else "local")[0] == 5
    qp = _handle(lmpc, 1, lockfree, 1)
    act, ef = _case_inputs(case)
    want = rc.expected(case)
    assert len(want[0]) == case.N > 65536
    _equal(qp.distinct_active_sets_device(act, ef), want, "default capacity")
    n, over, got = _direct(lmpc, qp, act, ef, case.N)
    assert (n, over) == (case.N, 0)
    _equal(got, want, "capacity = N")


# ------------------------------------------------------------------------------------------------------ capacity edges
_EDGES = [("global", 1, 4099, 1), ("global", 5, 4099, 1), ("local", 2, 65536, 1), ("local", 1, 65536, 0), ("w1", 1, 65536, 1)]


@pytest.mark.parametrize("path,words,N,lockfree", _EDGES, ids=[f"{p}-w{w}" for p, w, _, _ in _EDGES])
def test_capacity_edges(lmpc, path, words, N, lockfree):
    assert rc.path_of(words, N, bool(lockfree)) == path
    case = rc.RegionCase(words, N, "all_distinct", "none")
    want = rc.expected(case)
    R = len(want[0])
    assert R == N
    qp = _handle(lmpc, words, lockfree)
    act, ef = _case_inputs(case)
    # exactly as many sets as room: fits, and no retry is needed
    n, over, got = _direct(lmpc, qp, act, ef, R)
    assert (n, over) == (R, 0)
    _equal(got, want, "capacity = R")
    # one fewer: overflow, reported with n_sets >= capacity; the wrapper repeats the call and is exact
    n, over, got = _direct(lmpc, qp, act, ef, R - 1)
    assert over == 1 and n >= R - 1, (n, over)
    _equal(qp.distinct_active_sets_device(act, ef, capacity=R - 1), want, "capacity = R - 1")
    # room for one set
    n, over, got = _direct(lmpc, qp, act, ef, 1)
    assert over == 1 and n >= 1, (n, over)
    _equal(qp.distinct_active_sets_device(act, ef, capacity=1), want, "capacity = 1")
    # and the call after all that is clean
    n, over, got = _direct(lmpc, qp, act, ef, R)
    assert (n, over) == (R, 0)
    _equal(got, want, "capacity = R again")


# ------------------------------------------------------------------------------------------- sequences on one handle
_SEQ = {"w1": (1, 65537, 1), "local": (1, 65537, 0), "global": (1, 4099, 1)}       # path -> (words, N, lockfree)


def test_lock_free_then_one_level_then_lock_free(lmpc):
    qp = _handle(lmpc, 1, fresh=True)
    big, small = rc.RegionCase(1, 65537, "tile_dense", "mixed"), rc.RegionCase(1, 4099, "tile_dense", "all_ok")
    other = rc.RegionCase(1, 100_003, "few", "none")
    assert rc.path_of(1, big.N) == "w1" and rc.path_of(1, small.N) == "global"
    for step, case in enumerate((big, small, big, small, other, big)):
        act, ef = _case_inputs(case)
        n, over, got = _direct(lmpc, qp, act, ef, 4096)
        assert over == 0 and n == len(rc.expected(case)[0]), (step, n, over)
        _equal(got, rc.expected(case), step)
        _equal(qp.distinct_active_sets_device(act, ef, capacity=4096), rc.expected(case), step)


@pytest.mark.parametrize("first,second", [(a, b) for a in _SEQ for b in _SEQ], ids=lambda p: p)
def test_overflow_then_a_call_that_fits(lmpc, first, second):
    """A direct call that overflows and is NOT repeated, then a call with the same capacity (the same table sizes) whose
    sets fit, on every pair of paths: the second is exact and reports no overflow."""
    cap = 512
    qp = _handle(lmpc, 1, fresh=True)
    fits_second = rc.RegionCase(1, _SEQ[second][1], "few", "mixed")
    a2, e2 = _case_inputs(fits_second)
    qp.set_option("region_lockfree", _SEQ[second][2])
    n, over, got = _direct(lmpc, qp, a2, e2, cap)                  # (the second path's tables exist at this size)
    assert over == 0
    _equal(got, rc.expected(fits_second), "before")
    w, N, lf = _SEQ[first]
    many = rc.RegionCase(w, N, "tile_dense", "all_ok")             # more sets than places, and than the 4 * 512 table slots
    assert rc.path_of(w, N, bool(lf)) == first and len(rc.expected(many)[0]) > 4 * cap
    qp.set_option("region_lockfree", lf)
    a1, e1 = _case_inputs(many)
    n, over, got = _direct(lmpc, qp, a1, e1, cap)
    assert over == 1 and n >= cap, (n, over)
    qp.set_option("region_lockfree", _SEQ[second][2])
    n, over, got = _direct(lmpc, qp, a2, e2, cap)
    _equal(got, rc.expected(fits_second), "after")
    assert (n, over) == (len(rc.expected(fits_second)[0]), 0), (n, over)


@pytest.mark.parametrize("path", list(_SEQ))
def test_same_call_twice_and_other_capacities(lmpc, path):
    """The tables are handed over clean (twice the same call), and follow a capacity that changes between calls."""
    w, N, lf = _SEQ[path]
    qp = _handle(lmpc, w, lf, fresh=True)
    case = rc.RegionCase(w, N, "tile_dense", "mixed")
    act, ef = _case_inputs(case)
    want = rc.expected(case)
    R = len(want[0])
    assert 2000 < R <= 4096
    for cap in (4096, 4096, 65536, 4096, 100, 16384, 4096):
        n, over, got = _direct(lmpc, qp, act, ef, cap)
        if cap >= R:
            assert (n, over) == (R, 0), (cap, n, over)
            _equal(got, want, cap)
        else:
            assert over == 1 and n >= cap, (cap, n, over)


# ----------------------------------------------------------------------------------------- DeviceRegionSampler's retry
def _qp_from_golden(lmpc, g):
    return lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=g["H"].shape[0])


def _sampler_check(lmpc, qp, theta, capacity):
    import torch
    sampler = lmpc.explicit.DeviceRegionSampler(qp, len(theta), capacity=capacity)
    m, c, f, solved = sampler.run(torch.from_numpy(np.ascontiguousarray(theta)).to(DEV))
    ef = sampler.ef.cpu().numpy()
    want = rc.reference(sampler.act.cpu().numpy(), ef)
    _equal((m, c, f), want, "sampler")
    assert solved == int((ef >= 1).sum())
    return sampler, len(want[0]), solved


@pytest.mark.parametrize("N,lockfree", [(70_000, 1), (70_000, 0), (20_000, 1)])
def test_sampler_retries_from_a_small_capacity_pendulum(lmpc, N, lockfree):
    # the CPU oracle finds 42 (N = 70 000) and 41 (N = 20 000) distinct sets on these samples: 4 -> 16 -> 64
    qp = _qp_from_golden(lmpc, load_golden("pendulum"))
    assert qp.words == 1
    qp.set_option("region_lockfree", lockfree)
    rng = np.random.default_rng(31)
    lb = np.array([-20.0] * 4 + [-20.0, 0.0] + [-2.0])
    ub = np.array([20.0] * 4 + [20.0, 0.0] + [2.0])
    sampler, R, solved = _sampler_check(lmpc, qp, lb + (ub - lb) * rng.random((N, 7)), 4)
    assert 17 <= R <= 243 and solved == N
    assert sampler.capacity >= max(R, 64) and sampler.capacity in (64, 256)


def test_sampler_retries_from_a_small_capacity_three_words(lmpc):
    # mass_spring_3in, theta uniform in +-MS3_BOX: the CPU oracle finds MS3_SETS distinct sets among the solved points
    qp = _qp_from_golden(lmpc, load_golden("mass_spring_3in"))
    assert qp.words == 3 and rc.path_of(3, 70_000) == "local"
    rng = np.random.default_rng(32)
    theta = rng.uniform(-MS3_BOX, MS3_BOX, (70_000, 12))
    start = MS3_SETS // 16
    sampler, R, solved = _sampler_check(lmpc, qp, theta, start)
    assert 100 <= R <= 4000 and R > 8 * start
    assert sampler.capacity >= R and sampler.capacity >= 16 * start


MS3_BOX, MS3_SETS = 0.25, 1021          # (+-0.2: 265 sets, +-0.3: 3128, +-0.5: 41 883; start 63 -> 252 -> 1008 -> 4032)
