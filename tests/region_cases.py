"""Case table of the region reduction's tests (tests/test_region_cases_host.py, tests/test_gpu_regions.py): synthetic
active-set masks and exit flags for `lmpc_distinct_active_sets_device` (csrc/lmpc_regions.hip), the exact reference
(np.unique), and the library's path and share rules restated so that a case can be shown to reach the kernel and the
branch it claims.  Numpy only: nothing of the library is imported here.

The reduction is a pure function of (active, exitflag): distinct rows of `active` among the samples with exit flag
>= 1, how many samples each has, the smallest sample index of each.  Three kernels do it:

  global   distinct_masks_kernel        one level: a wavefront groups its 64 samples, the leader inserts into the global
                                        hash table (claim / fill / publish).
  local    distinct_masks_local_kernel  words <= 4 and N >= 65536: a workgroup walks its share of 256-sample tiles and
                                        collects up to kLocalSets = 192 masks in an LDS table first; what does not fit
                                        goes straight to the global table.
  w1       distinct_masks_w1_kernel     words == 1, N >= 65536, "region_lockfree" on: every lane inserts its own key
                                        into an LDS table of kW1Tab = 1024 keys, then the workgroup's keys into global
                                        key / count / first tables; publish_w1_kernel makes them dense and clean again.

Mask families (region id -> mask, injective):
  few / tile_dense / all_distinct   word 0 = (id * ODD + C) mod 2^63, a bijection of the ids with the top bit clear (a
                                    one-word mask is therefore never all ones: that value is the lock-free kernel's
                                    empty key, and no solver produces it -- a row is never active at both bounds);
                                    word q > 0 = a 64-bit mix of (id, q).
  first_word_only / last_word_only  every word but the named one is the same nonzero constant for all regions; the
                                    named word differs in its HIGH half only for even ids and in its LOW half only for
                                    odd ids.  A kernel that leaves a word, or half a word, out of the comparison merges
                                    regions here; one that leaves it out of the hash only collides more.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

K_LOCAL_WORDS, K_LOCAL_SETS, K_W1_TAB = 4, 192, 1024        # lmpc_regions.hip
THRESHOLD = 65536                                           # N from which the two large-batch kernels are used
TILE = 256                                                  # samples per tile = threads per workgroup
GUARD = 64                                                  # sentinel rows before and behind the inputs (GPU tests)
SENT = np.int64(-0x25A5A5A5A5A5A5A6)                        # 0xDA5A...5A: top bit set, so no generated word 0
NUM_CU = (64, 256, 304)                                     # CU counts the share conditions are checked for

_ODD = np.uint64(0x9E3779B97F4A7C15)
_C0 = np.uint64(0x1234567)
_M63 = np.uint64((1 << 63) - 1)
_FIXED = np.uint64(0x0F0F00FF00F0F0F1)                      # the words that do NOT differ in the *_word_only families
_LOW = np.uint64(0x5EED5EED)                                # low half where only the high half differs
_HIGH = np.uint64(0x7ABCDEF1)                               # high half where only the low half differs

# words -> (n, general rows) of a `_random_qp`-style problem with m = n + rows = 20, 40, 128, 129, 300 constraint rows
# (a mask has 2 m bits).  Only the handle's `words` matters to the reduction.
SHAPES = {1: (6, 14), 2: (8, 32), 4: (8, 120), 5: (8, 121), 10: (8, 292)}
WORDS = tuple(SHAPES)


def words_of(m):
    return (2 * m + 63) // 64


def problem(words):
    """(H, f, f_theta, A, bu, bl, W, senses) of a strictly convex problem whose masks have `words` words."""
    n, mg = SHAPES[words]
    rng = np.random.default_rng(500 + words)
    nth = 3
    Hh = rng.standard_normal((n, n))
    H = Hh @ Hh.T + n * np.eye(n)
    A = rng.standard_normal((mg, n))
    m = n + mg
    bu = rng.uniform(0.5, 2.0, m)
    bl = -rng.uniform(0.5, 2.0, m)
    W = 0.3 * rng.standard_normal((m, nth))
    W[:n] = 0.0
    return H, np.zeros(n), rng.standard_normal((n, nth)), A, bu, bl, W, np.zeros(m, np.int32)


# ------------------------------------------------------------------------------------------------ the library's rules
def path_of(words, N, lockfree=True):
    """Kernel `lmpc_distinct_active_sets_device` takes: "w1", "local" or "global"."""
    if lockfree and words == 1 and N >= THRESHOLD:
        return "w1"
    if words <= K_LOCAL_WORDS and N >= THRESHOLD:
        return "local"
    return "global"


def share(N, num_cu, blocks_per_cu=0, path="local"):
    """(tiles per workgroup, workgroups) of the two large-batch kernels: "region_blocks" workgroups per CU (0 = the
    default: 1 for the two-level kernel, 2 for the lock-free one), each over an equal share of the 256-sample tiles."""
    tiles_all = (N + TILE - 1) // TILE
    want = num_cu * (blocks_per_cu if blocks_per_cu > 0 else (2 if path == "w1" else 1))
    tiles = (tiles_all + want - 1) // want
    return tiles, (tiles_all + tiles - 1) // tiles


def tiles_beyond(N, num_cu, blocks_per_cu=0, path="local"):
    """(tiles of the last workgroup's share that start at or beyond N, whether its last started tile is partial)."""
    tiles, grid = share(N, num_cu, blocks_per_cu, path)
    tiles_all = (N + TILE - 1) // TILE
    return grid * tiles - tiles_all, N % TILE != 0


def deep_share_size(num_cu):
    """All-distinct one-word batch that, with "region_blocks" 1, gives every workgroup of the lock-free kernel but the
    last a share of 5 tiles: 1280 distinct keys for an LDS table of 1024."""
    return (4 * num_cu + 1) * TILE


# ------------------------------------------------------------------------------------------------------------- masks
def _mix(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def masks_of(rid, words, family):
    """(len(rid), words) int64: the mask of every region id (ids below 2^31), by the family's rule."""
    rid = np.asarray(rid, np.uint64)
    assert rid.size == 0 or int(rid.max()) < 2 ** 31
    out = np.empty((len(rid), words), np.uint64)
    if family in ("first_word_only", "last_word_only"):
        assert words >= 2
        out[:] = _FIXED
        even = (rid & np.uint64(1)) == 0
        v = np.where(even, ((rid + np.uint64(1)) << np.uint64(32)) | _LOW, (_HIGH << np.uint64(32)) | (rid + np.uint64(1)))
        out[:, 0 if family == "first_word_only" else words - 1] = v
    else:
        out[:, 0] = (rid * _ODD + _C0) & _M63
        for q in range(1, words):
            out[:, q] = _mix(rid * np.uint64(words + 1) + np.uint64(q) + np.uint64(0xABCDEF))
    return out.view(np.int64)


def region_ids(family, N, seed=0):
    """Region id of every sample."""
    rng = np.random.default_rng(9000 + seed)
    if family == "few":                                    # 7 regions in runs of 1 ... 79 samples
        nrun = N // 16 + 2
        lens = rng.integers(1, 80, nrun)
        assert lens.sum() >= N
        return np.repeat(rng.integers(0, 7, nrun), lens)[:N].astype(np.int64)
    if family == "tile_dense":                             # a tile = one of 16 blocks of 256 regions, shuffled
        ntile = (N + TILE - 1) // TILE
        block = rng.integers(0, 16, ntile)
        within = np.argsort(rng.random((ntile, TILE)), axis=1)
        return (block[:, None] * TILE + within).reshape(-1)[:N].astype(np.int64)
    if family in ("all_distinct", "deep_share", "first_word_only", "last_word_only"):
        if family.endswith("_word_only"):                  # some 500 regions, each hit several times, and region 0
            nreg = min(N, 509)                             # (high half 1) next to region 1 (low half 2)
            return rng.integers(0, nreg, N).astype(np.int64)
        return rng.permutation(N).astype(np.int64)
    raise ValueError(family)


# ------------------------------------------------------------------------------------------------------------- flags
FLAGS = ("none", "all_ok", "mixed", "all_failed")


def flags_of(pattern, rid, seed=0):
    """int32 exit flags of the samples (None: the NULL pointer, every sample counts).

    "mixed": values from {-1, 0, 1, 2} (15 % of the samples fail), and on the first three regions that have two
    samples or more, in order of first appearance:
      A  its first sample fails (-1) and its second is solved: the reported first index has to move;
      B  every sample fails (-1 and 0 in turn): the set has to vanish;
      C  flags 2 and 0 in turn, beginning with 2: the set is kept by flag-2 samples alone."""
    N = len(rid)
    if pattern == "none":
        return None
    if pattern == "all_ok":
        return np.ones(N, np.int32)
    if pattern == "all_failed":
        return np.where(np.arange(N) % 2 == 0, -1, 0).astype(np.int32)
    assert pattern == "mixed"
    rng = np.random.default_rng(77 + seed)
    ef = rng.choice(np.array([-1, 0, 1, 2], np.int32), N, p=[0.08, 0.07, 0.55, 0.30])
    for role, where in zip("ABC", _mixed_regions(rid)):
        if role == "A":
            ef[where[0]], ef[where[1]] = -1, 1
        elif role == "B":
            ef[where] = np.where(np.arange(len(where)) % 2 == 0, -1, 0)
        else:
            ef[where] = np.where(np.arange(len(where)) % 2 == 0, 2, 0)
    return ef


def _mixed_regions(rid):
    """Sample indices of the (up to) three regions the "mixed" pattern shapes."""
    ids, first, counts = np.unique(rid, return_index=True, return_counts=True)
    multi = ids[counts >= 2][np.argsort(first[counts >= 2], kind="stable")][:3]
    return [np.flatnonzero(rid == r) for r in multi]


def mixed_facts(rid, ef):
    """What the "mixed" flags of a batch really do, from the flags alone: (regions whose first index moved, regions
    that vanished, regions kept by flag-2 samples only)."""
    ids, inv = np.unique(rid, return_inverse=True)
    ok, idx, R = ef >= 1, np.arange(len(rid)), len(ids)
    first_all, first_ok = np.full(R, len(rid)), np.full(R, len(rid))
    np.minimum.at(first_all, inv, idx)
    np.minimum.at(first_ok, inv[ok], idx[ok])
    n_ok, n_one = np.bincount(inv[ok], minlength=R), np.bincount(inv[ef == 1], minlength=R)
    n_fail = np.bincount(inv[~ok], minlength=R)
    moved = int(((n_ok > 0) & (first_ok != first_all)).sum())
    return moved, int((n_ok == 0).sum()), int(((n_ok > 0) & (n_one == 0) & (n_fail > 0)).sum())


# --------------------------------------------------------------------------------------------------------- reference
def reference(active, exitflag=None):
    """(masks (R, words) uint64, counts (R,), first (R,)): the distinct rows of `active` among the rows with
    exitflag >= 1 (all rows: exitflag None), their counts and their smallest row index in the UNFILTERED batch, sorted
    by (-count, first) -- the order `BatchedQP.distinct_active_sets_device` returns."""
    a = np.ascontiguousarray(np.asarray(active)).view(np.uint64)
    a = a.reshape(len(a), -1)
    keep = np.arange(len(a)) if exitflag is None else np.flatnonzero(np.asarray(exitflag) >= 1)
    if len(keep) == 0:
        return np.zeros((0, a.shape[1]), np.uint64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    um, ui, uc = np.unique(a[keep], axis=0, return_index=True, return_counts=True)
    first = keep[ui].astype(np.int64)
    order = np.lexsort((first, -uc))
    return um[order], uc[order].astype(np.int64), first[order]


# -------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class RegionCase:
    words: int
    N: int
    family: str
    flags: str
    seed: int = 0

    @property
    def name(self):
        return f"w{self.words}-N{self.N}-{self.family}-{self.flags}"


@lru_cache(maxsize=None)
def build(case):
    """(active (N, words) int64, exitflag (N,) int32 or None, region ids), read-only."""
    rid = region_ids(case.family, case.N, case.seed)
    act = masks_of(rid, case.words, case.family)
    ef = flags_of(case.flags, rid, case.seed)
    for a in (rid, act, ef):
        if a is not None:
            a.setflags(write=False)
    return act, ef, rid


@lru_cache(maxsize=None)
def expected(case):
    act, ef, _ = build(case)
    out = reference(act, ef)
    for a in out:
        a.setflags(write=False)
    return out


SMALL_N = (1, 63, 64, 65, 255, 257, 4099)                  # one-level kernel: a lane, a wavefront +- 1, a tile +- 1, 17 tiles
LARGE_N = (65535, 65536, 65537, 65536 + 255, 100_003)      # the threshold +- 1, a partial 257th tile, an odd size


def _cases():
    out = []
    for w in WORDS:
        for N in SMALL_N:
            out += [RegionCase(w, N, "few", "mixed"), RegionCase(w, N, "all_distinct", "none")]
        out += [RegionCase(w, 4099, "tile_dense", "all_ok"), RegionCase(w, 4099, "all_distinct", "mixed"),
                RegionCase(w, 4099, "few", "all_failed")]
        for N in LARGE_N:
            out += [RegionCase(w, N, "tile_dense", "mixed"), RegionCase(w, N, "few", "none")]
        out += [RegionCase(w, 65536, "all_distinct", "all_ok"), RegionCase(w, 100_003, "all_distinct", "mixed"),
                RegionCase(w, 100_003, "few", "all_failed")]
        if w >= 2:
            out += [RegionCase(w, 4099, "last_word_only", "none"), RegionCase(w, 4099, "first_word_only", "mixed"),
                    RegionCase(w, 65537, "first_word_only", "none"), RegionCase(w, 100_003, "last_word_only", "all_ok")]
    return tuple(out)


CASES = _cases()


def deep_share_case(num_cu):
    return RegionCase(1, deep_share_size(num_cu), "deep_share", "all_ok")


def variants(case):
    """(lockfree, region_blocks) settings a case is run with: both forms where words == 1, "region_blocks" 0 (default),
    1 and 3 on the two large-batch paths."""
    out = []
    for lockfree in ((1, 0) if case.words == 1 else (1,)):
        blocks = (0, 1, 3) if path_of(case.words, case.N, bool(lockfree)) != "global" else (0,)
        out += [(lockfree, b) for b in blocks]
    return out
