"""Host side of the region reduction's tests (no GPU): the cases of tests/region_cases.py reach the kernels and the
branches tests/test_gpu_regions.py claims for them -- shown from the case table and the reference alone, nothing of the
library is run."""
import numpy as np
import pytest

import region_cases as rc


def _paths(words, pred=lambda c: True):
    return {rc.path_of(c.words, c.N, bool(lf)) for c in rc.CASES if c.words == words and pred(c) for lf, _ in rc.variants(c)}


def test_every_path_is_reached_at_the_word_counts_it_serves():
    assert rc.WORDS == (1, 2, 4, 5, 10)
    for words, (n, mg) in rc.SHAPES.items():
        assert rc.words_of(n + mg) == words
    assert [n + mg for n, mg in rc.SHAPES.values()] == [20, 40, 128, 129, 300]
    assert _paths(1) == {"global", "local", "w1"}
    assert _paths(2) == {"global", "local"} and _paths(4) == {"global", "local"}
    for words in (5, 10):
        assert _paths(words, lambda c: c.N < rc.THRESHOLD) == {"global"}
        assert _paths(words, lambda c: c.N >= rc.THRESHOLD) == {"global"}
        assert any(c.N >= rc.THRESHOLD for c in rc.CASES if c.words == words)
    # the rule itself, at its edges
    assert rc.path_of(1, 65535) == "global" and rc.path_of(1, 65536) == "w1" and rc.path_of(1, 65536, False) == "local"
    assert rc.path_of(4, 65536) == "local" and rc.path_of(5, 65536) == "global" and rc.path_of(4, 65535) == "global"
    # sizes: the issue's, within its limits
    assert {c.N for c in rc.CASES} == set(rc.SMALL_N) | set(rc.LARGE_N)
    assert all(c.N <= 300_000 and c.words * c.N <= 3_000_000 for c in rc.CASES)
    assert len({c.name for c in rc.CASES}) == len(rc.CASES)
    # the large-batch paths run with region_blocks 0, 1 and 3, one-word cases in both forms
    big1 = next(c for c in rc.CASES if c.words == 1 and c.N == 65536)
    assert rc.variants(big1) == [(1, 0), (1, 1), (1, 3), (0, 0), (0, 1), (0, 3)]
    assert rc.variants(next(c for c in rc.CASES if c.words == 10 and c.N == 65536)) == [(1, 0)]


def test_share_arithmetic_and_tiles_beyond_the_batch():
    assert rc.share(65536, 256) == (1, 256) and rc.share(65536, 256, path="w1") == (1, 256)
    assert rc.share(65537, 256) == (2, 129) and rc.share(100_003, 256, 3) == (1, 391)
    assert rc.share(1_000_000, 256) == (16, 245) and rc.share(1_000_000, 256, path="w1") == (8, 489)
    # among the large sizes: a last workgroup with a tile wholly beyond N, and one whose last tile is partial, for
    # every CU count considered (region_blocks 1)
    for cu in rc.NUM_CU:
        beyond = {N: rc.tiles_beyond(N, cu, 1) for N in rc.LARGE_N}
        assert any(b >= 1 for b, _ in beyond.values()), (cu, beyond)
        assert any(partial for _, partial in beyond.values())
        assert any(b == 0 and not partial for b, partial in beyond.values())
    assert rc.tiles_beyond(65536 + 255, 256, 1) == (1, True)           # tile 256 partial, tile 257 beyond the batch


@pytest.mark.parametrize("case", [c for c in rc.CASES if c.family == "tile_dense"], ids=lambda c: c.name)
def test_tile_dense_fills_every_workgroups_lds_table(case):
    act, ef, rid = rc.build(case)
    ok = np.ones(case.N, bool) if ef is None else ef >= 1
    full = case.N // rc.TILE
    assert full >= 16
    a = act.view(np.uint64)
    for t in range(full):
        s = slice(t * rc.TILE, (t + 1) * rc.TILE)
        assert len(np.unique(a[s], axis=0)) == rc.TILE                 # 256 distinct masks in the tile ...
        assert len(np.unique(a[s][ok[s]], axis=0)) >= rc.K_LOCAL_SETS + 1, (t, ok[s].sum())   # ... 193 or more that count
    # only 4096 regions exist: the same sets arrive from many workgroups
    m, c, f = rc.expected(case)
    assert len(m) <= 4096 and (case.N < 65536 or c.max() >= 8)


@pytest.mark.parametrize("cu", rc.NUM_CU)
def test_deep_share_overfills_the_lock_free_lds_table(cu):
    case = rc.deep_share_case(cu)
    assert rc.path_of(1, case.N) == "w1" and case.N == (4 * cu + 1) * 256
    tiles, grid = rc.share(case.N, cu, 1, "w1")
    assert tiles == 5 and tiles * rc.TILE > rc.K_W1_TAB
    act, ef, rid = rc.build(case)
    keys = act.view(np.uint64)[:, 0]
    for g in (0, grid // 2, grid - 2):                                 # (the last workgroup holds what is left over)
        assert len(np.unique(keys[g * tiles * rc.TILE:(g + 1) * tiles * rc.TILE])) == 1280 > rc.K_W1_TAB
    assert len(np.unique(keys)) == case.N


def test_mixed_flags_move_a_first_index_drop_a_set_and_keep_one_by_flag_2():
    seen = 0
    for case in rc.CASES:
        if case.flags != "mixed":
            continue
        act, ef, rid = rc.build(case)
        assert set(np.unique(ef)) <= {-1, 0, 1, 2}
        moved, vanished, only2 = rc.mixed_facts(rid, ef)
        m, c, f = rc.expected(case)
        assert len(m) == len(np.unique(rid)) - vanished and c.sum() == (ef >= 1).sum()
        if case.family in ("few", "tile_dense", "first_word_only") and case.N >= 4099:
            seen += 1
            assert set(np.unique(ef)) == {-1, 0, 1, 2}
            assert moved >= 1 and vanished >= 1 and only2 >= 1, (case.name, moved, vanished, only2)
            # the reference shows the same: a first index that is not the region's first sample, a missing region
            a = act.view(np.uint64)
            where = rc._mixed_regions(rid)
            A, B, C = (a[w[0]] for w in where)
            row = lambda mask: np.flatnonzero((m == mask).all(axis=1))
            assert len(row(B)) == 0
            assert f[row(A)[0]] == where[0][1] != where[0][0]
            assert f[row(C)[0]] == where[2][0] and c[row(C)[0]] == (len(where[2]) + 1) // 2
    # per word count: "few" at 4099, "tile_dense" at the five large sizes; "first_word_only" at 4099 from two words on
    assert seen == 6 * len(rc.WORDS) + 4


def test_flag_patterns():
    rid = rc.region_ids("few", 1000)
    assert rc.flags_of("none", rid) is None and (rc.flags_of("all_ok", rid) == 1).all()
    bad = rc.flags_of("all_failed", rid)
    assert set(np.unique(bad)) == {-1, 0}
    act = rc.masks_of(rid, 2, "few")
    assert len(rc.reference(act, bad)[0]) == 0
    m, c, f = rc.reference(act)
    assert len(m) == 7 and c.sum() == 1000 and f.min() == 0
    assert np.array_equal(np.lexsort((f, -c)), np.arange(7))
    # flag 2 counts, flag 0 does not
    ef = np.array([0, 2, 1, -1], np.int32)
    m, c, f = rc.reference(rc.masks_of(np.array([5, 5, 6, 6]), 1, "few"), ef)
    assert c.tolist() == [1, 1] and f.tolist() == [1, 2]


@pytest.mark.parametrize("family,words", [(fam, w) for fam in ("few", "first_word_only", "last_word_only") for w in rc.WORDS
                                          if w >= 2 or fam == "few"])
def test_masks_are_injective_deterministic_and_never_the_empty_key(family, words):
    # ("few", "tile_dense", "all_distinct" and "deep_share" share one rule from region id to mask)
    ids = np.arange(70_000)
    a = rc.masks_of(ids, words, family).view(np.uint64)
    assert a.shape == (70_000, words) and rc.masks_of(ids, words, family).dtype == np.int64
    assert len(np.unique(a, axis=0)) == 70_000
    assert np.array_equal(a, rc.masks_of(ids, words, family).view(np.uint64))
    assert not (a == np.uint64(2 ** 64 - 1)).all(axis=1).any()
    if family.endswith("_word_only"):
        q = 0 if family == "first_word_only" else words - 1
        others = np.delete(a, q, axis=1)
        assert (others == others[0, 0]).all() and others[0, 0] != 0           # equal and nonzero everywhere else
        assert len(np.unique(a[:, q])) == 70_000
        even, odd = a[0::2, q], a[1::2, q]
        assert len(np.unique(even & np.uint64(0xFFFFFFFF))) == 1 and len(np.unique(even >> np.uint64(32))) == len(even)
        assert len(np.unique(odd >> np.uint64(32))) == 1 and len(np.unique(odd & np.uint64(0xFFFFFFFF))) == len(odd)
    else:
        for q in range(words):                                              # every word varies with the region
            assert len(np.unique(a[:, q])) > 69_000


def test_no_one_word_mask_of_the_table_is_all_ones_and_no_row_is_the_sentinel():
    sent = np.array([rc.SENT]).view(np.uint64)[0]
    for case in rc.CASES + tuple(rc.deep_share_case(cu) for cu in rc.NUM_CU):
        a = rc.build(case)[0].view(np.uint64)
        assert not (a == np.uint64(2 ** 64 - 1)).all(axis=1).any()
        assert not (a == sent).all(axis=1).any(), case.name


def test_word_only_cases_merge_under_a_comparison_that_drops_the_word():
    for case in rc.CASES:
        if not case.family.endswith("_word_only"):
            continue
        act, ef, rid = rc.build(case)
        q = 0 if case.family == "first_word_only" else case.words - 1
        R = len(rc.expected(case)[0])
        assert R >= 400
        dropped = np.delete(act, q, axis=1)
        assert len(rc.reference(dropped, ef)[0]) == 1
        # half a word dropped: about half of the regions merge
        half = act.copy(); half[:, q] &= 0xFFFFFFFF
        assert len(rc.reference(half, ef)[0]) < 0.6 * R
        half = act.copy(); half[:, q] >>= 32
        assert len(rc.reference(half, ef)[0]) < 0.6 * R


def test_reference_against_a_plain_loop():
    rng = np.random.default_rng(0)
    rid = rng.integers(0, 40, 3000)
    act = rc.masks_of(rid, 3, "few")
    ef = rng.choice(np.array([-1, 0, 1, 2], np.int32), 3000)
    seen = {}
    for i in range(3000):
        if ef[i] >= 1:
            k = tuple(int(v) for v in act[i].view(np.uint64))
            cnt, first = seen.get(k, (0, i))
            seen[k] = (cnt + 1, first)
    want = sorted(((-c, f, k) for k, (c, f) in seen.items()))
    m, c, f = rc.reference(act, ef)
    assert [(-int(ci), int(fi), tuple(int(v) for v in mi)) for mi, ci, fi in zip(m, c, f)] == want
