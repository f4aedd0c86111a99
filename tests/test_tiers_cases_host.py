"""Host side of the tiers pass's tests (no GPU): every case of tests/tiers_cases.py meets the conditions that keep
tests/test_gpu_tiers.py from passing emptily -- on the oracle alone, with the pack oracle.ldp.qp2ldp makes --, every
checker rejects a batch that misses its condition, the restated launch arithmetic is held against the source lines, and
the table reaches exactly the qp_tiers_kernel instantiations the built library holds (kernel NAMES from the AMDGPU
metadata notes; no code is read)."""
import ctypes
import os
import re
from dataclasses import replace

import numpy as np
import pytest

import tiers_cases as tc
from test_fast_fallback import LIB, _kernel_vgprs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linearmpc.jl_amd", "csrc")
_REF = {}


def _cond(case):
    if case not in _REF:
        th = tc.theta(case, tc.N_COND)
        _REF[case] = (th,) + tuple(tc.reference(case, th))
    return _REF[case]


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_case_meets_its_conditions_on_the_oracle(case):
    th, x, ef, it, act = _cond(case)
    tc.check_case(case, th, ef, it, act)
    # what the GPU test compares the list with is neither empty nor everything (m <= 2: no path there can be queued)
    fin = tc.must_finish(case.n, ef, it, act)
    assert fin.any() and (case.m <= 2 or not fin.all())
    want = tc.expected_list(case.n, ef, it, act)
    assert sum(len(w) for w in want) == int((~fin).sum()) and all(((w // 64) % 64 == s).all() for s, w in enumerate(want))
    # the smaller batches are prefixes of this one, a larger one repeats it; the further batches differ from it
    for N in tc.SIZES:
        assert np.array_equal(tc.theta(case, N), th[:N])
    assert np.array_equal(tc.theta(case, tc.N_COND + 65), np.vstack([th, th[:65]]))
    assert not np.array_equal(tc.theta(case, 65, batch=1), th[:65])


def test_tables_cover_what_the_issue_lists():
    assert tuple(c.n for c in tc.HARD) == tc.NS == tuple(c.n for c in tc.SOFT) and tc.instantiations() == set(tc.NS)
    assert all(c.m == 64 and c.nms == c.n and not c.soft for c in tc.HARD)
    assert all(c.m == 64 and {0, 63} <= set(c.soft) for c in tc.SOFT)
    assert [tc.scan_row_reals(n) for n in tc.WIDTH_N] == [4, 8, 12, 16]
    assert {tc.scan_row_reals(n) for n in tc.NS} == {4, 8, 12, 16}
    for n in tc.WIDTH_N:
        edge = [c for c in tc.EDGE if c.n == n]
        ms = {c.m for c in edge}
        assert set(tc.EDGE_M) <= ms
        line = tc.lds_line(n)
        assert tc.lds_bytes(n, line) <= 48 * 1024 < tc.lds_bytes(n, line + 1) and {line - 1, line, line + 1, line + 2} <= ms
        assert {c.nth for c in edge} >= {1, 16} and {c.nout for c in edge} == {1, n}
        assert all(c.nms == 0 for c in edge)                      # no simple bounds; HARD has ms = n
        assert any(c.n == n for c in tc.DUP)
    assert tc.lds_bytes(12, 64) <= 160 * 1024
    assert {w for _, w in tc.REFUSED_SETUP} == {"nth = 17", "m = 65", "n = 13", "an IMMUTABLE row", "an equality row", "a binary row"}
    for c, what in tc.REFUSED_SETUP:
        assert (c.nth == 17) + (c.m == 65) + (c.n == 13) + len(c.flags) == 1, c.name
    assert tc.FVAL.fval_bound > 0 and tc.STALL.progress_tol > 0
    # UNREACHED: at most two cells per instantiation, none of the cells the conditions name for every instantiation
    per_n = {}
    for (n, cell), why in tc.UNREACHED.items():
        per_n[n] = per_n.get(n, 0) + 1
        assert isinstance(why, str) and why
        assert cell == f"optimal at size {n}" or cell.startswith("pivot-singular infeasible at size"), cell
    assert all(v <= 2 for v in per_n.values())


def test_infeasible_finishes_cover_every_tier_for_one_n_per_row_width():
    """Count rule (size N + 1) and pivot rule (sizes 2 ... N, the dup cases) together: an append-only infeasible finish
    in every tier k = 1 ... N, that is at every working-set size 2 ... N + 1."""
    got = tc.infeasible_tiers()
    for n in tc.WIDTH_N:
        assert set(range(2, n + 2)) <= got[n], (n, sorted(got[n]))
    # ... and on the random family alone none below N + 1: without the dup cases tiers k < N never end a point infeasible
    for c in tc.HARD:
        th, x, ef, it, act = _cond(c)
        assert tc.stats(c, ef, it, act)["inf_sizes"] == [c.n + 1]


def test_restated_arithmetic_against_the_source_lines():
    k = open(os.path.join(CSRC, "lmpc_qp_tiers_kernel.hpp")).read()
    l = open(os.path.join(CSRC, "lmpc_qp_tiers.hip")).read()
    a = open(os.path.join(CSRC, "lmpc_api.hip")).read()
    w = open(os.path.join(CSRC, "lmpc_wave_layout.hpp")).read()
    assert "constexpr int qp_scan_row_reals(int n) { return n <= 2 ? 4 : (n <= 6 ? 8 : (n <= 10 ? 12 : 16)); }" in k
    assert "static constexpr int oB(int m) { return ((m * NR + m * (m + 1) / 2 + 1) & ~1); }" in k
    assert "static constexpr int reals(int m) { return oB(m) + 4 * m * 64; }" in k
    assert "const size_t lds = sizeof(double) * (size_t)QpTiersLds<N>::reals(h->P.m);" in l and "if (lds > 48 * 1024)" in l
    assert "const long long tiles = (nprob + 63) / 64;" in l
    assert "long long grid = std::min<long long>((long long)h->numCU, (tiles + 3) / 4);" in l
    assert "grid = ((grid + 15) / 16) * 16;" in l
    assert "const long long gw = (long long)blockIdx.x * 4 + wv, nw = (long long)gridDim.x * 4;" in k
    assert "const int shard = (int)(gw % kShards);" in k and "for (long long base = gw * 64; base < nprob; base += nw * 64) {" in k
    assert "constexpr int kShards = 64;" in w and tc.K_SHARDS == 64
    assert "return (((nprob + kShards - 1) / kShards + 64 * 32 + 256) + 255) & ~255ll;" in a
    assert "if (m < 64) { w0 |= lo << m; if (m > 0) w1 = lo >> (64 - m); }" in k and "else w1 = lo;" in k
    assert "constexpr int kQpTiersMaxNth = 16;" in k and "constexpr int KMAX = N + 1;" in k
    # the numbers
    assert [tc.lds_reals(2, 1), tc.lds_reals(7, 21), tc.lds_reals(7, 22), tc.lds_reals(12, 64)] == [262, 5860, 6150, 19488]
    assert [tc.grid(N, 256) for N in (1, 256, 257, 4096, 4097, 65536, 65537, 10 ** 6)] == [16, 16, 16, 16, 32, 256, 256, 256]
    assert [tc.grid(N, 304) for N in (65537, 77824, 77825)] == [272, 304, 304] and tc.grid(4096, 8) == 16
    assert all(tc.tile_segment(t) == (t % (4 * g)) % 64 for g in (16, 32, 256, 304) for t in (0, 63, 64, 65, 1023, 1024, 5000))
    assert [tc.seg_cap(N) for N in (1, 4096, 65536, 65600)] == [2560, 2560, 3328, 3584]
    # the two-word packing: lower sides start at bit m, cross into word 1 at row 64 - m, and fill word 1 alone at m = 64
    assert tc.pack_active(0b101, 0b010, 3) == (0b010101, 0)
    assert tc.pack_active(1, 1 << 31, 32) == (1 | 1 << 63, 0) and tc.pack_active(0, 1 << 31, 33) == (0, 1)
    assert tc.pack_active(0, 1 | 1 << 62, 63) == (1 << 63, 1 << 61) and tc.pack_active(1 << 63, 1 | 1 << 63, 64) == (1 << 63, 1 | 1 << 63)
    for m in (1, 2, 31, 32, 33, 63, 64):                       # ... the same bits the oracle's side_bits() reads back
        rng = np.random.default_rng(m)
        up = int(rng.integers(0, 1 << 62)) & ((1 << m) - 1)
        lo = (int(rng.integers(0, 1 << 62)) << 2 | 1 | (1 << (m - 1))) & ((1 << m) - 1) & ~up
        w0, w1 = tc.pack_active(up, lo, m)
        arr = np.array([[w0, w1][:tc.words(m)]], np.uint64)
        u, lw = tc.side_bits(arr, m)
        assert [int(b) for b in u[0]] == [(up >> j) & 1 for j in range(m)] and [int(b) for b in lw[0]] == [(lo >> j) & 1 for j in range(m)]


def test_rule_and_list_check_reject_what_they_must():
    case = tc.BY_NAME["hard-n7"]
    th, x, ef, it, act = _cond(case)
    fin = tc.must_finish(case.n, ef, it, act)
    nact = tc.popcount(act)
    assert fin[it == 1].all() and not fin[it > nact + 1].any() and fin[(ef == -1) & (it == nact + 1)].all()
    soft = tc.BY_NAME["soft-n7"]
    ths, xs, efs, its, acts = _cond(soft)
    fs = tc.must_finish(soft.n, efs, its, acts)
    ns = tc.popcount(acts)
    assert fs[efs == 2].any() and not fs[ns > soft.n + 1].any() and (ns > soft.n + 1).any()
    assert not tc.must_finish(12, *_cond(tc.STALL)[2:])[_cond(tc.STALL)[2] == -2].any()
    # the list check: the snapshot a correct pass leaves, then one point too many, one too few, a wrong segment, a tile in
    # two runs, a tile out of order
    want = tc.expected_list(case.n, ef, it, act)

    def snapshot(lists):
        counts = np.array([len(w) for w in lists], np.int32)
        lst = np.full((64, tc.seg_cap(len(it))), -1, np.int32)
        for s, w in enumerate(lists):
            lst[s, :len(w)] = w
        return counts, lst

    tc.check_list(*snapshot(want), want)
    s = next(k for k, w in enumerate(want) if len(w) >= 3)
    fin_pt = next(p for p in np.flatnonzero(fin) if (p // 64) % 64 == s)
    extra = [w.copy() for w in want]; extra[s] = np.sort(np.append(extra[s], fin_pt))
    with pytest.raises(AssertionError, match="queued but the rule says finished"):
        tc.check_list(*snapshot(extra), want)
    fewer = [w.copy() for w in want]; fewer[s] = fewer[s][1:]
    with pytest.raises(AssertionError, match="finished but the rule says queued"):
        tc.check_list(*snapshot(fewer), want)
    moved = [w.copy() for w in want]; moved[0] = np.concatenate([want[0], want[s]]); moved[s] = want[s][:0]
    with pytest.raises(AssertionError, match="segment 0"):
        tc.check_list(*snapshot(moved), want)
    swapped = [w.copy() for w in want]; swapped[s] = swapped[s][::-1]
    with pytest.raises(AssertionError, match="out of order"):
        tc.check_list(*snapshot(swapped), want)
    big = np.concatenate([ef] * 64), np.concatenate([it] * 64), np.concatenate([act] * 64)
    wb = tc.expected_list(case.n, *big)
    sb = next(k for k, w in enumerate(wb) if len(np.unique(w // 64)) >= 2 and (np.bincount(w // 64)[np.unique(w // 64)] >= 2).any())
    t0 = next(t for t in np.unique(wb[sb] // 64) if (wb[sb] // 64 == t).sum() >= 2)
    mine, rest = wb[sb][wb[sb] // 64 == t0], wb[sb][wb[sb] // 64 != t0]
    split = [w.copy() for w in wb]; split[sb] = np.concatenate([mine[:1], rest, mine[1:]])
    with pytest.raises(AssertionError, match="two runs"):
        tc.check_list(*snapshot(split), wb)
    free = [w.copy() for w in wb]; free[sb] = np.concatenate([rest, mine])          # (the order of the tiles is free)
    tc.check_list(*snapshot(free), wb)
    # a pass that queues everything, and one that never gets past iteration 1
    allq = [np.arange(len(it))[(np.arange(len(it)) // 64) % 64 == k] for k in range(64)]
    with pytest.raises(AssertionError, match="queued but the rule says finished"):
        tc.check_list(*snapshot(allq), want)
    tier0 = [np.flatnonzero((it != 1) & ((np.arange(len(it)) // 64) % 64 == k)) for k in range(64)]
    with pytest.raises(AssertionError, match="queued but the rule says finished"):
        tc.check_list(*snapshot(tier0), want)


def test_conditions_reject_batches_that_miss_one():
    def rejects(case, check, drop, what, with_th=False):
        """The case's batch with the points `drop` replaced by other points of it."""
        th, x, ef, it, act = _cond(case)
        idx = np.arange(len(it))
        bad = np.flatnonzero(drop(ef, it, act))
        assert len(bad), (case.name, what, "nothing to drop")
        good = np.flatnonzero(~drop(ef, it, act))
        idx[bad] = np.resize(good, len(bad))
        args = (case, th[idx], ef[idx], it[idx], act[idx]) if with_th else (case, ef[idx], it[idx], act[idx])
        with pytest.raises(AssertionError, match=what):
            check(*args)

    nact = tc.popcount
    fin = lambda c: (lambda ef, it, act: tc.must_finish(c.n, ef, it, act))
    h = tc.BY_NAME["hard-n7"]
    rejects(h, tc.check_hard_conditions, lambda ef, it, act: it == 1, "settled")
    for k in (1, 3, 6):
        rejects(h, tc.check_hard_conditions, lambda ef, it, act, k=k: (ef == 1) & (nact(act) == k) & (it == k + 1), "every size")
    rejects(h, tc.check_hard_conditions, lambda ef, it, act: (ef == -1) & (it == nact(act) + 1), "count rule")
    rejects(h, tc.check_hard_conditions, lambda ef, it, act: it > nact(act) + 1, "removal")
    rejects(h, tc.check_hard_conditions, lambda ef, it, act: tc.side_bits(act, 64)[1].any(axis=1), "lower side")
    with pytest.raises(AssertionError, match="N_COND"):
        tc.check_hard_conditions(h, *(a[:65] for a in _cond(h)[2:]))
    s = tc.BY_NAME["soft-n7"]
    rejects(s, tc.check_soft_conditions, lambda ef, it, act: ef == 2, "flag 2")
    rejects(s, tc.check_soft_conditions, lambda ef, it, act: (ef >= 1) & (nact(act) == 8), "size N \\+ 1")
    rejects(s, tc.check_soft_conditions, lambda ef, it, act: nact(act) > 8, "longer than")
    rejects(s, tc.check_soft_conditions, lambda ef, it, act: np.logical_or(*tc.side_bits(act, 64))[:, 63], "SOFT row 63")
    e = tc.BY_NAME[next(c.name for c in tc.EDGE if c.n == 7 and c.m == 33)]
    up_lo = lambda act, m: np.logical_or(*tc.side_bits(act, m))
    e31 = tc.BY_NAME[next(c.name for c in tc.EDGE if c.n == 7 and c.m == 31)]
    rejects(e31, tc.check_edge_conditions, lambda ef, it, act: up_lo(act, 31)[:, 30], "the last row")
    rejects(e, tc.check_edge_conditions, lambda ef, it, act: up_lo(act, 33)[:, 0], "the first")
    rejects(e, tc.check_edge_conditions, lambda ef, it, act: tc.side_bits(act, 33)[1][:, 31:].any(axis=1), "word 1")
    e63 = tc.BY_NAME[next(c.name for c in tc.EDGE if c.n == 7 and c.m == 63)]       # (m = 63: row 0 alone has its lower bit in word 0)
    rejects(e63, tc.check_edge_conditions, lambda ef, it, act: tc.side_bits(act, 63)[1][:, 0], "word 0")
    rejects(e, tc.check_edge_conditions, lambda ef, it, act: ~tc.must_finish(7, ef, it, act), "queued points")
    d = tc.BY_NAME["dup-n7"]
    _, a, b, gap = d.dep
    for k in (2, 5, 7):
        rejects(d, tc.check_dup_conditions, lambda ef, it, act, k=k: (nact(act) == k) & (it == k + 1), "pivot-singular")
    t = tc.BY_NAME["tie-n11"]
    rejects(t, tc.check_tie_conditions, lambda ef, it, act: up_lo(act, t.m)[:, t.dep[1]], "first of the two")
    rejects(tc.STALL, tc.check_stall_conditions, lambda ef, it, act: ef == -2, "stall guard")
    rejects(tc.SUM, tc.check_sum_conditions, lambda ef, it, act: it > nact(act) + 1, "all three", with_th=True)
    # fval_bound: the same batch under the default bound misses the condition
    th, x, ef, it, act = _cond(replace(tc.FVAL, fval_bound=0.0))
    with pytest.raises(AssertionError, match="fval_bound"):
        tc.check_fval_conditions(tc.FVAL, th, ef, it, act)


def _names(pattern):
    assert os.path.exists(LIB), "build the library first"
    return _kernel_vgprs(LIB, pattern)


def test_case_table_reaches_every_instantiation_of_the_library():
    built = set()
    for k in _names(r"4lmpc15qp_tiers_kernelILi\d+EE"):
        m = re.search(r"15qp_tiers_kernelILi(\d+)EE", k)
        assert m, k
        built.add(int(m.group(1)))
    assert len(built) == 11 and built == tc.instantiations(), sorted(built ^ tc.instantiations())


def test_front_pass_record_and_snapshot_are_declared_and_exported():
    import linearmpc_jl_amd as lmpc
    L = lmpc.lib()
    for sym in ("lmpc_front_pass_info", "lmpc_work_list_read"):
        assert sym in lmpc.SYMBOLS and hasattr(L, sym)
    W = len(lmpc.BatchedQP.FRONT_PASS_FIELDS)
    out = (ctypes.c_int32 * (4 * W))()
    assert L.lmpc_front_pass_info(None, out, 4) == -100 and L.lmpc_work_list_read(None, out, None, 0) == -100 and W == 8
    header = open(os.path.join(ROOT, "include", "lmpc_hip.h")).read()
    assert "#define LMPC_FRONT_INFO_WORDS 8" in header and "#define LMPC_LIST_SHARDS 64" in header
    assert "int lmpc_front_pass_info(const lmpc_handle *h, int32_t *out, int max);" in header
    assert "long long lmpc_work_list_read(lmpc_handle *h, int32_t *counts, int32_t *list, long long list_words);" in header
    Q = lmpc.BatchedQP
    assert (Q.FRONT_SCREEN, Q.FRONT_TIERS, Q.WALK_LANE, Q.WALK_WAVE, Q.WALK_ROW, Q.LIST_SHARDS) == (1, 2, 1, 2, 3, 64)
    for name, v in (("LMPC_FRONT_SCREEN", 1), ("LMPC_FRONT_TIERS", 2), ("LMPC_WALK_LANE", 1), ("LMPC_WALK_WAVE", 2), ("LMPC_WALK_ROW", 3)):
        assert f"#define {name} {v}" in header


def test_tiers_cases_imports_nothing_of_the_library():
    import ast
    tree = ast.parse(open(tc.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert not names & {"linearmpc_jl_amd", "torch", "ctypes"}, names
