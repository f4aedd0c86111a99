"""Host side of the variational chain's tests (no GPU): the oracle's trace only observes, every N of tests/avi_cases.py
meets the conditions that keep tests/test_gpu_avi.py from passing emptily -- on the oracle alone, with the pack
oracle.avi.qp2avi makes --, the checkers reject what they must, the restated launch arithmetic is held against the source
lines, and the table reaches exactly the instantiations the built library holds (kernel NAMES from the AMDGPU metadata
notes; no code is read).  Prints the census per N: depths, reasons, (NA, r) coverage."""
import ctypes
import os
import re

import numpy as np
import pytest

import avi_cases as ac
from oracle import avi as oavi
from test_fast_fallback import LIB, _kernel_vgprs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linearmpc.jl_amd", "csrc")
_REF = {}


def _cond(case, iter_limit=0):
    key = (case, iter_limit)
    if key not in _REF:
        th = ac.theta(case, ac.N_COND)
        _REF[key] = (th,) + tuple(ac.reference(case, th, iter_limit=iter_limit))
    return _REF[key]


def test_trace_only_observes():
    """oracle_avi_solve_batch_trace gives oracle_avi_solve_batch's bits, cold, warm and at an iteration limit, and its
    words agree with what the outputs do show."""
    for case in (ac.BY_NAME["wide-n6"], ac.BY_NAME["near-n6"], ac.BY_NAME["base-n3"]):
        P = ac.host_pack(case)
        th = ac.theta(case, 1000)
        for lim in (0, case.n + 2):
            a = oavi.solve_batch(P, th, ac.settings(lim))
            b = oavi.solve_batch_trace(P, th, ac.settings(lim))
            assert all(np.array_equal(u, v) for u, v in zip(a, b[:4])), (case.name, lim)
            tr, ef, it, nact = b[4], b[1], b[2], ac.popcount(b[3])
            assert np.array_equal(tr.broken, ef == -2) and (tr.max_na >= nact).all() and (tr.max_na <= case.n + 1).all()
            assert ((tr.nremove > 0) <= tr.blocked).all() and (tr.block_na[~tr.blocked] == -1).all()
            assert ((tr.rm_map != 0) == (tr.nremove > 0)).all()
            clean = (ef == 1) & ~tr.singular
            assert np.array_equal(it[clean], (nact + 2 * tr.nremove + 1)[clean]), "appends + removals + 1 iterations"
        w = oavi.solve_batch(P, th, warm=a[3])
        wt = oavi.solve_batch_trace(P, th, warm=a[3])
        assert all(np.array_equal(u, v) for u, v in zip(w, wt[:4]))


@pytest.mark.parametrize("n", ac.NS)
def test_every_n_meets_its_conditions_on_the_oracle(n):
    results = [(c,) + _cond(c)[2:] for c in ac.census_cases(n)]
    cs, pairs = ac.check_n_conditions(n, results)
    for name, c in cs.items():
        print(name, {k: v for k, v in c.items() if k != "pairs"})
    print(f"n = {n}: (NA, r) reached {len(pairs)} of {len(ac.all_pairs(n))}, unreached {sorted(ac.all_pairs(n) - pairs)}")
    for case, ef, it, act, tr in results:
        th = _cond(case)[0]
        for N in ac.SIZES:
            assert np.array_equal(ac.theta(case, N), th[:N])
        assert np.array_equal(ac.theta(case, ac.N_COND + 65), np.vstack([th, th[:65]]))
        for kf in ac.KFIRSTS:
            l0, l1 = ac.expected_lists(n, kf, ef, tr)
            fin = ac.first_finish(n, kf, ef, tr)
            assert sum(map(len, l0)) == int((~fin).sum()) and all(((w // 64) % 64 == s).all() for s, w in enumerate(l0))
            assert sum(map(len, l1)) == 0, "well-posed problems at the default limit: the lane kernel finishes its list"
        # iter_limit = N + 2: list 1 is the points the oracle stops at the limit, and nothing else
        th, x, efl, itl, actl, trl = _cond(case, n + 2)
        l0, l1 = ac.expected_lists(n, ac.default_kfirst(n), efl, trl)
        assert np.array_equal(np.sort(np.concatenate(l1)), np.flatnonzero(efl == -4))
    assert sum(int((_cond(c, n + 2)[2] == -4).sum()) for c in ac.census_cases(n)) >= 8, "the limit acts"


def test_near_singular_family_and_the_calm_case():
    for case in ac.NEAR:
        th, x, ef, it, act, tr = _cond(case)
        print(case.name, ac.check_near_conditions(case, ef, tr), ac.census(case.n, ef, it, act, tr)[3])
        l0, l1 = ac.expected_lists(case.n, ac.default_kfirst(case.n), ef, tr)
        assert sum(map(len, l1)) == int(tr.singular.sum()) > 0
        H = ac.problem(case)[0]
        np.linalg.cholesky((H + H.T) / 2)                 # (the test lmpc_setup applies)
    with pytest.raises(AssertionError, match="singular"):
        th, x, ef, it, act, tr = _cond(ac.BY_NAME["base-n6"])
        ac.check_near_conditions(ac.BY_NAME["base-n6"], ef, tr)
    th, x, ef, it, act, tr = _cond(ac.CALM)
    assert (it == 1).all() and (ef == 1).all()
    for kf in ac.KFIRSTS:
        assert sum(map(len, ac.expected_lists(ac.CALM.n, kf, ef, tr)[0])) == 0


def test_tables_cover_what_the_issue_lists():
    for fam in (ac.BASE, ac.SKEW, ac.WIDE):
        assert tuple(c.n for c in fam) == ac.NS
    assert all(c.m == c.n and c.nout <= c.n and 2 * c.m <= 64 for c in ac.BY_NAME.values())
    assert {c.nout for c in ac.BASE} >= {1, 2, 8} and any(c.nout == c.n for c in ac.BASE)
    assert ac.KFIRSTS == (1, 2, 3, 0) and ac.SIZES == (1, 63, 64, 65) and ac.N_COND == 64 * ac.K_SHARDS
    inst = ac.instantiations()
    assert len(inst["tiers"]) == 20 and len(inst["lane"]) == 14 and len(inst["slab"]) == 4
    # unreached pairs: at most two per N, each with the reason in the table's comment
    assert all(ac.UNREACHED_PAIRS[n] == {(1, 0), (n, n - 1)} for n in ac.NS)
    assert all(len(ac.all_pairs(n)) == n * (n + 1) // 2 for n in ac.NS)


def test_restated_arithmetic_against_the_source_lines():
    k = open(os.path.join(CSRC, "lmpc_avi_tiers_kernel.hpp")).read()
    g = open(os.path.join(CSRC, "lmpc_avi_kernel.hpp")).read()
    t = open(os.path.join(CSRC, "lmpc_avi_tiers.hip")).read()
    a = open(os.path.join(CSRC, "lmpc_avi.hip")).read()
    assert "static constexpr int NP = N + (N & 1);" in k
    assert "static constexpr int oMR = 0, oG = N * NP, oSd = oG + ((N * N + 1) & ~1);" in k and "static constexpr int reals = oSd + NP;" in k
    assert "const size_t lds = sizeof(double) * ((size_t)AviSmallLds<N>::reals + 4 * (size_t)h->A.nout * 64);" in t
    assert "static constexpr int kPark = 6 * N;" in k and "return AviSmallLds<N>::reals + 4 * AviLaneState<N>::kPark * 64;" in k
    assert "if (lds > 48 * 1024) {" in t
    assert "return ((tiles + kShards - 1) / kShards) * 64 + 64;" in a
    assert "long long g = (long long)h->numCU * occ;" in a and "const long long need = (tiles + 3) / 4;" in a
    assert "if (h->aviChainGroups > 0 && g > h->aviChainGroups) g = h->aviChainGroups;" in a and "g = ((g + 15) / 16) * 16;" in a
    assert "long long grid = (long long)h->numCU * (h->aviWaves > 0 ? h->aviWaves : 16);" in a
    assert "const long long fit = (long long)(((size_t)1 << 30) / (sizeof(double) * slabR + sizeof(int32_t) * slabI));" in a
    assert "if (h->aviChainGroups > 0) grid = std::min<long long>(grid, h->aviChainGroups);" in a
    assert "if (listed) grid = std::max<long long>(kShards, (grid / kShards) * kShards);" in a
    assert "std::min<long long>(tiles, (long long)h->numCU * 4)" in a
    assert "return 2 * avi_tri(cap + 1) + 8ll * (cap + 1) + 4ll * n + 2ll * m;" in g
    assert "return (cap + 1) + (long long)m; }" in g
    assert "constexpr size_t kAviLdsPack = 64 * 1024;" in a and "const bool small = P.m == P.n && P.n <= 8 && P.nout <= P.n;" in a
    assert "h->S.iter_limit > h->aviTiersN + 1" in a and "warm == nullptr" in a
    assert "const int shard = (int)(gw % kShards);" in k
    assert "active[pid * words] = (uint64_t)up | ((uint64_t)lo << N);" in k
    # the numbers
    assert [ac.small_lds_reals(n) for n in ac.NS] == [10, 26, 36, 62, 78, 114, 136]
    assert [ac.tiers_lds_bytes(n, n) for n in (2, 8)] == [8 * (10 + 512), 8 * (136 + 2048)]
    assert all(ac.tiers_lds_bytes(n, n) <= ac.LDS_ATTR_LINE for n in ac.NS)
    assert [ac.lane_lds_bytes(n) for n in (2, 3, 4, 8)] == [24656, 37072, 49440, 99392] and ac.lane_needs_attribute() == 4
    assert ac.lane_lds_bytes(8) <= 160 * 1024
    assert [ac.seg_cap(N) for N in (1, 4096, 4097, 4161, 8192, 8193, 10 ** 6)] == [128, 128, 192, 192, 192, 256, 15744]
    assert [ac.chain_grid(N, 256, 2) for N in (1, 4096, 4161, 131072, 131073, 10 ** 6)] == [16, 16, 32, 512, 512, 512]
    assert [ac.chain_grid(4161, 256, 2, cap) for cap in (0, 1, 16, 17, 100)] == [32, 16, 16, 32, 32]
    assert ac.chain_grid(10 ** 6, 256, 3, 1) == 16 and ac.chain_grid(10 ** 6, 304, 1) == 304
    assert all(ac.tile_segment(t) == (t % (4 * g)) % 64 for g in (16, 32, 512) for t in (0, 63, 64, 65, 1023, 5000))
    assert ac.scratch_reals(8, 90, 11) == 2 * 78 + 96 + 32 + 180 and ac.scratch_ints(90, 11) == 102
    assert ac.slab_grid(777, 256, 8, 20, 0, False) == 13 and ac.slab_grid(10 ** 6, 256, 8, 20, 0, False) == 4096
    assert ac.slab_grid(4096, 256, 6, 6, 0, True) == 64 and ac.slab_grid(10 ** 6, 256, 6, 6, 0, True) == 1024
    assert ac.slab_grid(10 ** 6, 256, 6, 6, 0, True, cap=1) == 64 and ac.slab_grid(10 ** 6, 256, 6, 6, 0, True, cap=200) == 192
    assert ac.slab_grid(10 ** 6, 256, 8, 90, 3, False, cap=1) == 1 and ac.slab_grid(130, 256, 8, 90, 3, False, waves=4) == 3
    # the pack: the three 4-aligned blocks of the small case, and the 64 KiB line of the slab kernel's LDS copy
    base = lambda n, m, nth, nout: 2 * m * n + m * m + 2 * m + m * nth + nout * n + nout + nout * nth
    assert base(6, 6, 5, 2) == 174 and ac.pack_reals(6, 6, 5, 2) == (174 + 2) + 60 + (18 + 2) + 6
    assert base(3, 3, 3, 1) == 49 and ac.pack_reals(3, 3, 3, 1) == 52 + 18 + 2 + 9 + 3 + 3
    assert ac.pack_reals(9, 9, 3, 1) == base(9, 9, 3, 1) and ac.pack_reals(4, 5, 3, 1) == base(4, 5, 3, 1)
    for lo, hi in ((ac.SLAB_UNDER, ac.SLAB_OVER), (ac.SLAB_UNDER_PROX, ac.SLAB_OVER_PROX)):
        assert ac.pack_bytes(lo.n, lo.m, lo.nth, lo.nout, lo.prox) <= ac.LDS_PACK_LINE < ac.pack_bytes(hi.n, hi.m, hi.nth, hi.nout, hi.prox)
        assert hi.m == lo.m + 1 and lo.prox == hi.prox, "the smallest m over the line and the largest under it"
        assert lo.ms < lo.n and lo.soft and max(lo.soft) < lo.m and lo.n + 1 + len(lo.soft) <= 160, "outside the small case"
    assert (ac.SLAB_UNDER.m, ac.SLAB_UNDER_PROX.m) == (80, 79)
    # the one-word packing
    assert ac.pack_active(0b101, 0b010, 3) == 0b010101 and ac.pack_active(1, 1 << 7, 8) == 1 | 1 << 15
    arr = np.array([[ac.pack_active(0b0110, 0b1001, 4)]], np.uint64)
    assert int(ac.popcount(arr)[0]) == 4


def test_rules_and_list_check_reject_what_they_must():
    case = ac.BY_NAME["wide-n6"]
    th, x, ef, it, act, tr = _cond(case)
    nact = ac.popcount(act)
    # the blocked-yet-append-only points: the outputs' rule (iters == rows + 1) would let the tiers finish them
    bao = tr.blocked & (tr.nremove == 0) & (ef == 1) & (tr.max_na <= 3)
    assert bao.any() and (it[bao] == nact[bao] + 1).all() and not ac.tiers_finish(6, 3, ef, tr)[bao].any()
    for k in (1, 2, 3):
        fin = ac.tiers_finish(6, k, ef, tr)
        assert fin[it == 1].all() and not fin[tr.nremove > 0].any() and not fin[nact > k].any()
        assert (ac.tiers_finish(6, k, ef, tr) <= ac.tiers_finish(6, min(k + 1, 3), ef, tr)).all()
    assert ac.lane_finish(ef, tr).all()
    thl, xl, efl, itl, actl, trl = _cond(case, 8)
    assert np.array_equal(~ac.lane_finish(efl, trl), efl == -4) and (efl == -4).any()
    assert ac.uses_chain(6, 8) and not ac.uses_chain(6, 7) and not ac.uses_chain(6, 8, warm=True) and not ac.uses_chain(6, 8, option=False)
    want = ac.expected_lists(6, 3, ef, tr)[0]

    def snapshot(lists):
        counts = np.array([len(w) for w in lists], np.int32)
        lst = np.full((64, ac.seg_cap(len(ef))), -1, np.int32)
        for s, w in enumerate(lists):
            lst[s, :len(w)] = w
        return counts, lst

    ac.check_list(*snapshot(want), want)
    fin = ac.tiers_finish(6, 3, ef, tr)
    s = next(k for k, w in enumerate(want) if len(w) >= 3)
    fin_pt = next(p for p in np.flatnonzero(fin) if (p // 64) % 64 == s)
    extra = [w.copy() for w in want]; extra[s] = np.sort(np.append(extra[s], fin_pt))
    with pytest.raises(AssertionError, match="queued but the rule says finished"):
        ac.check_list(*snapshot(extra), want)
    fewer = [w.copy() for w in want]; fewer[s] = fewer[s][1:]
    with pytest.raises(AssertionError, match="finished but the rule says queued"):
        ac.check_list(*snapshot(fewer), want)
    swapped = [w.copy() for w in want]; swapped[s] = swapped[s][::-1]
    with pytest.raises(AssertionError, match="out of order"):
        ac.check_list(*snapshot(swapped), want)
    ac.check_list(*snapshot(swapped), want, runs=False)
    over = snapshot(want); over[0][s] = over[1].shape[1] + 1
    with pytest.raises(AssertionError, match="beyond seg_cap"):
        ac.check_list(*over, want)
    # a first launch that queues everything, and the outputs' rule in place of the trace's
    allq = ac.by_segment(np.arange(len(ef)))
    with pytest.raises(AssertionError, match="queued but the rule says finished"):
        ac.check_list(*snapshot(allq), want)
    naive = ac.by_segment(np.flatnonzero(~((it == nact + 1) & (ef == 1) & (nact <= 3))))
    with pytest.raises(AssertionError, match="finished but the rule says queued"):
        ac.check_list(*snapshot(naive), want)


def test_case_table_reaches_every_instantiation_of_the_library():
    assert os.path.exists(LIB), "build the library first"
    tiers, lane, slab = set(), set(), set()
    for k in _kernel_vgprs(LIB, r"4lmpc16avi_tiers_kernelILi\d+ELi\d+ELb\d+EE"):
        m = re.search(r"16avi_tiers_kernelILi(\d+)ELi(\d+)ELb(\d)EE", k)
        tiers.add((int(m.group(1)), int(m.group(2)), bool(int(m.group(3)))))
    for k in _kernel_vgprs(LIB, r"4lmpc15avi_lane_kernelILi\d+ELb\d+EE"):
        m = re.search(r"15avi_lane_kernelILi(\d+)ELb(\d)EE", k)
        lane.add((int(m.group(1)), bool(int(m.group(2)))))
    for k in _kernel_vgprs(LIB, r"4lmpc10avi_kernelILb\d+ELb\d+EE"):
        m = re.search(r"10avi_kernelILb(\d)ELb(\d)EE", k)
        slab.add((bool(int(m.group(1))), bool(int(m.group(2)))))
    inst = ac.instantiations()
    assert tiers == inst["tiers"], sorted(tiers ^ inst["tiers"])
    assert lane == inst["lane"], sorted(lane ^ inst["lane"])
    assert slab == inst["slab"], sorted(slab ^ inst["slab"])
    assert len(tiers) + len(lane) + len(slab) == 38


def test_record_snapshot_and_option_are_declared_and_exported():
    import linearmpc_jl_amd as lmpc
    L = lmpc.lib()
    for sym in ("lmpc_avi_launch_info", "lmpc_avi_list_read"):
        assert sym in lmpc.SYMBOLS and hasattr(L, sym)
    Q = lmpc.BatchedQP
    W = len(Q.AVI_LAUNCH_FIELDS)
    out = (ctypes.c_int32 * (Q.AVI_LAUNCHES_KEPT * W))()
    assert L.lmpc_avi_launch_info(None, out, 8) == -100 and L.lmpc_avi_list_read(None, 0, out, None, 0) == -100
    assert W == 12 and Q.AVI_LAUNCHES_KEPT == 8 >= 6
    header = open(os.path.join(ROOT, "include", "lmpc_hip.h")).read()
    assert "#define LMPC_AVI_INFO_WORDS 12" in header and "#define LMPC_AVI_INFO_KEPT 8" in header
    assert "int lmpc_avi_launch_info(const lmpc_handle *h, int32_t *out, int max);" in header
    assert "long long lmpc_avi_list_read(lmpc_handle *h, int which, int32_t *counts, int32_t *list, long long list_words);" in header
    assert (Q.AVI_TIERS, Q.AVI_LANE, Q.AVI_SLAB) == (ac.STAGE_TIERS, ac.STAGE_LANE, ac.STAGE_SLAB) == (1, 2, 3)
    for name, v in (("LMPC_AVI_TIERS", 1), ("LMPC_AVI_LANE", 2), ("LMPC_AVI_SLAB", 3)):
        assert f"#define {name} {v}" in header
    assert '"avi_chain_groups"' in header and "#define LMPC_FRONT_INFO_WORDS 8" in header


def test_avi_cases_imports_nothing_of_the_library():
    import ast
    tree = ast.parse(open(ac.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add(node.module or "")
    assert not [n for n in names if "linearmpc" in n or n == "torch"], names
