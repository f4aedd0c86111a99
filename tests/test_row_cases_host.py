"""Host side of the row path's tests (no GPU): every case of tests/row_cases.py meets the conditions that keep
tests/test_gpu_row.py from passing emptily -- on the oracle alone, with the pack oracle.ldp.qp2ldp makes --, the
condition checkers reject batches that miss one, the launch arithmetic restated in row_cases.py matches the committed
tables of lmpc_row_kernel.hpp / lmpc_row_inst.hip, and the case table claims exactly the row_kernel instantiations that
launch_row / launch_row_bnb spell and the built library holds (kernel NAMES from the AMDGPU metadata notes).

The conditions, each a floor of FLOOR = 8 points of the 400-point cold batch unless the table exempts a case (reasons
next to the table): points settled at iteration 1; append-only points; points that remove a row again; infeasible
points; exit flag 2 where rows are SOFT; for EVERY 16-row constraint slot r < (m + 15) / 16 final active sets that hold
a row of it, upper and lower side counted apart (where m = 1 (mod 16) the last slot IS the last row); the iteration
limit where one is set; on the deep cases final sets of capacity - 1 rows and of the whole capacity; final sets beyond
16 rows on every case of a two-position-slot shape; the two-pass shares; no final set beyond capFull; searches: summed
iterations beyond twice the relaxation's plus two, every binary row in every solved point's final set, a binary that
changes its side between points."""
import os
import re
from dataclasses import replace

import numpy as np
import pytest

import row_cases as rc
import wave_cases as wc
from test_fast_fallback import LIB, _kernel_vgprs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "linearmpc.jl_amd", "csrc")
_REF = {}
ids = lambda c: c.name


def _cold(case):
    if case not in _REF:
        th = rc.theta(case)
        _REF[case] = (th,) + tuple(rc.reference(case, th))
    return _REF[case]


@pytest.mark.parametrize("case", rc.PLAIN + rc.PLAIN_F32, ids=ids)
def test_plain_case_meets_the_conditions_on_the_oracle(case):
    th, x, ef, it, act = _cold(case)
    st = rc.check_row_conditions(case, ef, it, act)
    if case.w.iter_limit:
        assert (it[ef == -4] == case.w.iter_limit).all(), st
    e = rc.expected(case)
    assert e is not None and e["pass"] == 1 and e["cap"] <= e["shape"][3]
    for N in rc.batch_sizes(e["nwv"]):
        assert np.array_equal(rc.theta(case, N), th[:N])


@pytest.mark.parametrize("case", rc.BNB, ids=ids)
def test_search_case_meets_the_conditions_on_the_oracle(case):
    th, x, ef, it, act = _cold(case)
    st = rc.check_search_conditions(case, ef, it, rc.relaxed_iters(case, th), act)
    e = rc.expected(case)
    assert e is not None and e["inst"][5] == 1, st
    assert e["pass"] == (0 if case.mode == "full" else 1)


@pytest.mark.parametrize("case", [rc.DEEP_STACK, rc.DEEP_STACK_F32], ids=ids)
def test_deep_stack_search_leaves_the_binaries_free_at_the_root(case):
    th = rc.theta(case, rc.N_DEEP_STACK)
    x, ef, it, act = rc.reference(case, th)
    rel = rc.relaxed_active(case, th)
    st = rc.check_deep_stack(case, ef, act, rel)
    assert st["upper_among_last"] and st["lower_among_last"], st
    assert rc.expected(case)["inst"][1:] == (3, 4, 4, 48, 1) and case.w.nbin > 32
    with pytest.raises(AssertionError, match="free at the root"):
        rc.check_deep_stack(case, ef, act, act)              # (every binary on a bound at the root: no depth to speak of)
    # the table's other searches do NOT meet it: half of their binaries sit on a bound at the root
    other = rc.BY_NAME["bnb-n46-m64-b34" + ("-f32" if case.f32 else "")]
    tho = rc.theta(other, rc.N_DEEP_STACK)
    xo, efo, ito, acto = rc.reference(other, tho)
    with pytest.raises(AssertionError, match="free at the root"):
        rc.check_deep_stack(other, efo, acto, rc.relaxed_active(other, tho))


@pytest.mark.parametrize("case", [rc.NTH0, rc.NTH0_F32], ids=ids)
def test_problem_without_parameters(case):
    th, x, ef, it, act = _cold(case)
    assert th.shape == (wc.N_COND, 0)
    wc.check_nth0(case.w, ef, it, act)
    assert rc.expected(case)["inst"][1:5] == (1, 4, 10, 16)


@pytest.mark.parametrize("kind", ["none", "all"])
@pytest.mark.parametrize("name", rc.SHARE_CASES)
def test_two_pass_shares_none_and_all(name, kind):
    for case in (rc.BY_NAME[name], rc.BY_NAME[name + "-f32"]):
        th = rc.theta(case, batch=2, scales=rc.SHARE_SCALES[kind])
        x, ef, it, act = rc.reference(case, th)
        wc.check_two_pass_share(case.w, act, rc.expected(case)["cap"], kind)
        assert (wc.popcount(act) <= case.cap_full).all()


@pytest.mark.parametrize("kind", ["all-infeasible", "all-settled"])
@pytest.mark.parametrize("name", rc.LIMIT_BATCH_CASES)
def test_limit_batches(name, kind):
    for case in (rc.BY_NAME[name], rc.BY_NAME[name + "-f32"]):
        x, ef, it, act = rc.reference(case, wc.limit_theta(case.w, kind))
        wc.check_limit_batch(case.w, ef, it, act, kind)


@pytest.mark.parametrize("name", rc.NOUT_CASES)
def test_several_outputs_keep_the_instantiation(name):
    case = rc.BY_NAME[name]
    for nout in (case.n // 2, case.n):
        c = replace(case, nout=nout)
        e = rc.expected(c)
        assert e is not None and e["inst"] == rc.expected(case)["inst"]
        assert rc.reference(c, rc.theta(c))[0].shape == (wc.N_COND, nout)


def test_conditions_reject_batches_that_miss_one():
    case = rc.BY_NAME["s2-n20-m90-nth17-soft"]
    th, x, ef, it, act = _cold(case)
    rc.check_row_conditions(case, ef, it, act)
    nact = wc.popcount(act)
    up, lo = wc.side_bits(act, case.m)

    def missed_by(c, EF, IT, ACT):
        """The conditions check_row_conditions names as missed (the second entry of its assertion's message)."""
        with pytest.raises(AssertionError) as err:
            rc.check_row_conditions(c, EF, IT, ACT)
        arg = err.value.args[0]
        assert isinstance(arg, tuple) and arg[0] == c.name and isinstance(arg[1], list), arg
        return arg[1]

    def rejects(drop, what, c=case, EF=ef, IT=it, ACT=act):
        """The batch with the points `drop` replaced by settled ones misses the condition `what` (its full wording)."""
        idx = np.arange(len(IT))
        assert drop.any(), what
        idx[np.flatnonzero(drop)] = np.flatnonzero((IT == 1) & (EF == 1) & ~drop)[0]
        assert what in missed_by(c, EF[idx], IT[idx], ACT[idx]), what

    rejects((it == nact + 1) & (it > 1) & (ef >= 1), "append-only")
    rejects((it > nact + 1) & (ef >= 1), "rows removed again")
    rejects(ef == -1, "infeasible points")
    rejects(ef == 2, "exit flag 2")
    rejects(nact > 16, "working sets beyond 16 rows")
    for r in range((case.m + 15) // 16):                    # per 16 rows: every slot on its own
        rejects(up[:, 16 * r:16 * r + 16].any(axis=1), "an upper side active in every 16-row slot")
        rejects(lo[:, 16 * r:16 * r + 16].any(axis=1), "a lower side active in every 16-row slot")
    idx = np.resize(np.flatnonzero(it != 1), len(it))
    assert "settled at iteration 1" in missed_by(case, ef[idx], it[idx], act[idx])
    with pytest.raises(AssertionError, match="N_COND"):
        rc.check_row_conditions(case, ef[:65], it[:65], act[:65])
    # a set beyond capFull: beyond every kernel of the library
    big = np.array(act, copy=True)
    big[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    with pytest.raises(AssertionError, match="capFull"):
        rc.check_row_conditions(case, ef, it, big)
    # m = 1 (mod 16), not (mod 64): the last row -- and that it is the narrowing of row_cases.problem that makes it active
    c1 = rc.BY_NAME["s1-n10-m49-nth5"]
    th1, x1, ef1, it1, act1 = _cold(c1)
    u1, l1 = wc.side_bits(act1, c1.m)
    rejects(u1[:, -1] | l1[:, -1], "the last row, alone in its slot, active", c1, ef1, it1, act1)
    Hn, Hw = rc.problem(c1), wc.problem(c1.w)
    assert Hn[4][-1] == c1.w.last * Hw[4][-1] and Hn[5][-1] == c1.w.last * Hw[5][-1]
    # the iteration limit, the deep working sets, the share that keeps the statistics from a 16-row first pass
    cl = rc.BY_NAME["s1-n10-m63-nth5-limit"]
    thl, xl, efl, itl, actl = _cold(cl)
    rejects(efl == -4, "iteration limit reached", cl, efl, itl, actl)
    for name in ("s1-n15-m64-nth6-deep", "s2-n30-m96-nth6-deep", "s2-n31-m96-nth6-deep"):
        cd = rc.BY_NAME[name]
        thd, xd, efd, itd, actd = _cold(cd)
        nd = wc.popcount(actd)
        rejects(nd == cd.full - 1, "working sets of capacity - 1 rows", cd, efd, itd, actd)
        rejects(nd == cd.full, "working sets that fill the capacity", cd, efd, itd, actd)
    c2 = rc.BY_NAME["t2-n48-m160-nth5"]
    th2, x2, ef2, it2, act2 = _cold(c2)
    rejects(wc.popcount(act2) > 16, "beyond16_share", c2, ef2, it2, act2)
    with pytest.raises(AssertionError, match="two-pass share"):
        rc.check_row_conditions(replace(c2, share="none"), ef2, it2, act2)
    cm = rc.BY_NAME["s1-n12-m56-nth16-c8"]
    thm, xm, efm, itm, actm = _cold(cm)
    assert cm.share == "most" and rc.check_share(cm, actm, 8, "most")[0] > wc.N_COND // 2
    half = np.array(actm, copy=True)
    half[np.flatnonzero(wc.popcount(actm) > 8)[:150]] = 0    # (150 of the sets beyond 8 rows emptied: no longer most)
    with pytest.raises(AssertionError, match="two-pass share"):
        rc.check_share(cm, half, 8, "most")
    # work-list segments behind the tiers pass (tiles of 64 points): a batch whose removing points all lie in one tile
    one = np.zeros(wc.N_FILL, bool)
    one[:64] = True
    with pytest.raises(AssertionError, match="work-list segments"):
        rc.check_segments(one, "all-filled", rc.TIERS_BLOCK)
    with pytest.raises(AssertionError, match="work-list segments"):
        rc.check_segments(np.ones(wc.N_FILL, bool), "some-empty", rc.TIERS_BLOCK)
    cs = rc.BY_NAME["t2-n40-m100-nth2-slow"]
    ths, xs, efs, its, acts = _cold(cs)
    rejects(wc.popcount(acts) > 64, "working sets beyond 64 rows", cs, efs, its, acts)


def test_tiers_list_case_fills_the_segments_as_the_gpu_test_needs():
    """Work-list mode behind the tiers pass: wavefront gw of that pass takes the tiles (64 points) gw, gw + nw, ... and
    writes to segment gw % 64, nw a multiple of 64 -- tile t goes to segment t % 64.  A point that removes a row again is
    certainly left to the list.  At N_COND the segments 7 ... 63 hold nothing and one holds FLOOR such points; at
    N_FILL every segment does."""
    src = open(os.path.join(CSRC, "lmpc_qp_tiers_kernel.hpp")).read()
    assert "const long long gw = (long long)blockIdx.x * 4 + wv, nw = (long long)gridDim.x * 4;" in src
    assert "const int shard = (int)(gw % kShards);" in src and "for (long long base = gw * 64; base < nprob; base += nw * 64) {" in src
    assert "grid = ((grid + 15) / 16) * 16;" in open(os.path.join(CSRC, "lmpc_qp_tiers.hip")).read()
    case = rc.LIST_TIERS
    assert 2 <= case.n <= 12 and case.m <= 64 and 1 <= case.w.nth <= 16 and not case.f32 and not case.w.nsoft
    th, x, ef, it, act = _cold(case)
    removing = (it > wc.popcount(act) + 1) & (ef >= 1)
    assert rc.check_segments(removing, "some-empty", rc.TIERS_BLOCK)[1] >= wc.FLOOR
    assert not np.bincount((np.arange(wc.N_COND) // 64) % 64, weights=removing, minlength=64)[7:].any()
    reps = -(-wc.N_FILL // wc.N_COND)
    assert rc.check_segments(np.concatenate([removing] * reps)[:wc.N_FILL], "all-filled", rc.TIERS_BLOCK)[0] >= wc.FLOOR


def test_search_conditions_reject_batches_that_miss_one():
    case = rc.BY_NAME["bnb-n14-m32-b5"]
    th, x, ef, it, act = _cold(case)
    itr = rc.relaxed_iters(case, th)
    rc.check_search_conditions(case, ef, it, itr, act)
    with pytest.raises(AssertionError, match="several nodes"):
        rc.check_search_conditions(case, ef, itr, itr, act)
    with pytest.raises(AssertionError, match="solved searches"):
        rc.check_search_conditions(case, np.full_like(ef, -1), it, itr, act)
    one = np.flatnonzero(ef >= 1)[:1].repeat(len(ef))
    with pytest.raises(AssertionError, match="changes its side"):
        rc.check_search_conditions(case, ef[one], it[one], itr[one] * 0, act[one])
    loose = np.array(act, copy=True)
    loose[:, 0] &= ~np.uint64(1)                             # binary row 0 (upper side) out of every final set ...
    loose[:, (case.m + 0) >> 6] &= ~(np.uint64(1) << np.uint64(case.m & 63))         # ... and its lower side
    with pytest.raises(AssertionError, match="binary row outside"):
        rc.check_search_conditions(case, ef, it, itr, loose)


def test_tables_cover_what_the_issue_lists():
    plain = rc.PLAIN
    by_shape = {}
    for c in plain:
        by_shape.setdefault(rc.expected(c)["shape"], []).append(c)
    assert set(by_shape) == set(rc.SHAPES)
    # variable slots: full widths and one beyond the previous slot; n = 1, 2 on the one-slot shape
    assert {c.n for c in plain} >= {1, 2, 15, 16, 17, 30, 31, 32, 33, 48, 49, 64}
    assert {c.n for c in by_shape[(1, 1, 4, 16)]} >= {1, 2}
    # ... PER SHAPE: the last variable slot full (lane 15 carries a variable) and one variable beyond the slot before
    for sh, cs in by_shape.items():
        ns = {c.n for c in cs}
        assert max(ns) == 16 * sh[1], (sh, sorted(ns))
    # ({2, 2, 6, 32} runs at n = 31, its own capacity, and from n = 32 on through "wave_cap1" 32 -- a capacity of 32 rows
    # exists at no smaller n, so n = 17 cannot reach it)
    assert {c.n for c in by_shape[(2, 2, 6, 31)]} >= {16, 17, 32} and {c.n for c in by_shape[(2, 2, 6, 32)]} == {31, 32}
    assert all(rc.launch_for(17, 90, 4, 1, c, 8)["shape"] != (2, 2, 6, 32) for c in range(1, 19))
    for sh in ((1, 4, 10, 16), (2, 4, 10, 31), (2, 4, 10, 32)):
        assert {c.n for c in by_shape[sh]} >= {33, 48, 49, 64}, (sh, sorted(c.n for c in by_shape[sh]))
    # constraint slots: 16 MS, 16 (MS - 1) + 1 and one in between, per MS
    for MS in (4, 6, 10):
        ms = {c.m for sh, cs in by_shape.items() if sh[2] == MS for c in cs}
        assert 16 * MS in ms and 16 * (MS - 1) + 1 in ms and any(16 * (MS - 1) + 1 < v < 16 * MS for v in ms), (MS, sorted(ms))
    # capacity: deep cases at 16, 31 and 32 rows
    assert {c.full for c in plain if c.w.deep} >= {16, 31, 32}          # (and 11: the tiers-list case)
    # first passes
    caps = {(rc.expected(c)["shape"], rc.expected(c)["cap"]) for c in plain if c.share}
    assert caps >= {((1, 4, 10, 16), 16), ((2, 4, 10, 31), 31), ((2, 4, 10, 32), 32), ((1, 1, 4, 16), 8), ((2, 2, 6, 31), 8)}
    assert all(c.share == "most" for c in plain if rc.expected(c)["cap"] == 8)          # (8 rows: most points outgrow them)
    assert any(c.slow and c.n <= 64 and c.w.cap == 64 for c in plain)
    # the aux block: the same shape at n = 48, m = 160 with four and with three wavefronts per workgroup
    a, b = rc.expected(rc.BY_NAME["t2-n48-m160-nth5"]), rc.expected(rc.BY_NAME["t2-n48-m160-nth33-aux"])
    assert a["shape"] == b["shape"] and a["aux"] == b["aux"] == 1 and (a["nwv"], b["nwv"]) == (4, 3)
    assert {c.w.nth for c in plain + (rc.NTH0,)} >= {0, 1, 16, 17, 33}
    assert any(c.w.onesided for c in plain) and any(c.w.imm for c in plain) and any(c.w.dup for c in plain)
    assert any(c.w.nsoft for c in plain) and any(c.w.iter_limit for c in plain)
    assert {c.name for c in rc.PLAIN_F32} == {c.name + "-f32" for c in plain}
    # searches: both real types; m = 17 / 32 and 49 / 64; binaries in every register slot of the stack; both first-pass rules
    for f32 in (False, True):
        b = [c for c in rc.BNB if c.f32 == f32]
        assert {c.m for c in b if rc.expected(c)["shape"] == (1, 1, 2, 16)} == {17, 32}
        assert {c.m for c in b if rc.expected(c)["shape"][0] == 3} >= {49, 64}
        nb = sorted(c.w.nbin for c in b)
        assert any(v <= 16 for v in nb) and any(17 <= v <= 32 for v in nb) and any(33 <= v <= 47 for v in nb)
        assert {(rc.expected(c)["cap"], rc.expected(c)["pass"]) for c in b if c.mode == "default"} == {(44, 1), (48, 1)}
        assert {rc.expected(c)["shape"][3] for c in b if c.mode == "full" and c.full > 16} == {44, 48}
        assert any(c.mode == "cap1" and rc.expected(c)["cap"] == 20 and c.share == "most" for c in b)
    # refusals the arithmetic can state
    assert rc.expected(rc.REFUSE_WIDE) is None and rc.expected(rc.REFUSE_M) is None and rc.expected(rc.REFUSE_BIN) is None
    assert rc.launch_for(64, 160, 5, 1, 31, 8) is not None                  # (the wide case's problem class itself is covered)


# ---------------------------------------------------------------------------------------------------------------------
# the restated arithmetic against the sources
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_restated_layout_sizes_match_the_committed_tables():
    src = _src("lmpc_row_kernel.hpp")

    def table(name):
        m = re.search(r"constexpr int " + name + r"\[\d+\] = \{([^}]*)\}", src)
        assert m, name
        return [int(v) for v in m.group(1).replace("\n", " ").split(",")]

    # rowp_size: the literal sizes of the padded layouts, and that every committed column of a table fits inside its size
    m = re.search(r"constexpr int rowp_size\(int capp\) \{ return capp == 48 \? (\d+) : \(capp == 44 \? (\d+) : \(capp == 16 \? (\d+) : rowp_cb\(capp, capp - 1\)\)\); \}", src)
    assert m, "rowp_size"
    assert tuple(int(v) for v in m.groups()) == (rc.rowp_size(48), rc.rowp_size(44), rc.rowp_size(16))
    for name, capp, lrow in (("k48", 48, 49), ("k44", 44, 45), ("k16", 16, 17)):
        cbm = table(name)
        assert len(cbm) == capp - 1
        # column t holds rows t + 1 .. capp - 1 at cbm[t] + p, one padding entry on top: all inside the size
        assert max(cbm[t] + lrow - 1 for t in range(capp - 1)) < rc.rowp_size(capp) + (lrow - capp), name
        assert min(cbm[t] + (t & ~3) for t in range(capp - 1)) >= 0, name
    k31 = table("k31")
    assert len(k31) == 30 and rc.rowp_size(31) == rc.rowp_cb(31, 30) == 538 and rc.rowp_size(32) == rc.rowp_cb(32, 31)
    assert max(k31[t] + 30 for t in range(30)) < rc.rowp_size(31)
    # the helper formulas, textually
    for text in ("while ((nwv * ps) % 32 != 16) ps++;",
                 "return !(capp == 44 && rs == 4);",
                 "for (int q = 0; q < 16; q++, ps += 4)",
                 "return 16 * ms + ((rs == 4 && ms % 4 == 0) ? 4 : 2);",
                 "return ((ms > 6 && s >= 2) || (s >= 3 && rs == 8)) ? 256 : 512;",
                 "return ((ms > 6 && s >= 2) || (s >= 3 && rs == 8)) ? 1 : ((s == 1 && ms <= 6) ? LMPC_ROW_WPS1 : 2);",
                 "#define LMPC_ROW_WPS1 3",
                 "return (16 * ms < 48 ? 16 * ms : 48) - 1;",
                 "return 64 * s + ((rowp_size(capp) + 3) & ~3);",
                 "return 16 * s + 16;",
                 "return (front + 15) & ~(size_t)15;",
                 "return P.oGf - P.odu;"):
        assert text in src, text
    # values at the points the launches use
    assert [rc.row_ps(16, w) for w in (6, 8)] == [184, 174] and rc.row_ps(31, 8) == 538 and rc.row_ps(31, 4) == 540
    assert rc.row_ps(16, 7) > 0 and rc.row_ps4(48, 8) == -1 and rc.row_ps4(48, 4) % 4 == 0
    assert rc.row_mpad(4, 4) == 68 and rc.row_mpad(4, 8) == 66 and rc.row_mpad(10, 4) == 162
    assert rc.row_bnb_depth_max(2) == 31 and rc.row_bnb_depth_max(4) == 47


def test_restated_shape_tables_and_launcher_match_the_source():
    src = _src("lmpc_row_inst.hip")

    def shapes(name):
        m = re.search(r"constexpr RowShape " + name + r"\[\] = \{(.*?)\n\};", src, re.S)
        assert m, name
        return tuple(tuple(int(v) for v in t) for t in re.findall(r"\{(\d+), (\d+), (\d+), (\d+)\}", m.group(1)))

    assert shapes("kRowShapes") == rc.SHAPES and shapes("kRowShapesBnb") == rc.SHAPES_BNB
    for text in ("return n <= 16 * sh.NS && m <= 16 * sh.MS && cap <= sh.CAPP && m <= 256",
                 "for (int nwv : {8, 7, 6, 5, 4, 3, 2, 1}) {",
                 "const size_t mt = (size_t)((n + 3) & ~3) * row_mpad(sh.MS, (int)rs);",
                 "size_t lds = rs * (32 + mt + (size_t)nwv * 4 * ps + 2) + sizeof(int32_t) * ((size_t)m + sh.CAPP) + 16;",
                 "lds = row_aux_offset(front) + rs * (size_t)row_aux_reals(h->W) + 16;",
                 "int blocks = (int)(kLdsMax / lds);",
                 "const int maxw = 4 * row_waves_per_simd(sh.S, sh.MS, (int)rs);",
                 "if (waves > bestWaves) {",
                 "if (full <= 32 && row_launch_for(h, full, rs, &rl)) cap = full;",
                 "else if ((h->rowKernel > 0 || fits) && row_launch_for(h, 31, rs, &rl)) cap = 31;",
                 "if (h->S.iter_limit < 2 || h->nBinary > 47) return 0;",
                 "const int c1 = h->nBinary + 4 <= 44 ? 44 : 48;",
                 "if (h->waveTwoPass == 0 || full <= 52) return 0;"):
        assert text in src, text
    assert "constexpr size_t kLdsMax = 160 * 1024;" in _src("lmpc_internal.hpp") and rc.LDS_MAX == 160 * 1024
    # the only pass / first of two: launch_wave_inst's rule, which `expected` restates
    assert "if (rcap >= capW && !(h->bigPath && h->capFull > capW)) {" in _src("lmpc_wave_launch.hpp")
    assert "h->capFull = P.n + 2 + P.nsoft;" in _src("lmpc_api.hip")


def _spelled():
    """The instantiations launch_row / launch_row_bnb name, per real type (LMPC_ROW_REAL: double and float units)."""
    src = _src("lmpc_row_inst.hip")
    plain = {tuple(int(v) for v in t) for t in re.findall(r"return LMPC_ROW\((\d+), (\d+), (\d+), (\d+)\);", src)}
    bnb = {tuple(int(v) for v in t) for t in re.findall(r"launch_row_shape<R, (\d+), (\d+), (\d+), (\d+), true>", src)}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    reals = {8 if r == "double" else 4 for r in re.findall(r"-DLMPC_ROW_REAL=(\w+) -DLMPC_ROW_HELPERS=1|-DLMPC_ROW_REAL=(\w+) -c", mk) for r in r if r}
    reals_bnb = {8 if r == "double" else 4 for r in re.findall(r"-DLMPC_ROW_REAL=(\w+) -DLMPC_ROW_BNB=1", mk)}
    return {(rs,) + sh + (0,) for rs in reals for sh in plain} | {(rs,) + sh + (1,) for rs in reals_bnb for sh in bnb}


def _built():
    assert os.path.exists(LIB), "build the library first"
    out = set()
    for k in _kernel_vgprs(LIB, r"4lmpc10row_kernelI[df]"):
        m = re.search(r"10row_kernelI([df])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE", k)
        assert m, k
        R, S, NS, MS, CAPP, B = m.groups()
        out.add((8 if R == "d" else 4, int(S), int(NS), int(MS), int(CAPP), int(B)))
    return out


def test_case_table_claims_exactly_the_instantiations_spelled_and_built():
    want = rc.instantiations()
    assert len(rc.built()) == 18 and not rc.UNREACHED
    assert want == rc.built(), sorted(want ^ rc.built())
    assert want == _spelled(), sorted(want ^ _spelled())
    assert want == _built(), sorted(want ^ _built())


def test_launch_record_entry_point_is_exported_and_refuses_bad_arguments():
    import ctypes
    import linearmpc_jl_amd as lmpc
    L = lmpc.lib()
    assert "lmpc_row_launch_info" in lmpc.SYMBOLS and hasattr(L, "lmpc_row_launch_info")
    out = (ctypes.c_int32 * 80)()
    assert L.lmpc_row_launch_info(None, out, 4) == -100 and len(lmpc.BatchedQP.ROW_LAUNCH_FIELDS) == 20
    header = open(os.path.join(ROOT, "include", "lmpc_hip.h")).read()
    assert "#define LMPC_ROW_INFO_WORDS 20" in header and "int lmpc_row_launch_info(const lmpc_handle *h, int32_t *out, int max);" in header


def test_row_cases_imports_nothing_of_the_library():
    import ast
    tree = ast.parse(open(rc.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert not names & {"linearmpc_jl_amd", "torch", "ctypes"}, names
