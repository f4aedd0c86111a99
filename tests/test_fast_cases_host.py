"""Host side of the one-launch kernel's tests (no GPU): every case of tests/fast_cases.py meets the conditions that keep
tests/test_gpu_fast.py from passing emptily -- on the oracle alone, with the pack oracle.ldp.qp2ldp makes --, and the
case table covers exactly the fast_kernel / fast_kernel_multi instantiations the built library holds (kernel NAMES
from the AMDGPU metadata notes; no code is read)."""
import os
import re

import numpy as np
import pytest

import fast_cases as fc
from test_fast_fallback import LIB, _kernel_vgprs


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_case_meets_the_conditions_on_the_oracle(case):
    th = fc.theta(case, fc.N_COND)
    x, ef, it, act = fc.reference(case, th)
    st = fc.check_fast_conditions(case, it, act, ef)
    assert st["failed"] == 0, st
    # the smaller batches are prefixes of this one; the further batches of the several-batches tests differ from it
    assert np.array_equal(fc.theta(case, 65), th[:65]) and not np.array_equal(fc.theta(case, 65, batch=1), th[:65])


def test_conditions_reject_batches_that_miss_one():
    case = fc.BY_PAIR[(3, 5)]
    th = fc.theta(case, fc.N_COND)
    x, ef, it, act = fc.reference(case, th)
    fc.check_fast_conditions(case, it, act, ef)
    rem = fc.removing(it, act)
    keep = np.flatnonzero(~rem)
    pad = np.resize(keep, len(it))                           # the same batch without a single removing point
    with pytest.raises(AssertionError, match="removed"):
        fc.check_fast_conditions(case, it[pad], act[pad], ef[pad])
    fc.check_fast_conditions(fc.BY_PAIR[(2, 5)], it[pad], act[pad], ef[pad])     # (not asked of n = 2)
    hard = np.resize(np.flatnonzero(it > 1), len(it))
    with pytest.raises(AssertionError, match="settled"):
        fc.check_fast_conditions(case, it[hard], act[hard], ef[hard])
    # every third point queued: no workgroup's 512 problems hold more than kFastPay of them
    case5 = fc.BY_PAIR[(5, 7)]
    x, ef5, it5, act5 = fc.reference(case5, fc.theta(case5, fc.N_COND))
    sett, queued = np.flatnonzero(it5 == 1), np.flatnonzero(it5 > 1)
    thin = np.array([queued[i % len(queued)] if i % 3 == 0 else sett[i % len(sett)] for i in range(len(it5))])
    with pytest.raises(AssertionError, match="kFastPay"):
        fc.check_fast_conditions(case5, it5[thin], act5[thin], ef5[thin])
    with pytest.raises(AssertionError, match="1000"):
        fc.check_fast_conditions(case, it[:65], act[:65], ef[:65])


def test_iteration_limit_case_fails_points_on_the_oracle():
    case = fc.LIMIT_CASE
    assert case.n == 5 and case.iter_limit == fc.ITER_LIMIT_MIN
    x, ef, it, act = fc.reference(case, fc.theta(case, fc.N_COND))
    assert (ef == -4).sum() >= 8 and (it[ef == -4] == fc.ITER_LIMIT_MIN).all() and (ef == 1).sum() >= 1000


def test_case_table_covers_every_instantiation_of_the_library():
    assert os.path.exists(LIB), "build the library first"
    names = _kernel_vgprs(LIB, r"fast_kernel(_multi)?ILi\d+E")
    found = {"plain": set(), "gather": set(), "multi": set()}
    for k in names:
        m = re.search(r"fast_kernel(_multi)?ILi(\d+)ELi(\d+)ELi(\d+)E(?:Lb([01])E)?E", k)
        assert m, k
        form = "multi" if m.group(1) else ("gather" if m.group(5) == "1" else "plain")
        found[form].add((int(m.group(2)), int(m.group(3)), int(m.group(4))))
    want = fc.instantiations()
    assert len(want) == 56 == len(fc.CASES)
    for form in ("plain", "gather", "multi"):
        assert found[form] == want, (form, sorted(found[form] ^ want))
    # one pair per NT for the record paths and the several-batches launch: both parities of NT (LASTB 512 / 1024),
    # the single half piece and the eight pieces, n = 5 wherever it is instantiated
    assert [c.nth for c in fc.NT_CASES] == [1, 2, 3, 7, 8, 9, 15, 16]
    assert all(c.n == 5 for c in fc.NT_CASES if c.nth <= 8) and all(c.n in (3, 4) for c in fc.NT_CASES if c.nth > 8)


def test_gather_layouts_cover_every_block_state():
    state = {b: set() for b in "rdp"}
    nup = set()
    for c in fc.CASES:
        nx, nr, nd, nu_, np_ = c.layout
        assert nx >= 1 and min(c.layout) >= 0 and sum(c.layout) == c.nth and nu_ <= c.gather_nout, c
        assert c.gather_nout in (1, c.n)
        nup.add("nu" if (nu_ == c.gather_nout and nu_ > 1) else nu_)
        for b, w in zip("rdp", (nr, nd, np_)):
            assert not (w == 0 and b in c.null)
            state[b].add("absent" if w == 0 else ("null" if b in c.null else "present"))
        th = fc.theta(c, 5)
        g = fc.gather_blocks(c, th)
        parts = [g["state"], g["reference"], g["disturbance"], g["control"][:, :nu_], g["parameter"]]
        assert np.array_equal(np.hstack([p for p in parts if p is not None and p.shape[1]]), th)
        assert np.isnan(g["control"][:, nu_:]).all()
    assert all(s == {"absent", "present", "null"} for s in state.values()), state
    assert {0, 1, "nu"} <= nup, nup
    assert {c.use_w for c in fc.CASES} == {True, False}


def test_fast_cases_imports_nothing_of_the_library():
    import ast
    tree = ast.parse(open(fc.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert not names & {"linearmpc_jl_amd", "torch", "ctypes"}, names
