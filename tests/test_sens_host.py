"""Differentiable solve on the host (lmpc_solve_vjp_host / lmpc_solve_jacobian_host): no GPU.  The host twins run the
kernels' arithmetic from a raw pack; they are held bit for bit to the numpy restatement of the contract
(sens_reference.py) on every case of sens_cases.py, and the contract itself to the truth: the same formula solved
densely in extended precision, central differences of the oracle, and the explicit-MPC builder's region laws."""
import ctypes
import os

import numpy as np
import pytest

import sens_cases as sc
import sens_reference as sr
import sens_truth as st
from conftest import load_golden
from oracle import ldp as oldp

N_JAC = 257                     # Jacobians are compared on this prefix of a batch (every synthetic size and special is in it)
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "linearmpc.jl_amd", "lib", "liblmpc_hip.so")


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


_CACHE = {}


def _data(lmpc, case):
    """pack, batch and the reference's results of a case (computed once)."""
    if case.name not in _CACHE:
        S = lmpc.default_settings()
        pack = sc.host_pack(case)
        b = sc.build(case, pack)
        cache = sr.derived(pack)
        v, sv = sr.sens(pack, b["active"], b["exitflag"], b["xbar"], S.rho_soft, S.zero_tol, cache)
        J, sj = sr.sens(pack, b["active"][:N_JAC], b["exitflag"][:N_JAC], None, S.rho_soft, S.zero_tol, cache)
        _CACHE[case.name] = dict(pack=pack, batch=b, cache=cache, vjp=v, status=sv, jac=J, jstatus=sj, S=S)
    return _CACHE[case.name]


def _host_call(lmpc, pack, active, exitflag, xbar):
    """The host twin on guarded outputs: (result, status) after checking the guards and that no sentinel is left."""
    L = lmpc.lib()
    n, m, ms, nth, nout = (int(pack[k]) for k in ("n", "m", "ms", "nth", "nout"))
    N, G = len(active), sc.GUARD
    per = nth if xbar is not None else nout * nth
    out = np.full((N + 2 * G, per), sc.SENT)
    status = np.full(N + 2 * G, sc.SENT_I, np.int32)
    arrs = [np.ascontiguousarray(pack[k], dtype=np.float64) for k in ("M", "du", "dl", "Dth", "Rout", "x0", "Xth")]
    sense = np.ascontiguousarray(pack["sense"], dtype=np.int32)
    act = np.ascontiguousarray(active, dtype=np.uint64)
    ef = np.ascontiguousarray(exitflag, dtype=np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    head = (n, m, ms, nth, nout, *[vp(a) for a in arrs], vp(sense), None, 0, N, vp(act), vp(ef))
    po, ps = ctypes.c_void_p(out[G:].ctypes.data), ctypes.c_void_p(status[G:].ctypes.data)
    if xbar is not None:
        xb = np.ascontiguousarray(xbar, dtype=np.float64)
        rc = L.lmpc_solve_vjp_host(*head, vp(xb), po, ps)
    else:
        rc = L.lmpc_solve_jacobian_host(*head, po, ps)
    assert rc == 1, lmpc._cabi.last_error()
    assert (out[:G] == sc.SENT).all() and (out[N + G:] == sc.SENT).all(), "an output guard row was written"
    assert (status[:G] == sc.SENT_I).all() and (status[N + G:] == sc.SENT_I).all(), "a status guard was written"
    assert not (out[G:N + G] == sc.SENT).any() and not (status[G:N + G] == sc.SENT_I).any(), "an output row was not written"
    return out[G:N + G], status[G:N + G]


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_case_conditions(lmpc, case):
    d = _data(lmpc, case)
    sc.check_conditions(case, d["pack"], d["batch"], d["status"])


def test_conditions_reject_batches_that_miss_them(lmpc):
    case = sc.BY_NAME["own-n12-m76-nth17"]
    d = _data(lmpc, case)
    pack, b, status = d["pack"], d["batch"], d["status"]
    sc.check_conditions(case, pack, b, status)

    def cut(keep):
        return {k: (v[keep] if isinstance(v, np.ndarray) and len(v) == len(status) else v) for k, v in b.items()}, status[keep]

    sz = sc.set_sizes(b["active"], pack["m"])
    with pytest.raises(AssertionError, match="wavefront kinds"):            # no wavefront that is all queued
        keep = np.ones(len(status), bool)
        keep[64:128] = False
        sc.check_conditions(case, pack, *cut(np.nonzero(keep)[0]))
    with pytest.raises(AssertionError, match="empty work list"):            # the batch opens with queued points
        sc.check_conditions(case, pack, *cut(np.r_[64:128, 0:64, 128:len(status)]))
    with pytest.raises(AssertionError, match="statuses"):                   # no singular set
        sc.check_conditions(case, pack, *cut(np.nonzero(status != -1)[0]))
    with pytest.raises(AssertionError, match="statuses"):                   # nothing beyond the 64 rows
        sc.check_conditions(case, pack, *cut(np.nonzero(sz <= 64)[0]))
    with pytest.raises(AssertionError, match="synthetic sizes missing"):    # every set of 33 rows replaced by one of 32
        act = b["active"].copy()
        act[(sz == 33) & b["synthetic"]] = act[np.nonzero((sz == 32) & b["synthetic"] & (status == 1))[0][0]]
        sc.check_conditions(case, pack, dict(b, active=act), status)


def test_table_conditions(lmpc):
    sc.check_table(sc.CASES, {c.name: _data(lmpc, c)["status"] for c in sc.CASES})
    with pytest.raises(AssertionError):
        sc.check_table(sc.CASES[:1], {sc.CASES[0].name: _data(lmpc, sc.CASES[0])["status"]})


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_host_twins_equal_the_reference_bit_for_bit(lmpc, case):
    d = _data(lmpc, case)
    b = d["batch"]
    v, s = _host_call(lmpc, d["pack"], b["active"], b["exitflag"], b["xbar"])
    assert np.array_equal(s, d["status"])
    assert np.array_equal(v, d["vjp"])
    J, sj = _host_call(lmpc, d["pack"], b["active"][:N_JAC], b["exitflag"][:N_JAC], None)
    assert np.array_equal(sj, d["jstatus"])
    assert np.array_equal(J.reshape(d["jac"].shape), d["jac"])
    assert (v[s != 1] == 0).all() and (J[sj != 1] == 0).all()
    # the Python wrapper of the twins
    v2, s2 = lmpc.solver.sens_host(d["pack"], b["active"][:65], b["exitflag"][:65], b["xbar"][:65])
    assert np.array_equal(v2, d["vjp"][:65]) and np.array_equal(s2, d["status"][:65])


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_jacobian_rows_equal_the_vjp_of_unit_vectors(lmpc, case):
    d = _data(lmpc, case)
    b, pack = d["batch"], d["pack"]
    nout = pack["nout"]
    for r in sorted({0, nout // 2, nout - 1}):
        e = np.zeros((N_JAC, nout))
        e[:, r] = 1.0
        v, s = _host_call(lmpc, pack, b["active"][:N_JAC], b["exitflag"][:N_JAC], e)
        assert np.array_equal(s, d["jstatus"])
        assert np.array_equal(v, d["jac"][:, r, :]), r
        vr, _ = sr.sens(pack, b["active"][:N_JAC], b["exitflag"][:N_JAC], e, d["S"].rho_soft, d["S"].zero_tol, d["cache"])
        assert np.array_equal(vr, d["jac"][:, r, :]), r


# Measured on the CPU over every distinct set with status 1 of every case's batch (the host twin's Jacobian, which is the
# reference's bit for bit), against the dense solve in np.longdouble:
#     max |J - Jtrue| / (eps cond(K_A) ||Jtrue||_inf)            = 5.15   (fast-n5-nth7)      -> bound 64
#     max |J - Jtrue| / (eps cond(K_A) || sum of |terms| ||_inf) = 2.51   (own-n63-m80-nth1)  -> bound 32
# each bound the next power of two at or above 8 x the measured maximum.  The first measure is undefined where J = 0 --
# a set that pins every output at its own bound -- and blows up where ||J||_inf is the rounding residue of cancelling
# terms (measured there: up to 9.6e14); it is asserted on the sets with ||Jtrue||_inf above 1e-6 of the terms' size.
# The second measure covers every set.  cond(K_A) reaches 1.3e11 in the table (SOFT-heavy sets): the K form loses
# those digits, which is accepted.
TRUTH_BOUND_J, TRUTH_MEASURED_J = 64.0, 5.15
TRUTH_BOUND_TERMS, TRUTH_MEASURED_TERMS = 32.0, 2.51


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_reference_against_the_dense_solve_in_extended_precision(lmpc, case):
    d = _data(lmpc, case)
    b, pack = d["batch"], d["pack"]
    J, s = lmpc.solver.sens_host(pack, b["active"], b["exitflag"])
    assert np.array_equal(J[:N_JAC], d["jac"]) and np.array_equal(s, d["status"])
    rows = sr.rows_of(b["active"], pack["m"])
    done = np.nonzero(s == 1)[0]
    _, first = np.unique(rows[done], axis=0, return_index=True)
    worst_j = worst_t = 0.0
    for i in done[first]:
        r = np.nonzero(rows[i])[0]
        Jt, cond = st.dense_jacobian(pack, r, d["S"].rho_soft)
        ej, et = st.scaled_errors(J[i], Jt, cond, st.dense_terms(pack, r, d["S"].rho_soft))
        worst_j, worst_t = max(worst_j, ej or 0.0), max(worst_t, et)
    print(f"{case.name}: {len(first)} sets, scaled error {worst_j:.3g} (||J||), {worst_t:.3g} (terms)")
    assert worst_j <= TRUTH_BOUND_J and worst_t <= TRUTH_BOUND_TERMS


# Central differences of the oracle's x (h = 1e-6) against the Jacobian, relative to max(1, max |J|) of the point, on
# the columns whose two neighbouring solves kept the active set and that marginal_report does not flag.  Measured:
# 1.49e-9 (mr1-n4-m40-nth7, 1309 columns), 5.25e-10 (mr2-n3-m65-nth2, 386 columns) -> bound 2^-26 = 1.49e-8.
FD_BOUND, FD_MEASURED = 2.0 ** -26, 1.49e-9


@pytest.mark.parametrize("name,min_cols", [("wave-mr1-n4-m40-nth7", 1000), ("wave-mr2-n3-m65-nth2", 300)])
def test_jacobian_against_central_differences_of_the_oracle(lmpc, name, min_cols):
    case = sc.BY_NAME[name]
    pack = sc.host_pack(case)
    L = sc.ldp_of(pack)
    th = sc.theta(case, 200)
    FD, keep, ef, act = st.central_differences(L, th)
    rep = oldp.marginal_report(L, th, max_list=10 ** 9)
    marginal = np.zeros(len(th), bool)
    marginal[rep["primal_marginal_first"]] = True
    marginal[rep["dual_marginal_first"]] = True
    keep &= ~marginal[:, None]
    J, s = lmpc.solver.sens_host(pack, act, ef)
    assert (s[ef >= 1] == 1).all()
    rel = (np.abs(FD - J).max(axis=1) / np.maximum(np.abs(J).max(axis=(1, 2)), 1.0)[:, None])[keep]
    print(f"{name}: {keep.sum()} columns, max relative difference {rel.max():.3g}")
    assert keep.sum() >= min_cols
    assert rel.max() <= FD_BOUND


# lmpc_explicit_region's F (the builder's KKT form) against the Jacobian of the region's mask, in the two measures above
# with F in the place of Jtrue.  Measured: pendulum (16 regions) 0.591 (||J||) and 0.321 (terms); soft_doc (84 regions)
# 73217 and 64955 -- there the difference is the BUILDER's: its KKT form carries an error of the order eps / rho_soft on
# regions with an active SOFT row whatever cond(K_A) is (the worst regions have ONE active row, cond(K_A) = 1, where this
# Jacobian is within 1.3e-16 of the dense solve and F within 6.5e-11).  Bounds: the next power of two at or above 8 x.
EXPLICIT_BOUNDS = {"pendulum": (8.0, 4.0), "soft_doc": (2.0 ** 20, 2.0 ** 19)}


@pytest.mark.parametrize("name,N", [("pendulum", 40000), ("soft_doc", 20000)])
def test_explicit_region_laws_equal_the_jacobian(lmpc, name, N):
    import bench
    g = load_golden(name)
    L = oldp.qp2ldp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=g["H"].shape[0])
    pack = sc.pack_of(L)
    th = bench.make_theta(name, N, 11, False)
    _, ef, _, act = oldp.solve_batch(L, th)
    ec = lmpc.explicit.ExplicitController.build_ldp(pack, th, act, ef)
    S = lmpc.default_settings()
    regions = ec.info()["regions"]
    assert regions >= 10
    masks = np.array([ec.region(r)["mask"] for r in range(regions)], np.uint64)
    J, s = lmpc.solver.sens_host(pack, masks, np.ones(regions, np.int32))
    Jr, sr_ = sr.sens(pack, masks, np.ones(regions, np.int32), None, S.rho_soft, S.zero_tol)
    assert np.array_equal(J, Jr) and np.array_equal(s, sr_) and (s == 1).all()
    rows = sr.rows_of(masks, L.m)
    worst_j = worst_t = 0.0
    for r in range(regions):
        a = np.nonzero(rows[r])[0]
        Jt, cond = st.dense_jacobian(pack, a, S.rho_soft)
        ej, et = st.scaled_errors(J[r], np.asarray(ec.region(r)["F"], np.longdouble), cond, st.dense_terms(pack, a, S.rho_soft))
        if float(np.abs(Jt).sum(axis=1).max()) <= st.CANCELLED * st.dense_terms(pack, a, S.rho_soft):
            ej = None
        worst_j, worst_t = max(worst_j, ej or 0.0), max(worst_t, et)
    print(f"{name}: {regions} regions, scaled difference {worst_j:.6g} (||J||), {worst_t:.6g} (terms)")
    assert worst_j <= EXPLICIT_BOUNDS[name][0] and worst_t <= EXPLICIT_BOUNDS[name][1]


def test_kernel_instantiations_in_the_library_equal_the_tables(lmpc):
    from test_fast_fallback import _kernel_vgprs
    assert os.path.exists(LIB), "build the library first"
    built = set(_kernel_vgprs(LIB, r"sens_(lane|wave)_kernel"))
    want = {f"_ZN4lmpc16sens_lane_kernelILi{cap}ELb{j}EEEvNS_8SensArgsE" for cap in sc.CAPS for j in (0, 1)} | \
           {f"_ZN4lmpc16sens_wave_kernelILb{j}EEEvNS_8SensArgsE" for j in (0, 1)}
    assert built == want, sorted(built ^ want)
    # ... and every one is reached by a case of the table: the dispatch's record for each (case, option, call)
    reached = set()
    for case in sc.CASES:
        pack = sc.host_pack(case)
        for option in (0,) + sc.CAPS:
            for jac in (0, 1):
                rec = sc.expected_record(pack, sc.N_COND, jac, option)
                reached.add(f"_ZN4lmpc16sens_lane_kernelILi{rec['CAP']}ELb{jac}EEEvNS_8SensArgsE")
                if rec["list_pass"]:
                    reached.add(f"_ZN4lmpc16sens_wave_kernelILb{jac}EEEvNS_8SensArgsE")
    assert reached == want
    assert {sc.lane_cap(sc.host_pack(c)) for c in sc.CASES} == set(sc.CAPS), "the automatic choice reaches both capacities"


def test_every_new_symbol_is_declared_and_exported(lmpc):
    new = ("lmpc_solve_vjp_device", "lmpc_solve_jacobian_device", "lmpc_solve_vjp", "lmpc_solve_jacobian",
           "lmpc_solve_vjp_host", "lmpc_solve_jacobian_host", "lmpc_sens_launch_info")
    header = open(os.path.join(os.path.dirname(LIB), "..", "..", "include", "lmpc_hip.h")).read()
    for name in new:
        assert name in lmpc.SYMBOLS and hasattr(lmpc.lib(), name) and f"int {name}(" in header, name
    assert lmpc.lib().lmpc_abi_version() == 2


def test_refusals_and_argument_errors(lmpc):
    case = sc.BY_NAME["own-n5-m25-nth1"]
    pack = sc.host_pack(case)
    act = np.zeros((3, case.words), np.uint64)
    ef = np.ones(3, np.int32)
    xb = np.ones((3, pack["nout"]))

    def code(**kw):
        p = dict(pack)
        args = dict(active=act, exitflag=ef, xbar=xb)
        for k, v in kw.items():
            (args if k in ("active", "exitflag", "xbar", "settings", "is_avi") else p)[k] = v
        with pytest.raises(lmpc.LmpcError) as e:
            lmpc.solver.sens_host(p, **args)
        return e.value.code

    binary = pack["sense"].copy()
    binary[0] |= 16
    assert code(sense=binary) == -103                                      # BINARY rows
    assert code(is_avi=True) == -103
    prox = lmpc.default_settings()
    prox.eps_prox = 1e-3
    assert code(settings=prox) == -103
    assert code(nth=0, Dth=np.zeros((pack["m"], 0)), Xth=np.zeros((pack["nout"], 0))) == -100      # no parameter
    assert code(nout=pack["n"] + 1, Rout=np.zeros((pack["n"] + 1, pack["n"])), x0=np.zeros(pack["n"] + 1),
                Xth=np.zeros((pack["n"] + 1, 1)), xbar=np.ones((3, pack["n"] + 1))) == -100
    L = lmpc.lib()
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    arrs = [np.ascontiguousarray(pack[k], dtype=np.float64) for k in ("M", "du", "dl", "Dth", "Rout", "x0", "Xth")]
    head = [int(pack[k]) for k in ("n", "m", "ms", "nth", "nout")] + [vp(a) for a in arrs] + [vp(pack["sense"]), None, 0]
    out, status = np.zeros((3, 1)), np.zeros(3, np.int32)
    assert L.lmpc_solve_vjp_host(*head, 3, vp(act), vp(ef), None, vp(out), vp(status)) == -100       # xbar NULL
    assert L.lmpc_solve_vjp_host(*head, 3, None, vp(ef), vp(xb), vp(out), vp(status)) == -100
    assert L.lmpc_solve_jacobian_host(*head, 3, vp(act), vp(ef), None, vp(status)) == -100           # J NULL
    assert L.lmpc_solve_vjp_host(*head, -1, vp(act), vp(ef), vp(xb), vp(out), vp(status)) == -100
    assert L.lmpc_solve_vjp_host(*head, 0, None, None, None, None, None) == 1                         # nothing to do
    # status may be NULL; a different rho_soft / zero_tol is used
    assert L.lmpc_solve_vjp_host(*head, 3, vp(act), vp(ef), vp(xb), vp(out), None) == 1
    S = lmpc.default_settings()
    S.rho_soft, S.zero_tol = 1e-3, 1e-9
    d = _data(lmpc, case)
    b = d["batch"]
    v, s = lmpc.solver.sens_host(pack, b["active"][:257], b["exitflag"][:257], b["xbar"][:257], settings=S)
    vr, sr_ = sr.sens(pack, b["active"][:257], b["exitflag"][:257], b["xbar"][:257], 1e-3, 1e-9, d["cache"])
    assert np.array_equal(v, vr) and np.array_equal(s, sr_) and not np.array_equal(v, d["vjp"][:257])
    assert lmpc.lib().lmpc_sens_launch_info(None, None, 0) == -100
