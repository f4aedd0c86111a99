"""Scenario loop adjoint on the GPU: the taped forward run (lmpc_simulate_scenario_taped*), the backward sweep
(lmpc_scenario_vjp*: scenario_adjoint_kernel<NX> between the VJPs of the differentiable solve) and the torch layer.
Everything is held bit for bit to the numpy restatement of the contract (scenario_adjoint_reference.py) on the GPU's own
tape, which is itself held to the host reference loop (scenario_reference.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 3                    # sentinel records in front of and behind every output
SENT, SENT_I = -7.25e300, -2025


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


@pytest.fixture(scope="module")
def torch():
    import torch as mod
    return mod


def _sweep_cases():
    import scenario_reference as sr
    # nx = 1 .. 8 unrolled, 9 / 17 / 32 the generic form
    return list(sr.SWEEP)


def _size_cases():
    import scenario_reference as sr
    return [c for c in sr.SIZES if c.S in (1, 255, 256, 257)]


def _params(pick):
    import scenario_reference as sr
    return [pytest.param(c, id=c.name) for c in pick(sr)]


_CACHE = {}


def _setup(lmpc, torch, case):
    """Handle, inputs on the device and everything the reference sweep needs, once per case."""
    if case.name in _CACHE:
        return _CACHE[case.name]
    import scenario_adjoint_reference as sar
    import scenario_reference as sr
    from test_gpu_scenario import _mpc
    data = sr.case_data(case)
    mpc = _mpc(lmpc, data.prob)
    model = mpc.control_model()
    dims, previews = sr.dims_of(data.prob)
    nx, nu, wr, nd, nup, wp = dims
    plant = sr.plant_of(data.prob)
    ny = plant.C.shape[0]
    dyn, meas = sar.plant_rows(plant, nx, nu, nd)
    obs = None if data.kf is None else data.kf.codegen_arrays()
    if obs is not None:
        model.set_observer(*obs, nx, nu, nd, ny)
    dev = torch.device("cuda", model.device)
    T, S = case.T, case.S
    ten = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[..., :T])).to(dev)
    uprev0 = np.tile(np.asarray(mpc.uprev, float)[:nup], (S, 1))
    kw = dict(nd=nd, ny=ny, r=ten(data.r) if wr else None, d=ten(data.d), p=ten(data.p), noise=ten(data.noise),
              r_preview=previews[0], d_preview=previews[1], p_preview=previews[2], r_width=wr, d_width=nd, p_width=wp,
              use_observer=obs is not None, warm=case.warm)
    pack = model.ldp()
    d = dict(case=case, data=data, mpc=mpc, model=model, dims=dims, dims5=(nx, nu, nd, ny, nup), previews=previews, dyn=dyn,
             meas=meas, obs=obs, dev=dev, kw=kw, uprev0=uprev0, pack=pack, cache=sar.sens_ref.derived(pack),
             blocks=sar.case_blocks(case, data, dims, previews), cot=sar.cotangents(case, nx, nu))
    _CACHE[case.name] = d
    return d


def _forward(torch, d, tape, want=("U", "X", "Y", "Ym", "Xhat"), xhat=None):
    x = torch.from_numpy(d["data"].x0.copy()).to(d["dev"])
    up = torch.from_numpy(d["uprev0"].copy()).to(d["dev"]) if d["dims"][4] else None
    out = d["model"].simulate_scenario(x, d["case"].T, d["dyn"], d["meas"], uprev=up, want=want, tape=tape, xhat=xhat, **d["kw"])
    torch.cuda.synchronize()
    d["model"].check()
    return out


def _reference(d, active, flags, Xb, Ub, xhat_given=False):
    import scenario_adjoint_reference as sar
    S = d["mpc"].settings
    return sar.adjoint(d["pack"], d["dims5"], d["dyn"], d["meas"], active, flags, Xb, Ub, d["blocks"], d["obs"], xhat_given,
                       S.rho_soft, S.zero_tol, d["cache"])


def _vjp_guarded(lmpc, torch, d, tape, Xb, Ub):
    """lmpc_scenario_vjp_device on outputs with sentinel guard records around each: a dict of numpy arrays in the
    reference's layout, after checking that no guard was written and no record left unwritten."""
    from linearmpc_jl_amd._cabi import ScenarioGrad, ScenarioTape, check
    model, dev, desc = d["model"], d["dev"], tape["desc"]
    N, T, nx, nu, nup = (tape[k] for k in ("N", "T", "nx", "nu", "nup"))
    f64 = torch.float64
    bufs, views = {}, {}

    def guarded(name, rows, w, dtype=f64, sent=SENT):
        if rows * w == 0:
            return None
        t = torch.full(((rows + 2 * GUARD) * w,), sent, dtype=dtype, device=dev)
        bufs[name], views[name] = (t, rows, w), t[GUARD * w:(GUARD + rows) * w]
        return views[name].data_ptr()

    ptrs = dict(x0bar=guarded("x0bar", N, nx), xhat0bar=guarded("xhat0bar", N, nx) if tape["xhat_given"] else None,
                uprev0bar=guarded("uprev0bar", N, nup), status_min=guarded("status_min", N, 1, torch.int32, SENT_I))
    shape = {}
    for name in ("r", "d", "p"):
        b = getattr(desc, name)
        shape[name] = (max(int(b.T), 1), N, int(b.w))
        ptrs[name + "bar"] = guarded(name + "bar", shape[name][0] * N, int(b.w)) if b.w > 0 else None
    tx = None if Xb is None else torch.from_numpy(Xb).to(dev)
    tu = None if Ub is None else torch.from_numpy(Ub).to(dev)
    g = ScenarioGrad(None if tx is None else tx.data_ptr(), None if tu is None else tu.data_ptr(), ptrs["x0bar"], ptrs["xhat0bar"],
                     ptrs["uprev0bar"], ptrs["rbar"], ptrs["dbar"], ptrs["pbar"], ptrs["status_min"])
    ct = ScenarioTape(tape["active"].data_ptr(), tape["flag"].data_ptr())
    st = torch.cuda.current_stream(dev).cuda_stream
    check(lmpc.lib().lmpc_scenario_vjp_device(model._h, N, T, ctypes.byref(desc), ctypes.byref(ct), ctypes.byref(g),
                                              ctypes.c_void_p(st)), model._h)
    torch.cuda.synchronize()
    model.check()
    out = dict(xhat0bar=None, rbar=None, dbar=None, pbar=None)
    for name, (t, rows, w) in bufs.items():
        a = t.cpu().numpy()
        sent = SENT_I if name == "status_min" else SENT
        assert (a[:GUARD * w] == sent).all() and (a[(GUARD + rows) * w:] == sent).all(), (name, "a guard record was written")
        body = a[GUARD * w:(GUARD + rows) * w]
        assert not (body == sent).any(), (name, "an output record was not written")
        out[name] = body.reshape(shape[name[0]]) if name[1:] == "bar" else (body if name == "status_min" else body.reshape(rows, w))
    if nup == 0:
        out["uprev0bar"] = np.zeros((N, 0))
    return out


def _assert_equal(adj, got):
    for k in ("x0bar", "xhat0bar", "uprev0bar", "rbar", "dbar", "pbar", "status_min"):
        a, b = getattr(adj, k), got[k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))


def _vjp_record(torch, d, tape):
    """The launch record of ONE lmpc_solve_vjp_device call on the first slice of the tape: what a step of the sweep enqueues
    (the sweep's own VJPs leave the handle's ring of derivative calls alone)."""
    model = d["model"]
    seen = model.sens_launch_info()
    xb = torch.zeros((tape["N"], model.nout), dtype=torch.float64, device=d["dev"])
    model.solve_vjp_device(tape["active"][0], tape["flag"][0], xb)
    torch.cuda.synchronize()
    rec = model.sens_launch_info(since=seen[-1]["seq"] if seen else 0)
    assert len(rec) == 1
    return rec[0]


def _tape_arrays(tape):
    return tape["active"].cpu().numpy().view(np.uint64), tape["flag"].cpu().numpy()


def _run_case(lmpc, torch, case, options=()):
    d = _setup(lmpc, torch, case)
    model = d["model"]
    for name, value in options:
        model.set_option(name, value)
    out = _forward(torch, d, True)
    act, flg = _tape_arrays(out["tape"])
    seen, calls = model.scenario_adjoint_launch_info(), model.sens_launch_info()
    got = _vjp_guarded(lmpc, torch, d, out["tape"], *d["cot"])
    assert model.sens_launch_info() == calls                     # the record of the caller's own derivative calls stays
    adj = _reference(d, act, flg, *d["cot"])
    _assert_equal(adj, got)
    rec = model.scenario_adjoint_launch_info(since=seen[-1]["seq"] if seen else 0)
    assert len(rec) == 1
    return d, out, adj, rec[0]


# ------------------------------------------------------------------ first the launch record
def test_launch_record(lmpc, torch):
    import scenario_adjoint_reference as sar
    import scenario_reference as sr
    for case, nxt in ((sr.SWEEP[4 * 3 + 2], 4), (_sweep_cases()[4 * 9], 0), (sr.PREVIEWS[1], 6)):
        d, out, adj, rec = _run_case(lmpc, torch, case)
        nth = d["model"].nth
        tile = min(nth, 32)
        assert rec["NX"] == nxt and rec["grid"] == (case.S + 255) // 256 and rec["T"] == case.T and rec["nprob"] == case.S
        assert rec["tile"] == tile and rec["lds"] == 256 * (tile | 1) * 8 and 2 * rec["lds"] <= 160 * 1024
        sens = _vjp_record(torch, d, out["tape"])
        assert rec["list_pass"] == sens["list_pass"]
        if case is sr.PREVIEWS[1]:
            assert nth == 64 and rec["list_pass"] == 1           # the wide record in two slices; sets of 10 rows are listed
            sar.check_conditions(d["blocks"], adj, sr.popcount(_tape_arrays(out["tape"])[0]), case.T, need_clamp=True, need_big=True)


# ------------------------------------------------------------------ the taped forward
@pytest.mark.parametrize("case", _params(lambda sr: sr.SWEEP[12:16] + sr.PREVIEWS + [sr.COST]))
def test_taped_forward_equals_the_plain_one_and_the_reference_tape(lmpc, torch, case):
    import scenario_reference as sr
    from conftest import oracle_ldp_from
    from test_gpu_scenario import _oracle_settings
    d = _setup(lmpc, torch, case)
    plain, taped = _forward(torch, d, False), _forward(torch, d, True)
    for k in ("U", "X", "Y", "Ym", "Xhat", "x", "uprev", "flag_min"):
        assert torch.equal(plain[k], taped[k]), k
    assert "tape" not in plain
    ref = sr.run_case(case, oracle_ldp_from(d["pack"]), d["data"], settings=_oracle_settings(d["mpc"]))
    act, flg = _tape_arrays(taped["tape"])
    assert np.array_equal(act, ref.active) and np.array_equal(flg, ref.flags)
    assert np.array_equal(taped["U"].cpu().numpy(), ref.us) and np.array_equal(taped["X"].cpu().numpy(), ref.xs)


# ------------------------------------------------------------------ the sweep, bit for bit
@pytest.mark.parametrize("case", _params(lambda sr: _sweep_cases()))
def test_every_state_size_equals_the_reference(lmpc, torch, case):
    d, out, adj, rec = _run_case(lmpc, torch, case)
    assert rec["NX"] == (case.nx if case.nx <= 8 else 0)
    assert (adj.status_min == 1).all()


@pytest.mark.parametrize("case", _params(lambda sr: _size_cases()))
def test_batch_sizes_around_the_workgroup(lmpc, torch, case):
    _run_case(lmpc, torch, case)


@pytest.mark.parametrize("case", _params(lambda sr: sr.PREVIEWS + [sr.COST]))
def test_previews_clamps_and_soft_rows(lmpc, torch, case):
    import scenario_adjoint_reference as sar
    import scenario_reference as sr
    d, out, adj, rec = _run_case(lmpc, torch, case)
    sar.check_conditions(d["blocks"], adj, sr.popcount(_tape_arrays(out["tape"])[0]), case.T,
                         need_clamp=any(l is not None for l in case.lengths), need_big=case.soft)


@pytest.mark.parametrize("options", [(("sens_cap", 5),), (("sens_cap", 8),), (("sens_force_list", 1),)], ids=str)
def test_vjp_options_give_the_same_bits(lmpc, torch, options):
    import scenario_reference as sr
    try:
        d, out, adj, rec = _run_case(lmpc, torch, sr.COST, options)
        cap = dict(options).get("sens_cap")
        info = _vjp_record(torch, d, out["tape"])
        assert rec["list_pass"] == 1                             # sets of 10 rows: beyond either capacity
        assert (cap is None or info["CAP"] == cap) and (("sens_force_list", 1) not in options or info["cap"] == 0)
    finally:
        model = _setup(lmpc, torch, sr.COST)["model"]
        model.set_option("sens_cap", 0)
        model.set_option("sens_force_list", 0)


@pytest.mark.parametrize("case", _params(lambda sr: [sr.SWEEP[4 * 3 + 3], sr.PREVIEWS[1]]))
def test_tapes_with_failed_flags(lmpc, torch, case):
    d = _setup(lmpc, torch, case)
    out = _forward(torch, d, True)
    tape = out["tape"]
    rng = np.random.default_rng(6)
    hit = rng.random((case.T, case.S)) < 0.1
    hit[:, 0] = False
    hit[-1, 1], hit[0, 2] = True, True
    tape["flag"][torch.from_numpy(hit).to(d["dev"])] = -1
    act, flg = _tape_arrays(tape)
    assert (flg[hit] == -1).all()
    got = _vjp_guarded(lmpc, torch, d, tape, *d["cot"])
    adj = _reference(d, act, flg, *d["cot"])
    _assert_equal(adj, got)
    assert np.array_equal(got["status_min"] == 0, hit.any(axis=0)) and set(np.unique(got["status_min"])) == {0, 1}


def test_absent_cotangents_and_a_given_xhat(lmpc, torch):
    import scenario_reference as sr
    case = sr.SWEEP[4 * 3 + 2]
    d = _setup(lmpc, torch, case)
    Xb, Ub = d["cot"]
    xhat = torch.from_numpy(d["data"].x0.copy()).to(d["dev"])    # the observer starts where it would without one ...
    out = _forward(torch, d, True, xhat=xhat)
    act, flg = _tape_arrays(out["tape"])
    assert out["tape"]["xhat_given"]
    got = _vjp_guarded(lmpc, torch, d, out["tape"], Xb, Ub)      # ... but its gradient is its own
    adj = _reference(d, act, flg, Xb, Ub, xhat_given=True)
    _assert_equal(adj, got)
    assert (got["xhat0bar"] != 0).any()
    plain = _forward(torch, d, True)
    act, flg = _tape_arrays(plain["tape"])
    for xb, ub in ((None, Ub), (Xb, None)):
        _assert_equal(_reference(d, act, flg, xb, ub), _vjp_guarded(lmpc, torch, d, plain["tape"], xb, ub))


# ------------------------------------------------------------------ host-pointer twins, the handle's scratch
def test_host_pointer_twins(lmpc, torch):
    import scenario_reference as sr
    from linearmpc_jl_amd._cabi import Block, ScenarioGrad, ScenarioTape, check
    case = sr.PREVIEWS[0]                                        # per-scenario r, shared d, per-scenario p, no observer
    d = _setup(lmpc, torch, case)
    model, data, T, S = d["model"], d["data"], case.T, case.S
    nx, nu, wr, nd, nup, wp = d["dims"]
    dev_out = _forward(torch, d, True)
    vp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    keep = []

    def block(a, H):
        a = np.ascontiguousarray(np.swapaxes(a[..., :T], -1, -2))          # column after column
        keep.append(a)
        w, Tc = a.shape[-1], a.shape[-2]
        return Block(a.ctypes.data, w * Tc if a.ndim == 3 else 0, w, Tc, 0, H)

    desc, hk = model.scenario_descriptor(d["dyn"], nx, nd, d["meas"], d["dims5"][3], r=block(data.r, d["previews"][0]),
                                         d=block(data.d, d["previews"][1]), p=block(data.p, d["previews"][2]),
                                         noise=block(data.noise, 0), nuprev=nup, warm=case.warm)
    x, up = data.x0.copy(), d["uprev0"].copy()
    U, X, fm = np.empty((T, S, nu)), np.empty((T + 1, S, nx)), np.empty(S, np.int32)
    act, flg = np.zeros((T, S, model.words), np.uint64), np.zeros((T, S), np.int32)
    tape = ScenarioTape(act.ctypes.data, flg.ctypes.data)
    check(lmpc.lib().lmpc_simulate_scenario_taped(model._h, S, T, ctypes.byref(desc), vp(x), None, vp(up), vp(U), vp(X), vp(fm),
                                                  ctypes.byref(tape)), model._h)
    dact, dflg = _tape_arrays(dev_out["tape"])
    assert np.array_equal(act, dact) and np.array_equal(flg, dflg)
    assert np.array_equal(U, dev_out["U"].cpu().numpy()) and np.array_equal(X, dev_out["X"].cpu().numpy())
    assert np.array_equal(x, dev_out["x"].cpu().numpy()) and np.array_equal(fm, dev_out["flag_min"].cpu().numpy())
    Xb, Ub = d["cot"]
    adj = _reference(d, act, flg, Xb, Ub)
    got = dict(x0bar=np.full((S, nx), SENT), uprev0bar=np.full((S, nup), SENT), status_min=np.full(S, SENT_I, np.int32),
               xhat0bar=None, **{k + "bar": np.full(getattr(adj, k + "bar").shape, SENT) for k in ("r", "d", "p")})
    g = ScenarioGrad(Xb.ctypes.data, Ub.ctypes.data, got["x0bar"].ctypes.data, None, got["uprev0bar"].ctypes.data,
                     got["rbar"].ctypes.data, got["dbar"].ctypes.data, got["pbar"].ctypes.data, got["status_min"].ctypes.data)
    check(lmpc.lib().lmpc_scenario_vjp(model._h, S, T, ctypes.byref(desc), ctypes.byref(tape), ctypes.byref(g)), model._h)
    _assert_equal(adj, got)


def test_one_handle_through_a_sequence_and_its_scratch(lmpc, torch):
    import scenario_adjoint_reference as sar
    import scenario_reference as sr
    big, small = sr.SIZES[4], sr.SIZES[3]                        # size-nx5-S1000-T1, then S257: one problem, two batch sizes
    assert (big.nx, big.S, small.S) == (5, 1000, 257)
    d = _setup(lmpc, torch, big)
    model = d["model"]
    ds = dict(d, case=small, data=sr.case_data(small), cot=sar.cotangents(small, 5, d["dims"][1]))
    ds["uprev0"] = d["uprev0"][:small.S]
    ten = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[..., :small.T])).to(d["dev"])
    ds["kw"] = dict(d["kw"], r=ten(ds["data"].r), d=ten(ds["data"].d), p=ten(ds["data"].p), noise=ten(ds["data"].noise))
    ds["blocks"] = sar.case_blocks(small, ds["data"], d["dims"], d["previews"])

    def vjp(dd):
        out = _forward(torch, dd, True)
        got = _vjp_guarded(lmpc, torch, dd, out["tape"], *dd["cot"])
        _assert_equal(_reference(dd, *_tape_arrays(out["tape"]), *dd["cot"]), got)
        return out

    theta = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (300, model.nth))).to(d["dev"])
    vjp(d)                                                       # (what a handle allocates once and keeps is in place)
    model.solve_device(theta)
    torch.cuda.synchronize()
    model.release_scratch()
    base = lmpc.lib().lmpc_debug_live_blocks()
    first = vjp(d)
    x0, ef0 = model.solve_device(theta)                          # a plain solve between two sweeps ...
    plain = _forward(torch, d, False)                            # ... and a plain scenario run
    assert torch.equal(plain["U"], first["U"]) and torch.equal(plain["X"], first["X"])
    vjp(ds)                                                      # another N on the same handle
    grown = lmpc.lib().lmpc_debug_live_blocks()
    again = vjp(d)
    assert torch.equal(again["U"], first["U"])
    assert lmpc.lib().lmpc_debug_live_blocks() == grown > base   # nothing more is allocated from the second call on
    x1, ef1 = model.solve_device(theta)
    torch.cuda.synchronize()
    assert torch.equal(x0, x1) and torch.equal(ef0, ef1)
    del first, plain, again
    model.release_scratch()
    assert lmpc.lib().lmpc_debug_live_blocks() == base
    vjp(ds)                                                      # and everything comes back


def test_descriptors_of_different_width_share_the_scratch(lmpc, torch):
    # The doubles per scenario of the sweep's scratch follow the descriptor (2 nx + nuprev + nu + nth): on ONE handle a wide
    # descriptor, then a narrow one at a larger N, then the wide one again at that N -- each sweep against the reference,
    # and from then on nothing more is allocated.  theta = 11 entries read as [x(4); r(3); d(2); uprev(2)] or as
    # [x(7); d(2); uprev(2)] (a plant of seven states: any split of theta is a valid descriptor, the solves are box-bounded).
    import scenario_reference as sr
    d = _setup(lmpc, torch, sr.SWEEP[4 * 3])                     # nx4, no observer, cold
    model, dev = d["model"], d["dev"]
    nu, nd, T = 2, 2, 3
    assert model.nth == 11 and d["dims"] == (4, 2, 3, 2, 2, 0)
    rng = np.random.default_rng(31)
    ten = lambda a: torch.from_numpy(a).to(dev)

    def sweep(nx, N):
        with_r = nx == 4
        dyn = np.ascontiguousarray(0.3 * rng.standard_normal((nx, 1 + nx + nu + nd)))
        r = ten(rng.uniform(-0.5, 0.5, (N, 3, T))) if with_r else None
        out = model.simulate_scenario(ten(rng.uniform(-1, 1, (N, nx))), T, dyn, None, nd=nd, ny=0, r=r,
                                      d=ten(rng.uniform(-0.3, 0.3, (N, nd, T))), r_width=3 if with_r else 0, d_width=nd,
                                      uprev=torch.zeros((N, 2), dtype=torch.float64, device=dev), tape=True)
        torch.cuda.synchronize()
        model.check()
        dd = dict(d, dims5=(nx, nu, nd, 0, 2), dyn=dyn, meas=None, obs=None,
                  blocks=dict(r=(3, T, 0) if with_r else None, d=(nd, T, 0), p=None))
        Xb, Ub = rng.standard_normal((T + 1, N, nx)), rng.standard_normal((T, N, nu))
        got = _vjp_guarded(lmpc, torch, dd, out["tape"], Xb, Ub)
        _assert_equal(_reference(dd, *_tape_arrays(out["tape"]), Xb, Ub), got)
        assert (got["status_min"] == 1).any() and (got["x0bar"] != 0).any()

    model.release_scratch()
    sweep(7, 300)                                                # 29 doubles per scenario
    sweep(4, 400)                                                # 23 per scenario, more scenarios: the group grows
    sweep(7, 400)                                                # 29 again at the larger N: it has to grow once more
    blocks = lmpc.lib().lmpc_debug_live_blocks()
    for nx, N in ((4, 400), (7, 300), (7, 400), (4, 257)):
        sweep(nx, N)
    assert lmpc.lib().lmpc_debug_live_blocks() == blocks


def test_an_observer_that_is_not_the_plant(lmpc, torch):
    # The filters of the other cases are built from the true plant, so C-hat = C, Dd-hat = Dd, F-hat = F ...: here every
    # array of the observer differs from the plant's, and the sweep must read each where the contract says.
    import scenario_reference as sr
    case = sr.SWEEP[4 * 3 + 2]                                   # nx4, observer, cold
    d = _setup(lmpc, torch, case)
    model = d["model"]
    nx, nu, nd, ny, _ = d["dims5"]
    rng = np.random.default_rng(41)
    other = tuple(np.asarray(a, float) * (1.0 + 0.2 * rng.standard_normal(np.shape(a))) for a in d["obs"])
    model.set_observer(*other, nx, nu, nd, ny)
    try:
        d2 = dict(d, obs=other)
        out = _forward(torch, d2, True)
        act, flg = _tape_arrays(out["tape"])
        got = _vjp_guarded(lmpc, torch, d2, out["tape"], *d["cot"])
        adj = _reference(d2, act, flg, *d["cot"])
        _assert_equal(adj, got)
        assert np.isfinite(adj.x0bar).all() and not np.array_equal(adj.x0bar, _reference(d, act, flg, *d["cot"]).x0bar)
    finally:
        model.set_observer(*d["obs"], nx, nu, nd, ny)


# ------------------------------------------------------------------ torch
@pytest.mark.parametrize("case", _params(lambda sr: [sr.SWEEP[4 * 3 + 3], sr.PREVIEWS[0]]))
def test_autograd_equals_the_device_call_bit_for_bit(lmpc, torch, case):
    d = _setup(lmpc, torch, case)
    model, dev = d["model"], d["dev"]
    Xb, Ub = (torch.from_numpy(a).to(dev) for a in d["cot"])
    out = _forward(torch, d, True)
    g = model.scenario_vjp(out["tape"], Xbar=Xb, Ubar=Ub)
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    x = leaf(torch.from_numpy(d["data"].x0.copy()).to(dev))
    up = leaf(torch.from_numpy(d["uprev0"].copy()).to(dev))
    kw = dict(d["kw"])
    r, dd, p = leaf(kw.pop("r")), leaf(kw.pop("d")), leaf(kw.pop("p"))
    X, U, fm = model.simulate_scenario_autograd(x, case.T, d["dyn"], r=r, d=dd, p=p, uprev=up, measurement=d["meas"], **kw)
    assert X.requires_grad and U.requires_grad and not fm.requires_grad
    assert torch.equal(X, out["X"]) and torch.equal(U, out["U"]) and torch.equal(fm, out["flag_min"])
    pairs = [(x, g["x0bar"]), (up, g["uprev0bar"])] + [(t, g[k + "bar"]) for k, t in (("r", r), ("d", dd), ("p", p)) if t is not None]
    grads = torch.autograd.grad([X, U], [t for t, _ in pairs], [Xb, Ub])
    torch.cuda.synchronize()
    for (t, w), got in zip(pairs, grads):
        w = w if w.dim() == t.dim() else w.sum(0)                # a shared block: summed over scenarios
        assert got.shape == t.shape and torch.equal(got, w.reshape(t.shape))
    assert any(t.dim() == 2 for t in (r, dd, p) if t is not None) or case.name.startswith("nx")
    assert torch.equal(X.grad_fn.status_min, g["status_min"]) and (g["status_min"] == 1).all()
    # no input requires grad: the plain call, no tape
    blocks = lmpc.lib().lmpc_debug_live_blocks()
    X2, U2, _ = model.simulate_scenario_autograd(x.detach(), case.T, d["dyn"], r=d["kw"]["r"], d=d["kw"]["d"], p=d["kw"]["p"],
                                                 uprev=up.detach(), measurement=d["meas"], **kw)
    assert not X2.requires_grad and X2.grad_fn is None and torch.equal(X2, out["X"]) and torch.equal(U2, out["U"])
    assert lmpc.lib().lmpc_debug_live_blocks() == blocks


def test_simulation_keeps_the_tape_and_differentiates_the_run(lmpc, torch):
    import scenario_reference as sr
    from test_gpu_scenario import _plant
    case = sr.PREVIEWS[0]                                        # r per scenario and shorter than the run, d shared
    d = _setup(lmpc, torch, case)
    data, T = d["data"], case.T
    traj = {k: getattr(data, k) for k in ("r", "d", "p", "noise")}
    run = lambda **kw: lmpc.Simulation(d["mpc"], lmpc.Scenario(data.x0, N=T, **traj), _plant(lmpc, data.prob), warm=case.warm, **kw)
    plain, sim = run(), run(tape=True)
    for k in ("xs", "us", "ys", "flag_min", "x_final"):
        assert np.array_equal(getattr(plain, k), getattr(sim, k)), k
    with pytest.raises(ValueError, match="tape=True"):
        plain.vjp()
    Xb, Ub = d["cot"]
    Xb = Xb.copy()
    Xb[T] = 0.0                                                  # xs holds the states before each step
    g = sim.vjp(np.ascontiguousarray(Xb[:T].transpose(1, 2, 0)), np.ascontiguousarray(Ub.transpose(1, 2, 0)))
    adj = _reference(d, *_tape_arrays(sim._tape), Xb, Ub)
    per = lambda bar, like: np.concatenate([bar.transpose(1, 2, 0), np.zeros(bar.shape[1:] + (like.shape[-1] - bar.shape[0],))], axis=2)
    assert np.array_equal(g["x0"], adj.x0bar) and np.array_equal(g["status_min"], adj.status_min)
    assert np.array_equal(g["uprev"], adj.uprev0bar.sum(axis=0))
    assert g["r"].shape == data.r.shape and np.array_equal(g["r"], per(adj.rbar, data.r))
    assert g["d"].shape == data.d.shape and np.array_equal(g["d"], per(adj.dbar, data.d).sum(axis=0))
    assert g["p"].shape == data.p.shape and np.array_equal(g["p"], per(adj.pbar, data.p))
    with pytest.raises(lmpc.LmpcError, match="no adjoint") as e:
        lmpc.Simulation(d["mpc"], lmpc.Scenario(data.x0, N=T, process_noise=lmpc.Uniform(-np.ones(4), np.ones(4)), **traj),
                        _plant(lmpc, data.prob), tape=True)
    assert e.value.code == -103
