"""Host side of the nonlinear true plant (no GPU): the tracer against a plant function evaluated directly, the interpreter
on the CPU (lmpc_plant_program_eval_host) against the host restatement of tests/nonlinear_reference.py, the refusals of
lmpc_plant_program_check, the accuracy of the restated sine and cosine, the conditions that keep the closed-loop cases
of tests/test_gpu_nonlinear.py from passing emptily, and the reference's own warm-against-cold assertion
(test/runtests.jl:85-117) on the host reference loop."""
import ctypes
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lmpc():
    import linearmpc_jl_amd as mod
    return mod


def _trace(lmpc, f, Ts=None, **dims):
    return lmpc.NonlinearPlant(lambda x, u, d, q: f(x, u, d, q, lmpc), Ts=Ts, **dims)


def _inputs(dims, S, seed=0, scale=3.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-scale, scale, (S, dims["nx"])), rng.uniform(-2, 2, (S, dims["nu"])),
            rng.uniform(-1, 1, (S, dims["nd"])), rng.uniform(0.5, 1.5, (S, dims["nq"])))


# ------------------------------------------------------------------ 1. the tracer
def test_traced_cartpole_equals_the_function_evaluated_directly(lmpc):
    import nonlinear_reference as nr
    dims = {k: v for k, v in nr.CARTPOLE.items() if k != "Ts"}
    plant = _trace(lmpc, nr.cartpole, Ts=nr.CARTPOLE["Ts"], **dims)
    x, u, d, q = _inputs(dims, 500)
    x[:, 2] = np.linspace(-7.0, 7.0, 500)
    for qq in (q, nr.CARTPOLE_Q):
        want = nr.direct(nr.cartpole, x, u, d, qq, Ts=nr.CARTPOLE["Ts"])
        assert nr.same(nr.interpret(plant, x, u, d, qq), want)
    # structurally identical operations are one instruction: one SIN and one COS in the whole program
    ops = plant.ins[:, 0].tolist()
    assert ops.count(nr.OPS["SIN"]) == 1 and ops.count(nr.OPS["COS"]) == 1
    # the step itself: the last operations are Ts * f_a (MUL) and x_a + (ADD), never an FMA
    assert nr.OPS["FMA"] not in ops and np.any(plant.consts == 0.01)
    # and it is not the linearised plant
    assert not np.array_equal(want, x)


def test_traced_every_operation_program_equals_the_function_evaluated_directly(lmpc):
    import nonlinear_reference as nr
    plant = _trace(lmpc, nr.every_op, **nr.EVERY_OP)
    assert set(plant.ins[:, 0].tolist()) == set(nr.OPS.values())
    x, u, d, q = _inputs(nr.EVERY_OP, 300, seed=1)
    assert nr.same(nr.interpret(plant, x, u, d, q), nr.direct(nr.every_op, x, u, d, q))
    x, u, d, q = nr.special_values()
    assert nr.same(nr.interpret(plant, x, u, d, q), nr.direct(nr.every_op, x, u, d, q))


def test_traced_linear_plant_equals_the_row_sums(lmpc):
    import nonlinear_reference as nr
    import scenario_reference as sr
    rng = np.random.default_rng(3)
    nx, nu, nd = 5, 2, 2
    rows = rng.uniform(-1, 1, (nx, 1 + nx + nu + nd))
    plant = lmpc.NonlinearPlant(nr.linear_plant(rows, nx, nu, nd), nx, nu, nd)
    x, u, d, _ = _inputs(dict(nx=nx, nu=nu, nd=nd, nq=0), 200, seed=4)
    assert np.array_equal(nr.interpret(plant, x, u, d), sr.predict(rows, x, u, d))
    assert np.array_equal(plant.eval_host(x, u, d), sr.predict(rows, x, u, d))


def test_constants_fold_and_dead_code_is_dropped(lmpc):
    import nonlinear_reference as nr
    def f(x, u, d, q):
        unused = lmpc.sin(x[0]) * 3.0                        # never returned: no instruction
        k = lmpc.cos(0.5 + 0.25) * 2.0                        # constants only: folded with the restated cosine
        return [x[0] * k + (-0.0), 7.0]
    plant = lmpc.NonlinearPlant(f, 2, 0)
    ops = plant.ins[:, 0].tolist()
    assert nr.OPS["SIN"] not in ops and nr.OPS["COS"] not in ops
    want = float(nr.cos_(np.array([0.75]))[0]) * 2.0
    assert want in plant.consts.tolist() and 7.0 in plant.consts.tolist()
    assert any(c == 0.0 and math.copysign(1.0, c) < 0 for c in plant.consts.tolist())          # -0.0 kept apart from +0.0
    x = np.array([[1.5, 0.0], [-2.0, 1.0]])
    assert nr.same(plant.eval_host(x), np.stack([x[:, 0] * want + (-0.0), np.full(2, 7.0)], axis=1))


def test_slots_are_allocated_by_liveness(lmpc):
    # a chain of 200 operations over two inputs lives in a handful of slots
    def f(x, u, d, q):
        acc = x[0]
        for i in range(100):
            acc = acc * x[1] + float(i)
        return [acc, x[1]]
    plant = lmpc.NonlinearPlant(f, 2, 0)
    assert plant.ins.shape[0] >= 200 and plant.n_slots <= 4
    plant.check()


@pytest.mark.parametrize("name,f", [
    ("gt", lambda x, u, d, q: [x[0] if x[0] > 0 else x[1], x[1]]),
    ("bool", lambda x, u, d, q: [x[0] if x[0] else x[1], x[1]]),
    ("eq", lambda x, u, d, q: [x[0] if x[0] == 1.0 else x[1], x[1]]),
    ("numpy.sin", lambda x, u, d, q: [np.sin(x[0]), x[1]]),
    ("numpy.maximum", lambda x, u, d, q: [np.maximum(x[0], 0.0), x[1]]),
    ("float", lambda x, u, d, q: [math.sin(x[0]), x[1]]),
    ("pow", lambda x, u, d, q: [x[0] ** 0.5, x[1]]),
    ("pow", lambda x, u, d, q: [x[0] ** -1, x[1]]),
    ("pow", lambda x, u, d, q: [x[0] ** x[1], x[1]]),
    ("rpow", lambda x, u, d, q: [2.0 ** x[0], x[1]]),
    ("mod", lambda x, u, d, q: [x[0] % 2.0, x[1]]),
    ("f:", lambda x, u, d, q: [x[0]]),
    ("ADD", lambda x, u, d, q: [x[0] + "1", x[1]]),
])
def test_the_tracer_refuses_by_name(lmpc, name, f):
    with pytest.raises(lmpc.TraceError, match="^" + name.replace(".", r"\.")):
        lmpc.NonlinearPlant(f, 2, 0)


@pytest.mark.parametrize("name", ["sqrt", "exp", "tanh", "where"])
def test_unsupported_functions_are_refused_by_name(lmpc, name):
    from linearmpc_jl_amd import nonlinear
    with pytest.raises(lmpc.TraceError, match="^" + name):
        lmpc.NonlinearPlant(lambda x, u, d, q: [getattr(nonlinear, name)(x[0])], 1, 0)


def test_a_program_beyond_a_cap_is_refused_by_the_tracer(lmpc):
    def wide(x, u, d, q):                                   # 70 values live at once
        vals = [x[0] * float(i + 2) for i in range(70)]
        acc = vals[0]
        for v in vals[:0:-1]:
            acc = acc + v
        return [acc] + [vals[-1]]
    with pytest.raises(lmpc.TraceError, match="^n_slots"):
        lmpc.NonlinearPlant(wide, 2, 0)

    def long(x, u, d, q):
        acc = x[0]
        for i in range(600):
            acc = lmpc.sin(acc) + x[1]
        return [acc, x[1]]
    with pytest.raises(lmpc.TraceError, match="^n_ins"):
        lmpc.NonlinearPlant(long, 2, 0)


# ------------------------------------------------------------------ 2. the interpreter on the CPU
def _plant_of(lmpc, p):
    return lmpc.NonlinearPlant.from_arrays(p.nx, p.nu, p.nd, p.nq, p.n_slots, p.consts, p.ins, p.out_slot)


def test_eval_host_every_operation_over_special_values(lmpc):
    import nonlinear_reference as nr
    plant = _trace(lmpc, nr.every_op, **nr.EVERY_OP)
    x, u, d, q = nr.special_values()
    want = nr.interpret(plant, x, u, d, q)
    got = plant.eval_host(x, u, d, q)
    assert nr.same(got, want), np.argwhere(~(np.isnan(got) & np.isnan(want)) & (got.view(np.uint64) != want.view(np.uint64)))[:10]
    # what the header states about the selects and the signs
    bits = lambda v: np.asarray(v, np.float64).view(np.uint64)
    i = lambda a, b: int(np.flatnonzero((bits(x[:, 0]) == bits(a)) & (bits(x[:, 1]) == bits(b)))[0])      # the row with x0 = a, x1 = b
    assert np.signbit(got[i(-0.0, 0.0), 7]) == False and np.signbit(got[i(0.0, -0.0), 7]) == True       # MIN ties: the second operand
    assert got[i(np.nan, 1.0), 7] == 1.0 and np.isnan(got[i(1.0, np.nan), 7])
    assert got[i(np.nan, 1.0), 8] == 1.0 and np.isnan(got[i(1.0, np.nan), 8])
    assert np.isnan(got[i(np.inf, 1.0), 9]) and np.isnan(got[i(-np.inf, 1.0), 10]) and np.isnan(got[i(np.nan, 1.0), 9])
    assert got[i(-0.0, 1.0), 9] == 0.0 and not np.signbit(got[i(-0.0, 1.0), 9]) and got[i(0.0, 1.0), 10] == 1.0
    assert got[i(5e-324, 1.0), 9] == 5e-324 and got[i(-5e-324, 1.0), 5] == 5e-324 and got[i(5e-324, -1.0), 2] == -5e-324
    # beyond 2^20 the same operations run: defined, restated, no accuracy claimed
    assert np.isfinite(got[i(1e22, 1.0), 9])


@pytest.mark.parametrize("which", ["slots", "instructions"])
def test_eval_host_at_the_caps(lmpc, which):
    import nonlinear_reference as nr
    p = nr.slot_cap_program() if which == "slots" else nr.instruction_cap_program()
    assert (p.n_slots == nr.MAX_SLOTS) if which == "slots" else (p.ins.shape[0] == nr.MAX_INS)
    plant = _plant_of(lmpc, p)
    plant.check()
    x = np.random.default_rng(8).uniform(-2, 2, (65, p.nx))
    want = nr.interpret(p, x)
    assert np.array_equal(plant.eval_host(x), want) and np.isfinite(want).all() and np.abs(want).min() > 0


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_eval_host_cartpole_q_shared_and_per_scenario(lmpc, N):
    import nonlinear_reference as nr
    dims = {k: v for k, v in nr.CARTPOLE.items() if k != "Ts"}
    plant = _trace(lmpc, nr.cartpole, Ts=nr.CARTPOLE["Ts"], **dims)
    x, u, d, q = _inputs(dims, N, seed=N)
    per = plant.eval_host(x, u, d, q)
    assert np.array_equal(per, nr.interpret(plant, x, u, d, q))
    shared = plant.eval_host(x, u, d, q[0])
    assert np.array_equal(shared, nr.interpret(plant, x, u, d, q[0]))
    assert np.array_equal(shared[0], per[0]) and (N == 1 or not np.array_equal(shared[1:], per[1:]))


# ------------------------------------------------------------------ 3. the check
def _raw(lmpc, p, **over):
    """the struct of a program with some fields overwritten; returns (struct, keep-alive)"""
    from linearmpc_jl_amd._cabi import PlantProgram
    consts = np.ascontiguousarray(over.pop("consts", p.consts), dtype=np.float64)
    ins = np.ascontiguousarray(over.pop("ins", p.ins), dtype=np.int32)
    out = np.ascontiguousarray(over.pop("out_slot", p.out_slot), dtype=np.int32)
    f = dict(nx=p.nx, nu=p.nu, nd=p.nd, nq=p.nq, n_slots=p.n_slots, n_consts=consts.size, n_ins=ins.size // 5)
    null = over.pop("null", ())
    f.update(over)
    ptr = lambda a, name: None if name in null else a.ctypes.data
    s = PlantProgram(f["nx"], f["nu"], f["nd"], f["nq"], f["n_slots"], f["n_consts"], f["n_ins"], ptr(consts, "consts"),
                     ptr(ins, "ins"), ptr(out, "out_slot"))
    return s, (consts, ins, out)


def _edit(ins, row, col, val):
    ins = np.array(ins, np.int32)
    ins[row, col] = val
    return ins


def _refusals():
    import nonlinear_reference as nr
    O = nr.OPS
    # base program, nx = nu = nd = nq = 1, 3 slots, 1 constant:
    #   0 LOADX s0 <- x0; 1 LOADU s1 <- u0; 2 LOADD s2 <- d0; 3 ADD s0 <- s0 + s1; 4 LOADQ s1 <- q0; 5 CONST s2' ...; 6 FMA s0 <- fma(s0, s1, s2)
    base = nr.program(1, 1, 1, 1, 3, [2.5], [[O["LOADX"], 0, 0, 0, 0], [O["LOADU"], 1, 0, 0, 0], [O["LOADD"], 2, 0, 0, 0],
                                             [O["ADD"], 0, 0, 1, 0], [O["LOADQ"], 1, 0, 0, 0], [O["CONST"], 2, 0, 0, 0],
                                             [O["FMA"], 0, 0, 1, 2]], [0])
    E = lambda r, c, v: dict(ins=_edit(base.ins, r, c, v))
    big = np.tile(np.array([[O["LOADX"], 0, 0, 0, 0]], np.int32), (nr.MAX_INS + 1, 1))
    return base, [
        ("unknown opcode 0", r"ins\[3\]\.op", E(3, 0, 0)),
        ("unknown opcode 17", r"ins\[3\]\.op", E(3, 0, 17)),
        ("negative opcode", r"ins\[0\]\.op", E(0, 0, -1)),
        ("dst beyond the slot file", r"ins\[3\]\.dst", E(3, 1, 3)),
        ("dst negative", r"ins\[0\]\.dst", E(0, 1, -1)),
        ("slot operand beyond the slot file", r"ins\[3\]\.b", E(3, 3, 3)),
        ("slot operand negative", r"ins\[6\]\.c", E(6, 4, -2)),
        ("slot operand far out of range", r"ins\[3\]\.a", E(3, 2, 2 ** 30)),
        ("x index out of range", r"ins\[0\]\.a", E(0, 2, 1)),
        ("u index out of range", r"ins\[1\]\.a", E(1, 2, 1)),
        ("d index out of range", r"ins\[2\]\.a", E(2, 2, 5)),
        ("q index out of range", r"ins\[4\]\.a", E(4, 2, -1)),
        ("constant index out of range", r"ins\[5\]\.a", E(5, 2, 1)),
        ("slot read before it is written", r"ins\[0\]\.a", dict(ins=np.array([[O["NEG"], 0, 1, 0, 0]] + base.ins.tolist(), np.int32))),
        ("non-zero unused field", r"ins\[0\]\.b", E(0, 3, 1)),
        ("out_slot never written", r"out_slot\[0\]", dict(n_slots=4, out_slot=[3])),
        ("out_slot out of range", r"out_slot\[0\]", dict(out_slot=[3])),
        ("out_slot negative", r"out_slot\[0\]", dict(out_slot=[-1])),
        ("too many instructions", "n_ins", dict(ins=big)),
        ("too many slots", "n_slots", dict(n_slots=nr.MAX_SLOTS + 1)),
        ("no slots", "n_slots", dict(n_slots=0)),
        ("too many constants", "n_consts", dict(consts=np.zeros(nr.MAX_CONSTS + 1))),
        ("negative instruction count", "n_ins", dict(n_ins=-1)),
        ("nx beyond 32", "nx", dict(nx=33)),
        ("nx zero", "nx", dict(nx=0)),
        ("nq beyond 32", "nq", dict(nq=33)),
        ("nd negative", "nd", dict(nd=-1)),
        ("nu beyond 64", "nu", dict(nu=65)),
        ("NULL instructions", "ins", dict(null=("ins",))),
        ("NULL constants", "consts", dict(null=("consts",))),
        ("NULL out_slot", "out_slot", dict(null=("out_slot",))),
    ]


def test_the_base_program_of_the_refusals_passes(lmpc):
    import nonlinear_reference as nr
    base, _ = _refusals()
    s, keep = _raw(lmpc, base)
    assert lmpc.lib().lmpc_plant_program_check(ctypes.byref(s)) == 1
    x, u, d, q = np.array([[1.5]]), np.array([[0.25]]), np.array([[3.0]]), np.array([[2.0]])
    assert np.array_equal(_plant_of(lmpc, base).eval_host(x, u, d, q), nr.interpret(base, x, u, d, q))
    assert nr.interpret(base, x, u, d, q)[0, 0] == 1.75 * 2.0 + 2.5


@pytest.mark.parametrize("what,field,over", [pytest.param(*r, id=r[0]) for r in _refusals()[1]])
def test_program_check_refuses_and_names_the_field(lmpc, what, field, over):
    import re
    from linearmpc_jl_amd._cabi import last_error
    base, _ = _refusals()
    s, keep = _raw(lmpc, base, **dict(over))
    L = lmpc.lib()
    assert L.lmpc_plant_program_check(ctypes.byref(s)) == -100
    assert re.match(r"lmpc_plant_program_check: " + field + ":", last_error(None)), last_error(None)
    # nothing reaches an interpreter: the CPU entry point refuses the same program and writes nothing
    x, out = np.ones((3, 1)), np.full((3, 33), -7.0)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert L.lmpc_plant_program_eval_host(ctypes.byref(s), 3, vp(x), vp(x), vp(x), vp(x), 0, vp(out)) == -100
    assert re.match(r"lmpc_plant_program_eval_host: " + field + ":", last_error(None)), last_error(None)
    assert (out == -7.0).all()


def test_program_check_refuses_a_null_program(lmpc):
    from linearmpc_jl_amd._cabi import last_error
    assert lmpc.lib().lmpc_plant_program_check(None) == -100 and last_error(None).startswith("lmpc_plant_program_check: prog:")


# ------------------------------------------------------------------ 4. sine and cosine
def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_sine_and_cosine_are_within_two_ulp_of_numpy(lmpc):
    """Bound: 2 ulp -- each side's documented error is below 1 ulp.  Measured maxima (against numpy): 1.0 ulp for the sine
    and for the cosine on both point sets."""
    import nonlinear_reference as nr
    O = nr.OPS
    p = nr.program(1, 0, 0, 0, 2, [], [[O["LOADX"], 0, 0, 0, 0], [O["SIN"], 1, 0, 0, 0], [O["COS"], 0, 0, 0, 0]], [1])
    p2 = nr.program(1, 0, 0, 0, 2, [], p.ins, [0])
    rng = np.random.default_rng(2024)
    wide = rng.uniform(-100.0, 100.0, 10 ** 6)
    kmax = int(2.0 ** 20 / (0.5 * np.pi))
    near = rng.integers(-kmax, kmax + 1, 10 ** 4) * (0.5 * np.pi) + rng.uniform(-1e-6, 1e-6, 10 ** 4)
    assert np.abs(near).max() <= 2.0 ** 20 + 1.0
    worst = {}
    for name, pts in (("wide", wide), ("near", near)):
        s = _plant_of(lmpc, p).eval_host(pts[:, None])[:, 0]
        c = _plant_of(lmpc, p2).eval_host(pts[:, None])[:, 0]
        # the library's values are the restated ones (every fifth point: the restatement costs a Python call per fma;
        # 2 * 10^5 points are what it takes to see a coefficient's last bit, which moves about one result in 10^4)
        sub = slice(None, None, 5 if name == "wide" else 1)
        rs, rc = nr.sin_cos_(pts[sub])
        assert np.array_equal(s[sub], rs) and np.array_equal(c[sub], rc)
        worst[name] = (float(_ulps(s, np.sin(pts)).max()), float(_ulps(c, np.cos(pts)).max()))
    print("max ulp difference against numpy (sin, cos):", worst)
    assert max(max(v) for v in worst.values()) <= 2.0, worst
    assert set(np.unique(nr.quadrant(near)).astype(int)) == {0, 1, 2, 3}


# ------------------------------------------------------------------ 5. the closed-loop cases cannot pass emptily
@pytest.fixture(scope="module")
def cartpole_plant(lmpc):
    import nonlinear_reference as nr
    dims = {k: v for k, v in nr.CARTPOLE.items() if k != "Ts"}
    return _trace(lmpc, nr.cartpole, Ts=nr.CARTPOLE["Ts"], **dims)


@pytest.fixture(scope="module")
def host_ldp():
    import nonlinear_reference as nr
    import scenario_reference as sr
    return sr.host_ldp(nr.controller())


def _cases():
    import nonlinear_reference as nr
    return [pytest.param(c, id=c.name) for c in nr.CLOSED_LOOP + [nr.SPLIT]]


@pytest.mark.parametrize("case", _cases())
def test_closed_loop_cases_meet_their_conditions(cartpole_plant, host_ldp, case):
    import nonlinear_reference as nr
    data = nr.case_data(case)
    ref = nr.run_case(case, host_ldp, cartpole_plant, data)
    lin = nr.linearised_run(case, host_ldp, data)
    nr.check_conditions(case, ref, lin, data)


def test_the_checker_rejects_batches_that_miss_a_condition(cartpole_plant, host_ldp):
    import nonlinear_reference as nr
    case = nr.Case("narrow", S=40, T=6)
    data = nr.case_data(case)
    # (a) pole angles near the origin only: the reduction stays in quadrant 0
    small = nr.case_data(case)
    small.x0 = small.x0 * np.array([1.0, 1.0, 0.01, 1.0])
    ref = nr.run_case(case, host_ldp, cartpole_plant, small)
    with pytest.raises(AssertionError, match="quadrants"):
        nr.check_conditions(case, ref, nr.linearised_run(case, host_ldp, small), small)
    # (b) every first move saturated
    full = nr.case_data(nr.CLOSED_LOOP[0])
    whole = nr.run_case(nr.CLOSED_LOOP[0], host_ldp, cartpole_plant, full)
    keep = np.flatnonzero(nr.saturated(whole.us[0, :, 0]))
    far = nr.case_data(nr.CLOSED_LOOP[0])
    far.x0 = far.x0[keep]
    sub = nr.Case("saturated-only", S=keep.size)
    ref = nr.run_case(sub, host_ldp, cartpole_plant, far)
    with pytest.raises(AssertionError, match="saturated first moves"):
        nr.check_conditions(sub, ref, nr.linearised_run(sub, host_ldp, far), far)
    # (c) a loop that steps F, G: the "nonlinear" run IS the linearised one
    lin =nr.linearised_run(nr.CLOSED_LOOP[0], host_ldp, full)
    with pytest.raises(AssertionError, match="linearised"):
        nr.check_conditions(nr.CLOSED_LOOP[0], lin, lin, full)
    # (d) noise asked for and absent
    noisy = nr.Case("noisy", process=True)
    quiet = nr.run_case(nr.CLOSED_LOOP[0], host_ldp, cartpole_plant, full)
    with pytest.raises(AssertionError):
        nr.check_conditions(noisy, quiet, lin, full)
    # (e) an exit flag below 1
    bad = nr.run_case(nr.CLOSED_LOOP[0], host_ldp, cartpole_plant, full)
    bad.flags = bad.flags.copy()
    bad.flags[3, 5] = -1
    with pytest.raises(AssertionError):
        nr.check_conditions(nr.CLOSED_LOOP[0], bad, lin, full)


# ------------------------------------------------------------------ 6. the reference's own assertion
def test_hundred_steps_cold_against_warm_on_the_host_reference(cartpole_plant, host_ldp):
    """test/runtests.jl:85-117: the cart-pole from x = [5, 5, 0, 0], 100 closed-loop steps on the nonlinear dynamics, cold
    and warm started: |u_cold - u_warm| < 1e-9 at every step (the reference's tolerance)."""
    import nonlinear_reference as nr
    import scenario_reference as sr
    prob = nr.controller(Np=50, Nc=5)                      # the example's own horizons (mpc_examples: Np = 50, Nc = 5)
    ldp = sr.host_ldp(prob)
    dims, previews = sr.dims_of(prob)
    kw = dict(dims=dims, plant=sr.plant_of(prob), prog=cartpole_plant, x0=nr.HUNDRED["x0"][:1], T=nr.HUNDRED["T"], q=nr.CARTPOLE_Q,
              previews=previews)
    cold = nr.nonlinear_run(ldp, warm=False, **kw)
    warm = nr.nonlinear_run(ldp, warm=True, **kw)
    assert cold.flags.min() >= 1 and warm.flags.min() >= 1
    diff = float(np.abs(cold.us - warm.us).max())
    print("max |u_cold - u_warm| over 100 steps:", diff)
    assert diff < 1e-9, diff
    assert nr.saturated(cold.us[:, 0, 0]).any() and not nr.saturated(cold.us[:, 0, 0]).all()
