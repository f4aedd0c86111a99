"""Host side of tests/loop_reference.py (no GPU): the GPU tests of tests/test_gpu_loops.py demand bit equality with the
restated loops, so the restatement is pinned first -- its fused multiply-add against exact rational arithmetic, the
closed loop against the C oracle's whole-loop function (a second, independent statement of the same specification), the
observer steps against the scalar C loops, the parameter formation against a plain per-problem loop -- and every case
the GPU tests run is shown not to pass emptily."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import loop_reference as lr


def _round32(q):
    """A Fraction rounded to binary32, ties to even, without passing through binary64."""
    if q == 0:
        return np.float32(0.0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fr(2) ** e > a:
        e -= 1
    e = max(e, -126)                                     # subnormals share the smallest exponent
    ulp = Fr(2) ** (e - 23)
    n, rem = divmod(a, ulp)
    n = int(n)
    if rem * 2 > ulp or (rem * 2 == ulp and n % 2):
        n += 1
    return np.float32(sign * float(n * ulp))             # n * ulp is a binary32 value: float() and float32() are exact


def test_round32_is_the_rounding_of_numpy():
    rng = np.random.default_rng(0)
    for v in np.concatenate([rng.standard_normal(200), rng.standard_normal(50) * 1e-40, [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24]]):
        assert _round32(Fr(float(v))) == np.float32(v), v


def _operands(dtype):
    rng = np.random.default_rng(1)
    t = np.dtype(dtype).type
    a, b, c = (rng.standard_normal(150).astype(dtype) * t(10.0) ** rng.integers(-3, 4, 150).astype(dtype) for _ in range(3))
    # cancellation: c = -round(a * b), so that a * b + c is the rounding error of the product, lost without fusing
    a2, b2 = rng.standard_normal(100).astype(dtype), rng.standard_normal(100).astype(dtype)
    c2 = -(a2 * b2)
    # a tie of the separate operations: (1 + e)(1 - e) + e^2 with e the unit roundoff
    e = t(np.finfo(dtype).eps)
    a3, b3, c3 = np.array([1 + e, 1 + e], dtype), np.array([1 - e, 1 + e], dtype), np.array([e * e, -(1 + 2 * e)], dtype)
    return np.concatenate([a, a2, a3]), np.concatenate([b, b2, b3]), np.concatenate([c, c2, c3])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fma_is_exact(dtype):
    a, b, c = _operands(dtype)
    got = lr.fma(a, b, c, dtype)
    assert got.dtype == np.dtype(dtype)
    unfused = 0
    for i in range(len(a)):
        exact = Fr(float(a[i])) * Fr(float(b[i])) + Fr(float(c[i]))
        want = _round32(exact) if dtype == np.float32 else float(exact)          # float(Fraction) rounds correctly
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)
        unfused += (a[i] * b[i] + c[i]) != got[i]
    assert unfused >= 50                                  # the sample tells a fused from an unfused multiply-add


def test_plant_step_order_and_fusing():
    rng = np.random.default_rng(2)
    F, G = rng.standard_normal((5, 5)), rng.standard_normal((5, 2))
    x, u = rng.standard_normal((40, 5)), rng.standard_normal((40, 2))
    got = lr.plant_step(F, G, x, u)
    for s in range(40):
        for a in range(5):
            acc = 0.0
            for c in range(5):
                acc = float(Fr(F[a, c]) * Fr(x[s, c]) + Fr(acc))
            for l in range(2):
                acc = float(Fr(G[a, l]) * Fr(u[s, l]) + Fr(acc))
            assert got[s, a] == acc
    # the sample tells the documented order from G's terms first, and from separate multiply and add
    swapped = lr.plant_step(np.hstack([G, F])[:, :0], np.hstack([G, F]), x[:, :0], np.hstack([u, x]))
    assert not np.array_equal(swapped, got)
    assert not np.array_equal(x @ F.T + u @ G.T, got)


_SIM = lr.SIM_CASES + lr.SIM_F32
_BY_NAME = {c.name: c for c in _SIM + lr.REF_CASES}


@pytest.mark.parametrize("name", [c.name for c in _SIM])
def test_simulate_reference_equals_the_c_oracle_loop(name):
    # oracle.ldp.simulate (oracle_simulate) against the restated loop: every output, bit for bit, and the conditions
    from oracle import ldp as oldp
    case = _BY_NAME[name]
    dtype = np.float32 if case in lr.SIM_F32 else np.float64
    data = lr.loop_data(case)
    L = lr.loop_ldp(data)
    ref = lr.run_loop_case(case, L, data, dtype=dtype)
    old = oldp.simulate(L, data.x0, case.T, data.F, data.G, r=data.r, uprev=data.uprev, warm=case.warm, dtype=dtype)
    for key in ("U", "X", "x", "uprev", "flag_min"):
        assert ref[key].dtype == old[key].dtype and np.array_equal(ref[key], old[key]), (name, key)
    lr.check_loop_conditions(case, ref)
    assert L.nth == case.nx + data.nr + data.nup and np.isfinite(ref["X"]).all()


@pytest.mark.parametrize("name", [c.name for c in lr.REF_CASES])
def test_simulate_ref_cases_do_not_pass_emptily(name):
    case = _BY_NAME[name]
    data = lr.loop_data(case)
    L = lr.loop_ldp(data)
    ref = lr.run_loop_case(case, L, data, entry="ref")
    lr.check_loop_conditions(case, ref)
    H = case.Np if case.preview else 0
    assert L.nth == case.nx + case.ny * max(H, 1) + data.nup
    # theta's r-block, read back: column k, or columns k+1 .. k+H, held at the trajectory's own last column
    rt = data.rtraj if data.rtraj.ndim == 3 else np.broadcast_to(data.rtraj, (case.S,) + data.rtraj.shape)
    for k in (0, case.T // 2, case.T - 1):
        for i in range(max(H, 1)):
            col = min(k + 1 + i if H else k, rt.shape[-1] - 1)
            assert np.array_equal(ref["thetas"][k][:, case.nx + i * case.ny:case.nx + (i + 1) * case.ny], rt[:, :, col])
        if k and data.nup:
            assert np.array_equal(ref["thetas"][k][:, -data.nup:], ref["U"][k - 1][:, :data.nup])
    if case.r_cols and case.r_cols < case.T:
        assert not np.array_equal(rt[..., -1], rt[..., -2])                      # a clamp one column early would show


def test_simulate_ref_with_a_constant_trajectory_is_simulate():
    case = _BY_NAME["sim-lane-nx5-warm"]
    data = lr.loop_data(case)
    L = lr.loop_ldp(data)
    a = lr.simulate_reference(L, data.x0, case.T, data.F, data.G, r=data.r, warm=True)
    b = lr.simulate_ref_reference(L, data.x0, case.T, data.F, data.G, data.r[:, :, None], warm=True)
    for key in ("U", "X", "x", "uprev", "flag_min"):
        assert np.array_equal(a[key], b[key]), key


def test_case_lists_cover_what_they_must():
    sweep = set(lr.NX_SWEEP)
    assert sweep == {1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 32}
    for group in (lr.SIM_LANE, lr.SIM_WAVE):
        assert {(c.nx, c.warm) for c in group} == {(nx, w) for nx in sweep for w in (False, True)}
    assert {(c.nx, c.preview, c.warm) for c in lr.REF_SWEEP} == {(nx, p, w) for nx in sweep for p in (False, True) for w in (False, True)}
    assert {c.rr for c in lr.REF_SWEEP if c.preview} == {True, False} == {c.rr for c in lr.REF_SWEEP if not c.preview}
    assert {(c.nx, c.warm) for c in lr.SIM_F32} == {(nx, w) for nx in (2, 4, 8, 9, 17) for w in (False, True)}
    assert {(c.S, c.T) for c in lr.SIM_SIZES if c.nx == 3} == {(S, T) for S in (1, 255, 256, 257, 1000) for T in (1, 2)}
    assert {c.nx for c in lr.SIM_SIZES} == {3, 12}
    nth = {c.name: c.nx + c.nr + c.nup for c in lr.GATES}
    assert (nth["gate-nx8-nth16"], nth["gate-nx9-nth16"], nth["gate-nx8-nth17"]) == (16, 16, 17)
    assert {c.nu for c in lr.GATES} >= {lr.K_MAX_SIM_U, lr.K_MAX_SIM_U + 1}
    assert [c.nu for c in lr.WAVE_GATES] == [lr.K_MAX_SIM_U, lr.K_MAX_SIM_U + 1] and all(c.mg >= 40 for c in lr.WAVE_GATES)
    # a random initial uprev reaches every entry point, cold handles of every path included
    for group in (lr.SIM_LANE, lr.SIM_WAVE, lr.SIM_F32, lr.GATES, lr.WAVE_GATES, lr.LAYOUT, lr.REF_SWEEP, lr.REF_SHAPES):
        assert any(lr.loop_data(c).uprev is not None and lr.loop_data(c).uprev.any() for c in group if c.nx <= 9), group[0].name
    assert {(c.nup, c.nu) for c in lr.LAYOUT if c.nr} == {(0, 3), (1, 3), (3, 3)} and any(c.nr == 0 for c in lr.LAYOUT)
    assert any(c.r_cols and c.r_cols < c.T and not c.preview for c in lr.REF_SHAPES)
    assert any(c.r_cols and c.r_cols < c.T and c.preview for c in lr.REF_SHAPES)
    assert any(c.r_shared and c.preview for c in lr.REF_SHAPES) and any(c.r_shared and not c.preview for c in lr.REF_SHAPES)


def test_reference_imports_nothing_of_the_library():
    import ast
    src = open(lr.__file__).read()
    names = []
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            names += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            names.append(node.module or "")
    allowed = ("ctypes", "dataclasses", "types", "numpy", "oracle", "scenario_reference")
    assert names and all(n.split(".")[0] in allowed for n in names), names
    assert "import_module" not in src and "__import__" not in src


# ------------------------------------------------------------------ observer and the parameter kernels
@pytest.mark.parametrize("nx", lr.NX_SWEEP)
@pytest.mark.parametrize("nd", [0, 2])
def test_observer_steps_equal_the_scalar_c_loops(nx, nd):
    from oracle import observer as oobs
    for ny in (1, 3, nx + 2):
        dyn, meas, kt, x, u, y, d = lr.observer_data(nx, 2, nd, ny, 6)
        xp = lr.predict(dyn, x, u, d)
        xc = lr.correct(meas, kt, xp, y, d)
        for s in range(6):
            assert np.array_equal(oobs.c_predict(dyn.reshape(-1), x[s], u[s], d[s], nx, 2, nd), xp[s])
            assert np.array_equal(oobs.c_correct(meas.reshape(-1), kt.reshape(-1), xp[s], y[s], d[s], nx, ny, nd), xc[s])
        assert not np.array_equal(xc, xp) and not np.array_equal(xp, x)


@pytest.mark.parametrize("nph,nr", [(0, 2), (4, 1), (5, 3)])
def test_update_parameter_reference_equals_a_plain_loop(nph, nr):
    rng = np.random.default_rng(5)
    N, nu, nx, nd, nup, npar = 7, 3, 4, 2, 2, 2
    wr = nr * max(nph, 1)
    arrays = dict(control=rng.standard_normal((N, nu)), state=rng.standard_normal((N, nx)), reference=rng.standard_normal((N, wr)),
                  disturbance=rng.standard_normal((N, nd)), parameter=rng.standard_normal((N, npar)))
    t2s = rng.standard_normal((nr, nr * nph)) if nph else None
    flat = None if t2s is None else np.asarray(t2s, order="F").reshape(-1, order="F")      # as the layout stores it
    for absent in (None, "control", "reference", "disturbance", "parameter"):
        kw = {k: (None if k == absent else v) for k, v in arrays.items()}
        got = lr.update_parameter_reference(N, nu, nx, nr, nd, nup, npar, nph=nph, t2s=t2s, **kw)
        assert got.shape == (N, nx + nr + nd + nup + npar)
        for i in range(N):
            th = list(kw["state"][i])
            for e in range(nr):
                if kw["reference"] is None:
                    th.append(0.0)
                elif nph:
                    v = 0.0
                    for q in range(nr * nph):
                        v += kw["reference"][i, q] * flat[q * nr + e]
                    th.append(v)
                else:
                    th.append(kw["reference"][i, e])
            th += [0.0] * nd if kw["disturbance"] is None else list(kw["disturbance"][i])
            th += [0.0] * nup if kw["control"] is None else list(kw["control"][i, :nup])
            th += [0.0] * npar if kw["parameter"] is None else list(kw["parameter"][i])
            assert np.array_equal(got[i], th), (absent, i)
    if nph and nr > 1:                                     # the sample tells t2s[q * nr + e] from t2s[e * nr * nph + q]
        wrong = lr.update_parameter_reference(N, nu, nx, nr, nd, nup, npar, nph=nph, t2s=flat.reshape(nr, nr * nph), **arrays)
        assert not np.array_equal(wrong, lr.update_parameter_reference(N, nu, nx, nr, nd, nup, npar, nph=nph, t2s=t2s, **arrays))


def test_split_observer_reference():
    rng = np.random.default_rng(6)
    nx, nd, N = 3, 3, 5
    for ndm in (0, 1, nd):
        ndo = nd - ndm
        obs, meas = rng.standard_normal((N, nx + ndo)), rng.standard_normal((N, ndm))
        for m in (meas, None):
            st, di = lr.split_observer_reference(obs, m, nx, ndm, ndo)
            assert st.shape == (N, nx) and di.shape == (N, nd)
            for i in range(N):
                assert list(st[i]) == list(obs[i, :nx])
                assert list(di[i]) == ([0.0] * ndm if m is None else list(m[i])) + list(obs[i, nx:])
