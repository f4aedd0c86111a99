"""TEST INFRASTRUCTURE: the backward sweep of the scenario loop (include/lmpc_hip.h, "Scenario loop adjoint") restated
in numpy, one IEEE-754 operation at a time: every sum one chain of `loop_reference.fma` in index order, every other
operation one addition; step 2 is `sens_reference.sens`.  Nothing here calls the library.

A run is described by its tape -- active (T, S, words) and flags (T, S) -- the pack of the controller's LDP (a dict as
`BatchedQP.ldp()` returns it), the TRUE plant's rows, the observer's arrays and, per block of theta, the triple
(w, Tc, H): values per column, columns the forward was given (at most the steps of the run), preview length.
"""
from types import SimpleNamespace

import numpy as np

import sens_reference as sens_ref
from loop_reference import fma


def plant_rows(plant, nx, nu, nd):
    """(dyn, meas) of a scenario_reference plant: rows [f, F, G, Gd] and [h, C, Dd]."""
    ny = plant.C.shape[0]
    dyn = np.hstack([plant.f_offset[:, None], plant.F, plant.G, plant.Gd.reshape(nx, nd)])
    meas = np.hstack([plant.h_offset[:, None], plant.C, plant.Dd.reshape(ny, nd)])
    return dyn, meas


def _col(Tc, c):
    """the trajectory column that column c of a block is read from: the last one held"""
    return min(max(c, 0), Tc - 1)


def _chain(acc, Mt, v):
    """acc[:, c] = fma(Mt[a, c], v[:, a], acc[:, c]) over a ascending: a chain per (scenario, c)."""
    for a in range(Mt.shape[0]):
        acc = fma(Mt[a][None, :], v[:, a][:, None], acc)
    return acc


def adjoint(pack, dims, dyn, meas, active, flags, Xbar=None, Ubar=None, blocks=None, observer=None, xhat_given=False,
            rho_soft=1e-6, zero_tol=1e-11, cache=None):
    """dims = (nx, nu, nd, ny, nuprev); dyn (nx, 1+nx+nu+nd), meas (ny, 1+nx+nd): the true plant; observer: (dyn^, meas^,
    Kt) flat or shaped, or None; blocks: dict r / d / p -> (w, Tc, H) or None.  Xbar (T+1, S, nx), Ubar (T, S, nu) or
    None = zeros.  Returns a namespace: x0bar, xhat0bar (None unless an observer ran from a given xhat), uprev0bar, rbar /
    dbar / pbar (Tc, S, w) step-major or None, status_min, and per step ubars, thbars, statuses."""
    nx, nu, nd, ny, nup = dims
    T, S = np.asarray(flags).shape
    blocks = dict(blocks or {})
    obs = observer is not None
    F, G, Gd = dyn[:, 1:1 + nx], dyn[:, 1 + nx:1 + nx + nu], dyn[:, 1 + nx + nu:]
    if obs:
        C, Dd = meas[:, 1:1 + nx], meas[:, 1 + nx:]
        od = np.asarray(observer[0], float).reshape(nx, 1 + nx + nu + nd)
        om = np.asarray(observer[1], float).reshape(ny, 1 + nx + nd)
        kt = np.asarray(observer[2], float).reshape(ny, nx)
        Fh, Gh, Gdh = od[:, 1:1 + nx], od[:, 1 + nx:1 + nx + nu], od[:, 1 + nx + nu:]
        Ch, Ddh = om[:, 1:1 + nx], om[:, 1 + nx:]
    cache = cache if cache is not None else sens_ref.derived(pack)
    bar, spec = {}, {}
    for name in ("r", "d", "p"):
        b = blocks.get(name)
        spec[name] = None if (b is None or b[0] == 0) else tuple(int(v) for v in b)
        bar[name] = None if spec[name] is None else np.zeros((max(spec[name][1], 1), S, spec[name][0]))
    zx = np.zeros((S, nx))
    alpha = zx.copy() if Xbar is None else np.array(Xbar[T], float)
    beta, gamma = zx.copy(), np.zeros((S, nup))
    status_min = np.ones(S, np.int32)
    out = SimpleNamespace(ubars=[None] * T, thbars=[None] * T, statuses=[None] * T)
    for k in range(T - 1, -1, -1):
        # 1. ubar
        ub = np.zeros((S, nu)) if Ubar is None else np.array(Ubar[k], float)
        ub = _chain(ub, G, alpha)
        if obs:
            ub = _chain(ub, Gh, beta)
        ub[:, :nup] = ub[:, :nup] + gamma
        # 2. the solve's VJP on the tape slice
        thb, st = sens_ref.sens(pack, active[k], flags[k], ub, rho_soft, zero_tol, cache)
        status_min = st.astype(np.int32) if k == T - 1 else np.minimum(status_min, st).astype(np.int32)
        out.ubars[k], out.thbars[k], out.statuses[k] = ub, thb, st
        # 3. xi, eta
        xi = thb[:, :nx].copy()
        if obs:
            xi = _chain(xi, Fh, beta)
            eta = _chain(np.zeros((S, ny)), kt.T, xi)
        # 5. the direct use of d_k (with the carried alpha, beta)
        if bar["d"] is not None:
            dl = _chain(np.zeros((S, nd)), Gd, alpha)
            if obs:
                dl = _chain(dl, Gdh, beta)
                dl = _chain(dl, Dd, eta)
                dl = _chain(dl, -Ddh, eta)
            c = _col(spec["d"][1], k)
            bar["d"][c] = bar["d"][c] + dl
        # 4. alpha', beta'
        an = zx.copy() if Xbar is None else np.array(Xbar[k], float)
        an = _chain(an, F, alpha)
        if not obs:
            an = an + xi
        else:
            an = _chain(an, C, eta)
            beta = _chain(xi.copy(), -Ch, eta)
        alpha = an
        # 6. the blocks of theta-bar, in theta's order
        e = nx
        for name in ("r", "d"):
            if spec[name] is not None:
                w, Tc, H = spec[name]
                k0 = k + 1 if (name == "r" and H > 0) else k
                for q in range(w * max(H, 1)):
                    c = _col(Tc, k0 + q // w)
                    bar[name][c][:, q % w] = bar[name][c][:, q % w] + thb[:, e + q]
                e += w * max(H, 1)
        gamma = thb[:, e:e + nup].copy()
        e += nup
        if spec["p"] is not None:
            w, Tc, H = spec["p"]
            for q in range(w * max(H, 1)):
                c = _col(Tc, k + q // w)
                bar["p"][c][:, q % w] = bar["p"][c][:, q % w] + thb[:, e + q]
    own = obs and xhat_given
    out.x0bar = alpha + beta if (obs and not own) else alpha
    out.xhat0bar = beta if own else None
    out.uprev0bar = gamma
    out.rbar, out.dbar, out.pbar = bar["r"], bar["d"], bar["p"]
    out.status_min = status_min
    return out


# ------------------------------------------------------------------ what the CPU and the GPU tests share
def case_blocks(case, data, dims, previews):
    """name -> (w, Tc, H) of a scenario_reference case: the columns the forward is given are those of the run at most."""
    nx, nu, wr, nd, nup, wp = dims
    out = {}
    for name, w, a, H in (("r", wr, data.r, previews[0]), ("d", nd, data.d, previews[1]), ("p", wp, data.p, previews[2])):
        out[name] = None if (w == 0 or a is None) else (w, min(a.shape[-1], case.T), H)
    return out


def cotangents(case, nx, nu, seed=0):
    """(Xbar (T+1, S, nx), Ubar (T, S, nu)) of a case, deterministic in its name's seed."""
    rng = np.random.default_rng(9000 + case.seed + seed)
    return rng.standard_normal((case.T + 1, case.S, nx)), rng.standard_normal((case.T, case.S, nu))


def check_conditions(blocks, adj, active_sizes, T, need_clamp=False, need_big=False, lane_cap=8):
    """What keeps a case from passing emptily, from the reference's sweep alone: every gradient column is non-zero for
    some scenario; with need_clamp a block shorter than the run exists (its last column collects the held steps); with
    need_big a working set beyond the lane kernel's capacity is on the tape."""
    for name in ("x0bar", "uprev0bar", "rbar", "dbar", "pbar"):
        g = getattr(adj, name)
        if g is None or g.size == 0:
            continue
        flat = g.reshape(-1, g.shape[-1]) if name.endswith("0bar") else g
        nz = (flat != 0).any(axis=-2)
        if name == "rbar" and blocks["r"][2] > 0:
            nz = nz[1:]                                   # a previewed reference is read from column 1 on
        assert nz.all(), ("zero gradient column", name)
    if need_clamp:
        short = [n for n, b in blocks.items() if b is not None and b[1] < T]
        assert short, "no clamped column: every block is as long as the run"
    if need_big:
        assert int(np.max(active_sizes)) > lane_cap, ("no set beyond the lane capacity", int(np.max(active_sizes)))
    assert (adj.status_min == 1).any()
