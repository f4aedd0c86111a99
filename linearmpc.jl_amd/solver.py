"""`BatchedQP`: Python face of one `lmpc_handle` (include/lmpc_hip.h).

It stands where `mpc.opt_model` (a DAQPBase.Model) stands in the reference
(/root/reference/src/types.jl:141, setup.jl:11-13): set up once from the mpQP, then solved for
many parameter points.  All arithmetic happens in the HIP kernels behind the C ABI.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _cabi
from ._cabi import Block, LmpcError, Observer, ParamLayout, Settings, check, lib

_vp = ctypes.c_void_p


def _f64(a, order="C"):
    # aligned + requested order; no OWNDATA requirement (it would copy every reshaped view, 56 MB per
    # call for a 10^6-point theta)
    return np.require(np.asarray(a, dtype=np.float64), requirements=["A", order[0]])


def _ptr(a):
    return _vp(a.ctypes.data) if a is not None and a.size else None


def transform(H, f, f_theta, A, bu, bl, W, senses=None, nout=None, K=None, nx=0):
    """Host-only QP -> LDP transform (`lmpc_transform`; reference codegen.jl:239-280 `qp2ldp`).

    Returns a dict with row-major M, du, dl, Dth, Rout, x0, Xth (+ dims)."""
    H = _f64(H, "F")
    n = H.shape[0]
    f_theta = _f64(np.asarray(f_theta, float).reshape(n, -1), "F")
    nth = f_theta.shape[1]
    bu = _f64(np.asarray(bu, float).reshape(-1))
    bl = _f64(np.asarray(bl, float).reshape(-1))
    m = bu.size
    A = _f64(np.asarray(A, float).reshape(-1, n), "F")
    ms = m - A.shape[0]
    W = _f64(np.asarray(W, float).reshape(m, nth), "F")
    f = _f64(np.zeros(n) if f is None else np.asarray(f, float).reshape(n))
    nout = n if nout is None else int(nout)
    sense = np.ascontiguousarray(np.zeros(m, np.int32) if senses is None else senses, dtype=np.int32)
    Kf = None if K is None else _f64(np.asarray(K, float).reshape(nout, -1), "F")
    out = dict(M=np.empty((m, n)), du=np.empty(m), dl=np.empty(m), Dth=np.empty((m, nth)),
               Rout=np.empty((nout, n)), x0=np.empty(nout), Xth=np.empty((nout, nth)))
    rc = lib().lmpc_transform(n, m, ms, nth, nout, _ptr(H), _ptr(f), _ptr(f_theta), _ptr(A),
                              _ptr(bu), _ptr(bl), _ptr(W), _ptr(sense), _ptr(Kf) if Kf is not None else None,
                              int(nx if K is not None else 0),
                              *[_ptr(out[k]) for k in ("M", "du", "dl", "Dth", "Rout", "x0", "Xth")])
    check(rc)
    out.update(n=n, m=m, ms=ms, nth=nth, nout=nout, sense=sense)
    return out


def transform_avi(H, f, f_theta, A, bu, bl, W, senses=None, nout=None, K=None, nx=0):
    """Host-only transform of a NON-symmetric problem (`lmpc_transform_avi`; what an is_avi setup precomputes):
    dict with row-major ML, MR, G, du, dl, Dth, Rout, x0, Xth (+ dims)."""
    H = _f64(H, "F")
    n = H.shape[0]
    f_theta = _f64(np.asarray(f_theta, float).reshape(n, -1), "F")
    nth = f_theta.shape[1]
    bu = _f64(np.asarray(bu, float).reshape(-1))
    bl = _f64(np.asarray(bl, float).reshape(-1))
    m = bu.size
    A = _f64(np.asarray(A, float).reshape(-1, n), "F")
    ms = m - A.shape[0]
    W = _f64(np.asarray(W, float).reshape(m, nth), "F")
    f = _f64(np.zeros(n) if f is None else np.asarray(f, float).reshape(n))
    nout = n if nout is None else int(nout)
    sense = np.ascontiguousarray(np.zeros(m, np.int32) if senses is None else senses, dtype=np.int32)
    Kf = None if K is None else _f64(np.asarray(K, float).reshape(nout, -1), "F")
    out = dict(ML=np.empty((m, n)), MR=np.empty((m, n)), G=np.empty((m, m)), du=np.empty(m), dl=np.empty(m),
               Dth=np.empty((m, nth)), Rout=np.empty((nout, n)), x0=np.empty(nout), Xth=np.empty((nout, nth)))
    rc = lib().lmpc_transform_avi(n, m, ms, nth, nout, _ptr(H), _ptr(f), _ptr(f_theta), _ptr(A),
                                  _ptr(bu), _ptr(bl), _ptr(W), _ptr(sense), _ptr(Kf) if Kf is not None else None,
                                  int(nx if K is not None else 0),
                                  *[_ptr(out[k]) for k in ("ML", "MR", "G", "du", "dl", "Dth", "Rout", "x0", "Xth")])
    check(rc)
    out.update(n=n, m=m, ms=ms, nth=nth, nout=nout, sense=sense)
    return out


def _dev_arg(t, name, dtype, numel, device, optional=True):
    """Validate a CUDA tensor handed to a *_device entry point as a raw pointer: the kernels write
    through it with a fixed element size and a dense layout, so a wrong dtype, a strided view or a
    tensor on another GPU would silently corrupt memory.  Returns the pointer (or None)."""
    if t is None:
        if optional:
            return None
        raise ValueError(f"{name} is required")
    if not t.is_cuda or t.device.index != device:
        raise ValueError(f"{name} must be a CUDA tensor on cuda:{device}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.numel() != numel:
        raise ValueError(f"{name} must hold {numel} elements, got {t.numel()}")
    return _vp(t.data_ptr())


def _mask_dtypes():
    import torch
    return (torch.int64, torch.uint64) if hasattr(torch, "uint64") else (torch.int64,)


def sens_host(pack, active, exitflag, xbar=None, settings: Settings | None = None, is_avi=False):
    """`lmpc_solve_vjp_host` (xbar given: returns (thbar (N, nth), status)) / `lmpc_solve_jacobian_host` (xbar None:
    returns (J (N, nout, nth), status)): the derivative kernels' arithmetic on the CPU from a raw LDP pack, a dict as
    `BatchedQP.ldp()` / `transform` return it.  Needs no GPU and no handle."""
    n, m, ms, nth, nout = (int(pack[k]) for k in ("n", "m", "ms", "nth", "nout"))
    arrs = [_f64(np.asarray(pack[k], float).reshape(s)) for k, s in
            (("M", (m, n)), ("du", (m,)), ("dl", (m,)), ("Dth", (m, nth)), ("Rout", (nout, n)), ("x0", (nout,)),
             ("Xth", (nout, nth)))]
    sense = np.ascontiguousarray(pack["sense"], dtype=np.int32).reshape(m)
    words = (2 * m + 63) // 64
    act = np.ascontiguousarray(np.asarray(active, np.uint64).reshape(-1, words))
    N = act.shape[0]
    ef = np.ascontiguousarray(np.asarray(exitflag, np.int32).reshape(N))
    status = np.zeros(N, np.int32)
    sp = ctypes.cast(ctypes.pointer(settings), _vp) if settings is not None else None
    head = (n, m, ms, nth, nout, *[_ptr(a) for a in arrs], _ptr(sense), sp, int(bool(is_avi)), N, _ptr(act), _ptr(ef))
    if xbar is None:
        out = np.zeros((N, nout, nth))
        check(lib().lmpc_solve_jacobian_host(*head, _ptr(out), _ptr(status)))
    else:
        xb = _f64(np.asarray(xbar, float).reshape(N, nout))
        out = np.zeros((N, nth))
        check(lib().lmpc_solve_vjp_host(*head, _ptr(xb), _ptr(out), _ptr(status)))
    return out, status


PACK_BARS = ("M", "du", "dl", "Dth", "Rout", "x0", "Xth")


def _pack_bar_shapes(n, m, nth, nout):
    return dict(M=(m, n), du=(m,), dl=(m,), Dth=(m, nth), Rout=(nout, n), x0=(nout,), Xth=(nout, nth))


def pack_vjp_host(pack, theta, active, exitflag, xbar, settings: Settings | None = None, is_avi=False, want=PACK_BARS):
    """`lmpc_solve_pack_vjp_host`: the gradient of sum_p <xbar_p, x*_p> with respect to the LDP pack, summed over the
    batch, on the CPU from a raw pack (a dict as `BatchedQP.ldp()` / `transform` return it).  Returns a dict with the
    arrays named in `want` (of M, du, dl, Dth, Rout, x0, Xth; the others are passed as NULL), thbar (N, nth) and status."""
    n, m, ms, nth, nout = (int(pack[k]) for k in ("n", "m", "ms", "nth", "nout"))
    shapes = _pack_bar_shapes(n, m, nth, nout)
    arrs = [_f64(np.asarray(pack[k], float).reshape(shapes[k])) for k in PACK_BARS]
    sense = np.ascontiguousarray(pack["sense"], dtype=np.int32).reshape(m)
    words = (2 * m + 63) // 64
    act = np.ascontiguousarray(np.asarray(active, np.uint64).reshape(-1, words))
    N = act.shape[0]
    ef = np.ascontiguousarray(np.asarray(exitflag, np.int32).reshape(N))
    th = _f64(np.asarray(theta, float).reshape(N, nth))
    xb = _f64(np.asarray(xbar, float).reshape(N, nout))
    out = {k: np.full(shapes[k], np.nan) for k in PACK_BARS if k in want}
    out["thbar"], out["status"] = np.zeros((N, nth)), np.zeros(N, np.int32)
    sp = ctypes.cast(ctypes.pointer(settings), _vp) if settings is not None else None
    check(lib().lmpc_solve_pack_vjp_host(n, m, ms, nth, nout, *[_ptr(a) for a in arrs], _ptr(sense), sp, int(bool(is_avi)), N,
                                         _ptr(th), _ptr(act), _ptr(ef), _ptr(xb), *[_ptr(out.get(k)) for k in PACK_BARS],
                                         _ptr(out["thbar"]), _ptr(out["status"])))
    return out


def transform_vjp(H, f, f_theta, A, bu, bl, W, bars, senses=None, nout=None, K=None, nx=0):
    """`lmpc_transform_vjp`: the adjoint of `transform`.  bars: dict of gradients with respect to the transform's outputs
    (row-major M, du, dl, Dth, Rout, x0, Xth; a missing one counts as zero).  Returns a dict with the gradients H
    (symmetric), f, f_theta, A, bu, bl, W and K (nout x nx; None without a K)."""
    H = _f64(H, "F")
    n = H.shape[0]
    f_theta = _f64(np.asarray(f_theta, float).reshape(n, -1), "F")
    nth = f_theta.shape[1]
    bu = _f64(np.asarray(bu, float).reshape(-1))
    bl = _f64(np.asarray(bl, float).reshape(-1))
    m = bu.size
    A = _f64(np.asarray(A, float).reshape(-1, n), "F")
    mg = A.shape[0]
    ms = m - mg
    W = _f64(np.asarray(W, float).reshape(m, nth), "F")
    f = _f64(np.zeros(n) if f is None else np.asarray(f, float).reshape(n))
    nout = n if nout is None else int(nout)
    sense = np.ascontiguousarray(np.zeros(m, np.int32) if senses is None else senses, dtype=np.int32)
    Kf = None if K is None else _f64(np.asarray(K, float).reshape(nout, -1), "F")
    nx = int(nx if K is not None else 0)
    shapes = _pack_bar_shapes(n, m, nth, nout)
    ins = [None if bars.get(k) is None else _f64(np.asarray(bars[k], float).reshape(shapes[k])) for k in PACK_BARS]
    out = dict(H=np.zeros((n, n), order="F"), f=np.zeros(n), f_theta=np.zeros((n, nth), order="F"),
               A=np.zeros((mg, n), order="F"), bu=np.zeros(m), bl=np.zeros(m), W=np.zeros((m, nth), order="F"),
               K=None if K is None else np.zeros((nout, nx), order="F"))
    check(lib().lmpc_transform_vjp(n, m, ms, nth, nout, _ptr(H), _ptr(f), _ptr(f_theta), _ptr(A), _ptr(bu), _ptr(bl), _ptr(W),
                                   _ptr(sense), _ptr(Kf) if Kf is not None else None, nx, *[_ptr(a) for a in ins],
                                   *[_ptr(out[k]) for k in ("H", "f", "f_theta", "A", "bu", "bl", "W", "K")]))
    return out


def scenario_vjp_host(pack, sim, active, flag, Xbar=None, Ubar=None, observer=None, xhat_given=False,
                      settings: Settings | None = None, is_avi=False, want=("r", "d", "p")):
    """`lmpc_scenario_vjp_host`: the backward sweep of a taped scenario run on the CPU, no GPU and no handle.  pack: a raw
    LDP pack as `BatchedQP.ldp()` returns it.  sim: dict with nx, nu, nd, ny, plant (rows [f, F, G, Gd]), measurement
    (rows [h, C, Dd] or None), nuprev, use_observer and the blocks r, d, p as (w, T, H) (columns available, preview
    length) or None.  active (T, N, words) uint64 and flag (T, N) int32: the tape.  Xbar (T+1, N, nx), Ubar (T, N, nu) or
    None.  observer: (plant_dynamics, measurement_function, k_transpose) with use_observer.  Returns a dict: x0bar,
    xhat0bar (None unless xhat_given), uprev0bar, rbar / dbar / pbar step-major (Tc, N, w) or None, status_min."""
    n, m, ms, nth, nout = (int(pack[k]) for k in ("n", "m", "ms", "nth", "nout"))
    arrs = [_f64(np.asarray(pack[k], float).reshape(sh)) for k, sh in
            (("M", (m, n)), ("du", (m,)), ("dl", (m,)), ("Dth", (m, nth)), ("Rout", (nout, n)), ("x0", (nout,)),
             ("Xth", (nout, nth)))]
    sense = np.ascontiguousarray(pack["sense"], dtype=np.int32).reshape(m)
    words = (2 * m + 63) // 64
    flag = np.ascontiguousarray(np.asarray(flag, np.int32))
    T, N = (int(v) for v in flag.shape)
    act = np.ascontiguousarray(np.asarray(active, np.uint64).reshape(T, N, words))
    nx, nu, nd, ny, nup = (int(sim[k]) for k in ("nx", "nu", "nd", "ny", "nuprev"))
    use_obs = bool(sim.get("use_observer"))
    keep = [_f64(np.asarray(sim["plant"], float).reshape(-1)),
            None if sim.get("measurement") is None else _f64(np.asarray(sim["measurement"], float).reshape(-1))]
    d = _cabi.ScenarioSim()
    d.nx, d.nu, d.nd, d.ny = nx, nu, nd, ny
    d.plant = keep[0].ctypes.data
    d.measurement = None if keep[1] is None else keep[1].ctypes.data
    d.nuprev, d.use_observer, d.warm = nup, int(use_obs), 0
    out = dict(x0bar=np.zeros((N, nx)), xhat0bar=np.zeros((N, nx)) if (use_obs and xhat_given) else None,
               uprev0bar=np.zeros((N, nup)), status_min=np.zeros(N, np.int32), rbar=None, dbar=None, pbar=None)
    for name in ("r", "d", "p"):
        b = sim.get(name)
        if b is None:
            setattr(d, name, Block(None, 0, 0, 1, 0, 0))
            continue
        w, Tc, H = (int(v) for v in b)
        setattr(d, name, Block(None, 0, w, Tc, 0, H))
        if name in want and w > 0:
            out[name + "bar"] = np.full((max(Tc, 1), N, w), np.nan)      # (the call zeroes it)
    d.noise = Block(None, 0, 0, 1, 0, 0)
    od = None
    if use_obs and observer is not None:
        oa = [_f64(np.asarray(a, float).reshape(-1)) for a in observer]
        keep += oa
        od = ctypes.byref(Observer(nx, nu, nd, ny, *[a.ctypes.data for a in oa]))
    xb = None if Xbar is None else _f64(np.asarray(Xbar, float).reshape(T + 1, N, nx))
    ub = None if Ubar is None else _f64(np.asarray(Ubar, float).reshape(T, N, nu))
    ptr = lambda a: None if a is None else a.ctypes.data
    tape = _cabi.ScenarioTape(ptr(act), ptr(flag))
    g = _cabi.ScenarioGrad(ptr(xb), ptr(ub), ptr(out["x0bar"]), ptr(out["xhat0bar"]), ptr(out["uprev0bar"]), ptr(out["rbar"]),
                           ptr(out["dbar"]), ptr(out["pbar"]), ptr(out["status_min"]))
    sp = ctypes.cast(ctypes.pointer(settings), _vp) if settings is not None else None
    check(lib().lmpc_scenario_vjp_host(n, m, ms, nth, nout, *[_ptr(a) for a in arrs], _ptr(sense), sp, int(bool(is_avi)), od,
                                       N, T, ctypes.byref(d), ctypes.byref(tape), ctypes.byref(g)))
    return out


_AUTOGRAD_FN = None
_SCENARIO_FN = None


def _scenario_fn():
    """The torch.autograd.Function of `BatchedQP.simulate_scenario_autograd` (made on first use)."""
    global _SCENARIO_FN
    if _SCENARIO_FN is not None:
        return _SCENARIO_FN
    import torch

    class ScenarioFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, qp, T, plant, kw, x, uprev, r, d, p):
            det = lambda t: None if t is None else t.detach()
            out = qp.simulate_scenario(x.detach().clone(), T, plant, r=det(r), d=det(d), p=det(p),
                                       uprev=None if uprev is None else uprev.detach().clone(), want=("U", "X"), tape=True, **kw)
            ctx.qp, ctx.tape = qp, out["tape"]
            ctx.shapes = [None if t is None else tuple(t.shape) for t in (r, d, p)]
            ctx.status_min = None
            ctx.mark_non_differentiable(out["flag_min"])
            return out["X"], out["U"], out["flag_min"]

        @staticmethod
        def backward(ctx, Xbar, Ubar, _fbar):
            g = ctx.qp.scenario_vjp(ctx.tape, Xbar=None if Xbar is None else Xbar.contiguous(),
                                    Ubar=None if Ubar is None else Ubar.contiguous())
            ctx.status_min = g["status_min"]
            grads = []
            for name, shape in zip(("rbar", "dbar", "pbar"), ctx.shapes):
                t = g.get(name)
                if t is None or shape is None:
                    grads.append(None)
                else:                                  # a shared block: the per-scenario gradient summed over scenarios
                    grads.append(t if len(shape) == 3 else t.sum(0).reshape(shape))
            return (None, None, None, None, g["x0bar"], g["uprev0bar"] if ctx.tape["nup"] else None, *grads)

    _SCENARIO_FN = ScenarioFunction
    return ScenarioFunction


def _autograd_fn():
    """The torch.autograd.Function of `BatchedQP.solve_autograd` (made on first use: importing the package needs no torch)."""
    global _AUTOGRAD_FN
    if _AUTOGRAD_FN is not None:
        return _AUTOGRAD_FN
    import torch

    class SolveFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, theta, qp):
            th = theta.detach().contiguous()
            active = torch.empty((th.shape[0], qp.words), dtype=torch.int64, device=th.device)
            x, ef = qp.solve_device(th, active=active)
            ctx.qp = qp
            ctx.sens_status = None
            ctx.save_for_backward(active, ef)
            ctx.mark_non_differentiable(ef)
            return x, ef

        @staticmethod
        def backward(ctx, xbar, _efbar):
            active, ef = ctx.saved_tensors
            thbar, status = ctx.qp.solve_vjp_device(active, ef, xbar.contiguous())
            ctx.sens_status = ctx.qp.last_sens_status = status
            return thbar, None

    _AUTOGRAD_FN = SolveFunction
    return SolveFunction


_MPQP_FN = None


def _mpqp_fn():
    """The torch.autograd.Function of `solve_mpqp_autograd` (made on first use)."""
    global _MPQP_FN
    if _MPQP_FN is not None:
        return _MPQP_FN
    import torch

    class SolveMpqpFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, kw, H, f, f_theta, A, bu, bl, W, K, theta):
            host = lambda t: None if t is None else t.detach().cpu().numpy().astype(np.float64)
            data = [host(t) for t in (H, f, f_theta, A, bu, bl, W)]
            qp = BatchedQP.from_mpqp(*data, senses=kw["senses"], nout=kw["nout"], K=host(K), nx=kw["nx"],
                                     settings=kw["settings"], device=kw["device"])
            th = theta.detach().contiguous()
            active = torch.empty((th.shape[0], qp.words), dtype=torch.int64, device=th.device)
            x, ef = qp.solve_device(th, active=active)
            ctx.qp, ctx.kw, ctx.data, ctx.K = qp, kw, data, host(K)
            ctx.like = [None if t is None else (tuple(t.shape), t.dtype, t.device) for t in (H, f, f_theta, A, bu, bl, W, K)]
            ctx.sens_status = None
            ctx.save_for_backward(th, active, ef)
            ctx.mark_non_differentiable(ef)
            return x, ef

        @staticmethod
        def backward(ctx, xbar, _efbar):
            th, active, ef = ctx.saved_tensors
            need = ctx.needs_input_grad[1:9]
            # (with nothing but theta requiring grad no sum is asked for: the call is then stage 1 alone, the VJP's work)
            g = ctx.qp.solve_pack_vjp_device(th, active, ef, xbar.contiguous(), want_thbar=True,
                                             want=PACK_BARS if any(need) else ())
            ctx.sens_status = g["status"]
            grads = [None] * 8
            if any(need):
                bars = {k: g[k].cpu().numpy() for k in PACK_BARS}          # the one download of the G doubles
                kw = ctx.kw
                d = transform_vjp(*ctx.data, bars, senses=kw["senses"], nout=kw["nout"], K=ctx.K, nx=kw["nx"])
                for q, name in enumerate(("H", "f", "f_theta", "A", "bu", "bl", "W", "K")):
                    if need[q] and ctx.like[q] is not None and d[name] is not None:
                        shape, dtype, device = ctx.like[q]
                        grads[q] = torch.as_tensor(np.ascontiguousarray(d[name]), dtype=dtype, device=device).reshape(shape)
            return (None, *grads, g["thbar"] if ctx.needs_input_grad[9] else None)

    _MPQP_FN = SolveMpqpFunction
    return SolveMpqpFunction


def solve_mpqp_autograd(H, f, f_theta, A, bu, bl, W, theta, senses=None, nout=None, K=None, nx=0, settings=None, device=0):
    """The batched solve of an mpQP given as torch tensors, inside a torch graph: returns (x, exitflag), x carrying the
    gradient with respect to whichever of H, f, f_theta, A, bu, bl, W, K and theta require grad.  Forward: `from_mpqp`
    on the tensors' values, then `solve_device` with the masks kept.  Backward: ONE `solve_pack_vjp_device` (with thbar),
    one download of the summed pack gradient, `transform_vjp` on the host.  theta: (N, nth) float64 CUDA tensor on
    `device`; the data tensors may live anywhere.  The status of the backward is `x.grad_fn.sens_status`."""
    kw = dict(senses=senses, nout=nout, nx=int(nx), settings=settings, device=int(device))
    return _mpqp_fn().apply(kw, H, f, f_theta, A, bu, bl, W, K, theta)


class BatchedQP:
    """One condensed-MPC QP structure resident on one GPU, solved for batches of theta."""

    last_sens_status = None     # status tensor of the most recent backward of `solve_autograd`

    def __init__(self, handle, device):
        self._h = handle
        self.device = device
        dims = (ctypes.c_int32 * 6)()
        check(lib().lmpc_get_dims(self._h, ctypes.byref(dims)), self._h)
        self.n, self.m, self.ms, self.nth, self.nout, self.words = (int(v) for v in dims)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_mpqp(cls, H, f, f_theta, A, bu, bl, W, senses=None, nout=None, K=None, nx=0,
                  settings: Settings | None = None, device=0, break_points=None, is_avi=None):
        """DAQP.setup + DAQP.settings equivalent (reference setup.jl:11-13,26).  `break_points` / `is_avi` are the two
        keywords the reference passes to DAQP.setup (mpQP.break_points, !mpQP.is_symmetric): given, the call goes
        through lmpc_setup_ex; left None, lmpc_setup decides is_avi from H the way the reference does."""
        H = _f64(H, "F")
        n = H.shape[0]
        f_theta = _f64(np.asarray(f_theta, float).reshape(n, -1), "F")
        nth = f_theta.shape[1]
        bu = _f64(np.asarray(bu, float).reshape(-1))
        bl = _f64(np.asarray(bl, float).reshape(-1))
        m = bu.size
        A = _f64(np.asarray(A, float).reshape(-1, n), "F")
        ms = m - A.shape[0]
        W = _f64(np.asarray(W, float).reshape(m, nth), "F")
        f = _f64(np.zeros(n) if f is None else np.asarray(f, float).reshape(n))
        nout = n if nout is None else int(nout)
        sense = np.ascontiguousarray(np.zeros(m, np.int32) if senses is None else senses, dtype=np.int32)
        Kf = None if K is None else _f64(np.asarray(K, float).reshape(nout, -1), "F")
        h = _vp()
        sp = ctypes.cast(ctypes.pointer(settings), _vp) if settings is not None else None
        if break_points is None and is_avi is None:
            rc = lib().lmpc_setup(ctypes.byref(h), n, m, ms, nth, nout, _ptr(H), _ptr(f), _ptr(f_theta),
                                  _ptr(A), _ptr(bu), _ptr(bl), _ptr(W), _ptr(sense),
                                  _ptr(Kf) if Kf is not None else None, int(nx if K is not None else 0), sp, int(device))
        else:
            bp = np.ascontiguousarray(np.zeros(0, np.int32) if break_points is None else break_points, dtype=np.int32)
            rc = lib().lmpc_setup_ex(ctypes.byref(h), n, m, ms, nth, nout, _ptr(H), _ptr(f), _ptr(f_theta),
                                     _ptr(A), _ptr(bu), _ptr(bl), _ptr(W), _ptr(sense),
                                     _ptr(Kf) if Kf is not None else None, int(nx if K is not None else 0), sp,
                                     _ptr(bp) if bp.size else None, int(bp.size), int(bool(is_avi)), int(device))
        check(rc)
        return cls(h, device)

    @classmethod
    def from_ldp(cls, M, du, dl, Dth, Rout, x0, Xth, sense=None, ms=0,
                 settings: Settings | None = None, device=0):
        """Setup from the arrays the reference's code generator emits (codegen.jl:183-189)."""
        M = _f64(M)
        m, n = M.shape
        Dth = _f64(np.asarray(Dth, float).reshape(m, -1))
        nth = Dth.shape[1]
        Rout = _f64(np.asarray(Rout, float).reshape(-1, n))
        nout = Rout.shape[0]
        du, dl, x0 = _f64(du), _f64(dl), _f64(x0)
        Xth = _f64(np.asarray(Xth, float).reshape(nout, nth))
        sense = np.ascontiguousarray(np.zeros(m, np.int32) if sense is None else sense, dtype=np.int32)
        h = _vp()
        rc = lib().lmpc_setup_ldp(ctypes.byref(h), n, m, int(ms), nth, nout, _ptr(M), _ptr(du), _ptr(dl),
                                  _ptr(Dth), _ptr(Rout), _ptr(x0), _ptr(Xth), _ptr(sense),
                                  ctypes.cast(ctypes.pointer(settings), _vp) if settings is not None else None,
                                  int(device))
        check(rc)
        return cls(h, device)

    # ------------------------------------------------------------------ inspection
    @property
    def kernel_name(self) -> str:
        return lib().lmpc_kernel_name(self._h).decode()

    def wave_stats(self):
        """Working-set statistics of the wavefront kernel as the handle last saw them (lmpc_wave_stats): dict with the
        problems finished, how many of them stayed within 24 / 32 / 48 rows, and the first-pass capacity of the next
        call (0 = one pass)."""
        out = (ctypes.c_ulonglong * 5)()
        check(lib().lmpc_wave_stats(self._h, out), self._h)
        return {"problems": int(out[0]), "within_24": int(out[1]), "within_32": int(out[2]), "within_48": int(out[3]),
                "first_pass_rows": int(out[4])}

    WAVE_LAUNCH_FIELDS = ("seq", "real_bytes", "MR", "LDSC", "BNB", "PACKED", "NU", "GRAM", "SIM", "nwv", "level", "grid",
                          "qchunk", "pass", "cap", "big", "queue", "worklist", "lds", "nprob")

    def wave_launch_info(self, since=0):
        """The handle's most recent wavefront-kernel launches (lmpc_wave_launch_info; at most four are kept), oldest
        first: one dict per launch with the template arguments of the wave_kernel instantiation that ran (real_bytes,
        MR, LDSC, BNB, PACKED, NU, GRAM, SIM) and its launch shape (nwv, level, grid, qchunk, pass, cap, big, queue,
        worklist, lds, nprob).  "seq" numbers the launches of the handle's life from 1; `since` = keep only the
        launches with a larger number (pass the last "seq" seen before a call to get that call's launches)."""
        W = len(self.WAVE_LAUNCH_FIELDS)
        out = (ctypes.c_int32 * (4 * W))()
        k = lib().lmpc_wave_launch_info(self._h, out, 4)
        if k < 0:
            check(k, self._h)
        recs = [dict(zip(self.WAVE_LAUNCH_FIELDS, (int(v) for v in out[q * W:(q + 1) * W]))) for q in range(k)]
        return [r for r in recs if r["seq"] > since]

    ROW_LAUNCH_FIELDS = ("seq", "real_bytes", "S", "NS", "MS", "CAPP", "BNB", "nwv", "blocks", "grid", "ps", "lds", "aux",
                         "pass", "cap", "qchunk", "queue", "worklist", "nprob", "snap_bytes")

    def row_launch_info(self, since=0):
        """The handle's most recent row-kernel launches (lmpc_row_launch_info; at most four are kept), oldest first:
        one dict per launch with the template arguments of the row_kernel instantiation that ran (real_bytes, S, NS,
        MS, CAPP, BNB) and its launch shape (nwv, blocks per CU, grid, ps, lds, aux, pass, cap, qchunk, queue,
        worklist, nprob, snap_bytes).  "seq" numbers the row-kernel launches of the handle's life from 1; `since` as
        in wave_launch_info.  A batch the row kernel did not take leaves no entry."""
        W = len(self.ROW_LAUNCH_FIELDS)
        out = (ctypes.c_int32 * (4 * W))()
        k = lib().lmpc_row_launch_info(self._h, out, 4)
        if k < 0:
            check(k, self._h)
        recs = [dict(zip(self.ROW_LAUNCH_FIELDS, (int(v) for v in out[q * W:(q + 1) * W]))) for q in range(k)]
        return [r for r in recs if r["seq"] > since]

    FAST_LAUNCH_FIELDS = ("seq", "form", "staged", "tiles", "nstr", "dma", "grid", "batches", "lds", "dyn")
    FAST_PLAIN, FAST_GATHER, FAST_MULTI = 0, 1, 2

    def fast_launch_info(self):
        """The handle's most recent launch of the one-launch kernel (lmpc_fast_launch_info) as a dict: "seq" numbers
        the launches of the handle's life from 1, "form" is FAST_PLAIN / FAST_GATHER / FAST_MULTI, "staged" 1 if x and
        the exit flags were kept in LDS and stored once per workgroup, then the launch shape (tiles per workgroup,
        streaming wavefronts, ring depth, grid, batches, LDS bytes, ticket tiles).  None if there was no such launch."""
        out = (ctypes.c_int32 * len(self.FAST_LAUNCH_FIELDS))()
        k = lib().lmpc_fast_launch_info(self._h, out)
        if k < 0:
            check(k, self._h)
        return dict(zip(self.FAST_LAUNCH_FIELDS, (int(v) for v in out))) if k else None

    FRONT_PASS_FIELDS = ("seq", "kind", "N", "grid", "lds", "nprob", "seg_cap", "walker")
    FRONT_SCREEN, FRONT_TIERS = 1, 2
    WALK_LANE, WALK_WAVE, WALK_ROW = 1, 2, 3
    LIST_SHARDS = 64

    def front_pass_info(self, since=0):
        """The handle's most recent front-pass launches (lmpc_front_pass_info; at most four are kept), oldest first:
        one dict per launch with its kind (FRONT_SCREEN the screening pass, FRONT_TIERS the tiers pass), the template
        argument N of qp_tiers_kernel (0 for the screening pass), grid, lds, nprob, seg_cap and the kernel that walks
        the list (WALK_LANE / WALK_WAVE / WALK_ROW).  "seq" and `since` as in wave_launch_info.  A call without a front
        pass leaves no entry."""
        W = len(self.FRONT_PASS_FIELDS)
        out = (ctypes.c_int32 * (4 * W))()
        k = lib().lmpc_front_pass_info(self._h, out, 4)
        if k < 0:
            check(k, self._h)
        recs = [dict(zip(self.FRONT_PASS_FIELDS, (int(v) for v in out[q * W:(q + 1) * W]))) for q in range(k)]
        return [r for r in recs if r["seq"] > since]

    def work_list_read(self):
        """What the most recent front pass left on the work list (lmpc_work_list_read; needs set_option("list_snapshot",
        1) before the call): (counts, list) with counts the LIST_SHARDS segment counters and list a LIST_SHARDS x
        seg_cap int32 array of which row s holds counts[s] entries -- or None if no snapshot has been taken."""
        return self._list_read(lib().lmpc_work_list_read)

    def _list_read(self, read, *which):
        """(counts, list) of one list snapshot through its C reader: asked for the counts and seg_cap first, then, with
        room for them, for the segments"""
        counts = np.zeros(self.LIST_SHARDS, np.int32)
        seg = read(self._h, *which, _ptr(counts), None, 0)
        if seg < 0:
            check(int(seg), self._h)
        if seg == 0:
            return None
        lst = np.zeros((self.LIST_SHARDS, int(seg)), np.int32)
        seg2 = read(self._h, *which, _ptr(counts), _ptr(lst), lst.size)
        if seg2 != seg:
            check(int(seg2) if seg2 < 0 else -1, self._h)
        return counts, lst

    AVI_LAUNCH_FIELDS = ("seq", "stage", "N", "K", "LIST", "LDSC", "PROX", "grid", "lds", "occ", "nprob", "seg_cap")
    AVI_TIERS, AVI_LANE, AVI_SLAB = 1, 2, 3
    AVI_LAUNCHES_KEPT = 8

    def avi_launch_info(self, since=0):
        """The most recent launches of a variational handle's chain (lmpc_avi_launch_info; at most eight are kept: two
        calls and more), oldest first: one dict per launch with its stage (AVI_TIERS avi_tiers_kernel<N, K, false>,
        AVI_LANE avi_lane_kernel<N, LIST>, AVI_SLAB avi_kernel<LDSC, PROX>), the template arguments, grid, lds, the
        occupancy value the grid was sized with, nprob and the lists' seg_cap (0: no list).  "seq" and `since` as in
        wave_launch_info."""
        W, K = len(self.AVI_LAUNCH_FIELDS), self.AVI_LAUNCHES_KEPT
        out = (ctypes.c_int32 * (K * W))()
        k = lib().lmpc_avi_launch_info(self._h, out, K)
        if k < 0:
            check(k, self._h)
        recs = [dict(zip(self.AVI_LAUNCH_FIELDS, (int(v) for v in out[q * W:(q + 1) * W]))) for q in range(k)]
        return [r for r in recs if r["seq"] > since]

    def avi_list_read(self, which):
        """What the chain's launch over the whole batch (which = 0) or its lane kernel (1) left on its work list in the
        most recent call (lmpc_avi_list_read; needs set_option("list_snapshot", 1) before the call): (counts, list) as
        work_list_read -- or None if that call made no list."""
        return self._list_read(lib().lmpc_avi_list_read, int(which))

    def ldp(self):
        """The constant pack the kernels use (row-major) -- what tests hand to the oracle."""
        out = dict(M=np.empty((self.m, self.n)), du=np.empty(self.m), dl=np.empty(self.m),
                   Dth=np.empty((self.m, self.nth)), Rout=np.empty((self.nout, self.n)),
                   x0=np.empty(self.nout), Xth=np.empty((self.nout, self.nth)))
        sense = np.zeros(self.m, np.int32)
        check(lib().lmpc_get_ldp(self._h, *[_ptr(out[k]) for k in ("M", "du", "dl", "Dth", "Rout", "x0", "Xth")],
                                 _ptr(sense)), self._h)
        out.update(sense=sense, n=self.n, m=self.m, ms=self.ms, nth=self.nth, nout=self.nout)
        return out

    @property
    def is_avi(self) -> bool:
        """The handle was set up for a non-symmetric H (variational objective; reference setup.jl:13 is_avi)."""
        return bool(lib().lmpc_is_avi(self._h))

    def avi_pack(self):
        """The constant pack of a variational-inequality handle: ldp() (M = the scaled rows ML) plus MR and the full
        non-symmetric Gram matrix G -- what tests hand to the oracle's AVI solver."""
        out = self.ldp()
        out["ML"] = out["M"]
        out["MR"] = np.empty((self.m, self.n))
        out["G"] = np.empty((self.m, self.m))
        check(lib().lmpc_get_avi(self._h, _ptr(out["MR"]), _ptr(out["G"])), self._h)
        return out

    def prox_pack(self):
        """The extra arrays of a proximal-point handle (eps_prox > 0): (H + eps I)^-1, the full-length affine map of
        the unconstrained optimum, the outputs' feedback term -- what tests hand to the oracle next to avi_pack()."""
        out = dict(Hinv=np.empty((self.n, self.n)), x0f=np.empty(self.n), Xthf=np.empty((self.n, self.nth)),
                   Kth=np.empty((self.nout, self.nth)))
        lib().lmpc_get_prox.argtypes = [_vp] * 5
        lib().lmpc_get_prox.restype = ctypes.c_int
        check(lib().lmpc_get_prox(self._h, *[_ptr(out[k]) for k in ("Hinv", "x0f", "Xthf", "Kth")]), self._h)
        return out

    def set_settings(self, settings: Settings):
        check(lib().lmpc_set_settings(self._h, ctypes.byref(settings)), self._h)

    # ------------------------------------------------------------------ solving
    def solve(self, theta, warm=None, want_iters=True, want_active=True):
        """Host arrays in, host arrays out (`lmpc_solve_batch`)."""
        theta = _f64(np.asarray(theta, float).reshape(-1, self.nth) if self.nth else np.zeros((len(theta), 0)))
        N = theta.shape[0]
        # outputs are touched before the call: a device-to-host copy into pages the OS has not mapped
        # yet runs at a fraction of the PCIe rate (measured: 22 ms instead of 1.3 ms for 10^6 problems)
        x = np.zeros((N, self.nout))
        ef = np.zeros(N, np.int32)
        it = np.zeros(N, np.int32) if want_iters else None
        act = np.zeros((N, self.words), np.uint64) if want_active else None
        for a_ in (x, ef, it, act):
            if a_ is not None:
                a_.fill(0)
        w = None
        if warm is not None:
            w = np.ascontiguousarray(np.asarray(warm, np.uint64).reshape(N, self.words))
        check(lib().lmpc_solve_batch(self._h, N, _ptr(theta), _ptr(x), _ptr(ef),
                                     _ptr(it) if it is not None else None,
                                     _ptr(act) if act is not None else None,
                                     _ptr(w) if w is not None else None), self._h)
        return x, ef, it, act

    def solve_f32(self, theta, warm=None, want_iters=True, want_active=True):
        """Binary32 solve (`lmpc_solve_batch_f32`; reference codegen.jl:19 float_type="float"):
        float32 host arrays in and out, wavefront kernel."""
        theta = np.ascontiguousarray(np.asarray(theta, np.float32).reshape(-1, self.nth) if self.nth
                                     else np.zeros((len(theta), 0), np.float32))
        N = theta.shape[0]
        x = np.empty((N, self.nout), np.float32)
        ef = np.empty(N, np.int32)
        it = np.empty(N, np.int32) if want_iters else None
        act = np.zeros((N, self.words), np.uint64) if want_active else None
        w = None
        if warm is not None:
            w = np.ascontiguousarray(np.asarray(warm, np.uint64).reshape(N, self.words))
        check(lib().lmpc_solve_batch_f32(self._h, N, _ptr(theta), _ptr(x), _ptr(ef),
                                         _ptr(it) if it is not None else None,
                                         _ptr(act) if act is not None else None,
                                         _ptr(w) if w is not None else None), self._h)
        return x, ef, it, act

    def solve_one(self, theta):
        """DAQP.solve shape for one theta: (x*, exitflag) (`lmpc_solve_one`)."""
        theta = _f64(np.asarray(theta, float).reshape(self.nth))
        x = np.empty(self.nout)
        rc = lib().lmpc_solve_one(self._h, _ptr(theta), _ptr(x))
        if rc <= -100:
            raise LmpcError(rc, _cabi.last_error(self._h))
        return x, rc

    def solve_device(self, theta, x=None, exitflag=None, iters=None, active=None, warm=None, stream=None):
        """Device-resident batch (`lmpc_solve_batch_device`): torch CUDA tensors in and out, the
        launch is enqueued on `stream` (default: torch's current stream) and NOT synchronised."""
        import torch
        if not theta.is_cuda or theta.dtype not in (torch.float64, torch.float32) or not theta.is_contiguous():
            raise ValueError("theta must be a contiguous float64 (or float32: binary32 path) CUDA tensor of shape (N, nth)")
        if theta.device.index != self.device:
            raise ValueError("theta lives on a different GPU than this handle")
        N = theta.shape[0]
        dev = theta.device
        if x is None:
            x = torch.empty((N, self.nout), dtype=theta.dtype, device=dev)
        if x.dtype != theta.dtype:
            raise ValueError("x and theta must have the same dtype")
        if exitflag is None:
            exitflag = torch.empty(N, dtype=torch.int32, device=dev)
        if theta.dim() != 2 or theta.shape[1] != self.nth:
            raise ValueError(f"theta must have shape (N, {self.nth})")
        # `stream` is a raw hipStream_t: tensors this call allocated live on torch's current stream, so the
        # caller who passes a foreign stream must keep x / exitflag alive until that stream has finished
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        fn = lib().lmpc_solve_batch_device if theta.dtype == torch.float64 else lib().lmpc_solve_batch_f32_device

        def mask(t, name):
            if t is not None and t.dtype not in _mask_dtypes():
                raise ValueError(f"{name} must be a 64-bit integer tensor")
            return _dev_arg(t, name, t.dtype if t is not None else None, N * self.words, self.device)

        check(fn(
            self._h, N, _vp(theta.data_ptr()), _dev_arg(x, "x", theta.dtype, N * self.nout, self.device, False),
            _dev_arg(exitflag, "exitflag", torch.int32, N, self.device, False),
            _dev_arg(iters, "iters", torch.int32, N, self.device), mask(active, "active"), mask(warm, "warm"),
            _vp(st)), self._h)
        return x, exitflag

    def bind_device_call(self, theta, x, exitflag, stream):
        """`lmpc_solve_batch_device` with every argument validated and marshalled ONCE: returns a callable that
        enqueues the same call again (a loop over a fixed set of resident batches: the per-call Python work --
        tensor checks, ctypes conversions -- is ~5 us, a third of the 18 us a batch takes on the GPU)."""
        import torch
        if not (theta.is_cuda and theta.dtype == torch.float64 and theta.is_contiguous() and theta.dim() == 2
                and theta.shape[1] == self.nth and theta.device.index == self.device):
            raise ValueError("theta must be a contiguous float64 CUDA tensor of shape (N, nth) on this handle's GPU")
        N = int(theta.shape[0])
        args = (self._h, ctypes.c_int64(N), _vp(theta.data_ptr()),
                _dev_arg(x, "x", torch.float64, N * self.nout, self.device, False),
                _dev_arg(exitflag, "exitflag", torch.int32, N, self.device, False), None, None, None, _vp(stream))
        fn = lib().lmpc_solve_batch_device
        h = self._h
        keep = (theta, x, exitflag)

        def call():
            rc = fn(*args)
            if rc != _cabi.LMPC_OK:
                check(rc, h)
            return keep
        return call

    def bind_device_batches(self, thetas, xs, exitflags, stream):
        """`lmpc_solve_batches_device`: several resident batches of the same size in ONE call (on the handles the
        one-launch kernel covers: one kernel launch for up to eight of them).  Arguments validated and marshalled once;
        returns a callable that enqueues the same call again."""
        import torch
        nb = len(thetas)
        if not (nb == len(xs) == len(exitflags) and nb >= 1):
            raise ValueError("as many x and exitflag tensors as theta tensors")
        N = int(thetas[0].shape[0])
        for t in thetas:
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 2 and t.shape == (N, self.nth)
                    and t.device.index == self.device):
                raise ValueError("every theta must be a contiguous float64 CUDA tensor of shape (N, nth) on this handle's GPU")
        P = ctypes.c_void_p * nb
        tt = P(*[t.data_ptr() for t in thetas])
        xx = P(*[_dev_arg(x, "x", torch.float64, N * self.nout, self.device, False).value for x in xs])
        ff = P(*[_dev_arg(f, "exitflag", torch.int32, N, self.device, False).value for f in exitflags])
        args = (self._h, ctypes.c_int32(nb), ctypes.c_int64(N), ctypes.cast(tt, ctypes.c_void_p), ctypes.cast(xx, ctypes.c_void_p),
                ctypes.cast(ff, ctypes.c_void_p), _vp(stream))
        fn = lib().lmpc_solve_batches_device
        h = self._h
        keep = (list(thetas), list(xs), list(exitflags), tt, xx, ff)

        def call():
            rc = fn(*args)
            if rc != _cabi.LMPC_OK:
                check(rc, h)
            return keep
        return call

    def solve_batches_device(self, thetas, xs=None, exitflags=None, stream=None):
        """Several resident batches in one call; returns (xs, exitflags).  Enqueued on `stream` (default: torch's current
        stream), not synchronised."""
        import torch
        dev = torch.device("cuda", self.device)
        N = int(thetas[0].shape[0])
        xs = xs or [torch.empty((N, self.nout), dtype=torch.float64, device=dev) for _ in thetas]
        exitflags = exitflags or [torch.empty(N, dtype=torch.int32, device=dev) for _ in thetas]
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        self.bind_device_batches(thetas, xs, exitflags, st)()
        return xs, exitflags

    def simulate(self, x0, T, F, G, r=None, uprev=None, warm=True, want_x=True):
        """Batched closed loop (`lmpc_simulate`): N scenarios, T steps of solve + x <- F x + G u.

        Returns dict(x=final states, U=(T,N,nu), X=(T+1,N,nx) or None, uprev, flag_min)."""
        F = _f64(np.atleast_2d(F))
        nx = F.shape[0]
        nu = self.nout
        G = _f64(np.asarray(G, float).reshape(nx, nu))
        x = _f64(np.array(np.asarray(x0, float).reshape(-1, nx), copy=True))
        N = x.shape[0]
        nr = 0 if r is None else np.asarray(r).reshape(N, -1).shape[1]
        nup = self.nth - nx - nr
        if nup < 0 or nup > nu:
            raise ValueError("theta = [x; r; uprev] does not match this handle")
        rr = None if nr == 0 else _f64(np.asarray(r, float).reshape(N, nr))
        up = None
        if nup:
            up = _f64(np.zeros((N, nup)) if uprev is None else np.array(np.asarray(uprev, float).reshape(N, nup), copy=True))
        U = np.empty((T, N, nu))
        X = np.empty((T + 1, N, nx)) if want_x else None
        fm = np.empty(N, np.int32)
        check(lib().lmpc_simulate(self._h, N, int(T), nx, nr, nup, _ptr(F), _ptr(G), _ptr(x), _ptr(rr) if rr is not None else None,
                                  _ptr(up) if up is not None else None, _ptr(U), _ptr(X) if X is not None else None,
                                  _ptr(fm), int(bool(warm))), self._h)
        return dict(x=x, U=U, X=X, uprev=up, flag_min=fm)

    def simulate_f32(self, x0, T, F, G, r=None, uprev=None, warm=True, want_x=True):
        """Binary32 closed loop (`lmpc_simulate_f32`): float32 arrays in and out, wavefront kernel."""
        F = _f64(np.atleast_2d(F))
        nx = F.shape[0]
        nu = self.nout
        G = _f64(np.asarray(G, float).reshape(nx, nu))
        x = np.ascontiguousarray(np.array(np.asarray(x0, np.float32).reshape(-1, nx), copy=True))
        N = x.shape[0]
        nr = 0 if r is None else np.asarray(r).reshape(N, -1).shape[1]
        nup = self.nth - nx - nr
        if nup < 0 or nup > nu:
            raise ValueError("theta = [x; r; uprev] does not match this handle")
        rr = None if nr == 0 else np.ascontiguousarray(np.asarray(r, np.float32).reshape(N, nr))
        up = None
        if nup:
            up = np.ascontiguousarray(np.zeros((N, nup), np.float32) if uprev is None
                                      else np.array(np.asarray(uprev, np.float32).reshape(N, nup), copy=True))
        U = np.empty((T, N, nu), np.float32)
        X = np.empty((T + 1, N, nx), np.float32) if want_x else None
        fm = np.empty(N, np.int32)
        check(lib().lmpc_simulate_f32(self._h, N, int(T), nx, nr, nup, _ptr(F), _ptr(G), _ptr(x),
                                      _ptr(rr) if rr is not None else None, _ptr(up) if up is not None else None,
                                      _ptr(U), _ptr(X) if X is not None else None, _ptr(fm), int(bool(warm))), self._h)
        return dict(x=x, U=U, X=X, uprev=up, flag_min=fm)

    # ------------------------------------------------------------------ theta on the device, previews
    @staticmethod
    def _block(t, H=0, k0=0):
        """torch CUDA tensor (w,), (w, T) [shared] or (N, w, T) [per scenario] -> lmpc_block.
        The C side wants each matrix column by column (Julia layout), i.e. the (T, w) transpose."""
        import torch
        if t is None:
            return None, None
        if t.dim() == 1:
            t = t.reshape(-1, 1)
        per = t.dim() == 3
        keep = t.transpose(-1, -2).contiguous().to(torch.float64)          # (.., T, w): column after column
        w, T = int(t.shape[-2]), int(t.shape[-1])
        return Block(keep.data_ptr(), w * T if per else 0, w, T, int(k0), int(H)), keep

    def form_parameter_device(self, x, r=None, d=None, uprev=None, p=None, r_preview=0, d_preview=0,
                              p_preview=0, k0=0, theta=None, stream=None):
        """Batched form_parameter (`lmpc_form_parameter_device`; reference explicit.jl:54-63 with
        utils.jl:78-261 formatting).  x: (N, nx) CUDA tensor; r/d/p: (w,), (w, T) shared or (N, w, T);
        *_preview = horizon Np (0 = constant block); k0 = first trajectory column taken."""
        import torch
        N, nx = x.shape
        dev = x.device
        br, kr = self._block(r, r_preview, k0)
        bd, kd = self._block(d, d_preview, k0)
        bp, kp = self._block(p, p_preview, k0)
        nup = 0 if uprev is None else int(uprev.shape[1])
        if theta is None:
            theta = torch.empty((N, self.nth), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        check(lib().lmpc_form_parameter_device(
            self._h, N, _vp(theta.data_ptr()), _vp(x.data_ptr()), nx,
            ctypes.byref(br) if br is not None else None, ctypes.byref(bd) if bd is not None else None,
            _vp(uprev.data_ptr()) if uprev is not None else None, nup,
            ctypes.byref(bp) if bp is not None else None, _vp(st)), self._h)
        theta._lmpc_keep = (kr, kd, kp)          # the launch is asynchronous: keep the sources alive
        return theta

    def simulate_ref(self, x0, T, F, G, r, preview=0, uprev=None, warm=False):
        """Closed loop with a reference trajectory (`lmpc_simulate_ref_device`; reference
        simulation.jl:69-73,93-113).  r: (ny, Tr) shared or (N, ny, Tr); preview = Np for
        settings.reference_preview, 0 otherwise.  Host arrays in and out."""
        import torch
        dev = torch.device("cuda", self.device)
        F = _f64(np.atleast_2d(F))
        nx = F.shape[0]
        nu = self.nout
        G = _f64(np.asarray(G, float).reshape(nx, nu))
        x = torch.from_numpy(_f64(np.array(np.asarray(x0, float).reshape(-1, nx), copy=True))).to(dev)
        N = x.shape[0]
        rt = torch.from_numpy(np.asarray(r, float)).to(dev)
        br, keep = self._block(rt, preview, 0)
        nup = self.nth - nx - br.w * (preview if preview > 0 else 1)
        up = None
        if nup:
            up = torch.from_numpy(_f64(np.zeros((N, nup)) if uprev is None else np.asarray(uprev, float).reshape(N, nup))).to(dev)
        U = torch.empty((T, N, nu), dtype=torch.float64, device=dev)
        X = torch.empty((T + 1, N, nx), dtype=torch.float64, device=dev)
        fm = torch.empty(N, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        check(lib().lmpc_simulate_ref_device(self._h, N, int(T), nx, ctypes.byref(br), nup, _ptr(F), _ptr(G),
                                             _vp(x.data_ptr()), _vp(up.data_ptr()) if up is not None else None,
                                             _vp(U.data_ptr()), _vp(X.data_ptr()), _vp(fm.data_ptr()),
                                             int(bool(warm)), _vp(st)), self._h)
        torch.cuda.synchronize(dev)
        return dict(x=x.cpu().numpy(), U=U.cpu().numpy(), X=X.cpu().numpy(),
                    uprev=None if up is None else up.cpu().numpy(), flag_min=fm.cpu().numpy())

    # ------------------------------------------------------------------ scenario loop
    @staticmethod
    def sim_cost(nx, nu, C=None, Q=None, R=None, Rr=None, S=None, Ax=None, Au=None, lb=None, ub=None):
        """`lmpc_sim_cost` from host arrays (any may be None = zero): returns (struct, arrays to keep alive)."""
        keep = {}

        def mat(a, rows, cols, name):
            if a is None:
                return None
            a = np.asarray(a, float)
            if a.ndim == 1 and rows == cols and a.size == rows:          # a weight given by its diagonal
                a = np.diag(a)
            keep[name] = _f64(a.reshape(rows, cols))
            return keep[name].ctypes.data

        ny = 0 if C is None else int(np.atleast_2d(np.asarray(C, float)).reshape(-1, nx).shape[0])
        nc = 0 if lb is None else int(np.asarray(lb).size)
        c = _cabi.SimCost(ny, nc, mat(C, ny, nx, "C"), mat(Q, ny, ny, "Q"), mat(R, nu, nu, "R"), mat(Rr, nu, nu, "Rr"),
                          mat(S, nx, nu, "S"), mat(Ax, nc, nx, "Ax"), mat(Au, nc, nu, "Au"), mat(lb, nc, 1, "lb"),
                          mat(ub, nc, 1, "ub"))
        return c, keep

    def scenario_descriptor(self, plant, nx, nd=0, measurement=None, ny=0, r=None, d=None, p=None, noise=None,
                            nuprev=0, use_observer=False, warm=False, cost=None):
        """`lmpc_scenario_sim` from host constants and ready-made blocks (`Block` or None = left out).  Returns
        (struct, keep-alive list)."""
        pl = _f64(np.asarray(plant, float).reshape(-1))
        me = None if measurement is None else _f64(np.asarray(measurement, float).reshape(-1))
        s = _cabi.ScenarioSim()
        s.nx, s.nu, s.nd, s.ny = int(nx), self.nout, int(nd), int(ny)
        s.plant = pl.ctypes.data
        s.measurement = me.ctypes.data if me is not None else None
        for name, b in (("r", r), ("d", d), ("p", p), ("noise", noise)):
            setattr(s, name, b if b is not None else Block(None, 0, 0, 1, 0, 0))
        s.nuprev, s.use_observer, s.warm = int(nuprev), int(bool(use_observer)), int(bool(warm))
        keep = [pl, me]
        if cost is not None:
            c, ck = cost if isinstance(cost, tuple) else (cost, None)
            s.cost = ctypes.pointer(c)
            keep += [c, ck]
        return s, keep

    def scenario_check(self, desc, observer_dims="handle"):
        """`lmpc_scenario_check` of a descriptor against this handle's dimensions (host only)."""
        od = getattr(self, "_obs", None) if observer_dims == "handle" else observer_dims
        o = None if od is None else ctypes.byref(Observer(*[int(v) for v in od], None, None, None))
        check(lib().lmpc_scenario_check(self.nth, self.nout, o, ctypes.byref(desc)))

    def simulate_scenario(self, x, T, plant, measurement=None, nd=0, ny=0, r=None, d=None, p=None, noise=None,
                          r_preview=0, d_preview=0, p_preview=0, r_width=0, d_width=None, p_width=0, xhat=None,
                          uprev=None, use_observer=False, warm=False, cost=None, want=("U", "X"), want_cost=False,
                          want_violation=False, stream=None, launch=None, tape=False):
        """The scenario loop (`lmpc_simulate_scenario_device`): torch CUDA tensors in and out, enqueued on `stream`
        (default: torch's current stream), not synchronised.  `launch(desc, N, T, x, xhat, uprev, U, X, flag_min,
        stream)`, all but desc, N, T as ctypes pointers: another entry point taking the same descriptor and arrays
        (ExplicitController.simulate_scenario_device).

        x (N, nx) float64: true states, advanced in place; xhat (N, nx) or None; uprev (N, nuprev) or None (zeros
        when the handle's theta has a uprev block).  plant: nx rows [f_offset, F, G, Gd]; measurement: ny rows
        [h_offset, C, Dd] (host arrays).  r / d / p / noise: (w,), (w, Tc) shared or (N, w, Tc) per scenario, or None
        = zeros of width r_width / d_width (default nd) / p_width; *_preview = Np or 0.  cost: `sim_cost(...)`.
        want: which of "U", "X", "Y", "Ym", "Xhat", "D" to store.  Returns a dict of tensors (step-major, as the C
        side lays them out) plus x, xhat, uprev, flag_min and, if asked for, cost / violation.  tape=True: the taped
        run (`lmpc_simulate_scenario_taped_device`, the same outputs) and out["tape"], what `scenario_vjp` takes."""
        import torch
        f64, dv = torch.float64, self.device
        if not (x.is_cuda and x.dtype == f64 and x.is_contiguous() and x.dim() == 2 and x.device.index == dv):
            raise ValueError("x must be a contiguous float64 CUDA tensor of shape (N, nx) on this handle's GPU")
        N, nx = int(x.shape[0]), int(x.shape[1])
        dev, nu, T = x.device, self.nout, int(T)
        d_width = int(nd) if d_width is None else int(d_width)
        keep = []

        def block(t, w0, H):
            if t is None:
                return Block(None, 0, int(w0), 1, 0, int(H)) if w0 else None
            if t.dim() == 3 and t.shape[0] != N:
                raise ValueError("a per-scenario trajectory must have shape (N, w, T)")
            b, k = self._block(t.to(dev), H, 0)
            keep.append(k)
            return b

        br, bd = block(r, r_width, r_preview), block(d, d_width, d_preview)
        bp, bn = block(p, p_width, p_preview), block(noise, 0, 0)
        nup = self.nth - nx - sum(b.w * (b.H if b.H > 0 else 1) for b in (br, bd, bp) if b is not None)
        if uprev is None and 0 < nup <= nu:
            uprev = torch.zeros((N, nup), dtype=f64, device=dev)
        nup = 0 if uprev is None else int(uprev.shape[1])
        out = dict(x=x, xhat=xhat, uprev=uprev, flag_min=torch.empty(N, dtype=torch.int32, device=dev))
        shapes = dict(U=(T, N, nu), X=(T + 1, N, nx), Y=(T, N, ny), Ym=(T, N, ny), Xhat=(T, N, nx), D=(T, N, nd))
        for k in want:
            out[k] = torch.empty(shapes[k], dtype=f64, device=dev)
        desc, hk = self.scenario_descriptor(plant, nx, nd, measurement, ny, br, bd, bp, bn, nup, use_observer, warm, cost)
        keep.append(hk)
        ptr = lambda t: t.data_ptr() if t is not None else None
        desc.Y_traj, desc.Ym_traj = ptr(out.get("Y")), ptr(out.get("Ym"))
        desc.Xhat_traj, desc.D_traj = ptr(out.get("Xhat")), ptr(out.get("D"))
        if want_cost:
            out["cost"] = torch.empty(N, dtype=f64, device=dev)
            desc.cost_out = out["cost"].data_ptr()
        if want_violation:
            out["violation"] = torch.empty(N, dtype=f64, device=dev)
            desc.violation_out = out["violation"].data_ptr()
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        args = (_vp(x.data_ptr()), _dev_arg(xhat, "xhat", f64, N * nx, dv), _dev_arg(uprev, "uprev", f64, N * nup, dv),
                _vp(ptr(out.get("U"))), _vp(ptr(out.get("X"))), _vp(out["flag_min"].data_ptr()), _vp(st))
        if tape:
            if launch is not None:
                raise ValueError("tape=True is the plain scenario loop's: it cannot be combined with launch=")
            act = torch.empty((T, N, self.words), dtype=torch.int64, device=dev)
            flg = torch.empty((T, N), dtype=torch.int32, device=dev)
            ct = _cabi.ScenarioTape(act.data_ptr(), flg.data_ptr())
            check(lib().lmpc_simulate_scenario_taped_device(self._h, N, T, ctypes.byref(desc), *args[:-1], ctypes.byref(ct),
                                                            args[-1]), self._h)
            out["tape"] = dict(active=act, flag=flg, desc=desc, N=N, T=T, nx=nx, nu=nu, nup=nup,
                               xhat_given=xhat is not None, keep=keep)
        elif launch is not None:
            launch(desc, N, T, *args)
        else:
            check(lib().lmpc_simulate_scenario_device(self._h, N, T, ctypes.byref(desc), *args), self._h)
        out["_keep"] = keep                      # the launches are asynchronous: keep the sources alive
        return out

    SCENARIO_ADJOINT_FIELDS = ("seq", "NX", "grid", "lds", "T", "nprob", "list_pass", "tile")

    def scenario_adjoint_launch_info(self, since=0):
        """The handle's most recent backward sweeps (lmpc_scenario_adjoint_launch_info; at most four are kept), oldest
        first: NX of the scenario_adjoint_kernel instantiation (0: run-time nx), grid, lds, T, nprob, list_pass (1: the
        VJP's wavefront pass was enqueued), tile (entries of a theta-bar record staged at a time)."""
        W = len(self.SCENARIO_ADJOINT_FIELDS)
        out = (ctypes.c_int32 * (4 * W))()
        k = lib().lmpc_scenario_adjoint_launch_info(self._h, out, 4)
        if k < 0:
            check(k, self._h)
        recs = [dict(zip(self.SCENARIO_ADJOINT_FIELDS, (int(v) for v in out[q * W:(q + 1) * W]))) for q in range(k)]
        return [r for r in recs if r["seq"] > since]

    def scenario_vjp(self, tape, Xbar=None, Ubar=None, want=("r", "d", "p"), stream=None):
        """`lmpc_scenario_vjp_device` on the tape of `simulate_scenario(..., tape=True)`: the gradient of
        <Xbar, X> + <Ubar, U> (step-major CUDA tensors (T+1, N, nx) / (T, N, nu), None = zeros) with respect to the run's
        initial values and trajectories.  Enqueued on `stream` (default: torch's current stream), not synchronised.
        Returns a dict of tensors: x0bar (N, nx), xhat0bar (N, nx; only when the run was given an xhat), uprev0bar
        (N, nuprev), status_min (N,) int32 and, for each block of `want` the run's theta has, rbar / dbar / pbar as
        (N, w, Tc) views -- always per scenario: the gradient of a shared trajectory is their sum over scenarios.  With
        use_observer the sweep reads the handle's observer as it stands: it must still be the one the taped run used."""
        import torch
        f64, dv = torch.float64, self.device
        desc, N, T, nx, nu, nup = (tape[k] for k in ("desc", "N", "T", "nx", "nu", "nup"))
        dev = tape["flag"].device
        g = dict(x0bar=torch.empty((N, nx), dtype=f64, device=dev), uprev0bar=torch.empty((N, nup), dtype=f64, device=dev),
                 status_min=torch.empty(N, dtype=torch.int32, device=dev))
        if tape["xhat_given"]:
            g["xhat0bar"] = torch.empty((N, nx), dtype=f64, device=dev)
        raw = {}
        for name in ("r", "d", "p"):
            b = getattr(desc, name)
            if name in want and b.w > 0:
                raw[name] = torch.empty((max(int(b.T), 1), N, int(b.w)), dtype=f64, device=dev)
                g[name + "bar"] = raw[name].permute(1, 2, 0)
        ptr = lambda t: None if t is None else t.data_ptr()
        cg = _cabi.ScenarioGrad(_dev_arg(Xbar, "Xbar", f64, (T + 1) * N * nx, dv), _dev_arg(Ubar, "Ubar", f64, T * N * nu, dv),
                                g["x0bar"].data_ptr(), ptr(g.get("xhat0bar")), g["uprev0bar"].data_ptr(), ptr(raw.get("r")),
                                ptr(raw.get("d")), ptr(raw.get("p")), g["status_min"].data_ptr())
        ct = _cabi.ScenarioTape(tape["active"].data_ptr(), tape["flag"].data_ptr())
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        check(lib().lmpc_scenario_vjp_device(self._h, N, T, ctypes.byref(desc), ctypes.byref(ct), ctypes.byref(cg), _vp(st)),
              self._h)
        return g

    def simulate_scenario_autograd(self, x, T, plant, r=None, d=None, p=None, uprev=None, **kw):
        """The scenario loop inside a torch graph: returns (X, U, flag_min) -- X (T+1, N, nx) and U (T, N, nu) carry the
        gradient to whichever of x, uprev, r, d, p require it (forward: the taped run on copies of x and uprev; backward:
        ONE `scenario_vjp` on the current torch stream; a shared block's gradient is the per-scenario one summed over
        scenarios), flag_min is marked non-differentiable.  The `status_min` of the most recent backward is
        `X.grad_fn.status_min`.  kw: the other arguments of `simulate_scenario` (want / tape / launch excluded).  With no
        input requiring grad this is the plain call on copies of x and uprev, and no tape is allocated."""
        import torch
        ins = (x, uprev, r, d, p)
        if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ins)):
            out = self.simulate_scenario(x.detach().clone(), T, plant, r=r, d=d, p=p,
                                         uprev=None if uprev is None else uprev.detach().clone(), want=("U", "X"), **kw)
            return out["X"], out["U"], out["flag_min"]
        return _scenario_fn().apply(self, T, plant, kw, x, uprev, r, d, p)

    def uncertainty(self, N, nx, process=None, measurement_noise=None, Gw=None, seed=0, scenario_offset=0, step_offset=0,
                    plants=None, plant_index=None, W=None):
        """`lmpc_uncertainty` from its parts.  process / measurement_noise: None, an object with `lo` and `hi` (drawn on
        the device: uniform in the box, or, with `dist == 1`, Gaussian with means lo and standard deviations hi) or a CUDA tensor (w, Tc) shared / (N, w, Tc) per scenario (supplied draws).
        Gw (nx, nw) host array or None.  plants: (n_plants, nx, 1 + nx + nu + nd) host array or None; plant_index: int32
        CUDA tensor (N,) or None.  W: the (T, N, nx) CUDA tensor that takes W_traj, or None.  Returns (struct, keep-alive)."""
        un, keep = _cabi.Uncertainty(), []

        def source(dst, a):
            if a is None:
                return
            if hasattr(a, "lo") and hasattr(a, "hi"):
                lo, hi = _f64(np.asarray(a.lo, float).reshape(-1)), _f64(np.asarray(a.hi, float).reshape(-1))
                if lo.shape != hi.shape:
                    raise ValueError("lo and hi of a drawn noise source must have the same length")
                dst.w, dst.dist, dst.lo, dst.hi = lo.size, int(getattr(a, "dist", 0)), lo.ctypes.data, hi.ctypes.data
                keep.extend([lo, hi])
                return
            if a.dim() == 3 and a.shape[0] != N:
                raise ValueError("a per-scenario noise block must have shape (N, w, T)")
            b, k = self._block(a, 0, 0)
            dst.w, dst.src = b.w, b
            keep.append(k)

        source(un.process, process)
        source(un.measurement, measurement_noise)
        if Gw is not None:
            g = _f64(np.asarray(Gw, float).reshape(nx, -1))
            if g.shape[1] != un.process.w:
                raise ValueError(f"Gw must have shape ({nx}, {un.process.w}), got {g.shape}")
            un.Gw = g.ctypes.data
            keep.append(g)
        un.seed, un.scenario_offset, un.step_offset = int(seed), int(scenario_offset), int(step_offset)
        if plants is not None:
            tab = _f64(np.asarray(plants, float))
            if tab.ndim != 3 or tab.shape[1] != nx:
                raise ValueError("plants must have shape (n_plants, nx, 1 + nx + nu + nd)")
            un.n_plants, un.plants = tab.shape[0], tab.ctypes.data
            keep.append(tab)
        if plant_index is not None:
            import torch
            un.plant_index = _dev_arg(plant_index, "plant_index", torch.int32, N, self.device, False).value
            keep.append(plant_index)
        if W is not None:
            un.W_traj = W.data_ptr()
        return un, keep

    @staticmethod
    def _drawn_source(source):
        """`lmpc_noise` of an object with `lo` and `hi` (and `dist`): (struct, keep-alive)"""
        lo, hi = _f64(np.asarray(source.lo, float).reshape(-1)), _f64(np.asarray(source.hi, float).reshape(-1))
        if lo.shape != hi.shape:
            raise ValueError("lo and hi of a drawn noise source must have the same length")
        n = _cabi.Noise()
        n.w, n.dist, n.lo, n.hi = lo.size, int(getattr(source, "dist", 0)), lo.ctypes.data, hi.ctypes.data
        return n, (lo, hi)

    @staticmethod
    def noise_draw_host(source, N, T, seed=0, stream=0, scenario_offset=0, step_offset=0):
        """`lmpc_noise_draw_host`: the draws of a `Uniform` / `Gaussian` source on the CPU as a numpy array (N, w, T), a
        view of the (N, T, w) buffer the C side fills.  Needs no GPU and no handle."""
        n, keep = BatchedQP._drawn_source(source)
        out = np.empty((int(N), int(T), n.w))
        check(lib().lmpc_noise_draw_host(ctypes.byref(n), int(seed) & (2 ** 64 - 1), int(stream), int(scenario_offset), int(N),
                                         int(step_offset), int(T), _vp(out.ctypes.data)))
        return out.transpose(0, 2, 1)

    def noise_draw(self, source, N, T, seed=0, stream=0, scenario_offset=0, step_offset=0, noise_stream=None):
        """`lmpc_noise_draw_device`: the same draws made on this handle's GPU, one kernel, enqueued on `noise_stream`
        (default: torch's current stream), not synchronised.  Returns a CUDA tensor (N, w, T), a view of the contiguous
        (N, T, w) buffer: given back as `process=` / `measurement_noise=` it is the supplied block without a copy."""
        import torch
        n, keep = self._drawn_source(source)
        dev = torch.device("cuda", self.device)
        out = torch.empty((int(N), int(T), n.w), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if noise_stream is None else noise_stream
        check(lib().lmpc_noise_draw_device(self._h, ctypes.byref(n), int(seed) & (2 ** 64 - 1), int(stream), int(scenario_offset),
                                           int(N), int(step_offset), int(T), _vp(out.data_ptr()), _vp(st)), self._h)
        return out.transpose(1, 2)

    def uncertain_check(self, desc, un, observer_dims="handle"):
        """`lmpc_scenario_uncertain_check` of a descriptor and an uncertainty against this handle's dimensions (host only)."""
        od = getattr(self, "_obs", None) if observer_dims == "handle" else observer_dims
        o = None if od is None else ctypes.byref(Observer(*[int(v) for v in od], None, None, None))
        check(lib().lmpc_scenario_uncertain_check(self.nth, self.nout, o, ctypes.byref(desc), ctypes.byref(un)))

    def simulate_scenario_uncertain(self, x, T, plant, measurement=None, *, process=None, measurement_noise=None, Gw=None,
                                    seed=0, scenario_offset=0, step_offset=0, plants=None, plant_index=None,
                                    want=("U", "X"), **kw):
        """The scenario loop under uncertainty (`lmpc_simulate_scenario_uncertain_device`): `simulate_scenario` with
        additive process noise w_k = Gw e_k on the state, additive measurement noise and a table of plant variants
        (`uncertainty` says how each is given; `plant` stays the descriptor's plant and steps everyone without
        `plants`).  A drawn source is uniform in a box (`Uniform`) or Gaussian (`Gaussian`).
        want may name "W" (T, N, nx), the w_k that acted.  Everything else, and the dict returned, as `simulate_scenario`."""
        import torch
        N, nx = int(x.shape[0]), int(x.shape[1])
        W = torch.empty((int(T), N, nx), dtype=torch.float64, device=x.device) if "W" in want else None
        un, keep = self.uncertainty(N, nx, process, measurement_noise, Gw, seed, scenario_offset, step_offset, plants,
                                    plant_index, W)

        def launch(desc, n, t, *args):
            check(lib().lmpc_simulate_scenario_uncertain_device(self._h, n, t, ctypes.byref(desc), ctypes.byref(un), *args), self._h)

        out = self.simulate_scenario(x, T, plant, measurement, want=tuple(k for k in want if k != "W"), launch=launch, **kw)
        if W is not None:
            out["W"] = W
        out["_keep"].append(keep)
        return out

    def _plant_params(self, plant, params, N, dev):
        """q of a `NonlinearPlant` run as (CUDA tensor or None, q_shared): (nq,) shared by all, (N, nq) per scenario"""
        import torch
        if plant.nq == 0:
            return None, 1
        if params is None:
            raise ValueError(f"the plant has nq = {plant.nq} parameters: params is required")
        q = params if isinstance(params, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(params, float)))
        q = q.to(dev, torch.float64).contiguous()
        if tuple(q.shape) not in ((plant.nq,), (N, plant.nq)):
            raise ValueError(f"params must have shape ({plant.nq},) or ({N}, {plant.nq}), got {tuple(q.shape)}")
        return q, int(q.dim() == 1)

    def plant_program_eval_device(self, plant, x, u=None, d=None, params=None, stream=None):
        """`lmpc_plant_program_eval_device`: one step of a `NonlinearPlant` on CUDA tensors x (N, nx), u (N, nu),
        d (N, nd); returns x+ (N, nx), enqueued on `stream` (default: torch's current stream), not synchronised."""
        import torch
        f64, dv = torch.float64, self.device
        N, dev = int(x.shape[0]), x.device
        q, shared = self._plant_params(plant, params, N, dev)
        out = torch.empty((N, plant.nx), dtype=f64, device=dev)
        p, keep = plant.program()
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        check(lib().lmpc_plant_program_eval_device(
            self._h, ctypes.byref(p), N, _dev_arg(x, "x", f64, N * plant.nx, dv, False), _dev_arg(u, "u", f64, N * plant.nu, dv),
            _dev_arg(d, "d", f64, N * plant.nd, dv), _dev_arg(q, "params", f64, q.numel() if q is not None else 0, dv), shared,
            _vp(out.data_ptr()), _vp(st)), self._h)
        return out

    def simulate_scenario_nonlinear(self, x, T, plant, *, params=None, process=None, measurement_noise=None, Gw=None,
                                    seed=0, scenario_offset=0, step_offset=0, want=("U", "X"), **kw):
        """The scenario loop with a nonlinear true plant (`lmpc_simulate_scenario_nonlinear_device`):
        `simulate_scenario_uncertain` with the plant's row sums replaced by the program of `plant`, a `NonlinearPlant`
        (its linear measurement rows are the descriptor's).  params: its q, (nq,) shared or (N, nq) per scenario, a
        host array or a CUDA tensor.  No plant table.  Everything else as `simulate_scenario_uncertain`."""
        import torch
        N, nx = int(x.shape[0]), int(x.shape[1])
        if nx != plant.nx:
            raise ValueError(f"x has {nx} columns, the plant nx = {plant.nx}")
        W = torch.empty((int(T), N, nx), dtype=torch.float64, device=x.device) if "W" in want else None
        un, keep = self.uncertainty(N, nx, process, measurement_noise, Gw, seed, scenario_offset, step_offset, None, None, W)
        q, shared = self._plant_params(plant, params, N, x.device)
        p, pkeep = plant.program()

        def launch(desc, n, t, *args):
            desc.plant = None                         # ignored by this loop
            check(lib().lmpc_simulate_scenario_nonlinear_device(
                self._h, n, t, ctypes.byref(desc), ctypes.byref(un), ctypes.byref(p), _vp(q.data_ptr() if q is not None else None),
                shared, *args), self._h)

        kw.setdefault("nd", plant.nd)
        kw.setdefault("ny", plant.ny)
        out = self.simulate_scenario(x, T, np.zeros(1), plant.measurement_rows(), want=tuple(k for k in want if k != "W"),
                                     launch=launch, **kw)
        if W is not None:
            out["W"] = W
        out["_keep"].append([keep, pkeep, q])
        return out

    def offset_free_check(self, desc, n_offset_free, observer_dims="handle"):
        """`lmpc_scenario_offset_free_check` of a descriptor against this handle's dimensions (host only)."""
        od = getattr(self, "_obs", None) if observer_dims == "handle" else observer_dims
        o = None if od is None else ctypes.byref(Observer(*[int(v) for v in od], None, None, None))
        of = _cabi.OffsetFree(int(n_offset_free), None)
        check(lib().lmpc_scenario_offset_free_check(self.nth, self.nout, o, ctypes.byref(desc), ctypes.byref(of)))

    def simulate_scenario_offset_free(self, x, T, plant, measurement, n_offset_free, nd=0, ny=0, r=None, d=None, p=None,
                                      noise=None, r_preview=0, d_preview=0, p_preview=0, r_width=0, p_width=0, xaug=None,
                                      uprev=None, warm=False, cost=None, want=("U", "X"), want_cost=False,
                                      want_violation=False, stream=None):
        """The scenario loop with the offset-free observer (`lmpc_simulate_scenario_offset_free_device`): as
        `simulate_scenario`, with the handle's observer (`set_observer`, the AUGMENTED filter of nx + n_offset_free
        states) always in the loop.  nd: the MEASURED disturbances (rows of d, columns of the plant's Gd / Dd); the
        d block of theta is max(d_preview, 1) columns [d; dhat].  xaug (N, nx + n_offset_free) or None = [x; 0].
        want: any of "U", "X", "Y", "Ym", "Xhat", "D", "Dhat".  Returns the dict of `simulate_scenario` plus xaug."""
        import torch
        f64, dv = torch.float64, self.device
        if not (x.is_cuda and x.dtype == f64 and x.is_contiguous() and x.dim() == 2 and x.device.index == dv):
            raise ValueError("x must be a contiguous float64 CUDA tensor of shape (N, nx) on this handle's GPU")
        N, nx = int(x.shape[0]), int(x.shape[1])
        dev, nu, T, ndo = x.device, self.nout, int(T), int(n_offset_free)
        keep = []

        def block(t, w0, H):
            if t is None:
                return Block(None, 0, int(w0), 1, 0, int(H)) if (w0 or H) else None
            if t.dim() == 3 and t.shape[0] != N:
                raise ValueError("a per-scenario trajectory must have shape (N, w, T)")
            b, k = self._block(t.to(dev), H, 0)
            keep.append(k)
            return b

        br, bd = block(r, r_width, r_preview), block(d, 0, d_preview)       # no d: width 0, the preview length kept
        bp, bn = block(p, p_width, p_preview), block(noise, 0, 0)
        wid = lambda b: 0 if b is None else b.w * (b.H if b.H > 0 else 1)
        nup = self.nth - nx - wid(br) - (int(nd) + ndo) * max(int(d_preview), 1) - wid(bp)
        if uprev is None and 0 < nup <= nu:
            uprev = torch.zeros((N, nup), dtype=f64, device=dev)
        nup = 0 if uprev is None else int(uprev.shape[1])
        out = dict(x=x, xaug=xaug, uprev=uprev, flag_min=torch.empty(N, dtype=torch.int32, device=dev))
        shapes = dict(U=(T, N, nu), X=(T + 1, N, nx), Y=(T, N, ny), Ym=(T, N, ny), Xhat=(T, N, nx), D=(T, N, nd),
                      Dhat=(T, N, ndo))
        for k in want:
            out[k] = torch.empty(shapes[k], dtype=f64, device=dev)
        desc, hk = self.scenario_descriptor(plant, nx, nd, measurement, ny, br, bd, bp, bn, nup, True, warm, cost)
        keep.append(hk)
        ptr = lambda t: t.data_ptr() if t is not None else None
        desc.Y_traj, desc.Ym_traj = ptr(out.get("Y")), ptr(out.get("Ym"))
        desc.Xhat_traj, desc.D_traj = ptr(out.get("Xhat")), ptr(out.get("D"))
        of = _cabi.OffsetFree(ndo, ptr(out.get("Dhat")))
        if want_cost:
            out["cost"] = torch.empty(N, dtype=f64, device=dev)
            desc.cost_out = out["cost"].data_ptr()
        if want_violation:
            out["violation"] = torch.empty(N, dtype=f64, device=dev)
            desc.violation_out = out["violation"].data_ptr()
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        check(lib().lmpc_simulate_scenario_offset_free_device(
            self._h, N, T, ctypes.byref(desc), ctypes.byref(of), _vp(x.data_ptr()),
            _dev_arg(xaug, "xaug", f64, N * (nx + ndo), dv), _dev_arg(uprev, "uprev", f64, N * nup, dv),
            _vp(ptr(out.get("U"))), _vp(ptr(out.get("X"))), _vp(out["flag_min"].data_ptr()), _vp(st)), self._h)
        out["_keep"] = keep                      # the launches are asynchronous: keep the sources alive
        return out

    def evaluate_cost_device(self, X, U, cost, r=None, stream=None):
        """`lmpc_evaluate_cost_device`: X (>= T, N, nx) and U (T, N, nu) step-major CUDA tensors, cost =
        `sim_cost(...)`, r as in `simulate_scenario`.  Returns the (N,) cost tensor (not synchronised)."""
        import torch
        T, N, nu = (int(v) for v in U.shape)
        nx = int(X.shape[2])
        c, ck = cost
        br, kr = self._block(r, 0, 0)
        out = torch.empty(N, dtype=torch.float64, device=U.device)
        st = torch.cuda.current_stream(U.device).cuda_stream if stream is None else stream
        check(lib().lmpc_evaluate_cost_device(
            self._h, N, T, nx, nu, ctypes.byref(c), _dev_arg(X[:T], "X", torch.float64, T * N * nx, self.device, False),
            _dev_arg(U, "U", torch.float64, T * N * nu, self.device, False),
            ctypes.byref(br) if br is not None else None, _vp(out.data_ptr()), _vp(st)), self._h)
        out._lmpc_keep = (kr, ck)
        return out

    def constraint_violation_device(self, X, U, rows, per_step=False, stream=None):
        """`lmpc_constraint_violation_device`: worst violation per scenario (N,), or per step (T, N)."""
        import torch
        T, N, nu = (int(v) for v in U.shape)
        nx = int(X.shape[2])
        c, ck = rows
        out = torch.empty((T, N) if per_step else (N,), dtype=torch.float64, device=U.device)
        st = torch.cuda.current_stream(U.device).cuda_stream if stream is None else stream
        check(lib().lmpc_constraint_violation_device(
            self._h, N, T, nx, nu, ctypes.byref(c), _dev_arg(X[:T], "X", torch.float64, T * N * nx, self.device, False),
            _dev_arg(U, "U", torch.float64, T * N * nu, self.device, False),
            None if per_step else _vp(out.data_ptr()), _vp(out.data_ptr()) if per_step else None, _vp(st)), self._h)
        out._lmpc_keep = ck
        return out

    # ------------------------------------------------------------------ generated-controller entry point
    def set_parameter_layout(self, nx, nr=0, nd=0, nuprev=0, np_=0, preview_horizon=0, traj2setpoint=None):
        """`lmpc_set_parameter_layout`: N_STATE, N_REFERENCE, N_DISTURBANCE, N_CONTROL_PREV,
        N_AFFINE_PARAMETER of the generated header (reference codegen.jl:154-165); with reference
        condensation N_PREVIEW_HORIZON and mpc.traj2setpoint (nr x nr*Np; passed as the generator
        writes it, column by column)."""
        t2s = None
        if preview_horizon:
            t2s = _f64(np.asarray(traj2setpoint, float).reshape(nr, nr * preview_horizon), "F")
        lay = ParamLayout(int(nx), int(nr), int(nd), int(nuprev), int(np_), int(preview_horizon),
                          t2s.ctypes.data if t2s is not None else None)
        check(lib().lmpc_set_parameter_layout(self._h, ctypes.byref(lay)), self._h)
        self._layout = (int(nx), int(nr), int(nd), int(nuprev), int(np_), int(preview_horizon))

    def compute_control(self, control, state, reference=None, disturbance=None, affine_parameter=None, warm=False):
        """`lmpc_compute_control`: the generated `mpc_compute_control(control, state, reference,
        disturbance[, affine_parameter])` (reference codegen/mpc_update_qp.c:29-54) for N problems.
        `control` (N x nu) is read (previous control) and overwritten (u*), as in the C function;
        returns the exit flags."""
        nx, nr, nd, nup, npp, nph = self._layout
        if not (isinstance(control, np.ndarray) and control.dtype == np.float64 and control.flags.c_contiguous
                and control.flags.writeable):
            raise TypeError("control must be a writeable C-contiguous float64 array (it is updated in place)")
        N = control.size // self.nout if self.nout else 0
        control = control.reshape(N, self.nout)

        def arr(a, w):
            if a is None or w == 0:
                return None
            return _f64(np.asarray(a, float).reshape(N, w))

        st, rf = arr(state, nx), arr(reference, nr * (nph if nph else 1))
        ds, pr = arr(disturbance, nd), arr(affine_parameter, npp)
        ef = np.empty(N, np.int32)
        check(lib().lmpc_compute_control(self._h, N, _ptr(control), _ptr(st), _ptr(rf) if rf is not None else None,
                                         _ptr(ds) if ds is not None else None, _ptr(pr) if pr is not None else None,
                                         _ptr(ef), int(bool(warm))), self._h)
        return ef

    def compute_control_device(self, control, state, reference=None, disturbance=None, affine_parameter=None,
                               exitflag=None, warm=False, stream=None):
        """`lmpc_compute_control_device`: CUDA tensors in place, enqueued on the current (or given) stream."""
        import torch
        nx, nr, nd, nup, npp, nph = self._layout
        N = int(control.shape[0])
        dev = control.device
        if exitflag is None:
            exitflag = torch.empty(N, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        f64, d = torch.float64, self.device
        check(lib().lmpc_compute_control_device(
            self._h, N, _dev_arg(control, "control", f64, N * self.nout, d, False),
            _dev_arg(state, "state", f64, N * nx, d, nx == 0),
            _dev_arg(reference, "reference", f64, N * nr * (nph if nph else 1), d),
            _dev_arg(disturbance, "disturbance", f64, N * nd, d),
            _dev_arg(affine_parameter, "affine_parameter", f64, N * npp, d),
            _dev_arg(exitflag, "exitflag", torch.int32, N, d, False), int(bool(warm)), _vp(st)), self._h)
        return exitflag

    def compute_control_observer_device(self, control, observer_state, n_measured=0, reference=None,
                                        measured_disturbance=None, affine_parameter=None, exitflag=None,
                                        warm=False, stream=None):
        """`lmpc_compute_control_observer_device`: generated `mpc_compute_control_observer` of an offset-free
        observer for N scenarios (CUDA tensors; control in place)."""
        import torch
        nx, nr, nd, nup, npp, nph = self._layout
        N = int(control.shape[0])
        dev = control.device
        if exitflag is None:
            exitflag = torch.empty(N, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        f64, d = torch.float64, self.device
        nm = int(n_measured)
        check(lib().lmpc_compute_control_observer_device(
            self._h, N, _dev_arg(control, "control", f64, N * self.nout, d, False),
            _dev_arg(observer_state, "observer_state", f64, N * (nx + nd - nm), d, False), nm,
            _dev_arg(reference, "reference", f64, N * nr * (nph if nph else 1), d),
            _dev_arg(measured_disturbance, "measured_disturbance", f64, N * nm, d),
            _dev_arg(affine_parameter, "affine_parameter", f64, N * npp, d),
            _dev_arg(exitflag, "exitflag", torch.int32, N, d, False), int(bool(warm)), _vp(st)), self._h)
        return exitflag

    # ------------------------------------------------------------------ generated state observer
    def set_observer(self, plant_dynamics, measurement_function, k_transpose, nx, nu, nd, ny):
        """`lmpc_set_observer`: MPC_PLANT_DYNAMICS, MPC_MEASUREMENT_FUNCTION, K_TRANSPOSE_OBSERVER as the
        reference's code generator writes them (src/observer.jl:124-141)."""
        dyn = _f64(np.asarray(plant_dynamics, float).reshape(-1))
        mea = _f64(np.asarray(measurement_function, float).reshape(-1))
        kt = _f64(np.asarray(k_transpose, float).reshape(-1))
        assert dyn.size == nx * (1 + nx + nu + nd) and mea.size == ny * (1 + nx + nd) and kt.size == ny * nx
        o = Observer(int(nx), int(nu), int(nd), int(ny), dyn.ctypes.data, mea.ctypes.data, kt.ctypes.data)
        check(lib().lmpc_set_observer(self._h, ctypes.byref(o)), self._h)
        self._obs = (int(nx), int(nu), int(nd), int(ny))

    def _observer_call(self, fn_host, fn_dev, state, other, w_other, disturbance, stream):
        if getattr(self, "_obs", None) is None:           # the library says so (LMPC_ERR_BADARG)
            check(fn_host(self._h, 1, None, None, None), self._h)
        nx, nu, nd, ny = self._obs
        if isinstance(state, np.ndarray):
            if not (state.dtype == np.float64 and state.flags.c_contiguous and state.flags.writeable):
                raise TypeError("state must be a writeable C-contiguous float64 array (it is updated in place)")
            N = state.size // nx
            w_other = self._obs[w_other]                  # index into (nx, nu, nd, ny): control or measurement width
            oth = _f64(np.asarray(other, float).reshape(N, w_other)) if w_other else None
            dd = _f64(np.asarray(disturbance, float).reshape(N, nd)) if (disturbance is not None and nd) else None
            check(fn_host(self._h, N, _ptr(state), _ptr(oth) if oth is not None else None,
                          _ptr(dd) if dd is not None else None), self._h)
            return state
        import torch
        N = int(state.shape[0])
        st = torch.cuda.current_stream(state.device).cuda_stream if stream is None else stream
        p = lambda t: _vp(t.data_ptr()) if t is not None else None
        check(fn_dev(self._h, N, p(state), p(other), p(disturbance), _vp(st)), self._h)
        return state

    def predict_state(self, state, control, disturbance=None, stream=None):
        """`lmpc_predict_state[_device]` = generated mpc_predict_state for N scenarios; `state` (N x nx,
        numpy or CUDA tensor) is updated in place."""
        return self._observer_call(lib().lmpc_predict_state, lib().lmpc_predict_state_device, state, control,
                                   1, disturbance, stream)

    def correct_state(self, state, measurement, disturbance=None, stream=None):
        """`lmpc_correct_state[_device]` = generated mpc_correct_state for N scenarios, in place."""
        return self._observer_call(lib().lmpc_correct_state, lib().lmpc_correct_state_device, state, measurement,
                                   3, disturbance, stream)

    # ------------------------------------------------------------------ profiling
    def profile(self, enable=True):
        check(lib().lmpc_profile(self._h, int(bool(enable))), self._h)

    def profile_read(self):
        """(launches, avg ms whole call, avg ms screening kernel, avg ms iterating kernel) since the
        last read; HIP events recorded on the launch stream."""
        ms = (ctypes.c_double * 3)()
        cnt = lib().lmpc_profile_read(self._h, ctypes.byref(ms))
        return cnt, ms[0], ms[1], ms[2]

    def reserve(self, n, stream=None):
        """`lmpc_reserve`: allocate now what the first device call on a batch of n problems would allocate lazily."""
        lib().lmpc_reserve.argtypes = [_vp, ctypes.c_int64, _vp]
        lib().lmpc_reserve.restype = ctypes.c_int
        check(lib().lmpc_reserve(self._h, int(n), _vp(int(stream)) if stream else None), self._h)

    def release_scratch(self):
        """`lmpc_release_scratch`: give the staging / scratch buffers back (they grow with the largest batch)."""
        check(lib().lmpc_release_scratch(self._h), self._h)

    def set_option(self, name: str, value: int):
        check(lib().lmpc_set_option(self._h, name.encode(), int(value)), self._h)

    def distinct_active_sets_device(self, active, exitflag=None, capacity=65536, stream=None):
        """`lmpc_distinct_active_sets_device`: the distinct rows of a solved batch's `active` tensor (N x words int64
        CUDA tensor, as `solve_device(..., active=...)` fills it), reduced ON the device; only the distinct sets come
        back.  Returns (masks (R x words uint64), counts (R), first_index (R)) as numpy arrays sorted by decreasing
        count, ties by first index -- the order `explicit.unique_active_sets` gives."""
        import torch
        dev = active.device
        N = int(active.shape[0])
        if not (active.is_cuda and active.is_contiguous() and active.dtype in _mask_dtypes() and
                active.numel() == N * self.words):
            raise ValueError("active must be a contiguous (N, words) 64-bit integer CUDA tensor")
        if exitflag is not None and not (exitflag.is_cuda and exitflag.dtype == torch.int32 and exitflag.numel() == N):
            raise ValueError("exitflag must be an int32 CUDA tensor of length N")
        st = 0 if stream is None else int(stream)
        while True:
            masks = torch.empty((capacity, self.words), dtype=torch.int64, device=dev)
            counts = torch.empty(capacity, dtype=torch.int64, device=dev)
            first = torch.empty(capacity, dtype=torch.int64, device=dev)
            nset = torch.zeros(1, dtype=torch.int32, device=dev)
            torch.cuda.current_stream(dev).synchronize()         # (buffers above come from torch's stream)
            check(lib().lmpc_distinct_active_sets_device(
                self._h, N, _vp(active.data_ptr()), _vp(exitflag.data_ptr()) if exitflag is not None else None,
                int(capacity), _vp(masks.data_ptr()), _vp(counts.data_ptr()), _vp(first.data_ptr()),
                _vp(nset.data_ptr()), _vp(st) if st else None), self._h)
            over = lib().lmpc_distinct_active_sets_overflowed(self._h, _vp(st) if st else None)
            if over < 0:
                check(over, self._h)
            if over == 0:
                break
            if over == 2:
                raise LmpcError(-102, "lmpc_distinct_active_sets_device: table slot never published")
            capacity *= 4                                        # more regions than room: once more with more
        R = int(nset.item())
        m = masks[:R].cpu().numpy().view(np.uint64)
        c = counts[:R].cpu().numpy()
        f = first[:R].cpu().numpy()
        order = np.lexsort((f, -c))
        return m[order], c[order], f[order]

    # ------------------------------------------------------------------ differentiable solve
    SENS_LAUNCH_FIELDS = ("seq", "jac", "CAP", "cap", "grid", "block", "lds", "staged", "list_pass", "wave_grid", "wave_lds",
                          "nprob")
    SENS_DONE, SENS_FAILED_POINT, SENS_SINGULAR, SENS_TOO_MANY = 1, 0, -1, -7

    def sens_launch_info(self, since=0):
        """The handle's most recent derivative calls (lmpc_sens_launch_info; at most four are kept), oldest first: one
        dict per call with jac (1 Jacobian, 0 VJP), the template argument CAP of the sens_lane_kernel instantiation, the
        capacity it ran with (0: forced list pass), grid, block, lds, staged (bit 0: the derived pack in LDS, bit 1: the
        results leave through LDS as whole lines), list_pass (1: sens_wave_kernel was enqueued
        behind it), that kernel's grid and lds, nprob.  "seq" and `since` as in wave_launch_info."""
        W = len(self.SENS_LAUNCH_FIELDS)
        out = (ctypes.c_int32 * (4 * W))()
        k = lib().lmpc_sens_launch_info(self._h, out, 4)
        if k < 0:
            check(k, self._h)
        recs = [dict(zip(self.SENS_LAUNCH_FIELDS, (int(v) for v in out[q * W:(q + 1) * W]))) for q in range(k)]
        return [r for r in recs if r["seq"] > since]

    def _sens_device_args(self, active, exitflag, status):
        import torch
        if active is None or active.dtype not in _mask_dtypes() or active.dim() != 2 or active.shape[1] != self.words:
            raise ValueError(f"active must be a 64-bit integer CUDA tensor of shape (N, {self.words})")
        N = int(active.shape[0])
        dev = active.device
        if status is None:
            status = torch.empty(N, dtype=torch.int32, device=dev)
        return (N, dev, _dev_arg(active, "active", active.dtype, N * self.words, self.device, False),
                _dev_arg(exitflag, "exitflag", torch.int32, N, self.device, False), status,
                _dev_arg(status, "status", torch.int32, N, self.device, False))

    def solve_vjp_device(self, active, exitflag, xbar, thbar=None, status=None, stream=None):
        """`lmpc_solve_vjp_device`: thbar = (dx*/dtheta)' xbar per point from the solve's `active` masks and exit flags
        (CUDA tensors; xbar (N, nout) float64).  Enqueued on `stream` (default: torch's current stream), not
        synchronised.  Returns (thbar (N, nth), status (N,) int32: 1 done, 0 failed point, -1 singular, -7 beyond 64 rows)."""
        import torch
        N, dev, pa, pf, status, ps = self._sens_device_args(active, exitflag, status)
        if thbar is None:
            thbar = torch.empty((N, self.nth), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        check(lib().lmpc_solve_vjp_device(
            self._h, N, pa, pf, _dev_arg(xbar, "xbar", torch.float64, N * self.nout, self.device, False),
            _dev_arg(thbar, "thbar", torch.float64, N * self.nth, self.device, False), ps, _vp(st)), self._h)
        return thbar, status

    def solve_jacobian_device(self, active, exitflag, J=None, status=None, stream=None):
        """`lmpc_solve_jacobian_device`: J = dx*/dtheta per point, (N, nout, nth); arguments and status as
        `solve_vjp_device`."""
        import torch
        N, dev, pa, pf, status, ps = self._sens_device_args(active, exitflag, status)
        if J is None:
            J = torch.empty((N, self.nout, self.nth), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        check(lib().lmpc_solve_jacobian_device(
            self._h, N, pa, pf, _dev_arg(J, "J", torch.float64, N * self.nout * self.nth, self.device, False), ps, _vp(st)),
            self._h)
        return J, status

    def solve_vjp(self, active, exitflag, xbar):
        """Host arrays in and out (`lmpc_solve_vjp`; synchronous): (thbar, status)."""
        act = np.ascontiguousarray(np.asarray(active, np.uint64).reshape(-1, self.words))
        N = act.shape[0]
        ef = np.ascontiguousarray(np.asarray(exitflag, np.int32).reshape(N))
        xb = _f64(np.asarray(xbar, float).reshape(N, self.nout))
        out, status = np.zeros((N, self.nth)), np.zeros(N, np.int32)
        check(lib().lmpc_solve_vjp(self._h, N, _ptr(act), _ptr(ef), _ptr(xb), _ptr(out), _ptr(status)), self._h)
        return out, status

    def solve_jacobian(self, active, exitflag):
        """Host arrays in and out (`lmpc_solve_jacobian`; synchronous): (J (N, nout, nth), status)."""
        act = np.ascontiguousarray(np.asarray(active, np.uint64).reshape(-1, self.words))
        N = act.shape[0]
        ef = np.ascontiguousarray(np.asarray(exitflag, np.int32).reshape(N))
        out, status = np.zeros((N, self.nout, self.nth)), np.zeros(N, np.int32)
        check(lib().lmpc_solve_jacobian(self._h, N, _ptr(act), _ptr(ef), _ptr(out), _ptr(status)), self._h)
        return out, status

    # ------------------------------------------------------------------ gradient with respect to the pack
    PACK_GRAD_LAUNCH_FIELDS = ("seq", "CAP", "cap", "grid", "lds", "staged", "list_pass", "wave_grid", "reduce_grid",
                               "reduce_lds", "slab", "slabs", "tree_launches", "scratch_kib", "doubles", "nprob", "reduce_chunks")

    def pack_grad_launch_info(self, since=0):
        """The handle's most recent pack-gradient calls (lmpc_pack_grad_launch_info; at most four are kept), oldest
        first: CAP / cap of the pack_grad_lane_kernel, its grid on the first slab and LDS bytes, staged (bit 0: the derived
        pack in the lane kernel's LDS, bit 1: M and Rout in the reduce kernel's), list_pass and wave_grid of
        pack_grad_wave_kernel, the reduce kernel's grid and LDS bytes, slab (log2 of its points), slabs, the tree
        kernel's launches, the scratch in KiB, the doubles of one partial, nprob, reduce_chunks (the column chunks of M
        the reduce kernel's grid was split into on the first slab)."""
        W = len(self.PACK_GRAD_LAUNCH_FIELDS)
        out = (ctypes.c_int32 * (4 * W))()
        k = lib().lmpc_pack_grad_launch_info(self._h, out, 4)
        if k < 0:
            check(k, self._h)
        recs = [dict(zip(self.PACK_GRAD_LAUNCH_FIELDS, (int(v) for v in out[q * W:(q + 1) * W]))) for q in range(k)]
        return [r for r in recs if r["seq"] > since]

    def solve_pack_vjp_device(self, theta, active, exitflag, xbar, want_thbar=False, status=None, stream=None, out=None,
                              want=PACK_BARS, thbar=None):
        """`lmpc_solve_pack_vjp_device`: the gradient of sum_p <xbar_p, x*_p> with respect to the pack, summed over the
        batch (CUDA tensors; theta (N, nth), xbar (N, nout) float64).  Enqueued on `stream` (default: torch's current
        stream), not synchronised.  Returns a dict of device tensors M, du, dl, Dth, Rout, x0, Xth (those named in `want`;
        `out` may hold preallocated ones), status, and thbar (N, nth) with `want_thbar` (or a preallocated `thbar`)."""
        import torch
        N, dev, pa, pf, status, ps = self._sens_device_args(active, exitflag, status)
        shapes = _pack_bar_shapes(self.n, self.m, self.nth, self.nout)
        res = {}
        for k in PACK_BARS:
            if k in want:
                t = None if out is None else out.get(k)
                res[k] = torch.empty(shapes[k], dtype=torch.float64, device=dev) if t is None else t
        ptrs = [_dev_arg(res.get(k), k + "bar", torch.float64, int(np.prod(shapes[k])), self.device) if res.get(k) is not None
                and res[k].numel() else None for k in PACK_BARS]
        if thbar is None and want_thbar:
            thbar = torch.empty((N, self.nth), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        check(lib().lmpc_solve_pack_vjp_device(
            self._h, N, _dev_arg(theta, "theta", torch.float64, N * self.nth, self.device, False), pa, pf,
            _dev_arg(xbar, "xbar", torch.float64, N * self.nout, self.device, False), *ptrs,
            _dev_arg(thbar, "thbar", torch.float64, N * self.nth, self.device), ps, _vp(st)), self._h)
        res["status"] = status
        if thbar is not None:
            res["thbar"] = thbar
        return res

    def solve_pack_vjp(self, theta, active, exitflag, xbar, want=PACK_BARS):
        """Host arrays in and out (`lmpc_solve_pack_vjp`; synchronous): dict with the arrays named in `want`, thbar and
        status."""
        act = np.ascontiguousarray(np.asarray(active, np.uint64).reshape(-1, self.words))
        N = act.shape[0]
        ef = np.ascontiguousarray(np.asarray(exitflag, np.int32).reshape(N))
        th = _f64(np.asarray(theta, float).reshape(N, self.nth))
        xb = _f64(np.asarray(xbar, float).reshape(N, self.nout))
        shapes = _pack_bar_shapes(self.n, self.m, self.nth, self.nout)
        out = {k: np.full(shapes[k], np.nan) for k in PACK_BARS if k in want}
        out["thbar"], out["status"] = np.zeros((N, self.nth)), np.zeros(N, np.int32)
        check(lib().lmpc_solve_pack_vjp(self._h, N, _ptr(th), _ptr(act), _ptr(ef), _ptr(xb), *[_ptr(out.get(k)) for k in PACK_BARS],
                                        _ptr(out["thbar"]), _ptr(out["status"])), self._h)
        return out

    def solve_autograd(self, theta):
        """The batched solve inside a torch graph: returns (x, exitflag) with x = x*(theta) carrying the gradient
        (forward `solve_device` with the active sets kept, backward ONE `solve_vjp_device` on the current torch stream)
        and exitflag marked non-differentiable.  The status of the most recent backward is `x.grad_fn.sens_status`
        (an int32 CUDA tensor, None before the backward).  With a theta that does not require grad this is
        `solve_device` and nothing else: no masks are written or kept."""
        import torch
        if not (theta.requires_grad and torch.is_grad_enabled()):
            return self.solve_device(theta.detach())
        return _autograd_fn().apply(theta, self)

    def check(self):
        """`lmpc_check`: wait for the handle's GPU, then raise if a kernel reported an internal failure
        (problems with exit flag -8) since the last check."""
        check(lib().lmpc_check(self._h), self._h)

    def close(self):
        if self._h:
            lib().lmpc_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiQP:
    """One condensed-MPC QP structure replicated on several GPUs of this process (`lmpc_multi`,
    include/lmpc_hip.h): one call solves a batch across all of them -- the shape of the reference's
    caller, one process with one Theta (/root/reference/src/utils.jl:268-283)."""

    def __init__(self, handle):
        self._hm = handle
        self.ndev = int(lib().lmpc_multi_devices(self._hm))
        self.parts = [BatchedQP(lib().lmpc_multi_handle(self._hm, i), None) for i in range(self.ndev)]
        for q in self.parts:
            q.close = lambda: None                      # the multi handle owns them
        q0 = self.parts[0]
        self.n, self.m, self.ms, self.nth, self.nout, self.words = q0.n, q0.m, q0.ms, q0.nth, q0.nout, q0.words

    @classmethod
    def from_mpqp(cls, H, f, f_theta, A, bu, bl, W, senses=None, nout=None, K=None, nx=0,
                  settings: Settings | None = None, devices=None):
        """`lmpc_setup_multi`; devices = None: every visible GPU."""
        H = _f64(H, "F")
        n = H.shape[0]
        f_theta = _f64(np.asarray(f_theta, float).reshape(n, -1), "F")
        nth = f_theta.shape[1]
        bu = _f64(np.asarray(bu, float).reshape(-1))
        bl = _f64(np.asarray(bl, float).reshape(-1))
        m = bu.size
        A = _f64(np.asarray(A, float).reshape(-1, n), "F")
        ms = m - A.shape[0]
        W = _f64(np.asarray(W, float).reshape(m, nth), "F")
        f = _f64(np.zeros(n) if f is None else np.asarray(f, float).reshape(n))
        nout = n if nout is None else int(nout)
        sense = np.ascontiguousarray(np.zeros(m, np.int32) if senses is None else senses, dtype=np.int32)
        Kf = None if K is None else _f64(np.asarray(K, float).reshape(nout, -1), "F")
        devs = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        h = _vp()
        rc = lib().lmpc_setup_multi(ctypes.byref(h), n, m, ms, nth, nout, _ptr(H), _ptr(f), _ptr(f_theta),
                                    _ptr(A), _ptr(bu), _ptr(bl), _ptr(W), _ptr(sense),
                                    _ptr(Kf) if Kf is not None else None, int(nx if K is not None else 0),
                                    ctypes.cast(ctypes.pointer(settings), _vp) if settings is not None else None,
                                    _ptr(devs) if devs is not None else None, 0 if devs is None else int(devs.size))
        check(rc)
        return cls(h)

    def _check(self, rc):
        if rc != _cabi.LMPC_OK:
            raise LmpcError(rc, (lib().lmpc_multi_last_error(self._hm) or b"").decode())

    def set_option(self, name: str, value: int):
        """`lmpc_multi_set_option` ("transport": 0 RCCL pairs, 1 event-ordered peer copies)."""
        lib().lmpc_multi_set_option.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int]
        lib().lmpc_multi_set_option.restype = ctypes.c_int
        self._check(lib().lmpc_multi_set_option(self._hm, name.encode(), int(value)))

    @staticmethod
    def partition(N, ndev):
        """`lmpc_multi_partition`: shard d = [off[d], off[d+1])."""
        off = (ctypes.c_int64 * (ndev + 1))()
        lib().lmpc_multi_partition(int(N), int(ndev), off)
        return [int(v) for v in off]

    def solve(self, theta, warm=None, want_iters=True, want_active=True):
        """`lmpc_solve_batch_multi`: host arrays in and out, the batch split over the GPUs."""
        theta = _f64(np.asarray(theta, float).reshape(-1, self.nth) if self.nth else np.zeros((len(theta), 0)))
        N = theta.shape[0]
        x = np.zeros((N, self.nout))
        ef = np.zeros(N, np.int32)
        it = np.zeros(N, np.int32) if want_iters else None
        act = np.zeros((N, self.words), np.uint64) if want_active else None
        w = None if warm is None else np.ascontiguousarray(np.asarray(warm, np.uint64).reshape(N, self.words))
        self._check(lib().lmpc_solve_batch_multi(self._hm, N, _ptr(theta), _ptr(x), _ptr(ef),
                                                 _ptr(it) if it is not None else None,
                                                 _ptr(act) if act is not None else None,
                                                 _ptr(w) if w is not None else None))
        return x, ef, it, act

    def solve_device(self, thetas, gather=True):
        """`lmpc_solve_batch_multi_device`: thetas[d] = (N_d, nth) float64 CUDA tensor on device d.
        Returns (x shards, exit-flag shards, x gathered on the first device or None, flags gathered or None)."""
        import torch
        assert len(thetas) == self.ndev
        xs = [torch.empty((t.shape[0], self.nout), dtype=torch.float64, device=t.device) for t in thetas]
        fs = [torch.empty(t.shape[0], dtype=torch.int32, device=t.device) for t in thetas]
        for t in thetas:
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == self.nth):
                raise ValueError("every shard must be a contiguous float64 CUDA tensor of shape (N_d, nth)")
            torch.cuda.synchronize(t.device)            # the library launches on its own streams
        ntot = sum(int(t.shape[0]) for t in thetas)
        xr = torch.empty((ntot, self.nout), dtype=torch.float64, device=thetas[0].device) if gather else None
        fr = torch.empty(ntot, dtype=torch.int32, device=thetas[0].device) if gather else None
        arr = lambda ts: (ctypes.c_void_p * self.ndev)(*[t.data_ptr() for t in ts])
        nd = (ctypes.c_int64 * self.ndev)(*[int(t.shape[0]) for t in thetas])
        self._check(lib().lmpc_solve_batch_multi_device(
            self._hm, ctypes.cast(nd, _vp), ctypes.cast(arr(thetas), _vp), ctypes.cast(arr(xs), _vp),
            ctypes.cast(arr(fs), _vp), _vp(xr.data_ptr()) if gather else None, _vp(fr.data_ptr()) if gather else None))
        return xs, fs, xr, fr

    def close(self):
        if self._hm:
            for q in self.parts:
                q._h = None
            lib().lmpc_free_multi(self._hm)
            self._hm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
