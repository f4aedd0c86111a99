"""Mirror of the reference's closed-loop simulation (/root/reference/src/simulation.jl:1-134) for MANY scenarios
at once, on the scenario loop of the library (`lmpc_simulate_scenario_device`, include/lmpc_hip.h):

    Plant(F, G, Gd, f_offset, C, Dd, h_offset)    the true plant and its measurement (model.jl:17-30)
    Scenario(x0, N, r, d, p, noise)               simulation.jl:13-35; x0 (nx,) or (N_scen, nx); r, d, p, noise
                                                  (w, T) shared by all scenarios or (N_scen, w, T)
    Simulation(mpc, scenario, plant, observer)    simulation.jl:37-116 -> ts, ys, us, xs, rs, ds, xhats, yms, flag_min
    offset_free_observer(F, G, C, ...)            setup.jl:392-448: the augmented filter of set_offset_free_observer!
                                                  from given gains; as `observer=` it adds dhats
    evaluate_cost / constraint_violation          utils.jl:397-425, on the device
    Uniform(lo, hi)                               a noise source drawn on the device, uniform in the box [lo, hi]
    Gaussian(mean, std)                           a noise source drawn on the device, independent normal components
    noise_draw(source, ...)                       the draws of either on the host (`lmpc_noise_draw_host`)

Of the reference's plant hook (`Simulation(dynamics, mpc)`, `scenario.dynamics`) the two uses its manual, examples and
tests make are covered (`lmpc_simulate_scenario_uncertain_device`): additive process noise on the state --
`Scenario(process_noise=)` with `Simulation(Gw=, seed=)` -- and plants that are not the controller's model -- a list
of `Plant`s.  Draws made on the device are uniform (`Uniform`) or Gaussian (`Gaussian`: example/observer.jl's
`B*randn` is `Gaussian(0, 1)` with Gw = B, a covariance goes through Gw as its Cholesky factor); both are the stated
sequences of include/lmpc_hip.h, which a host restates bit for bit (`noise_draw`).  A NONLINEAR true plant -- the `true_dynamics` x + Ts f(x, u, d) of a controller built from `Model(f, h, xo, uo, Ts)`
(simulation.jl:40,110,126, model.jl:87) -- is a `NonlinearPlant` (nonlinear.py): a Python function traced into a plant
program that `lmpc_simulate_scenario_nonlinear_device` interprets, with `params=` as its per-scenario parameters.
Callbacks (`scenario.callback`) and a nonlinear measurement have no counterpart.  An MPC with reference condensation
is refused (its theta block is not a cut of r).
"""
from __future__ import annotations

import numpy as np

from .solver import BatchedQP

__all__ = ["Plant", "Scenario", "Simulation", "evaluate_cost", "constraint_violation", "OffsetFreeObserver",
           "offset_free_observer", "Uniform", "Gaussian", "noise_draw"]


class Plant:
    """x+ = F x + G u + Gd d + f_offset,  y = C x + Dd d + h_offset."""

    def __init__(self, F, G, Gd=None, f_offset=None, C=None, Dd=None, h_offset=None):
        self.F = np.atleast_2d(np.asarray(F, float))
        self.nx = self.F.shape[0]
        self.G = np.asarray(G, float).reshape(self.nx, -1)
        self.nu = self.G.shape[1]
        self.Gd = np.zeros((self.nx, 0)) if Gd is None else np.asarray(Gd, float).reshape(self.nx, -1)
        self.nd = self.Gd.shape[1]
        self.f_offset = np.zeros(self.nx) if f_offset is None else np.asarray(f_offset, float).reshape(self.nx)
        self.C = np.eye(self.nx) if C is None else np.asarray(C, float).reshape(-1, self.nx)
        self.ny = self.C.shape[0]
        self.Dd = np.zeros((self.ny, self.nd)) if Dd is None else np.asarray(Dd, float).reshape(self.ny, self.nd)
        self.h_offset = np.zeros(self.ny) if h_offset is None else np.asarray(h_offset, float).reshape(self.ny)

    def dynamics_rows(self):
        """MPC_PLANT_DYNAMICS layout (reference src/observer.jl:136): rows [f_offset_i, F_i, G_i, Gd_i]."""
        return np.ascontiguousarray(np.hstack([self.f_offset[:, None], self.F, self.G, self.Gd]))

    def measurement_rows(self):
        """MPC_MEASUREMENT_FUNCTION layout (:137): rows [h_offset_j, C_j, Dd_j]."""
        return np.ascontiguousarray(np.hstack([self.h_offset[:, None], self.C, self.Dd]))


class Uniform:
    """A noise source drawn on the device: component q uniform in [lo[q], hi[q]] (lo == hi: the constant), from the
    counter-based generator include/lmpc_hip.h states -- a draw depends on (seed, scenario, step, stream, component)
    alone."""

    def __init__(self, lo, hi):
        self.lo, self.hi = np.atleast_1d(np.asarray(lo, float)), np.atleast_1d(np.asarray(hi, float))
        if self.lo.shape != self.hi.shape or self.lo.ndim != 1:
            raise ValueError("lo and hi must be vectors of the same length")
        if not (np.isfinite(self.lo).all() and np.isfinite(self.hi).all() and (self.lo <= self.hi).all()):
            raise ValueError("the bounds must be finite with lo <= hi")


class Gaussian:
    """A noise source drawn on the device: component q normal with mean[q] and standard deviation std[q] (std == 0: the
    constant mean), independent components, by the Box-Muller sequence include/lmpc_hip.h states on the same
    counter-based generator as `Uniform` -- a draw depends on (seed, scenario, step, stream, component) alone.  A scalar
    mean or std is repeated to the other's length."""
    dist = 1                                      # LMPC_NOISE_GAUSSIAN

    def __init__(self, mean, std):
        mean, std = np.atleast_1d(np.asarray(mean, float)), np.atleast_1d(np.asarray(std, float))
        if mean.ndim != 1 or std.ndim != 1:
            raise ValueError("mean and std must be scalars or vectors")
        if mean.size == 1 and std.size > 1:
            mean = np.repeat(mean, std.size)
        if std.size == 1 and mean.size > 1:
            std = np.repeat(std, mean.size)
        if mean.shape != std.shape:
            raise ValueError("mean and std must have the same length")
        if not np.isfinite(mean).all():
            raise ValueError("the means must be finite")
        if not (np.isfinite(std).all() and (std >= 0).all()):
            raise ValueError("the standard deviations must be finite and not negative")
        self.mean, self.std = mean, std

    lo = property(lambda self: self.mean)         # the fields of lmpc_noise that carry them
    hi = property(lambda self: self.std)


def noise_draw(source, N, T, seed=0, stream=0, scenario_offset=0, step_offset=0):
    """`lmpc_noise_draw_host`: the e a `Uniform` or `Gaussian` source gives the loop for scenarios scenario_offset ..
    + N - 1 and steps step_offset .. + T - 1 (stream 0: process noise, 1: measurement noise), computed on the CPU:
    (N, w, T), the shape of a per-scenario supplied block.  Needs no GPU."""
    return BatchedQP.noise_draw_host(source, N, T, seed, stream, scenario_offset, step_offset)


class Scenario:
    """simulation.jl:13-35 for N_scen scenarios.  Trajectories keep their own length; `trajectory` gives them over
    the N steps of the run, cut or held at the last column (simulation.jl:69-88).  process_noise (added to the state
    through Simulation's Gw) and measurement_noise (added to ym, as `noise` is): a `Uniform` or a `Gaussian`, drawn on the device, or
    an array (w, T) / (N_scen, w, T) of supplied draws."""

    def __init__(self, x0, N=1000, r=None, d=None, p=None, noise=None, process_noise=None, measurement_noise=None):
        x0 = np.asarray(x0, float)
        self.single = x0.ndim == 1
        self.x0 = np.ascontiguousarray(np.atleast_2d(x0))
        self.n_scen, self.N = self.x0.shape[0], int(N)
        self.r, self.d, self.p, self.noise = (self._traj(a, k) for a, k in ((r, "r"), (d, "d"), (p, "p"), (noise, "noise")))
        if self.noise is not None and measurement_noise is not None:
            raise ValueError("noise and measurement_noise are the same slot: give one of them")
        self.process_noise, self.measurement_noise = (
            a if isinstance(a, (Uniform, Gaussian)) else self._traj(a, k)
            for a, k in ((process_noise, "process_noise"), (measurement_noise, "measurement_noise")))

    def _traj(self, a, name):
        if a is None or np.size(a) == 0:
            return None
        a = np.asarray(a, float)
        if a.ndim == 1:
            a = a[:, None]
        if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[0] != self.n_scen):
            raise ValueError(f"{name} must have shape (w, T) or ({self.n_scen}, w, T), got {a.shape}")
        return a

    def trajectory(self, name, w=0):
        """The (w, N) or (N_scen, w, N) array the reference's loop indexes: columns beyond the given ones repeat the
        last, columns beyond the run are cut; None -> zeros (w, N)."""
        a = getattr(self, name)
        if a is None:
            return np.zeros((w, self.N))
        Tc = a.shape[-1]
        idx = np.minimum(np.arange(self.N), Tc - 1)
        return np.ascontiguousarray(a[..., idx])

    def block_spec(self, name, H=0, w=0):
        """What becomes the `lmpc_block` of a trajectory: dict(data, stride, w, T, H) with `data` laid out column
        after column per scenario ((T, w) or (N_scen, T, w); None = zeros), stride 0 for a shared trajectory and
        w * T for one per scenario; the columns are those of the run (at most N)."""
        a = getattr(self, name)
        if a is None:
            return dict(data=None, stride=0, w=int(w), T=1, H=int(H))
        a = a[..., :self.N]
        w_, Tc = a.shape[-2], a.shape[-1]
        return dict(data=np.ascontiguousarray(np.swapaxes(a, -1, -2)), stride=w_ * Tc if a.ndim == 3 else 0,
                    w=int(w_), T=int(Tc), H=int(H))


def scenario_blocks(mpc, scenario, ndo=0):
    """The four block specs of a run: column or preview follows the MPC's settings as simulation.jl:74,81,89 (and
    the widths of theta) have it.  ndo: the last ndo of the controller's disturbances are an offset-free observer's
    estimates, the scenario's d holds the measured ones alone."""
    if mpc.reference_condensation:
        raise ValueError("reference condensation is not available in the scenario loop")
    Np = mpc.Np
    specs = {
        "r": scenario.block_spec("r", Np if (mpc.reference_preview and mpc.nr > 0) else 0, mpc.ny if mpc.nr > 0 else 0),
        "d": scenario.block_spec("d", Np if (mpc.disturbance_preview and mpc.nd > 0) else 0, mpc.nd_base - ndo),
        "p": scenario.block_spec("p", Np if (mpc.parameter_preview and mpc.np > 0) else 0, mpc.np_base),
        "noise": scenario.block_spec("noise", 0, 0),
    }
    if mpc.nr == 0:                          # no reference in theta: the trajectory only serves the cost
        specs["r"] = dict(data=None, stride=0, w=0, T=1, H=0)
    for k, w in (("r", mpc.ny if mpc.nr > 0 else 0), ("d", mpc.nd_base - ndo), ("p", mpc.np_base)):
        if specs[k]["data"] is not None and specs[k]["w"] != w:
            raise ValueError(f"{k} trajectory must have {w} rows, got {specs[k]['w']}")
    return specs


_OFFSET_FREE_METHODS = {"state": "state_disturbance", "state_disturbance": "state_disturbance", "velocity": "velocity",
                        "output": "output_disturbance", "output_disturbance": "output_disturbance", "general": "general"}


class OffsetFreeObserver:
    """The reference's OffsetFreeObserver (src/observer.jl:13-22) as arrays: the filter on [x; dhat] with
    Faug = [F Bd; 0 I], Gaug = [G; 0], Gdaug = [Gd; 0], Caug = [C Cd], gain Kaug (nx + ndo, ny)."""

    def __init__(self, Faug, Gaug, Gdaug, faug, Caug, Dd, h_offset, Kaug, nx, nd_measured, nd_offsetfree, Bd, Cd,
                 formulation):
        self.F, self.G, self.Gd, self.f_offset = Faug, Gaug, Gdaug, faug
        self.C, self.Dd, self.h_offset, self.K = Caug, Dd, h_offset, Kaug
        self.nx, self.nd_measured, self.nd_offsetfree = int(nx), int(nd_measured), int(nd_offsetfree)
        self.Bd, self.Cd, self.formulation = Bd, Cd, formulation

    def codegen_arrays(self):
        """MPC_PLANT_DYNAMICS, MPC_MEASUREMENT_FUNCTION, K_TRANSPOSE_OBSERVER of the augmented filter
        (src/observer.jl:139-141), flat."""
        dyn = np.hstack([self.f_offset[:, None], self.F, self.G, self.Gd])
        meas = np.hstack([self.h_offset[:, None], self.C, self.Dd])
        return np.ascontiguousarray(dyn).reshape(-1), np.ascontiguousarray(meas).reshape(-1), \
            np.ascontiguousarray(self.K.T).reshape(-1)


def offset_free_observer(F, G, C, Gd=None, Dd=None, f_offset=None, h_offset=None, method="state_disturbance", K=None,
                         Bd=None, Cd=None, Kx=None, Kd=None, Kaug=None):
    """`build_offset_free_observer` (reference src/setup.jl:392-448) WITHOUT its Riccati solve: the gains are given.
    Gd / Dd: the MEASURED disturbances' columns.  method (aliases of setup.jl:342-353): "state_disturbance" /
    "state" and "velocity" take the nominal gain K (nx, ny) and set Bd = K, Cd = I - C K, Kx = K, Kd = I;
    "output_disturbance" / "output" (Bd = 0, Cd = I) and "general" (Bd, Cd given) take Kx (nx, ny) and / or Kd (ndo, ny),
    or the whole gain Kaug (nx + ndo, ny).  Refuses a disturbance model with rank([F - I Bd; C Cd]) != nx + ndo
    (setup.jl:382-390)."""
    if method not in _OFFSET_FREE_METHODS:
        raise ValueError(f"Unknown offset-free method {method}")
    method = _OFFSET_FREE_METHODS[method]
    F = np.atleast_2d(np.asarray(F, float))
    nx = F.shape[0]
    G = np.asarray(G, float).reshape(nx, -1)
    C = np.asarray(C, float).reshape(-1, nx)
    ny = C.shape[0]
    Gd = np.zeros((nx, 0)) if Gd is None else np.asarray(Gd, float).reshape(nx, -1)
    ndm = Gd.shape[1]
    Dd = np.zeros((ny, ndm)) if Dd is None else np.asarray(Dd, float).reshape(ny, ndm)
    f_offset = np.zeros(nx) if f_offset is None else np.asarray(f_offset, float).reshape(nx)
    h_offset = np.zeros(ny) if h_offset is None else np.asarray(h_offset, float).reshape(ny)
    if method in ("state_disturbance", "velocity"):
        if K is None:
            raise ValueError(f"method {method} needs the nominal observer gain K ({nx}, {ny})")
        K = np.asarray(K, float)
        if K.shape != (nx, ny):
            raise ValueError(f"K must have size ({nx}, {ny})")
        Bd, Cd, Kx, Kd = K, np.eye(ny) - C @ K, K, np.eye(ny)
    elif method == "output_disturbance":
        Bd, Cd = np.zeros((nx, ny)), np.eye(ny)
    else:
        if Bd is None:
            raise ValueError("Method general requires Bd")
        if Cd is None:
            raise ValueError("Method general requires Cd")
    Bd, Cd = np.asarray(Bd, float), np.asarray(Cd, float)
    if Bd.ndim != 2 or Bd.shape[0] != nx:
        raise ValueError(f"Bd must have {nx} rows")
    ndo = Bd.shape[1]
    if Cd.shape != (ny, ndo):
        raise ValueError(f"Cd must have size ({ny}, {ndo})")
    if np.linalg.matrix_rank(np.block([[F - np.eye(nx), Bd], [C, Cd]])) != nx + ndo:
        raise ValueError("Offset-free disturbance model violates rank([F-I Bd; C Cd]) = nx + nd")
    if Kaug is not None:
        Kaug = np.asarray(Kaug, float)
        if Kaug.shape != (nx + ndo, ny):
            raise ValueError(f"Kaug must have size ({nx + ndo}, {ny})")
    elif Kx is not None or Kd is not None:
        Kx = np.zeros((nx, ny)) if Kx is None else np.asarray(Kx, float)
        Kd = np.zeros((ndo, ny)) if Kd is None else np.asarray(Kd, float)
        if Kx.shape != (nx, ny):
            raise ValueError(f"Kx must have size ({nx}, {ny})")
        if Kd.shape != (ndo, ny):
            raise ValueError(f"Kd must have size ({ndo}, {ny})")
        Kaug = np.vstack([Kx, Kd])
    else:
        raise ValueError(f"method {method} needs the gains Kx / Kd or Kaug (this package solves no Riccati equation)")
    nu = G.shape[1]
    Faug = np.block([[F, Bd], [np.zeros((ndo, nx)), np.eye(ndo)]])
    Gaug = np.vstack([G, np.zeros((ndo, nu))])
    Gdaug = np.vstack([Gd, np.zeros((ndo, ndm))])
    Caug = np.hstack([C, Cd])
    faug = np.concatenate([f_offset, np.zeros(ndo)])
    return OffsetFreeObserver(Faug, Gaug, Gdaug, faug, Caug, Dd, h_offset, Kaug, nx, ndm, ndo, Bd, Cd, method)


def _observer_arrays(observer):
    if observer is None:
        return None
    if hasattr(observer, "codegen_arrays"):
        observer = observer.codegen_arrays()
    dyn, meas, kt = (np.asarray(a, float) for a in observer)
    return dyn, meas, kt


class Simulation:
    """`Simulation(mpc, scenario)` of the reference for every scenario at once.  mpc: an `MPC` of this package;
    plant: the true `Plant`; observer: None, an object with `codegen_arrays()` or the triple (MPC_PLANT_DYNAMICS,
    MPC_MEASUREMENT_FUNCTION, K_TRANSPOSE_OBSERVER) of the generated observer (src/observer.jl:124-141).
    An `ExplicitMPC` runs the loop with its piecewise-affine law (`mode` 0, the default: lock-step, the faster form
    where both were measured; 1: run-ahead kernel; warm must be False) and adds `regions` (N_scen, N) int32, -1 = solved by the implicit path, and `stats`.
    Fields as in the reference, one leading scenario axis unless x0 was a single vector: xs, xhats (nx, N), us
    (nu, N), ys, yms (ny, N), rs, ds, ts, and flag_min (smallest exit flag per scenario).
    observer = `offset_free_observer(...)`: the offset-free loop (`lmpc_simulate_scenario_offset_free_device`); the plant
    and the scenario's d then carry the MEASURED disturbances alone (plant.nd == mpc.nd_base - ndo) and `dhats`
    (N_scen, ndo, N), the estimate the controller saw, is added.  Not available with an `ExplicitMPC`.
    Uncertainty (`lmpc_simulate_scenario_uncertain_device`): the scenario's process_noise e_k acts as w_k = Gw e_k on
    the state (Gw None: identity) and `ws` (N_scen, nx, N) is added; its measurement_noise is added to ym; plant = a
    list of `Plant`s of equal nx, nu, nd, ny: scenario i is stepped by plant plant_index[i] (default i mod the list's
    length) and all share the FIRST one's measurement rows; seed keys the draws of a `Uniform` or a `Gaussian`.  Without any of these
    the existing path runs unchanged; with an `ExplicitMPC` or an `OffsetFreeObserver` they raise ValueError.
    plant = a `NonlinearPlant` (`lmpc_simulate_scenario_nonlinear_device`): the true plant is its traced program, stepped
    on the device; params (nq,) or (N_scen, nq) are its q; process_noise, measurement_noise, Gw, seed and observer= as
    above; the measurement is its linear C, Dd, h_offset.  A list of plants, an `ExplicitMPC` or an `OffsetFreeObserver`
    raises ValueError.
    tape=True keeps every step's working set and exit flags (`lmpc_simulate_scenario_taped_device`; the run is the same
    bit for bit) so that `vjp` can differentiate the run.  The plain loop alone has an adjoint: an `ExplicitMPC`, an
    `OffsetFreeObserver`, noise drawn or supplied through the uncertain loop, a list of plants and a `NonlinearPlant` are
    refused here, before any call into the library (those loops are entry points of their own with no adjoint beside
    them): an LmpcError with the code of LMPC_ERR_UNSUPPORTED.  What the library itself refuses (BINARY rows, a
    variational or proximal-point controller) is refused by `vjp`, with the library's text."""

    def __init__(self, mpc, scenario, plant, observer=None, warm=False, cost=None, mode=0, Gw=None, seed=0, plant_index=None,
                 params=None, tape=False):
        import torch
        from .mpc import ExplicitMPC
        from .nonlinear import NonlinearPlant
        empc = mpc if isinstance(mpc, ExplicitMPC) else None
        plants = list(plant) if isinstance(plant, (list, tuple)) else None
        nonlinear = isinstance(plant, NonlinearPlant)
        if plants is not None and any(isinstance(q, NonlinearPlant) for q in plants):
            raise ValueError("a NonlinearPlant cannot be part of a list of plants: its params (per scenario) take the "
                             "ensemble's place")
        if nonlinear and empc is not None:
            raise ValueError("a NonlinearPlant is not available in the explicit controller's loop")
        if nonlinear and isinstance(observer, OffsetFreeObserver):
            raise ValueError("a NonlinearPlant is not available with an offset-free observer")
        if params is not None and not nonlinear:
            raise ValueError("params needs a NonlinearPlant")
        if plants is not None:
            if not plants:
                raise ValueError("the list of plants is empty")
            plant = plants[0]
            if any((q.nx, q.nu, q.nd, q.ny) != (plant.nx, plant.nu, plant.nd, plant.ny) for q in plants):
                raise ValueError("the plants of a list must agree in nx, nu, nd and ny")
        e_src, v_src = getattr(scenario, "process_noise", None), getattr(scenario, "measurement_noise", None)
        uncertain = plants is not None or e_src is not None or v_src is not None or Gw is not None or plant_index is not None
        if nonlinear and plant_index is not None:
            raise ValueError("plant_index needs a list of plants")
        if uncertain and (empc is not None or isinstance(observer, OffsetFreeObserver)):
            raise ValueError("process noise, measurement_noise, Gw, plant lists and plant_index are not available in the "
                             "explicit controller's loop or with an offset-free observer")
        if plant_index is not None and plants is None:
            raise ValueError("plant_index needs a list of plants")
        if Gw is not None and e_src is None:
            raise ValueError("Gw needs the scenario's process_noise")
        if empc is not None and isinstance(observer, OffsetFreeObserver):
            raise ValueError("the offset-free observer is not available in the explicit controller's loop")
        if tape and (empc is not None or uncertain or nonlinear or isinstance(observer, OffsetFreeObserver)):
            from ._cabi import LmpcError
            raise LmpcError(-103, "lmpc_scenario_vjp: the explicit, offset-free, uncertain and nonlinear scenario loops "
                                  "have no adjoint (the plain scenario loop alone is differentiated)")
        if empc is not None:                      # simulation.jl:37 with compute_control(empc, x), utils.jl:53-60
            if empc.controller is None:
                raise RuntimeError("Need to build a binary search tree to evaluate control law")
            if warm:
                raise ValueError("an explicit controller has no warm start")
            mpc = empc.mpc
            uprev0 = empc.uprev
        else:
            uprev0 = mpc.uprev
        # an explicit controller runs on the handle it was built on (its fallback solves and its observer live there)
        model: BatchedQP = mpc.control_model() if empc is None else empc.controller.qp
        self.mpc, self.scenario, self.plant, self.model = mpc, scenario, plant, model
        dev = torch.device("cuda", model.device)
        T, S = scenario.N, scenario.n_scen
        if plant.nx != mpc.nx or plant.nu != mpc.nu:
            raise ValueError("plant and controller disagree on nx / nu")
        off = observer if isinstance(observer, OffsetFreeObserver) else None
        ndo = 0 if off is None else off.nd_offsetfree
        if off is not None and off.nx != plant.nx:
            raise ValueError("plant and offset-free observer disagree on nx")
        if plant.nd != mpc.nd_base - ndo:
            raise ValueError(f"the plant has {plant.nd} disturbances, the controller's theta {mpc.nd_base}"
                             + (f" of which {ndo} are estimated" if ndo else ""))
        obs = _observer_arrays(observer)
        if obs is not None:
            model.set_observer(*obs, plant.nx + ndo, plant.nu, plant.nd, plant.ny)
        self._observer = None if obs is None else (obs, (plant.nx + ndo, plant.nu, plant.nd, plant.ny))
        specs = scenario_blocks(mpc, scenario, ndo)
        up = lambda sp: None if sp["data"] is None else torch.from_numpy(np.swapaxes(sp["data"], -1, -2).copy()).to(dev)
        x = torch.from_numpy(scenario.x0.copy()).to(dev)
        uprev = None
        if mpc.nuprev:
            uprev = torch.from_numpy(np.tile(np.asarray(uprev0, float)[:mpc.nuprev], (S, 1))).to(dev)
        run = model.simulate_scenario if empc is None else \
            (lambda *a, **kw: empc.controller.simulate_scenario_device(*a, mode=mode, **kw))
        want = ("U", "X", "Y", "Ym", "Xhat") + (("D",) if plant.nd else ())
        if uncertain or nonlinear:
            src = lambda a: a if (a is None or isinstance(a, (Uniform, Gaussian))) else torch.from_numpy(np.ascontiguousarray(a[..., :T])).to(dev)
            pidx = None if plant_index is None else torch.from_numpy(
                np.ascontiguousarray(np.asarray(plant_index).reshape(S).astype(np.int32))).to(dev)
            run = lambda *a, want, **kw: model.simulate_scenario_uncertain(
                *a, process=src(e_src), measurement_noise=src(v_src), Gw=Gw, seed=seed,
                plants=None if plants is None else np.stack([q.dynamics_rows() for q in plants]), plant_index=pidx,
                want=want + (("W",) if e_src is not None else ()), **kw)
        if nonlinear:                             # simulation.jl:40,110,126 with true_dynamics = x + Ts f(x, u, d) (model.jl:87)
            run = lambda x_, T_, rows, meas, want, **kw: model.simulate_scenario_nonlinear(
                x_, T_, plant, params=params, process=src(e_src), measurement_noise=src(v_src), Gw=Gw, seed=seed,
                want=want + (("W",) if e_src is not None else ()), **kw)
        if off is not None:                       # simulation.jl:37-116 with an OffsetFreeObserver (observer.jl:203-225)
            out = model.simulate_scenario_offset_free(
                x, T, plant.dynamics_rows(), plant.measurement_rows(), ndo, nd=plant.nd, ny=plant.ny,
                r=up(specs["r"]), d=up(specs["d"]), p=up(specs["p"]), noise=up(specs["noise"]),
                r_preview=specs["r"]["H"], d_preview=specs["d"]["H"], p_preview=specs["p"]["H"],
                r_width=specs["r"]["w"], p_width=specs["p"]["w"], uprev=uprev, warm=warm, cost=cost,
                want=want + ("Dhat",), want_cost=cost is not None, want_violation=cost is not None and cost[0].nc > 0)
        else:
            out = run(
                x, T, None if nonlinear else plant.dynamics_rows(), plant.measurement_rows(), nd=plant.nd, ny=plant.ny,
                r=up(specs["r"]), d=up(specs["d"]), p=up(specs["p"]), noise=up(specs["noise"]),
                r_preview=specs["r"]["H"], d_preview=specs["d"]["H"], p_preview=specs["p"]["H"],
                r_width=specs["r"]["w"], d_width=specs["d"]["w"], p_width=specs["p"]["w"], uprev=uprev,
                use_observer=obs is not None, warm=warm, cost=cost, want=want,
                want_cost=cost is not None, want_violation=cost is not None and cost[0].nc > 0, **({"tape": True} if tape else {}))
        self._tape = out.get("tape")
        torch.cuda.synchronize(dev)
        model.check()
        per = lambda t: np.ascontiguousarray(t.cpu().numpy().transpose(1, 2, 0))      # (T, S, w) -> (S, w, T)
        self.xs, self.us = per(out["X"][:T]), per(out["U"])
        self.ys, self.yms, self.xhats = per(out["Y"]), per(out["Ym"]), per(out["Xhat"])
        self.ds = per(out["D"]) if plant.nd else np.zeros((S, 0, T))
        if "W" in out:
            self.ws = per(out["W"])
        if off is not None:
            self.dhats = per(out["Dhat"])
            self.xaug_final = out["xaug"].cpu().numpy() if out["xaug"] is not None else None
        rs = scenario.trajectory("r", mpc.ny)
        self.rs = np.broadcast_to(rs, (S,) + rs.shape[-2:]).copy()
        self.x_final = out["x"].cpu().numpy()
        self.flag_min = out["flag_min"].cpu().numpy()
        self.cost = out["cost"].cpu().numpy() if "cost" in out else None
        self.violation = out["violation"].cpu().numpy() if "violation" in out else None
        self.ts = np.arange(T, dtype=float)
        if empc is not None:                      # per scenario and step: the region, -1 = solved by the implicit path
            self.regions = np.ascontiguousarray(out["regions"].cpu().numpy().T)
            self.stats = out["stats"]
        if scenario.single:
            for k in ("xs", "us", "ys", "yms", "xhats", "ds", "rs") + (("dhats",) if off is not None else ()) + \
                    (("ws",) if hasattr(self, "ws") else ()):
                setattr(self, k, getattr(self, k)[0])

    def vjp(self, xs_bar=None, us_bar=None):
        """The gradient of <xs_bar, xs> + <us_bar, us> of a run made with tape=True (`lmpc_scenario_vjp_device`).  xs_bar /
        us_bar: shaped like `xs` / `us` ((N_scen, w, N), or (w, N) for a single scenario; xs_bar may carry an N + 1-th column
        for the state after the last step), None = zeros.  Returns a dict of numpy arrays in the shapes of the inputs the run
        was given: x0 like the scenario's x0; r, d, p like the scenario's trajectories (a shared trajectory gets the sum over
        the scenarios, columns beyond the run zeros; a block theta does not hold is left out); uprev (nuprev,): the
        controller's one previous control, summed over the scenarios; status_min (N_scen,): 1 where every step was
        differentiated (BatchedQP.scenario_vjp).  The controller's handle is shared by every Simulation of the MPC: the
        run's own observer is put back on it first, so a Simulation made in between with another observer does not
        change the result."""
        import torch
        if self._tape is None:
            raise ValueError("Simulation.vjp needs a run made with tape=True")
        if self._observer is not None:
            self.model.set_observer(*self._observer[0], *self._observer[1])
        tape, sc = self._tape, self.scenario
        S, T, nx, nu = tape["N"], tape["T"], tape["nx"], tape["nu"]
        dev = tape["flag"].device

        def step_major(a, w, cols):
            if a is None:
                return None
            a = np.asarray(a, float)
            a = a[None] if a.ndim == 2 else a
            if a.shape[:2] != (S, w) or a.shape[2] not in cols:
                raise ValueError(f"a cotangent must have shape ({S}, {w}, {cols[0]}), got {a.shape}")
            full = np.zeros((cols[-1], S, w))
            full[:a.shape[2]] = a.transpose(2, 0, 1)
            return torch.from_numpy(full).to(dev)

        g = self.model.scenario_vjp(tape, Xbar=step_major(xs_bar, nx, (T, T + 1)), Ubar=step_major(us_bar, nu, (T,)))
        torch.cuda.synchronize(dev)
        x0 = g["x0bar"].cpu().numpy()
        out = dict(x0=x0[0] if sc.single else x0, status_min=g["status_min"].cpu().numpy())
        if tape["nup"]:
            out["uprev"] = g["uprev0bar"].cpu().numpy().sum(axis=0)
        for k in ("r", "d", "p"):
            a = getattr(sc, k)
            if a is None or k + "bar" not in g:
                continue
            bar = g[k + "bar"].cpu().numpy()                   # (S, w, Tc): the columns of the run
            full = np.zeros((S,) + a.shape[-2:])
            full[..., :bar.shape[-1]] = bar
            out[k] = full if a.ndim == 3 else full.sum(axis=0)
        return out


_scoring = {}


def _scoring_model(device=0):
    """The scoring kernels read nothing of a handle but its GPU: any handle serves, this one holds a 1 x 1 problem."""
    if device not in _scoring:
        one = np.ones((1, 1))
        _scoring[device] = BatchedQP.from_mpqp(one, np.zeros(1), one, np.zeros((0, 1)), np.ones(1), -np.ones(1), one * 0.0,
                                               device=device)
    return _scoring[device]


def _step_major(a, w):
    """(w, T) or (S, w, T) host array -> (T, S, w) contiguous, and whether it was a single scenario."""
    a = np.asarray(a, float)
    if a.ndim == 1:
        a = a.reshape(w, -1) if w else a[None]
    single = a.ndim == 2
    a = a[None] if single else a
    return np.ascontiguousarray(a.transpose(2, 0, 1)), single


def evaluate_cost(sim, C=None, Q=None, R=None, Rr=None, S=None, xs=None, us=None, rs=None, model=None):
    """`evaluate_cost(mpc, xs, us, rs; Q, R, Rr, S)` (utils.jl:397-411) on the device: 0.5 sum_k (C x_k - r_k)'Q(..) +
    u'Ru + du'Rr du + x'Su per scenario.  `sim`: a Simulation (its xs, us, rs and handle), or None with xs, us
    [, rs] given as (w, T) / (N_scen, w, T) arrays.  C defaults to the simulation's plant.C.  Returns a float for a
    single scenario, else an (N_scen,) array."""
    import torch
    if sim is not None:
        xs = sim.xs if xs is None else xs
        us = sim.us if us is None else us
        rs = sim.rs if rs is None else rs
        model = sim.model if model is None else model
        C = sim.plant.C if C is None else C
    model = _scoring_model() if model is None else model
    dev = torch.device("cuda", model.device)
    xs = np.asarray(xs, float)
    nx = xs.shape[-2] if xs.ndim > 1 else 1
    us = np.asarray(us, float)
    nu = us.shape[-2] if us.ndim > 1 else 1
    X, single = _step_major(xs, nx)
    U, _ = _step_major(us, nu)
    cost = BatchedQP.sim_cost(nx, nu, C=C, Q=Q, R=R, Rr=Rr, S=S)
    r = None
    if rs is not None and np.size(rs) and cost[0].ny > 0:
        rs = np.asarray(rs, float).reshape((-1, cost[0].ny, X.shape[0]) if np.ndim(rs) != 2 else (cost[0].ny, -1))
        r = torch.from_numpy(np.ascontiguousarray(rs)).to(dev)
    out = model.evaluate_cost_device(torch.from_numpy(X).to(dev), torch.from_numpy(U).to(dev), cost, r)
    torch.cuda.synchronize(dev)
    out = out.cpu().numpy()
    return float(out[0]) if single else out


def constraint_violation(Ax, Au, lb, ub, xs, us, model=None):
    """`constraint_violation(c, xs, us)` (utils.jl:417-425) on the device for rows lb <= Ax x + Au u <= ub: the
    violation max(lb - v, v - ub, 0) over the rows, per step.  xs (nx,) / us (nu,): one number; (nx, T) / (nu, T):
    an array of T; (N_scen, nx, T): (N_scen, T)."""
    import torch
    lb, ub = np.asarray(lb, float).reshape(-1), np.asarray(ub, float).reshape(-1)
    nc = lb.size
    nx = np.asarray(Ax, float).reshape(nc, -1).shape[1] if Ax is not None else np.asarray(xs).shape[-2 if np.ndim(xs) > 1 else 0]
    nu = np.asarray(Au, float).reshape(nc, -1).shape[1] if Au is not None else np.asarray(us).shape[-2 if np.ndim(us) > 1 else 0]
    xs, us = np.asarray(xs, float), np.asarray(us, float)
    point = xs.ndim == 1
    if point:
        xs, us = xs.reshape(nx, 1), us.reshape(nu, 1)
    if xs.shape[-1] != us.shape[-1]:
        raise AssertionError("xs and us must have as many columns")           # utils.jl:423
    X, single = _step_major(xs, nx)
    U, _ = _step_major(us, nu)
    model = _scoring_model() if model is None else model
    dev = torch.device("cuda", model.device)
    rows = BatchedQP.sim_cost(nx, nu, Ax=Ax, Au=Au, lb=lb, ub=ub)
    out = model.constraint_violation_device(torch.from_numpy(X).to(dev), torch.from_numpy(U).to(dev), rows, per_step=True)
    torch.cuda.synchronize(dev)
    out = out.cpu().numpy().T                                                  # (S, T)
    return float(out[0, 0]) if point else (out[0] if single else out)
