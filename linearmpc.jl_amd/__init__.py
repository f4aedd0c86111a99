"""linearmpc.jl_amd -- MI355X-native batched QP backend for LinearMPC.jl's online path.

The directory name carries a dot, so import it through the repo-root alias:

    import linearmpc_jl_amd as lmpc

Contents: the HIP kernels + C ABI (csrc/, built to lib/liblmpc_hip.so), the ctypes binding
(_cabi), `BatchedQP` (solver), the host-side mirror of the reference interface (mpc), of its closed-loop simulation (simulation) and the
one-process-per-GPU sharding helpers (shard).  Importing the package does not need a GPU;
setting up or solving does, and there is no CPU fallback.
"""
from ._cabi import LIB_PATH, SYMBOLS, LmpcError, Settings, default_settings, default_settings_f32, lib  # noqa: F401
from .solver import (BatchedQP, MultiQP, pack_vjp_host, scenario_vjp_host, sens_host, solve_mpqp_autograd, transform,  # noqa: F401
                     transform_avi, transform_vjp)
from .mpc import MPC, MPQP, ExplicitMPC, GeneratedController  # noqa: F401
from .shard import gather_shards, shard_bounds, shard_counts, solve_sharded  # noqa: F401
from .simulation import (Gaussian, OffsetFreeObserver, Plant, Scenario, Simulation, Uniform, constraint_violation, evaluate_cost,  # noqa: F401
                         noise_draw, offset_free_observer)
from .nonlinear import NonlinearPlant, TraceError, abs_, cos, fma, maximum, minimum, sin  # noqa: F401
from . import explicit  # noqa: F401

__all__ = ["BatchedQP", "MultiQP", "transform", "transform_avi", "sens_host", "scenario_vjp_host", "pack_vjp_host", "transform_vjp", "solve_mpqp_autograd", "MPC", "MPQP", "ExplicitMPC", "GeneratedController", "Settings", "default_settings", "default_settings_f32", "LmpcError",
           "gather_shards", "shard_bounds", "shard_counts", "solve_sharded", "explicit", "lib", "LIB_PATH", "Plant", "Scenario", "Simulation", "evaluate_cost", "constraint_violation",
           "OffsetFreeObserver", "offset_free_observer", "Uniform", "Gaussian", "noise_draw", "SYMBOLS",
           "NonlinearPlant", "TraceError", "sin", "cos", "fma", "minimum", "maximum", "abs_"]
