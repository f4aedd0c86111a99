"""ctypes binding of liblmpc_hip.so -- the same entry points a Julia `ccall` would bind
(include/lmpc_hip.h; Julia stub in INTEGRATION.md).

There is no CPU fallback anywhere in this package: if the shared library is missing the import
fails loudly, and if no HIP device is present every setup/solve call raises `LmpcError`.
"""
from __future__ import annotations

import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
# LMPC_HIP_LIB: another build of the same library (A/B of compiler flags); default = the in-tree build
LIB_PATH = os.environ.get("LMPC_HIP_LIB") or os.path.join(_PKG, "lib", "liblmpc_hip.so")

LMPC_OK = 1
ERR_NAMES = {-1: "INFEASIBLE", -5: "NONCONVEX", -6: "OVERDETERMINED", -100: "BADARG",
             -101: "NOGPU", -102: "HIP", -103: "UNSUPPORTED"}

# every symbol include/lmpc_hip.h declares (tests check the library exports all of them)
SYMBOLS = (
    "lmpc_abi_version", "lmpc_default_settings", "lmpc_setup", "lmpc_setup_ldp", "lmpc_transform",
    "lmpc_get_ldp", "lmpc_get_dims", "lmpc_active_words", "lmpc_set_settings",
    "lmpc_solve_batch", "lmpc_solve_batch_device", "lmpc_solve_batches_device", "lmpc_solve_one",
    "lmpc_default_settings_f32", "lmpc_solve_batch_f32", "lmpc_solve_batch_f32_device", "lmpc_simulate",
    "lmpc_simulate_device", "lmpc_simulate_f32", "lmpc_simulate_f32_device", "lmpc_form_parameter_device", "lmpc_simulate_ref_device", "lmpc_kernel_name",
    "lmpc_set_parameter_layout", "lmpc_compute_control", "lmpc_compute_control_device",
    "lmpc_set_observer", "lmpc_predict_state", "lmpc_correct_state", "lmpc_predict_state_device",
    "lmpc_correct_state_device", "lmpc_compute_control_observer_device",
    "lmpc_profile", "lmpc_profile_read", "lmpc_set_option", "lmpc_free", "lmpc_last_error",
    "lmpc_setup_multi", "lmpc_multi_devices", "lmpc_multi_handle", "lmpc_multi_partition",
    "lmpc_solve_batch_multi", "lmpc_solve_batch_multi_device", "lmpc_multi_last_error", "lmpc_free_multi",
    "lmpc_pin_host", "lmpc_unpin_host", "lmpc_release_scratch", "lmpc_check",
    "lmpc_distinct_active_sets_device", "lmpc_distinct_active_sets_overflowed", "lmpc_wave_stats", "lmpc_wave_launch_info",
    "lmpc_row_launch_info", "lmpc_fast_launch_info", "lmpc_front_pass_info", "lmpc_work_list_read", "lmpc_avi_launch_info", "lmpc_avi_list_read",
    "lmpc_debug_live_blocks",
    "lmpc_setup_ex", "lmpc_is_avi", "lmpc_get_avi", "lmpc_transform_avi", "lmpc_multi_set_option", "lmpc_discover_regions_device", "lmpc_reserve", "lmpc_get_prox",
    "lmpc_explicit_default_opts", "lmpc_explicit_build_ldp", "lmpc_explicit_build", "lmpc_explicit_info",
    "lmpc_explicit_region", "lmpc_explicit_blob", "lmpc_explicit_training", "lmpc_explicit_locate_host",
    "lmpc_explicit_eval_device", "lmpc_explicit_eval", "lmpc_explicit_last_error", "lmpc_explicit_free",
    "lmpc_scenario_check", "lmpc_simulate_scenario_device", "lmpc_simulate_scenario", "lmpc_evaluate_cost_device",
    "lmpc_constraint_violation_device",
    "lmpc_explicit_scenario_check", "lmpc_explicit_simulate_scenario_device", "lmpc_explicit_simulate_scenario",
    "lmpc_scenario_offset_free_check", "lmpc_simulate_scenario_offset_free_device", "lmpc_simulate_scenario_offset_free",
    "lmpc_scenario_uncertain_check", "lmpc_simulate_scenario_uncertain_device", "lmpc_simulate_scenario_uncertain",
    "lmpc_plant_program_check", "lmpc_plant_program_eval_host", "lmpc_plant_program_eval_device",
    "lmpc_simulate_scenario_nonlinear_device", "lmpc_simulate_scenario_nonlinear",
    "lmpc_noise_draw_host", "lmpc_noise_draw_device",
    "lmpc_solve_vjp_device", "lmpc_solve_jacobian_device", "lmpc_solve_vjp", "lmpc_solve_jacobian",
    "lmpc_solve_vjp_host", "lmpc_solve_jacobian_host", "lmpc_sens_launch_info",
    "lmpc_simulate_scenario_taped_device", "lmpc_simulate_scenario_taped", "lmpc_scenario_vjp_device", "lmpc_scenario_vjp",
    "lmpc_scenario_vjp_host", "lmpc_scenario_adjoint_launch_info",
    "lmpc_solve_pack_vjp_device", "lmpc_solve_pack_vjp", "lmpc_solve_pack_vjp_host", "lmpc_pack_grad_launch_info",
    "lmpc_transform_vjp",
)


class LmpcError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__(f"lmpc error {code} ({ERR_NAMES.get(code, '?')}): {msg}")


class Settings(ctypes.Structure):
    """`lmpc_settings`; defaults are DAQP's as documented in reference docs/src/manual/solver.md:49-56."""
    _fields_ = [("primal_tol", ctypes.c_double), ("dual_tol", ctypes.c_double),
                ("zero_tol", ctypes.c_double), ("progress_tol", ctypes.c_double),
                ("fval_bound", ctypes.c_double), ("rho_soft", ctypes.c_double),
                ("cycle_tol", ctypes.c_int32), ("iter_limit", ctypes.c_int32),
                ("eps_prox", ctypes.c_double), ("eta_prox", ctypes.c_double)]


class Block(ctypes.Structure):
    """`lmpc_block`: one block of theta cut from a (w x T, column-major) trajectory on the device."""
    _fields_ = [("src", ctypes.c_void_p), ("stride", ctypes.c_int64), ("w", ctypes.c_int32),
                ("T", ctypes.c_int32), ("k0", ctypes.c_int32), ("H", ctypes.c_int32)]


class ParamLayout(ctypes.Structure):
    """`lmpc_param_layout`: the N_STATE ... N_AFFINE_PARAMETER constants of the generated header
    (reference codegen.jl:154-165) and, for reference condensation, N_PREVIEW_HORIZON + traj2setpoint."""
    _fields_ = [("n_state", ctypes.c_int32), ("n_reference", ctypes.c_int32), ("n_disturbance", ctypes.c_int32),
                ("n_control_prev", ctypes.c_int32), ("n_affine_parameter", ctypes.c_int32),
                ("n_preview_horizon", ctypes.c_int32), ("traj2setpoint", ctypes.c_void_p)]


class Observer(ctypes.Structure):
    """`lmpc_observer`: the generated observer's arrays (reference src/observer.jl:124-141)."""
    _fields_ = [("n_state", ctypes.c_int32), ("n_control", ctypes.c_int32), ("n_disturbance", ctypes.c_int32),
                ("n_measurement", ctypes.c_int32), ("plant_dynamics", ctypes.c_void_p),
                ("measurement_function", ctypes.c_void_p), ("k_transpose", ctypes.c_void_p)]


class SimCost(ctypes.Structure):
    """`lmpc_sim_cost`: weights of evaluate_cost and rows of constraint_violation (reference utils.jl:397-425)."""
    _fields_ = [("ny", ctypes.c_int32), ("nc", ctypes.c_int32)] + \
               [(k, ctypes.c_void_p) for k in ("C", "Q", "R", "Rr", "S", "Ax", "Au", "lb", "ub")]


class ScenarioSim(ctypes.Structure):
    """`lmpc_scenario_sim`: descriptor of the scenario loop (lmpc_simulate_scenario*)."""
    _fields_ = [("nx", ctypes.c_int32), ("nu", ctypes.c_int32), ("nd", ctypes.c_int32), ("ny", ctypes.c_int32),
                ("plant", ctypes.c_void_p), ("measurement", ctypes.c_void_p),
                ("r", Block), ("d", Block), ("p", Block), ("noise", Block),
                ("nuprev", ctypes.c_int32), ("use_observer", ctypes.c_int32), ("warm", ctypes.c_int32),
                ("Y_traj", ctypes.c_void_p), ("Ym_traj", ctypes.c_void_p), ("Xhat_traj", ctypes.c_void_p),
                ("D_traj", ctypes.c_void_p), ("cost", ctypes.POINTER(SimCost)),
                ("cost_out", ctypes.c_void_p), ("violation_out", ctypes.c_void_p)]


class ScenarioTape(ctypes.Structure):
    """`lmpc_scenario_tape`: every step's final working set and exit flags of a taped scenario run, step-major."""
    _fields_ = [("active", ctypes.c_void_p), ("flag", ctypes.c_void_p)]


class ScenarioGrad(ctypes.Structure):
    """`lmpc_scenario_grad`: cotangents in, gradients out of `lmpc_scenario_vjp*`."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("Xbar", "Ubar", "x0bar", "xhat0bar", "uprev0bar", "rbar", "dbar", "pbar",
                                               "status_min")]


class OffsetFree(ctypes.Structure):
    """`lmpc_offset_free`: the offset-free part of a scenario run (lmpc_simulate_scenario_offset_free*)."""
    _fields_ = [("n_offset_free", ctypes.c_int32), ("Dhat_traj", ctypes.c_void_p)]


class Noise(ctypes.Structure):
    """`lmpc_noise`: one noise source of the uncertain scenario loop, supplied (`src`) or drawn: uniform in the box
    [lo, hi] (dist 0) or Gaussian with means lo and standard deviations hi (dist 1)."""
    _fields_ = [("w", ctypes.c_int32), ("dist", ctypes.c_int32), ("src", Block), ("lo", ctypes.c_void_p), ("hi", ctypes.c_void_p)]


class Uncertainty(ctypes.Structure):
    """`lmpc_uncertainty`: process / measurement noise and the plant table (lmpc_simulate_scenario_uncertain*)."""
    _fields_ = [("process", Noise), ("Gw", ctypes.c_void_p), ("measurement", Noise), ("seed", ctypes.c_uint64),
                ("scenario_offset", ctypes.c_int64), ("step_offset", ctypes.c_int32), ("n_plants", ctypes.c_int32),
                ("plants", ctypes.c_void_p), ("plant_index", ctypes.c_void_p), ("W_traj", ctypes.c_void_p)]


class PlantProgram(ctypes.Structure):
    """`lmpc_plant_program`: a nonlinear plant as a straight-line program (lmpc_simulate_scenario_nonlinear*)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("nx", "nu", "nd", "nq", "n_slots", "n_consts", "n_ins")] + \
               [("consts", ctypes.c_void_p), ("ins", ctypes.c_void_p), ("out_slot", ctypes.c_void_p)]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C linearmpc.jl_amd/csrc)")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    L.lmpc_abi_version.restype = i32
    L.lmpc_default_settings.argtypes = [ctypes.POINTER(Settings)]
    L.lmpc_default_settings.restype = None
    L.lmpc_setup.argtypes = [ctypes.POINTER(vp)] + [i32] * 5 + [vp] * 9 + [i32, vp, i32]
    L.lmpc_setup.restype = i32
    L.lmpc_setup_ex.argtypes = [ctypes.POINTER(vp)] + [i32] * 5 + [vp] * 9 + [i32, vp, vp, i32, i32, i32]
    L.lmpc_setup_ex.restype = i32
    L.lmpc_transform_avi.argtypes = [i32] * 5 + [vp] * 9 + [i32] + [vp] * 9
    L.lmpc_transform_avi.restype = i32
    L.lmpc_is_avi.argtypes = [vp]
    L.lmpc_is_avi.restype = i32
    L.lmpc_get_avi.argtypes = [vp, vp, vp]
    L.lmpc_get_avi.restype = i32
    L.lmpc_setup_ldp.argtypes = [ctypes.POINTER(vp)] + [i32] * 5 + [vp] * 9 + [i32]
    L.lmpc_setup_ldp.restype = i32
    L.lmpc_transform.argtypes = [i32] * 5 + [vp] * 9 + [i32] + [vp] * 7
    L.lmpc_transform.restype = i32
    L.lmpc_get_ldp.argtypes = [vp] * 9
    L.lmpc_get_ldp.restype = i32
    L.lmpc_get_dims.argtypes = [vp, ctypes.POINTER(ctypes.c_int32 * 6)]
    L.lmpc_get_dims.restype = i32
    L.lmpc_active_words.argtypes = [vp]
    L.lmpc_active_words.restype = i32
    L.lmpc_set_settings.argtypes = [vp, ctypes.POINTER(Settings)]
    L.lmpc_set_settings.restype = i32
    L.lmpc_solve_batch.argtypes = [vp, i64] + [vp] * 6
    L.lmpc_solve_batch.restype = i32
    L.lmpc_solve_batch_device.argtypes = [vp, i64] + [vp] * 7
    L.lmpc_solve_batch_device.restype = i32
    if hasattr(L, "lmpc_solve_batches_device"):
        L.lmpc_solve_batches_device.argtypes = [vp, i32, i64, vp, vp, vp, vp]
        L.lmpc_solve_batches_device.restype = i32
    L.lmpc_default_settings_f32.argtypes = [ctypes.POINTER(Settings)]
    L.lmpc_default_settings_f32.restype = None
    L.lmpc_solve_batch_f32.argtypes = [vp, i64] + [vp] * 6
    L.lmpc_solve_batch_f32.restype = i32
    L.lmpc_solve_batch_f32_device.argtypes = [vp, i64] + [vp] * 7
    L.lmpc_solve_batch_f32_device.restype = i32
    L.lmpc_solve_one.argtypes = [vp, vp, vp]
    L.lmpc_solve_one.restype = i32
    L.lmpc_simulate.argtypes = [vp, i64] + [i32] * 4 + [vp] * 8 + [i32]
    L.lmpc_simulate.restype = i32
    L.lmpc_simulate_device.argtypes = [vp, i64] + [i32] * 4 + [vp] * 8 + [i32, vp]
    L.lmpc_simulate_device.restype = i32
    L.lmpc_simulate_f32.argtypes = [vp, i64] + [i32] * 4 + [vp] * 8 + [i32]
    L.lmpc_simulate_f32.restype = i32
    L.lmpc_simulate_f32_device.argtypes = [vp, i64] + [i32] * 4 + [vp] * 8 + [i32, vp]
    L.lmpc_simulate_f32_device.restype = i32
    bp = ctypes.POINTER(Block)
    L.lmpc_form_parameter_device.argtypes = [vp, i64, vp, vp, i32, bp, bp, vp, i32, bp, vp]
    L.lmpc_form_parameter_device.restype = i32
    L.lmpc_simulate_ref_device.argtypes = [vp, i64, i32, i32, bp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.lmpc_simulate_ref_device.restype = i32
    L.lmpc_set_parameter_layout.argtypes = [vp, ctypes.POINTER(ParamLayout)]
    L.lmpc_set_parameter_layout.restype = i32
    L.lmpc_compute_control.argtypes = [vp, i64] + [vp] * 6 + [i32]
    L.lmpc_compute_control.restype = i32
    L.lmpc_compute_control_device.argtypes = [vp, i64] + [vp] * 6 + [i32, vp]
    L.lmpc_compute_control_device.restype = i32
    L.lmpc_set_observer.argtypes = [vp, ctypes.POINTER(Observer)]
    L.lmpc_set_observer.restype = i32
    for fn in (L.lmpc_predict_state, L.lmpc_correct_state):
        fn.argtypes = [vp, i64, vp, vp, vp]
        fn.restype = i32
    for fn in (L.lmpc_predict_state_device, L.lmpc_correct_state_device):
        fn.argtypes = [vp, i64, vp, vp, vp, vp]
        fn.restype = i32
    L.lmpc_compute_control_observer_device.argtypes = [vp, i64, vp, vp, i32, vp, vp, vp, vp, i32, vp]
    L.lmpc_compute_control_observer_device.restype = i32
    L.lmpc_kernel_name.argtypes = [vp]
    L.lmpc_kernel_name.restype = ctypes.c_char_p
    L.lmpc_profile.argtypes = [vp, i32]
    L.lmpc_profile.restype = i32
    L.lmpc_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double * 3)]
    L.lmpc_profile_read.restype = i32
    L.lmpc_set_option.argtypes = [vp, ctypes.c_char_p, i32]
    L.lmpc_set_option.restype = i32
    L.lmpc_free.argtypes = [vp]
    L.lmpc_free.restype = None
    L.lmpc_setup_multi.argtypes = [ctypes.POINTER(vp)] + [i32] * 5 + [vp] * 9 + [i32, vp, vp, i32]
    L.lmpc_setup_multi.restype = i32
    L.lmpc_multi_devices.argtypes = [vp]
    L.lmpc_multi_devices.restype = i32
    L.lmpc_multi_handle.argtypes = [vp, i32]
    L.lmpc_multi_handle.restype = vp
    L.lmpc_multi_partition.argtypes = [i64, i32, ctypes.POINTER(i64)]
    L.lmpc_multi_partition.restype = None
    L.lmpc_solve_batch_multi.argtypes = [vp, i64] + [vp] * 6
    L.lmpc_solve_batch_multi.restype = i32
    L.lmpc_solve_batch_multi_device.argtypes = [vp] + [vp] * 6
    L.lmpc_solve_batch_multi_device.restype = i32
    L.lmpc_multi_last_error.argtypes = [vp]
    L.lmpc_multi_last_error.restype = ctypes.c_char_p
    L.lmpc_free_multi.argtypes = [vp]
    L.lmpc_free_multi.restype = None
    L.lmpc_release_scratch.argtypes = [vp]
    L.lmpc_release_scratch.restype = i32
    if hasattr(L, "lmpc_distinct_active_sets_device"):
        L.lmpc_distinct_active_sets_device.argtypes = [vp, ctypes.c_int64, vp, vp, i32, vp, vp, vp, vp, vp]
        L.lmpc_distinct_active_sets_device.restype = i32
        L.lmpc_distinct_active_sets_overflowed.argtypes = [vp, vp]
        L.lmpc_distinct_active_sets_overflowed.restype = i32
    if hasattr(L, "lmpc_wave_stats"):
        L.lmpc_wave_stats.argtypes = [vp, vp]
        L.lmpc_wave_stats.restype = i32
    if hasattr(L, "lmpc_wave_launch_info"):
        L.lmpc_wave_launch_info.argtypes = [vp, vp, i32]
        L.lmpc_wave_launch_info.restype = i32
    if hasattr(L, "lmpc_row_launch_info"):
        L.lmpc_row_launch_info.argtypes = [vp, vp, i32]
        L.lmpc_row_launch_info.restype = i32
    if hasattr(L, "lmpc_fast_launch_info"):
        L.lmpc_fast_launch_info.argtypes = [vp, vp]
        L.lmpc_fast_launch_info.restype = i32
    if hasattr(L, "lmpc_front_pass_info"):
        L.lmpc_front_pass_info.argtypes = [vp, vp, i32]
        L.lmpc_front_pass_info.restype = i32
    if hasattr(L, "lmpc_avi_launch_info"):
        L.lmpc_avi_launch_info.argtypes = [vp, vp, i32]
        L.lmpc_avi_launch_info.restype = i32
    if hasattr(L, "lmpc_avi_list_read"):
        L.lmpc_avi_list_read.argtypes = [vp, i32, vp, vp, ctypes.c_longlong]
        L.lmpc_avi_list_read.restype = ctypes.c_longlong
    if hasattr(L, "lmpc_debug_live_blocks"):
        L.lmpc_debug_live_blocks.argtypes = []
        L.lmpc_debug_live_blocks.restype = ctypes.c_int64
    if hasattr(L, "lmpc_work_list_read"):
        L.lmpc_work_list_read.argtypes = [vp, vp, vp, ctypes.c_longlong]
        L.lmpc_work_list_read.restype = ctypes.c_longlong
    if hasattr(L, "lmpc_check"):              # (an older build selected with LMPC_HIP_LIB for an A/B lacks it)
        L.lmpc_check.argtypes = [vp]
        L.lmpc_check.restype = i32
    L.lmpc_pin_host.argtypes = [vp, ctypes.c_size_t]
    L.lmpc_pin_host.restype = i32
    L.lmpc_unpin_host.argtypes = [vp]
    L.lmpc_unpin_host.restype = i32
    L.lmpc_last_error.argtypes = [vp]
    L.lmpc_last_error.restype = ctypes.c_char_p
    sp = ctypes.POINTER(ScenarioSim)
    L.lmpc_scenario_check.argtypes = [i32, i32, ctypes.POINTER(Observer), sp]
    L.lmpc_scenario_check.restype = i32
    L.lmpc_simulate_scenario_device.argtypes = [vp, i64, i32, sp] + [vp] * 7
    L.lmpc_simulate_scenario_device.restype = i32
    L.lmpc_simulate_scenario.argtypes = [vp, i64, i32, sp] + [vp] * 6
    L.lmpc_simulate_scenario.restype = i32
    L.lmpc_evaluate_cost_device.argtypes = [vp, i64, i32, i32, i32, ctypes.POINTER(SimCost), vp, vp, bp, vp, vp]
    L.lmpc_evaluate_cost_device.restype = i32
    L.lmpc_constraint_violation_device.argtypes = [vp, i64, i32, i32, i32, ctypes.POINTER(SimCost), vp, vp, vp, vp, vp]
    L.lmpc_constraint_violation_device.restype = i32
    L.lmpc_explicit_scenario_check.argtypes = [i32, i32, ctypes.POINTER(Observer), sp, i32]
    L.lmpc_explicit_scenario_check.restype = i32
    op = ctypes.POINTER(OffsetFree)
    L.lmpc_scenario_offset_free_check.argtypes = [i32, i32, ctypes.POINTER(Observer), sp, op]
    L.lmpc_scenario_offset_free_check.restype = i32
    L.lmpc_simulate_scenario_offset_free_device.argtypes = [vp, i64, i32, sp, op] + [vp] * 7
    L.lmpc_simulate_scenario_offset_free_device.restype = i32
    L.lmpc_simulate_scenario_offset_free.argtypes = [vp, i64, i32, sp, op] + [vp] * 6
    L.lmpc_simulate_scenario_offset_free.restype = i32
    up = ctypes.POINTER(Uncertainty)
    L.lmpc_scenario_uncertain_check.argtypes = [i32, i32, ctypes.POINTER(Observer), sp, up]
    L.lmpc_scenario_uncertain_check.restype = i32
    L.lmpc_simulate_scenario_uncertain_device.argtypes = [vp, i64, i32, sp, up] + [vp] * 7
    L.lmpc_simulate_scenario_uncertain_device.restype = i32
    L.lmpc_simulate_scenario_uncertain.argtypes = [vp, i64, i32, sp, up] + [vp] * 6
    L.lmpc_simulate_scenario_uncertain.restype = i32
    pp = ctypes.POINTER(PlantProgram)
    L.lmpc_plant_program_check.argtypes = [pp]
    L.lmpc_plant_program_check.restype = i32
    L.lmpc_plant_program_eval_host.argtypes = [pp, i64, vp, vp, vp, vp, i32, vp]
    L.lmpc_plant_program_eval_host.restype = i32
    L.lmpc_plant_program_eval_device.argtypes = [vp, pp, i64, vp, vp, vp, vp, i32, vp, vp]
    L.lmpc_plant_program_eval_device.restype = i32
    L.lmpc_simulate_scenario_nonlinear_device.argtypes = [vp, i64, i32, sp, up, pp, vp, i32] + [vp] * 7
    L.lmpc_simulate_scenario_nonlinear_device.restype = i32
    L.lmpc_simulate_scenario_nonlinear.argtypes = [vp, i64, i32, sp, up, pp, vp, i32] + [vp] * 6
    L.lmpc_simulate_scenario_nonlinear.restype = i32
    if hasattr(L, "lmpc_noise_draw_host"):    # (an older build selected with LMPC_HIP_LIB for an A/B lacks them)
        npn = ctypes.POINTER(Noise)
        L.lmpc_noise_draw_host.argtypes = [npn, ctypes.c_uint64, i32, i64, i64, ctypes.c_int32, i32, vp]
        L.lmpc_noise_draw_host.restype = i32
        L.lmpc_noise_draw_device.argtypes = [vp, npn, ctypes.c_uint64, i32, i64, i64, ctypes.c_int32, i32, vp, vp]
        L.lmpc_noise_draw_device.restype = i32
    if hasattr(L, "lmpc_solve_vjp_device"):   # (an older build selected with LMPC_HIP_LIB for an A/B lacks them)
        L.lmpc_solve_vjp_device.argtypes = [vp, i64] + [vp] * 6
        L.lmpc_solve_vjp_device.restype = i32
        L.lmpc_solve_jacobian_device.argtypes = [vp, i64] + [vp] * 5
        L.lmpc_solve_jacobian_device.restype = i32
        L.lmpc_solve_vjp.argtypes = [vp, i64] + [vp] * 5
        L.lmpc_solve_vjp.restype = i32
        L.lmpc_solve_jacobian.argtypes = [vp, i64] + [vp] * 4
        L.lmpc_solve_jacobian.restype = i32
        L.lmpc_solve_vjp_host.argtypes = [i32] * 5 + [vp] * 9 + [i32, i64] + [vp] * 5
        L.lmpc_solve_vjp_host.restype = i32
        L.lmpc_solve_jacobian_host.argtypes = [i32] * 5 + [vp] * 9 + [i32, i64] + [vp] * 4
        L.lmpc_solve_jacobian_host.restype = i32
        L.lmpc_sens_launch_info.argtypes = [vp, vp, i32]
        L.lmpc_sens_launch_info.restype = i32
    if hasattr(L, "lmpc_solve_pack_vjp_device"):   # (an older build selected with LMPC_HIP_LIB for an A/B lacks them)
        L.lmpc_solve_pack_vjp_device.argtypes = [vp, i64] + [vp] * 14
        L.lmpc_solve_pack_vjp_device.restype = i32
        L.lmpc_solve_pack_vjp.argtypes = [vp, i64] + [vp] * 13
        L.lmpc_solve_pack_vjp.restype = i32
        L.lmpc_solve_pack_vjp_host.argtypes = [i32] * 5 + [vp] * 9 + [i32, i64] + [vp] * 13
        L.lmpc_solve_pack_vjp_host.restype = i32
        L.lmpc_pack_grad_launch_info.argtypes = [vp, vp, i32]
        L.lmpc_pack_grad_launch_info.restype = i32
        L.lmpc_transform_vjp.argtypes = [i32] * 5 + [vp] * 9 + [i32] + [vp] * 15
        L.lmpc_transform_vjp.restype = i32
    if hasattr(L, "lmpc_scenario_vjp_device"):   # (an older build selected with LMPC_HIP_LIB for an A/B lacks them)
        tp, gp = ctypes.POINTER(ScenarioTape), ctypes.POINTER(ScenarioGrad)
        L.lmpc_simulate_scenario_taped_device.argtypes = [vp, i64, i32, sp] + [vp] * 6 + [tp, vp]
        L.lmpc_simulate_scenario_taped_device.restype = i32
        L.lmpc_simulate_scenario_taped.argtypes = [vp, i64, i32, sp] + [vp] * 6 + [tp]
        L.lmpc_simulate_scenario_taped.restype = i32
        L.lmpc_scenario_vjp_device.argtypes = [vp, i64, i32, sp, tp, gp, vp]
        L.lmpc_scenario_vjp_device.restype = i32
        L.lmpc_scenario_vjp.argtypes = [vp, i64, i32, sp, tp, gp]
        L.lmpc_scenario_vjp.restype = i32
        L.lmpc_scenario_vjp_host.argtypes = [i32] * 5 + [vp] * 9 + [i32, ctypes.POINTER(Observer), i64, i32, sp, tp, gp]
        L.lmpc_scenario_vjp_host.restype = i32
        L.lmpc_scenario_adjoint_launch_info.argtypes = [vp, vp, i32]
        L.lmpc_scenario_adjoint_launch_info.restype = i32
    _lib = L
    return L


def default_settings() -> Settings:
    s = Settings()
    lib().lmpc_default_settings(ctypes.byref(s))
    return s


def default_settings_f32() -> Settings:
    s = Settings()
    lib().lmpc_default_settings_f32(ctypes.byref(s))
    return s


def last_error(handle=None) -> str:
    return (lib().lmpc_last_error(handle) or b"").decode()


def check(rc, handle=None):
    if rc != LMPC_OK:
        raise LmpcError(rc, last_error(handle))
