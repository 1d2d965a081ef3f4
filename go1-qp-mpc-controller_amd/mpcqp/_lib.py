"""ctypes view of libmpcqp.so (include/mpcqp.h, include/mpcqp_debug.h).

The shared library is built in-tree (go1-qp-mpc-controller_amd/lib/libmpcqp.so) by
``make -C go1-qp-mpc-controller_amd`` / ``__graft_entry__.build()``.  There is no fallback:
if the library is missing or has no HIP device, the call fails loudly.  ``load(debug=True)``
opens lib/libmpcqp_debug.so instead: the same ABI plus the cross-check solvers (tests only).
"""
import ctypes
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# MPCQP_LIB / MPCQP_DEBUG_LIB override the in-tree libraries (A/B kernel experiments only).
LIB_PATH = os.environ.get("MPCQP_LIB") or os.path.join(PKG_ROOT, "lib", "libmpcqp.so")
DEBUG_LIB_PATH = os.environ.get("MPCQP_DEBUG_LIB") or os.path.join(PKG_ROOT, "lib", "libmpcqp_debug.so")

STATE_DIM, NUM_LEG, NUM_DOF, CONSTRAINT_DIM = 13, 4, 12, 20
MAX_HORIZON = 20
DENSE_MAX_HORIZON = 10  # the dense K^-1 path (debug selection) serves horizons up to this
SOLVER_AUTO, SOLVER_DENSE, SOLVER_RICCATI, SOLVER_WAVE = 0, 1, 2, 3  # 1, 2: debug library only
OSQP_INFTY = 1e30

# record layout (include/mpcqp.h MPCQP_REC_*)
REC_X0, REC_EULER, REC_ROT, REC_INERTIA = 0, 13, 16, 25
REC_MASS, REC_MU, REC_FZMIN, REC_FZMAX, REC_DT, REC_CONTACTS, REC_XREF = 34, 35, 36, 37, 38, 39, 44


# raw robot-state row (include/mpcqp.h MPCQP_ST_*)
ST_EULER, ST_POS, ST_ANG_VEL, ST_LIN_VEL, ST_ROT = 0, 3, 6, 9, 12
ST_EULER_D, ST_POS_D, ST_ANG_VEL_D, ST_LIN_VEL_D, ST_FEET = 21, 24, 27, 30, 33
ST_MASS, ST_INERTIA, ST_MU, ST_FZMIN, ST_FZMAX, ST_DT, ST_CONTACTS, ST_SIZE = 45, 46, 55, 56, 57, 58, 59, 64
# torque-map record layout (include/mpcqp.h MPCQP_TQ_*)
TQ_JFOOT, TQ_FKIN, TQ_KM, TQ_GRAV, TQ_CONTACTS, TQ_SIZE = 0, 36, 48, 51, 63, 68
# leg-plan input row and window sizes (include/mpcqp.h MPCQP_PL_*, MPCQP_PLAN_*; the output row is
# legplan.PLAN_OUT_DTYPE)
PL_ROT_Z, PL_FOOT_FORCE, PL_MOVEMENT_MODE, PL_SIZE = 0, 9, 13, 16
PO_SIZE = 108
PLAN_CONTACT_WINDOW, PLAN_TERRAIN_WINDOW = 60, 100
# state front end: sensor row and optional output row (include/mpcqp.h MPCQP_SN_*, MPCQP_EO_*)
SN_QUAT, SN_JOINT_POS, SN_JOINT_VEL, SN_IMU_ACC, SN_IMU_ANG_VEL, SN_SIZE = 0, 4, 16, 28, 31, 36
EO_FOOT_POS_REL, EO_FOOT_VEL_REL, EO_FOOT_VEL_ABS, EO_CONTACT_W, EO_X, EO_DIAG_P, EO_DET = 0, 12, 24, 36, 40, 58, 76
EO_SIZE = 80
BAL_SIZE = 72  # balance record (include/mpcqp.h MPCQP_BAL_*; the offsets are balance.BAL_*)
# command stage: command row and slot (include/mpcqp.h MPCQP_CM_*, MPCQP_CS_*)
CM_VEL, CM_RATE, CM_MODE_REQUEST, CM_SIZE = 0, 3, 6, 8
CS_INIT, CS_BODY_HEIGHT, CS_CTRL_STATE, CS_PREV_CTRL_STATE, CS_KP_LINEAR, CS_SIZE = 0, 1, 2, 3, 4, 8
# policy stage: slot and optional output row (include/mpcqp.h MPCQP_PS_*, MPCQP_PY_*)
PS_INIT, PS_TICK, PS_SERVO_TIME, PS_MODE, PS_PREV_ACTION, PS_TARGET, PS_SIZE = 0, 1, 2, 3, 4, 16, 28
PY_OBS, PY_RAW, PY_ACTION, PY_TARGET, PY_TORQUE, PY_STATUS, PY_UPDATED, PY_SIZE = 0, 48, 60, 72, 84, 96, 97, 100
# plant stage: slot, init row and optional output row (include/mpcqp.h MPCQP_PN_*, MPCQP_PI_*, MPCQP_PT_*)
PN_INIT, PN_POS, PN_QUAT, PN_LIN_VEL, PN_ANG_VEL, PN_JOINT_POS, PN_JOINT_VEL = 0, 1, 4, 8, 11, 14, 26
PN_FOOT, PN_CONTACT, PN_ACC, PN_STATUS, PN_SIZE = 38, 50, 54, 57, 64
PI_POS, PI_QUAT, PI_JOINT_POS, PI_SIZE = 0, 3, 7, 20
PT_POS, PT_QUAT, PT_EULER, PT_LIN_VEL, PT_ANG_VEL, PT_CONTACTS, PT_GRF, PT_FOOT, PT_ACC = 0, 3, 7, 10, 13, 16, 20, 32, 44
PT_STATUS, PT_SIZE = 47, 48
# terrain row of the plant stage (include/mpcqp.h MPCQP_TR_*)
TR_NORMAL, TR_OFFSET, TR_MU, TR_SIZE = 0, 3, 4, 8
# height-field header row of the plant stage (include/mpcqp.h MPCQP_HF_*)
HF_X0, HF_Y0, HF_CELL, HF_MU, HF_NX, HF_NY, HF_OFFSET, HF_SIZE = 0, 1, 2, 3, 4, 5, 6, 8


def rec_feet(N):
    return REC_XREF + 13 * N


def rec_size(N):
    return REC_XREF + 25 * N + (N & 1)


# OSQP 0.6 status values
STATUS_SOLVED = 1
STATUS_SOLVED_INACCURATE = 2
STATUS_PRIMAL_INFEASIBLE_INACCURATE = 3
STATUS_DUAL_INFEASIBLE_INACCURATE = 4
STATUS_MAX_ITER_REACHED = -2
STATUS_PRIMAL_INFEASIBLE = -3
STATUS_DUAL_INFEASIBLE = -4
STATUS_NON_CVX = -7
STATUS_NAN_INPUT = -100
STATUS_UNSOLVED = -10

ERR_OK, ERR_INVALID_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_ALLOC = 0, 1, 2, 3, 4


class Params(ctypes.Structure):
    """mpcqp_params."""
    _fields_ = [
        ("horizon", ctypes.c_int32), ("max_iter", ctypes.c_int32), ("scaling", ctypes.c_int32),
        ("check_termination", ctypes.c_int32), ("adaptive_rho", ctypes.c_int32),
        ("adaptive_rho_interval", ctypes.c_int32), ("scaled_termination", ctypes.c_int32),
        ("warm_start", ctypes.c_int32),
        ("q_weights", ctypes.c_double * 13), ("r_weights", ctypes.c_double * 12),
        ("rho", ctypes.c_double), ("sigma", ctypes.c_double), ("alpha", ctypes.c_double),
        ("eps_abs", ctypes.c_double), ("eps_rel", ctypes.c_double),
        ("eps_prim_inf", ctypes.c_double), ("eps_dual_inf", ctypes.c_double),
        ("adaptive_rho_tolerance", ctypes.c_double),
    ]


class BalanceParams(ctypes.Structure):
    """mpcqp_balance_params."""
    _fields_ = [("q_diag", ctypes.c_double * 6), ("r", ctypes.c_double), ("mu", ctypes.c_double),
                ("f_min", ctypes.c_double), ("f_max", ctypes.c_double)]


class BalanceGains(ctypes.Structure):
    """mpcqp_balance_gains."""
    _fields_ = [("kp_linear", ctypes.c_double * 3), ("kd_linear", ctypes.c_double * 3),
                ("kp_angular", ctypes.c_double * 3), ("kd_angular", ctypes.c_double * 3)]


class CommandParams(ctypes.Structure):
    """mpcqp_command_params."""
    _fields_ = [("body_height_init", ctypes.c_double), ("body_height_max", ctypes.c_double),
                ("body_height_min", ctypes.c_double), ("vel_lock_threshold", ctypes.c_double),
                ("kp_linear", ctypes.c_double * 3), ("kp_linear_lock_x", ctypes.c_double),
                ("kp_linear_lock_y", ctypes.c_double)]


class PolicyParams(ctypes.Structure):
    """mpcqp_policy_params."""
    _fields_ = [
        ("n_hidden", ctypes.c_int32), ("hidden", ctypes.c_int32 * 3), ("servo_clamp", ctypes.c_int32),
        ("decimation", ctypes.c_int32), ("obs_scale", ctypes.c_double * 36), ("clip_obs", ctypes.c_double),
        ("clip_action", ctypes.c_double), ("action_scale", ctypes.c_double),
        ("default_joint_pos", ctypes.c_double * 12), ("pose_lower", ctypes.c_double * 12),
        ("pose_upper", ctypes.c_double * 12), ("kp_walk", ctypes.c_double * 12), ("kd_walk", ctypes.c_double * 12),
        ("kp_servo", ctypes.c_double * 12), ("kd_servo", ctypes.c_double * 12), ("stand_pos", ctypes.c_double * 12),
        ("servo_ticks", ctypes.c_double),
    ]


class PlanParams(ctypes.Structure):
    """mpcqp_plan_params."""
    _fields_ = [
        ("default_foot_pos", ctypes.c_double * 12), ("kp_foot", ctypes.c_double * 12),
        ("kd_foot", ctypes.c_double * 12), ("gait_counter_speed", ctypes.c_double * 4),
        ("gait_counter_init", ctypes.c_double * 4), ("counter_per_gait", ctypes.c_double),
        ("counter_per_swing", ctypes.c_double), ("control_dt", ctypes.c_double),
        ("foot_force_low", ctypes.c_double), ("foot_delta_x_limit", ctypes.c_double),
        ("foot_delta_y_limit", ctypes.c_double), ("swing_clearance1", ctypes.c_double),
        ("swing_clearance2", ctypes.c_double), ("terrain", ctypes.c_int32), ("use_terrain_adapt", ctypes.c_int32),
    ]


class EstimatorParams(ctypes.Structure):
    """mpcqp_est_params."""
    _fields_ = [
        ("rho_fix", ctypes.c_double * 20), ("rho_opt", ctypes.c_double * 12),
        ("process_noise_pimu", ctypes.c_double), ("process_noise_vimu", ctypes.c_double),
        ("process_noise_pfoot", ctypes.c_double), ("sensor_noise_pimu_rel_foot", ctypes.c_double),
        ("sensor_noise_vimu_rel_foot", ctypes.c_double), ("sensor_noise_zfoot", ctypes.c_double),
        ("height_noise_no_flat", ctypes.c_double), ("init_height", ctypes.c_double), ("init_cov", ctypes.c_double),
        ("gravity", ctypes.c_double), ("contact_force_scale", ctypes.c_double), ("drift_threshold", ctypes.c_double),
        ("drift_divisor", ctypes.c_double), ("assume_flat_ground", ctypes.c_int32), ("pad_", ctypes.c_int32),
    ]


class PlantParams(ctypes.Structure):
    """mpcqp_plant_params."""
    _fields_ = [
        ("rho_fix", ctypes.c_double * 20), ("rho_opt", ctypes.c_double * 12), ("mass", ctypes.c_double),
        ("inertia", ctypes.c_double * 9), ("mu", ctypes.c_double), ("gravity", ctypes.c_double),
        ("joint_inertia", ctypes.c_double * 3), ("joint_damping", ctypes.c_double * 3),
        ("default_joint_pos", ctypes.c_double * 12), ("min_height", ctypes.c_double),
        ("substeps", ctypes.c_int32), ("pad_", ctypes.c_int32),
    ]


class EpisodeParams(ctypes.Structure):
    """mpcqp_episode_params."""
    _fields_ = [
        ("dt", ctypes.c_double), ("tilt_max", ctypes.c_double), ("height_min", ctypes.c_double),
        ("height_max", ctypes.c_double), ("seed", ctypes.c_uint32 * 2), ("max_ticks", ctypes.c_int32),
        ("pool_count", ctypes.c_int32), ("script_count", ctypes.c_int32), ("script_segments", ctypes.c_int32),
        ("log_len", ctypes.c_int32), ("pad_", ctypes.c_int32),
    ]


class EpisodeBuffers(ctypes.Structure):
    """mpcqp_episode_buffers."""
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "d_plant_out", "d_plant_state", "d_plant_init", "d_joint_torques", "d_sensors", "d_cmd", "d_results", "d_pool",
        "d_scripts", "d_states", "d_counter", "d_log", "d_totals", "d_est_state", "d_plan_state", "d_cmd_state",
        "d_policy_state", "d_warm")] + [(name, ctypes.c_int32) for name in (
            "est_state_size", "plan_state_size", "cmd_state_size", "policy_state_size", "warm_size", "pad_")]


class DisturbParams(ctypes.Structure):
    """mpcqp_disturb_params."""
    _fields_ = [
        ("load_mass_max", ctypes.c_double), ("gravity", ctypes.c_double), ("load_point", ctypes.c_double * 3),
        ("bias_acc", ctypes.c_double), ("bias_gyro", ctypes.c_double), ("push_force", ctypes.c_double * 2),
        ("push_point", ctypes.c_double * 3), ("sigma", ctypes.c_double * 4), ("seed", ctypes.c_uint32 * 2),
        ("push_start", ctypes.c_int32), ("push_interval", ctypes.c_int32), ("push_duration", ctypes.c_int32),
        ("dir_count", ctypes.c_int32),
    ]


class DisturbBuffers(ctypes.Structure):
    """mpcqp_disturb_buffers."""
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "d_episode_state", "d_wrench", "d_sensors", "d_sensors_noisy", "d_dirs", "d_disturb_out")]


class Result(ctypes.Structure):
    """mpcqp_result."""
    _fields_ = [
        ("u0", ctypes.c_double * 12), ("f_body", ctypes.c_double * 12),
        ("obj_val", ctypes.c_double), ("pri_res", ctypes.c_double), ("dua_res", ctypes.c_double),
        ("rho", ctypes.c_double), ("status", ctypes.c_int32), ("iters", ctypes.c_int32),
        ("rho_updates", ctypes.c_int32), ("nan_legs", ctypes.c_int32),
    ]


RESULT_DTYPE = np.dtype([
    ("u0", "f8", 12), ("f_body", "f8", 12), ("obj_val", "f8"), ("pri_res", "f8"),
    ("dua_res", "f8"), ("rho", "f8"), ("status", "i4"), ("iters", "i4"),
    ("rho_updates", "i4"), ("nan_legs", "i4"),
])
RESULT_DOUBLES = RESULT_DTYPE.itemsize // 8  # 30

# every symbol declared by include/mpcqp.h and include/mpcqp_debug.h
EXPORTED = [
    "mpcqp_default_params", "mpcqp_record_size", "mpcqp_create", "mpcqp_destroy", "mpcqp_reserve",
    "mpcqp_solve_batch_device", "mpcqp_solve_batch_host", "mpcqp_build_qp_device",
    "mpcqp_status_str", "mpcqp_error_str", "mpcqp_last_error",
    "mpcqp_debug_solve_trace_device", "mpcqp_abi_sizes", "mpcqp_handle_slots", "mpcqp_solve_threads",
    "mpcqp_debug_set_solver", "mpcqp_debug_wave_selftest", "mpcqp_joint_torques_device",
    "mpcqp_warm_state_size", "mpcqp_solve_batch_warm_device",
    "mpcqp_balance_default_params", "mpcqp_balance_solve_device", "mpcqp_assemble_records_device",
    "mpcqp_balance_solve_host", "mpcqp_solve_batch_warm_host",
    "mpcqp_debug_scale_image_doubles", "mpcqp_debug_scale_image_device", "mpcqp_copy_warm_slots_device",
    "mpcqp_handoff_counts",
    "mpcqp_debug_set_split", "mpcqp_debug_split_parts",
    "mpcqp_set_order_hint", "mpcqp_debug_launch_order",
    "mpcqp_plan_default_params", "mpcqp_plan_state_size", "mpcqp_leg_plan_device",
    "mpcqp_est_default_params", "mpcqp_est_params_size", "mpcqp_estimator_state_size",
    "mpcqp_state_estimate_device",
    "mpcqp_command_default_params", "mpcqp_command_state_size", "mpcqp_command_device",
    "mpcqp_balance_default_gains", "mpcqp_assemble_balance_device",
    "mpcqp_balance_solve_typed_device", "mpcqp_solve_batch_warm_typed_device", "mpcqp_leg_plan_typed_device",
    "mpcqp_policy_default_params", "mpcqp_policy_params_size", "mpcqp_policy_create", "mpcqp_policy_destroy",
    "mpcqp_policy_state_size", "mpcqp_policy_device",
    "mpcqp_plant_default_params", "mpcqp_plant_params_size", "mpcqp_plant_state_size", "mpcqp_plant_step_device",
    "mpcqp_episode_default_params", "mpcqp_episode_params_size", "mpcqp_episode_buffers_size",
    "mpcqp_episode_state_size", "mpcqp_episode_device",
    "mpcqp_plant_step_wrench_device", "mpcqp_disturb_default_params", "mpcqp_disturb_params_size",
    "mpcqp_disturb_buffers_size", "mpcqp_disturb_device",
    "mpcqp_plant_step_terrain_device", "mpcqp_plant_step_field_device",
]

_libs = {}


class MpcQpError(RuntimeError):
    pass


def load(debug=False):
    """Load libmpcqp.so, or libmpcqp_debug.so with debug=True (raises if it has not been built)."""
    if debug in _libs:
        return _libs[debug]
    path = DEBUG_LIB_PATH if debug else LIB_PATH
    if not os.path.exists(path):
        raise MpcQpError(f"{path} not built: run `make -C {PKG_ROOT}` (or __graft_entry__.build())")
    L = ctypes.CDLL(path)
    vp, dp, i32 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int32
    L.mpcqp_default_params.argtypes = [ctypes.POINTER(Params), i32]
    L.mpcqp_default_params.restype = None
    L.mpcqp_record_size.argtypes = [i32]
    L.mpcqp_record_size.restype = i32
    L.mpcqp_create.argtypes = [ctypes.POINTER(Params), i32, ctypes.POINTER(vp)]
    L.mpcqp_create.restype = i32
    L.mpcqp_destroy.argtypes = [vp]
    L.mpcqp_destroy.restype = i32
    L.mpcqp_reserve.argtypes = [vp, i32]
    L.mpcqp_reserve.restype = i32
    L.mpcqp_solve_batch_device.argtypes = [vp, vp, i32, vp, vp, vp]
    L.mpcqp_solve_batch_device.restype = i32
    L.mpcqp_solve_batch_host.argtypes = [vp, dp, i32, vp, dp]
    L.mpcqp_solve_batch_host.restype = i32
    L.mpcqp_build_qp_device.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.mpcqp_build_qp_device.restype = i32
    L.mpcqp_status_str.argtypes = [i32]
    L.mpcqp_status_str.restype = ctypes.c_char_p
    L.mpcqp_error_str.argtypes = [i32]
    L.mpcqp_error_str.restype = ctypes.c_char_p
    L.mpcqp_last_error.argtypes = [vp]
    L.mpcqp_last_error.restype = ctypes.c_char_p
    L.mpcqp_debug_solve_trace_device.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp]
    L.mpcqp_debug_solve_trace_device.restype = i32
    L.mpcqp_abi_sizes.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.mpcqp_abi_sizes.restype = i32
    L.mpcqp_handle_slots.argtypes = [vp]
    L.mpcqp_handle_slots.restype = i32
    L.mpcqp_solve_threads.argtypes = [i32]
    L.mpcqp_solve_threads.restype = i32
    L.mpcqp_debug_set_solver.argtypes = [vp, i32]
    L.mpcqp_debug_set_solver.restype = i32
    L.mpcqp_debug_wave_selftest.argtypes = [vp, vp]
    L.mpcqp_debug_wave_selftest.restype = i32
    if hasattr(L, "mpcqp_debug_scale_image_device"):  # (absent from older experiment builds)
        L.mpcqp_debug_scale_image_doubles.argtypes = [i32]
        L.mpcqp_debug_scale_image_doubles.restype = i32
        L.mpcqp_debug_scale_image_device.argtypes = [vp, vp, i32, vp, vp, vp]
        L.mpcqp_debug_scale_image_device.restype = i32
    L.mpcqp_joint_torques_device.argtypes = [vp, vp, i32, vp, vp, vp]
    L.mpcqp_joint_torques_device.restype = i32
    L.mpcqp_warm_state_size.argtypes = [i32]
    L.mpcqp_warm_state_size.restype = i32
    L.mpcqp_solve_batch_warm_device.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.mpcqp_solve_batch_warm_device.restype = i32
    L.mpcqp_solve_batch_warm_host.argtypes = [vp, dp, i32, vp, vp, dp]
    L.mpcqp_solve_batch_warm_host.restype = i32
    L.mpcqp_balance_default_params.argtypes = [ctypes.POINTER(BalanceParams)]
    L.mpcqp_balance_default_params.restype = None
    L.mpcqp_balance_solve_device.argtypes = [vp, ctypes.POINTER(BalanceParams), vp, i32, vp, vp]
    L.mpcqp_balance_solve_device.restype = i32
    L.mpcqp_balance_solve_host.argtypes = [vp, ctypes.POINTER(BalanceParams), dp, i32, vp]
    L.mpcqp_balance_solve_host.restype = i32
    L.mpcqp_assemble_records_device.argtypes = [i32, vp, i32, vp, vp]
    L.mpcqp_assemble_records_device.restype = i32
    L.mpcqp_copy_warm_slots_device.argtypes = [i32, vp, vp, vp, vp, i32, vp]
    L.mpcqp_copy_warm_slots_device.restype = i32
    L.mpcqp_handoff_counts.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.mpcqp_handoff_counts.restype = i32
    L.mpcqp_debug_set_split.argtypes = [vp, i32]
    L.mpcqp_debug_set_split.restype = i32
    L.mpcqp_debug_split_parts.argtypes = [vp, i32]
    L.mpcqp_debug_split_parts.restype = i32
    if hasattr(L, "mpcqp_set_order_hint"):  # (absent from an older library given by MPCQP_LIB for an A/B)
        L.mpcqp_set_order_hint.argtypes = [vp, i32]
        L.mpcqp_set_order_hint.restype = i32
        L.mpcqp_debug_launch_order.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), i32]
        L.mpcqp_debug_launch_order.restype = i32
    L.mpcqp_plan_default_params.argtypes = [ctypes.POINTER(PlanParams)]
    L.mpcqp_plan_default_params.restype = None
    L.mpcqp_plan_state_size.argtypes = []
    L.mpcqp_plan_state_size.restype = i32
    L.mpcqp_leg_plan_device.argtypes = [ctypes.POINTER(PlanParams), ctypes.c_double, vp, vp, i32, vp, vp, vp, vp]
    L.mpcqp_leg_plan_device.restype = i32
    L.mpcqp_est_default_params.argtypes = [ctypes.POINTER(EstimatorParams)]
    L.mpcqp_est_default_params.restype = None
    L.mpcqp_est_params_size.argtypes = []
    L.mpcqp_est_params_size.restype = i32
    L.mpcqp_estimator_state_size.argtypes = []
    L.mpcqp_estimator_state_size.restype = i32
    L.mpcqp_state_estimate_device.argtypes = [ctypes.POINTER(EstimatorParams), ctypes.c_double, vp, vp, vp, i32, vp,
                                              vp, vp, vp]
    L.mpcqp_state_estimate_device.restype = i32
    L.mpcqp_command_default_params.argtypes = [ctypes.POINTER(CommandParams)]
    L.mpcqp_command_default_params.restype = None
    L.mpcqp_command_state_size.argtypes = []
    L.mpcqp_command_state_size.restype = i32
    L.mpcqp_command_device.argtypes = [ctypes.POINTER(CommandParams), ctypes.c_double, vp, vp, vp, i32, vp, vp]
    L.mpcqp_command_device.restype = i32
    L.mpcqp_balance_default_gains.argtypes = [ctypes.POINTER(BalanceGains)]
    L.mpcqp_balance_default_gains.restype = None
    L.mpcqp_assemble_balance_device.argtypes = [ctypes.POINTER(BalanceGains), vp, vp, vp, i32, vp, vp]
    L.mpcqp_assemble_balance_device.restype = i32
    L.mpcqp_balance_solve_typed_device.argtypes = [vp, ctypes.POINTER(BalanceParams), vp, i32, vp, i32, vp, vp]
    L.mpcqp_balance_solve_typed_device.restype = i32
    L.mpcqp_solve_batch_warm_typed_device.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp]
    L.mpcqp_solve_batch_warm_typed_device.restype = i32
    L.mpcqp_leg_plan_typed_device.argtypes = [ctypes.POINTER(PlanParams), ctypes.c_double, vp, vp, i32, vp, vp, vp,
                                              vp, vp]
    L.mpcqp_leg_plan_typed_device.restype = i32
    if hasattr(L, "mpcqp_policy_device"):  # (absent from an older library given by MPCQP_LIB for an A/B)
        fpp = ctypes.POINTER(ctypes.POINTER(ctypes.c_float))
        L.mpcqp_policy_default_params.argtypes = [ctypes.POINTER(PolicyParams)]
        L.mpcqp_policy_default_params.restype = None
        L.mpcqp_policy_params_size.argtypes = []
        L.mpcqp_policy_params_size.restype = i32
        L.mpcqp_policy_create.argtypes = [ctypes.POINTER(PolicyParams), fpp, fpp, i32, ctypes.POINTER(vp)]
        L.mpcqp_policy_create.restype = i32
        L.mpcqp_policy_destroy.argtypes = [vp]
        L.mpcqp_policy_destroy.restype = i32
        L.mpcqp_policy_state_size.argtypes = []
        L.mpcqp_policy_state_size.restype = i32
        L.mpcqp_policy_device.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp]
        L.mpcqp_policy_device.restype = i32
        if L.mpcqp_policy_params_size() != ctypes.sizeof(PolicyParams):
            raise MpcQpError(f"ABI mismatch: mpcqp_policy_params is {L.mpcqp_policy_params_size()} bytes in C, "
                             f"{ctypes.sizeof(PolicyParams)} in ctypes")
    if hasattr(L, "mpcqp_plant_step_device"):  # (absent from an older library given by MPCQP_LIB for an A/B)
        L.mpcqp_plant_default_params.argtypes = [ctypes.POINTER(PlantParams)]
        L.mpcqp_plant_default_params.restype = None
        L.mpcqp_plant_params_size.argtypes = []
        L.mpcqp_plant_params_size.restype = i32
        L.mpcqp_plant_state_size.argtypes = []
        L.mpcqp_plant_state_size.restype = i32
        L.mpcqp_plant_step_device.argtypes = [ctypes.POINTER(PlantParams), ctypes.c_double, vp, i32, vp, vp, vp, vp,
                                              vp, vp, vp, vp]
        L.mpcqp_plant_step_device.restype = i32
        if L.mpcqp_plant_params_size() != ctypes.sizeof(PlantParams):
            raise MpcQpError(f"ABI mismatch: mpcqp_plant_params is {L.mpcqp_plant_params_size()} bytes in C, "
                             f"{ctypes.sizeof(PlantParams)} in ctypes")
    if hasattr(L, "mpcqp_episode_device"):  # (absent from an older library given by MPCQP_LIB for an A/B)
        L.mpcqp_episode_default_params.argtypes = [ctypes.POINTER(EpisodeParams)]
        L.mpcqp_episode_default_params.restype = None
        for name in ("mpcqp_episode_params_size", "mpcqp_episode_buffers_size", "mpcqp_episode_state_size"):
            getattr(L, name).argtypes = []
            getattr(L, name).restype = i32
        L.mpcqp_episode_device.argtypes = [ctypes.POINTER(EpisodeParams), ctypes.POINTER(EpisodeBuffers), i32, vp, vp]
        L.mpcqp_episode_device.restype = i32
        if (L.mpcqp_episode_params_size() != ctypes.sizeof(EpisodeParams) or
                L.mpcqp_episode_buffers_size() != ctypes.sizeof(EpisodeBuffers)):
            raise MpcQpError(f"ABI mismatch: mpcqp_episode_params / _buffers are {L.mpcqp_episode_params_size()} / "
                             f"{L.mpcqp_episode_buffers_size()} bytes in C, {ctypes.sizeof(EpisodeParams)} / "
                             f"{ctypes.sizeof(EpisodeBuffers)} in ctypes")
    if hasattr(L, "mpcqp_disturb_device"):  # (absent from an older library given by MPCQP_LIB for an A/B)
        L.mpcqp_plant_step_wrench_device.argtypes = [ctypes.POINTER(PlantParams), ctypes.c_double, vp, vp, i32, vp, vp,
                                                     vp, vp, vp, vp, vp, vp]
        L.mpcqp_plant_step_wrench_device.restype = i32
        L.mpcqp_disturb_default_params.argtypes = [ctypes.POINTER(DisturbParams)]
        L.mpcqp_disturb_default_params.restype = None
        for name in ("mpcqp_disturb_params_size", "mpcqp_disturb_buffers_size"):
            getattr(L, name).argtypes = []
            getattr(L, name).restype = i32
        L.mpcqp_disturb_device.argtypes = [ctypes.POINTER(DisturbParams), ctypes.POINTER(DisturbBuffers), i32, vp]
        L.mpcqp_disturb_device.restype = i32
        if (L.mpcqp_disturb_params_size() != ctypes.sizeof(DisturbParams) or
                L.mpcqp_disturb_buffers_size() != ctypes.sizeof(DisturbBuffers)):
            raise MpcQpError(f"ABI mismatch: mpcqp_disturb_params / _buffers are {L.mpcqp_disturb_params_size()} / "
                             f"{L.mpcqp_disturb_buffers_size()} bytes in C, {ctypes.sizeof(DisturbParams)} / "
                             f"{ctypes.sizeof(DisturbBuffers)} in ctypes")
    if hasattr(L, "mpcqp_plant_step_terrain_device"):  # (absent from an older library given by MPCQP_LIB for an A/B)
        L.mpcqp_plant_step_terrain_device.argtypes = [ctypes.POINTER(PlantParams), ctypes.c_double, vp, vp, vp, i32, vp,
                                                      i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.mpcqp_plant_step_terrain_device.restype = i32
    if hasattr(L, "mpcqp_plant_step_field_device"):
        L.mpcqp_plant_step_field_device.argtypes = [ctypes.POINTER(PlantParams), ctypes.c_double, vp, vp, vp, i32, vp,
                                                    i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.mpcqp_plant_step_field_device.restype = i32
    if L.mpcqp_est_params_size() != ctypes.sizeof(EstimatorParams):
        raise MpcQpError(f"ABI mismatch: mpcqp_est_params is {L.mpcqp_est_params_size()} bytes in C, "
                         f"{ctypes.sizeof(EstimatorParams)} in ctypes")
    ps, rs = i32(0), i32(0)
    L.mpcqp_abi_sizes(ctypes.byref(ps), ctypes.byref(rs))
    if ps.value != ctypes.sizeof(Params) or rs.value != ctypes.sizeof(Result):
        raise MpcQpError(f"ABI mismatch: C sizes {ps.value}/{rs.value} vs ctypes "
                         f"{ctypes.sizeof(Params)}/{ctypes.sizeof(Result)}")
    _libs[debug] = L
    return L


def override(struct, over, special=None):
    """Apply keyword overrides to a parameter structure and return it.  A c_double array field takes anything that
    flattens to exactly its length; any other field is set; a name that is not a field raises AttributeError
    (setattr on a ctypes structure would accept and ignore it).  ``special`` maps a name to ``set(struct, value)``
    for the overrides that are not a plain field assignment."""
    fields = dict(struct._fields_)
    for k, v in over.items():
        if special and k in special:
            special[k](struct, v)
        elif k not in fields:
            raise AttributeError(f"{type(struct).__name__} has no field {k!r}")
        elif issubclass(fields[k], ctypes.Array) and fields[k]._type_ is ctypes.c_double:
            arr = getattr(struct, k)
            flat = np.asarray(v, dtype=np.float64).reshape(-1)
            if flat.size != len(arr):
                raise ValueError(f"{k}: expected {len(arr)} values, got {flat.size}")
            arr[:] = flat.tolist()
        else:
            setattr(struct, k, v)
    return struct


def set_seed(struct, v):
    """The ``seed`` override of the episode and disturbance parameters: one 64-bit integer into uint32[2]."""
    struct.seed[0], struct.seed[1] = int(v) & 0xFFFFFFFF, (int(v) >> 32) & 0xFFFFFFFF


def default_params(horizon=10, **over):
    """mpcqp_default_params + keyword overrides (q_weights/r_weights accept sequences)."""
    p = Params()
    load().mpcqp_default_params(ctypes.byref(p), horizon)
    return override(p, over)


def assemble_records_device(horizon, d_states, batch, d_records, stream=0):
    """mpcqp_assemble_records_device: raw-state rows [batch][ST_SIZE] -> MPC records, on the device."""
    check(load().mpcqp_assemble_records_device(int(horizon), d_states, int(batch), d_records, stream or None),
          None, "mpcqp_assemble_records_device")


def copy_warm_slots_device(horizon, d_src, d_src_idx, d_dst, d_dst_idx, count, stream=None):
    """mpcqp_copy_warm_slots_device: slot d_dst[dst_idx[i]] = slot d_src[src_idx[i]] (device int32
    index arrays, None = identity), i < count."""
    check(load().mpcqp_copy_warm_slots_device(int(horizon), d_src, d_src_idx or None, d_dst, d_dst_idx or None,
                                                int(count), stream or None), None, "mpcqp_copy_warm_slots_device")


def default_balance_params(**over):
    """mpcqp_balance_default_params (A1RobotControl.cpp:11-15) + keyword overrides."""
    bp = BalanceParams()
    load().mpcqp_balance_default_params(ctypes.byref(bp))
    return override(bp, over)


def check(rc, handle=None, what="mpcqp", lib=None):
    if rc != ERR_OK:
        L = lib or load()
        msg = L.mpcqp_error_str(rc).decode()
        if handle:
            msg += ": " + L.mpcqp_last_error(handle).decode()
        raise MpcQpError(f"{what} failed ({rc}): {msg}")


def status_str(s):
    return load().mpcqp_status_str(int(s)).decode()
