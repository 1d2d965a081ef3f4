"""Upstream leg plan of the control tick (host side of mpcqp_leg_plan_device).

Per robot and per tick the device stage runs ``A1RobotControl::update_plan``
(src/a1_cpp/src/A1RobotControl.cpp:148-202), ``generate_swing_legs_ctrl`` (:204-287) and the terrain
adaptation of ``compute_grf`` (:335-376), and writes the contacts, the swing-leg PD force and the
terrain-adapted ``root_euler_d[1]`` into the rows the assemble / solve / torque-map stages read.  The
controller's persistent state (gait counters, swing start points, the 13 moving-window filters) lives
in a per-robot device slot of ``plan_state_size()`` doubles; zero-filled = a freshly reset controller.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import PL_FOOT_FORCE, PL_MOVEMENT_MODE, PL_ROT_Z, PL_SIZE, PlanParams, check, load, override

# the output row (include/mpcqp.h MPCQP_PO_*), [leg][xyz] where 12 wide, flags as 0.0 / 1.0
PLAN_OUT_DTYPE = np.dtype([
    ("foot_pos_target_rel", "f8", (4, 3)), ("foot_pos_target_abs", "f8", (4, 3)),
    ("foot_pos_target_world", "f8", (4, 3)), ("foot_pos_cur", "f8", (4, 3)),
    ("foot_pos_target", "f8", (4, 3)), ("foot_forces_kin", "f8", (4, 3)),
    ("foot_pos_recent_contact", "f8", (4, 3)), ("gait_counter", "f8", 4), ("plan_contacts", "f8", 4),
    ("early_contacts", "f8", 4), ("contacts", "f8", 4), ("plane", "f8", 3), ("angle_cos", "f8"),
    ("terrain_pitch_angle", "f8"), ("pad", "f8", 3),
])
assert PLAN_OUT_DTYPE.itemsize == 8 * _lib.PO_SIZE

def default_plan_params(**over):
    """mpcqp_plan_default_params (A1CtrlStates::reset(), A1Params.h:38-45) + keyword overrides; the
    [4][3] fields accept anything that flattens to 12 values leg-major."""
    p = PlanParams()
    load().mpcqp_plan_default_params(ctypes.byref(p))
    return override(p, over)


def plan_state_size():
    """Doubles per robot of the plan slot (mpcqp_plan_state_size)."""
    return int(load().mpcqp_plan_state_size())


def pack_plan_inputs(rot_z, foot_force, movement_mode):
    """Plan input rows [B, PL_SIZE] (include/mpcqp.h MPCQP_PL_*): rot_z [B,3,3] root_rot_mat_z,
    foot_force [B,4], movement_mode [B] or scalar (0 standstill, nonzero walk)."""
    rz = np.asarray(rot_z, dtype=np.float64)
    B = rz.shape[0]
    row = np.zeros((B, PL_SIZE))
    row[:, PL_ROT_Z:PL_ROT_Z + 9] = rz.reshape(B, 9)
    row[:, PL_FOOT_FORCE:PL_FOOT_FORCE + 4] = np.asarray(foot_force, dtype=np.float64).reshape(B, 4)
    row[:, PL_MOVEMENT_MODE] = (np.broadcast_to(np.asarray(movement_mode), (B,)) != 0).astype(np.float64)
    return row


def unpack_plan_inputs(rows):
    """Inverse of pack_plan_inputs: (rot_z [B,3,3], foot_force [B,4], movement_mode [B] int)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, PL_SIZE)
    return (rows[:, PL_ROT_Z:PL_ROT_Z + 9].reshape(-1, 3, 3).copy(), rows[:, PL_FOOT_FORCE:PL_FOOT_FORCE + 4].copy(),
            (rows[:, PL_MOVEMENT_MODE] != 0).astype(np.int64))


def leg_plan_device(plan, dt, d_states, d_plan_in, batch, d_plan_state, d_tq_records=0, d_plan_out=0, stream=0):
    """mpcqp_leg_plan_device on device pointers (ints; 0 for the optional ones)."""
    check(load().mpcqp_leg_plan_device(ctypes.byref(plan), float(dt), d_states, d_plan_in, int(batch), d_plan_state,
                                       d_tq_records or None, d_plan_out or None, stream or None),
          None, "mpcqp_leg_plan_device")


def leg_plan_typed_device(plan, dt, d_states, d_plan_in, batch, d_plan_state, d_tq_records=0, d_plan_out=0, d_type=0,
                          stream=0):
    """mpcqp_leg_plan_typed_device: the plan tick with the terrain adaptation only for the robots with
    d_type[b] == 1 (A1RobotControl.cpp:335); d_type a device int32 [batch] pointer, 0 = mpcqp_leg_plan_device."""
    check(load().mpcqp_leg_plan_typed_device(ctypes.byref(plan), float(dt), d_states, d_plan_in, int(batch),
                                             d_plan_state, d_tq_records or None, d_plan_out or None, d_type or None,
                                             stream or None), None, "mpcqp_leg_plan_typed_device")
