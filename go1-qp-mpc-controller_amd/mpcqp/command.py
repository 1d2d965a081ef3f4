"""Command stage of the control tick (host side of mpcqp_command_device).

Per robot and per tick the device stage runs the joystick command block at the top of ``main_update``
(src/a1_cpp/src/GazeboA1ROS.cpp:122-188): the body height with its clamp, the walk / stand toggle,
``root_lin_vel_d`` / ``root_ang_vel_d``, the ``root_euler_d`` integration, ``root_pos_d``, ``movement_mode``
and the position lock that zeroes or restores ``kp_linear``.  The caller writes one command row per robot
(the ``joy_cmd_*`` members, already scaled as ``joy_callback`` does, :390-416); what the block keeps between
ticks lives in a per-robot device slot of ``command_state_size()`` doubles, zero-filled = fresh.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import CM_MODE_REQUEST, CM_RATE, CM_SIZE, CM_VEL, CommandParams, check, load, override

# the slot (include/mpcqp.h MPCQP_CS_*); flags and states as 0.0 / 1.0
CMD_STATE_DTYPE = np.dtype([
    ("init", "f8"), ("body_height", "f8"), ("ctrl_state", "f8"), ("prev_ctrl_state", "f8"),
    ("kp_linear", "f8", 3), ("pad", "f8"),
])
assert CMD_STATE_DTYPE.itemsize == 8 * _lib.CS_SIZE


def default_command_params(**over):
    """mpcqp_command_default_params (GazeboA1ROS.h:133, A1Params.h:16-17, GazeboA1ROS.cpp:180,
    Go1CtrlStates.hpp:279-281, :304-305) + keyword overrides (kp_linear: a sequence of 3)."""
    p = CommandParams()
    load().mpcqp_command_default_params(ctypes.byref(p))
    return override(p, over)


def command_state_size():
    """Doubles per robot of the command slot (mpcqp_command_state_size)."""
    return int(load().mpcqp_command_state_size())


def pack_commands(vel, rate, mode_request):
    """Command rows [B, CM_SIZE] (include/mpcqp.h MPCQP_CM_*): vel [B,3] joy_cmd_velx / vely / velz, rate [B,3]
    roll / pitch / yaw rate, mode_request [B] or scalar (nonzero = joy_cmd_ctrl_state_change_request)."""
    v = np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    B = v.shape[0]
    row = np.zeros((B, CM_SIZE))
    row[:, CM_VEL:CM_VEL + 3] = v
    row[:, CM_RATE:CM_RATE + 3] = np.asarray(rate, dtype=np.float64).reshape(B, 3)
    row[:, CM_MODE_REQUEST] = (np.broadcast_to(np.asarray(mode_request), (B,)) != 0).astype(np.float64)
    return row


def command_device(cp, dt, d_cmd, d_states, d_plan_in, batch, d_cmd_state, stream=0):
    """mpcqp_command_device on device pointers (ints)."""
    check(load().mpcqp_command_device(ctypes.byref(cp), float(dt), d_cmd, d_states, d_plan_in, int(batch),
                                      d_cmd_state, stream or None), None, "mpcqp_command_device")
