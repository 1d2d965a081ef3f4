"""State front end of the control tick (host side of mpcqp_state_estimate_device).

Per robot and per tick the device stage runs the pose callback (src/a1_cpp/src/GazeboA1ROS.cpp:242-289:
rotation matrix, Euler angles and yaw rotation from the quaternion, leg forward kinematics and Jacobian,
foot positions and velocities), the IMU callback's ``root_ang_vel = R imu_ang_vel`` (:306) and
``A1BasicEKF::init_state`` / ``update_estimation`` (src/a1_cpp/src/A1BasicEKF.cpp:55-164), and writes
root_euler, root_pos, root_ang_vel, root_lin_vel, root_rot_mat and foot_pos_abs into the MPCQP_ST_* row,
root_rot_mat_z into the MPCQP_PL_* row and j_foot into the MPCQP_TQ_* row.  The filter's x and P live in a
per-robot device slot of ``estimator_state_size()`` doubles; zero-filled = ``is_inited() == false``.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import (SN_IMU_ACC, SN_IMU_ANG_VEL, SN_JOINT_POS, SN_JOINT_VEL, SN_QUAT, SN_SIZE, EstimatorParams, check,
                   load, override)

# the output row (include/mpcqp.h MPCQP_EO_*)
EST_OUT_DTYPE = np.dtype([
    ("foot_pos_rel", "f8", (4, 3)), ("foot_vel_rel", "f8", (4, 3)), ("foot_vel_abs", "f8", (4, 3)),
    ("contact_weights", "f8", 4), ("x", "f8", 18), ("diag_P", "f8", 18), ("det", "f8"), ("pad", "f8", 3),
])
assert EST_OUT_DTYPE.itemsize == 8 * _lib.EO_SIZE

# slot layout (csrc/mpcqp_estimate.hip ES_*)
_ES_INIT, _ES_X, _ES_P, _NS = 0, 4, 24, 18

def default_estimator_params(**over):
    """mpcqp_est_default_params (GazeboA1ROS.cpp:72-98, A1BasicEKF.h:16-21) + keyword overrides; rho_fix
    accepts anything that flattens to [4][5], rho_opt to [4][3]."""
    p = EstimatorParams()
    load().mpcqp_est_default_params(ctypes.byref(p))
    return override(p, over)


def estimator_state_size():
    """Doubles per robot of the estimator slot (mpcqp_estimator_state_size)."""
    return int(load().mpcqp_estimator_state_size())


def pack_sensors(quat, joint_pos, joint_vel, imu_acc, imu_ang_vel):
    """Sensor rows [B, SN_SIZE] (include/mpcqp.h MPCQP_SN_*): quat [B,4] as w, x, y, z; joint_pos and
    joint_vel [B,12] (FL FR RL RR x hip, thigh, calf); imu_acc, imu_ang_vel [B,3] body frame."""
    q = np.asarray(quat, dtype=np.float64).reshape(-1, 4)
    B = q.shape[0]
    row = np.zeros((B, SN_SIZE))
    row[:, SN_QUAT:SN_QUAT + 4] = q
    row[:, SN_JOINT_POS:SN_JOINT_POS + 12] = np.asarray(joint_pos, dtype=np.float64).reshape(B, 12)
    row[:, SN_JOINT_VEL:SN_JOINT_VEL + 12] = np.asarray(joint_vel, dtype=np.float64).reshape(B, 12)
    row[:, SN_IMU_ACC:SN_IMU_ACC + 3] = np.asarray(imu_acc, dtype=np.float64).reshape(B, 3)
    row[:, SN_IMU_ANG_VEL:SN_IMU_ANG_VEL + 3] = np.asarray(imu_ang_vel, dtype=np.float64).reshape(B, 3)
    return row


def unpack_sensors(rows):
    """Inverse of pack_sensors: (quat, joint_pos, joint_vel, imu_acc, imu_ang_vel)."""
    r = np.asarray(rows, dtype=np.float64).reshape(-1, SN_SIZE)
    return (r[:, SN_QUAT:SN_QUAT + 4].copy(), r[:, SN_JOINT_POS:SN_JOINT_POS + 12].copy(),
            r[:, SN_JOINT_VEL:SN_JOINT_VEL + 12].copy(), r[:, SN_IMU_ACC:SN_IMU_ACC + 3].copy(),
            r[:, SN_IMU_ANG_VEL:SN_IMU_ANG_VEL + 3].copy())


def pack_estimator_slot(x, P, size=None):
    """Slots [B, estimator_state_size()] of initialized filters holding x [B,18] and P [B,18,18] (to start
    a filter from a chosen state).  `size` overrides the slot size (tests without the library)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, _NS)
    B = x.shape[0]
    P = np.asarray(P, dtype=np.float64).reshape(B, _NS * _NS)
    n = int(size) if size is not None else estimator_state_size()
    slot = np.zeros((B, n))
    slot[:, _ES_INIT] = 1.0
    slot[:, _ES_X:_ES_X + _NS] = x
    slot[:, _ES_P:_ES_P + _NS * _NS] = P
    return slot


def unpack_estimator_slot(slots):
    """(inited [B] bool, x [B,18], P [B,18,18]) of downloaded slots."""
    s = np.asarray(slots, dtype=np.float64)
    s = s.reshape(-1, s.shape[-1])
    return (s[:, _ES_INIT] != 0.0, s[:, _ES_X:_ES_X + _NS].copy(),
            s[:, _ES_P:_ES_P + _NS * _NS].reshape(-1, _NS, _NS).copy())


def state_estimate_device(est, dt, d_sensors, d_plan_in, d_states, batch, d_est_state, d_tq_records=0, d_est_out=0,
                          stream=0):
    """mpcqp_state_estimate_device on device pointers (ints; 0 for the optional ones)."""
    check(load().mpcqp_state_estimate_device(ctypes.byref(est), float(dt), d_sensors or None, d_plan_in or None,
                                             d_states or None, int(batch), d_est_state or None, d_tq_records or None,
                                             d_est_out or None, stream or None),
          None, "mpcqp_state_estimate_device")
