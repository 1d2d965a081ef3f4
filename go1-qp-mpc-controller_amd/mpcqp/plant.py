"""Plant stage of the control tick (host side of mpcqp_plant_step_device).

Per robot and per tick the device stage advances a rigid-body model of the robot by one control period
under the tick's joint torques and writes the next tick's sensor-level rows: a single rigid trunk on
massless stance legs (a held foot turns the joint torques into the ground reaction f = -R J^-T tau),
joint-space swing legs, flat ground, semi-implicit Euler in ``substeps`` substeps.  Left out: leg mass, the
swing legs' reaction on the trunk, foot slip, terrain, joint limits, and impact dynamics beyond zeroing the
landing foot's velocity.  The state lives in a per-robot device slot of ``plant_state_size()`` doubles;
zero-filled = fresh, and zeroing a robot's slots is how a fleet resets a fallen robot (a robot whose status
is not 0 is frozen until then).  The episode stage (episode.py) does that on the device: it ends a fallen
robot's episode, zeroes its slots over two ticks and restarts it from a drawn start row.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import PI_JOINT_POS, PI_POS, PI_QUAT, PI_SIZE, PlantParams, check, load, override

# the slot (include/mpcqp.h MPCQP_PN_*) and the output row (MPCQP_PT_*)
PLANT_STATE_DTYPE = np.dtype([
    ("init", "f8"), ("pos", "f8", 3), ("quat", "f8", 4), ("lin_vel", "f8", 3), ("ang_vel", "f8", 3),
    ("joint_pos", "f8", 12), ("joint_vel", "f8", 12), ("foot", "f8", (4, 3)), ("contact", "f8", 4),
    ("acc", "f8", 3), ("status", "f8"), ("pad", "f8", 6),
])
assert PLANT_STATE_DTYPE.itemsize == 8 * _lib.PN_SIZE
PLANT_OUT_DTYPE = np.dtype([
    ("pos", "f8", 3), ("quat", "f8", 4), ("euler", "f8", 3), ("lin_vel", "f8", 3), ("ang_vel", "f8", 3),
    ("contacts", "f8", 4), ("grf", "f8", (4, 3)), ("foot", "f8", (4, 3)), ("acc", "f8", 3), ("status", "f8"),
])
assert PLANT_OUT_DTYPE.itemsize == 8 * _lib.PT_SIZE

PLANT_OK, PLANT_OUT_OF_REACH, PLANT_FALLEN, PLANT_BAD_TORQUE = 0, 1, 2, 3

def default_plant_params(**over):
    """mpcqp_plant_default_params + keyword overrides; the array fields accept anything that flattens to
    their size (rho_fix [4][5], rho_opt [4][3], inertia [3][3], ...)."""
    p = PlantParams()
    load().mpcqp_plant_default_params(ctypes.byref(p))
    return override(p, over)


def plant_state_size():
    """Doubles per robot of the plant slot (mpcqp_plant_state_size)."""
    return int(load().mpcqp_plant_state_size())


def pack_plant_init(pos, quat, joint_pos):
    """Init rows [B, PI_SIZE] (include/mpcqp.h MPCQP_PI_*): pos [B,3], quat [B,4] as w, x, y, z, joint_pos
    [B,12] (FL FR RL RR x hip, thigh, calf)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    B = pos.shape[0]
    row = np.zeros((B, PI_SIZE))
    row[:, PI_POS:PI_POS + 3] = pos
    row[:, PI_QUAT:PI_QUAT + 4] = np.asarray(quat, dtype=np.float64).reshape(B, 4)
    row[:, PI_JOINT_POS:PI_JOINT_POS + 12] = np.asarray(joint_pos, dtype=np.float64).reshape(B, 12)
    return row


def plant_step_device(pp, dt, d_torques, batch, d_plant_state, d_init=0, d_sensors=0, d_plan_in=0, d_states=0,
                      d_tq_records=0, d_plant_out=0, stream=0):
    """mpcqp_plant_step_device on device pointers (ints; 0 for the optional ones)."""
    check(load().mpcqp_plant_step_device(ctypes.byref(pp), float(dt), d_torques or None, int(batch),
                                         d_plant_state or None, d_init or None, d_sensors or None, d_plan_in or None,
                                         d_states or None, d_tq_records or None, d_plant_out or None, stream or None),
          None, "mpcqp_plant_step_device")
