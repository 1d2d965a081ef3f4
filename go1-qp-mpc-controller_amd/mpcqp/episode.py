"""Episode stage of the control tick (host side of mpcqp_episode_device).

The last stage of a tick that ends with the plant.  Per robot the device stage accumulates the episode's
metrics, decides when the episode ends (a plant status, the envelope, the time-out), writes the episode into a
per-robot log ring and per-robot totals, and restarts the robot over two ticks from a start row drawn on the
device (Philox4x32-10 on robot and episode index) out of a pool the host builds, under a command script that
restarts with it.  T replays of such a tick are a Monte-Carlo evaluation of the fleet with no host write in
between; include/mpcqp.h has the statement, tests/episode_reference.py the numpy restatement.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import EpisodeBuffers, EpisodeParams, check, load, override, set_seed

# include/mpcqp.h MPCQP_EP_*, MPCQP_ES_*, MPCQP_EM_*, MPCQP_EL_*, MPCQP_ET_*
END_FRESH, END_OUT_OF_REACH, END_FALLEN, END_BAD_TORQUE, END_ENVELOPE, END_TIMEOUT, END_COUNT = 0, 1, 2, 3, 4, 5, 6
END_NAMES = ("fresh", "out_of_reach", "fallen", "bad_torque", "envelope", "timeout")
POOL_INIT, POOL_EULER_D, POOL_POS_D, POOL_SIZE = 0, 20, 23, 28
SEG_TICK, SEG_CMD, SEG_SIZE = 0, 1, 8
ES_SIZE, EL_SIZE, ET_SIZE = 24, 24, 8

_METRICS = [("tilt2_max", "f8"), ("z_min", "f8"), ("z_max", "f8"), ("energy", "f8"), ("tau2", "f8"),
            ("err_v", "f8", 3), ("iters", "f8"), ("not_solved", "f8"), ("low_contact", "f8"),
            ("start", "f8", 3), ("end", "f8", 3)]
EPISODE_STATE_DTYPE = np.dtype([("phase", "f8"), ("tick", "f8"), ("episode", "f8"), ("pool", "f8"), ("script", "f8"),
                                ("seg", "f8")] + _METRICS + [("pad", "f8", 1)])
EPISODE_LOG_DTYPE = np.dtype([("episode", "f8"), ("pool", "f8"), ("script", "f8"), ("length", "f8"),
                              ("reason", "f8")] + _METRICS + [("pad", "f8", 2)])
EPISODE_TOTALS_DTYPE = np.dtype([("episodes", "f8"), ("ticks", "f8"), ("reason", "f8", END_COUNT)])
assert EPISODE_STATE_DTYPE.itemsize == 8 * ES_SIZE and EPISODE_LOG_DTYPE.itemsize == 8 * EL_SIZE
assert EPISODE_TOTALS_DTYPE.itemsize == 8 * ET_SIZE


def default_episode_params(**over):
    """mpcqp_episode_default_params + keyword overrides; ``seed`` is one 64-bit integer."""
    p = EpisodeParams()
    load().mpcqp_episode_default_params(ctypes.byref(p))
    return override(p, over, {"seed": set_seed})


def episode_state_size():
    """Doubles per robot of the episode slot (mpcqp_episode_state_size)."""
    return int(load().mpcqp_episode_state_size())


def pack_episode_pool(init_rows, euler_d, pos_d):
    """Pool rows [P, POOL_SIZE]: plant init rows [P, PI_SIZE] (pack_plant_init) and the desired values that live
    in the caller's state row, root_euler_d [P,3] and root_pos_d [P,3]."""
    init_rows = np.asarray(init_rows, dtype=np.float64).reshape(-1, _lib.PI_SIZE)
    P = init_rows.shape[0]
    row = np.zeros((P, POOL_SIZE))
    row[:, POOL_INIT:POOL_INIT + _lib.PI_SIZE] = init_rows
    row[:, POOL_EULER_D:POOL_EULER_D + 3] = np.asarray(euler_d, dtype=np.float64).reshape(P, 3)
    row[:, POOL_POS_D:POOL_POS_D + 3] = np.asarray(pos_d, dtype=np.float64).reshape(P, 3)
    return row


def pack_episode_scripts(scripts, segments=None):
    """Scripts [S, segments, SEG_SIZE] from a list of scripts, each a list of segments
    ``(tick, vel[3], rate[3], mode_request)`` sorted by tick; unused segments get tick -1, which ends the list."""
    n = max(len(s) for s in scripts) if segments is None else int(segments)
    out = np.zeros((len(scripts), max(n, 1), SEG_SIZE))
    out[:, :, SEG_TICK] = -1.0
    for i, sc in enumerate(scripts):
        if len(sc) > out.shape[1]:
            raise ValueError(f"script {i} has {len(sc)} segments, more than {out.shape[1]}")
        last = -1
        for j, (tick, vel, rate, request) in enumerate(sc):
            if int(tick) <= last:
                raise ValueError(f"script {i}: the segments are not sorted by tick")
            last = int(tick)
            out[i, j, SEG_TICK] = float(int(tick))
            out[i, j, SEG_CMD:SEG_CMD + 3] = vel
            out[i, j, SEG_CMD + 3:SEG_CMD + 6] = rate
            out[i, j, SEG_CMD + 6] = 1.0 if request else 0.0
    return out


def episode_buffers(d_plant_out, d_plant_state, d_plant_init=0, d_joint_torques=0, d_sensors=0, d_cmd=0, d_results=0,
                    d_pool=0, d_scripts=0, d_states=0, d_counter=0, d_log=0, d_totals=0, d_est_state=0,
                    est_state_size=0, d_plan_state=0, plan_state_size=0, d_cmd_state=0, cmd_state_size=0,
                    d_policy_state=0, policy_state_size=0, d_warm=0, warm_size=0):
    """mpcqp_episode_buffers from device pointers (ints; 0 = NULL) and the slots' row sizes in doubles."""
    bf = EpisodeBuffers()
    for name in ("d_plant_out", "d_plant_state", "d_plant_init", "d_joint_torques", "d_sensors", "d_cmd", "d_results",
                 "d_pool", "d_scripts", "d_states", "d_counter", "d_log", "d_totals", "d_est_state", "d_plan_state",
                 "d_cmd_state", "d_policy_state", "d_warm"):
        setattr(bf, name, locals()[name] or None)
    bf.est_state_size, bf.plan_state_size, bf.cmd_state_size = int(est_state_size), int(plan_state_size), int(cmd_state_size)
    bf.policy_state_size, bf.warm_size = int(policy_state_size), int(warm_size)
    return bf


def episode_device(ep, buffers, batch, d_episode_state, stream=0):
    """mpcqp_episode_device: one episode tick, enqueued on `stream` (buffers: an EpisodeBuffers)."""
    check(load().mpcqp_episode_device(ctypes.byref(ep), ctypes.byref(buffers), int(batch), d_episode_state or None,
                                      stream or None), None, "mpcqp_episode_device")
