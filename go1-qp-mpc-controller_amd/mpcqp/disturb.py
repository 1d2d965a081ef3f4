"""Disturbance stage of the control tick (host side of mpcqp_disturb_device and mpcqp_plant_step_wrench_device).

The first stage of a tick that has the plant and the episode stage.  Per robot and per tick the device stage
draws what the world does to the robot: a push (one per window of ``push_interval`` ticks, at a drawn tick inside
it, of a drawn magnitude, direction and application point), the weight of a payload drawn once per episode, and
sensor noise on the joint angles, joint rates and the IMU sample with IMU biases drawn once per episode.  The push
and the load go into a wrench row the plant applies; the noise goes into a second sensor row, written out of
place, that the estimator and the policy stage read.  The stage keeps no state: every draw is Philox4x32-10 on
(robot, episode, stream, index) under the key ``seed``, so ``disturbance_of`` recomputes on the host what any
logged episode was subjected to.  include/mpcqp.h has the statement, tests/disturb_reference.py the numpy
restatement.  Left out: noise on the quaternion and the foot forces, the payload's inertia, per-robot plant mass
and friction, terrain, foot slip.
"""
import ctypes

import numpy as np

from ._lib import DisturbBuffers, DisturbParams, check, load, override, set_seed

# include/mpcqp.h MPCQP_PW_*, MPCQP_DO_*, MPCQP_DS_*
PW_FORCE0, PW_POINT0, PW_FORCE1, PW_POINT1, PW_SIZE = 0, 3, 6, 9, 12
DO_PUSH_ACTIVE, DO_PUSH_WINDOW, DO_PUSH_FORCE, DO_PUSH_DIR, DO_PUSH_POINT, DO_LOAD_POINT = 0, 1, 2, 3, 4, 7
DO_LOAD_FORCE, DO_BIAS_ACC, DO_BIAS_GYRO, DO_SIZE = 10, 11, 14, 20
DS_JOINT_POS, DS_JOINT_VEL, DS_IMU_ACC, DS_IMU_ANG_VEL = 0, 1, 2, 3

DISTURB_OUT_DTYPE = np.dtype([
    ("push_active", "f8"), ("push_window", "f8"), ("push_force", "f8"), ("push_dir", "f8"), ("push_point", "f8", 3),
    ("load_point", "f8", 3), ("load_force", "f8"), ("bias_acc", "f8", 3), ("bias_gyro", "f8", 3), ("pad", "f8", 3),
])
assert DISTURB_OUT_DTYPE.itemsize == 8 * DO_SIZE

def default_disturb_params(**over):
    """mpcqp_disturb_default_params (everything off) + keyword overrides; ``seed`` is one 64-bit integer."""
    p = DisturbParams()
    load().mpcqp_disturb_default_params(ctypes.byref(p))
    return override(p, over, {"seed": set_seed})


def pack_push_dirs(count):
    """Direction table [count, 4] for ``d_dirs``: evenly spaced horizontal unit vectors (x, y, 0, 0), row i at
    the angle 2 pi i / count."""
    count = int(count)
    if count < 1:
        raise ValueError("pack_push_dirs: count must be at least 1")
    a = 2.0 * np.pi * np.arange(count) / count
    d = np.zeros((count, 4))
    d[:, 0], d[:, 1] = np.cos(a), np.sin(a)
    return d


def disturb_buffers(d_episode_state, d_wrench, d_sensors=0, d_sensors_noisy=0, d_dirs=0, d_disturb_out=0):
    """mpcqp_disturb_buffers from device pointers (ints; 0 = NULL)."""
    bf = DisturbBuffers()
    for name in ("d_episode_state", "d_wrench", "d_sensors", "d_sensors_noisy", "d_dirs", "d_disturb_out"):
        setattr(bf, name, locals()[name] or None)
    return bf


def disturb_device(dp, buffers, batch, stream=0):
    """mpcqp_disturb_device: one disturbance tick, enqueued on `stream` (buffers: a DisturbBuffers)."""
    check(load().mpcqp_disturb_device(ctypes.byref(dp), ctypes.byref(buffers), int(batch), stream or None), None,
          "mpcqp_disturb_device")


def plant_step_wrench_device(pp, dt, d_torques, d_wrench, batch, d_plant_state, d_init=0, d_sensors=0, d_plan_in=0,
                             d_states=0, d_tq_records=0, d_plant_out=0, stream=0):
    """mpcqp_plant_step_wrench_device on device pointers (ints; 0 for the optional ones, d_wrench among them)."""
    check(load().mpcqp_plant_step_wrench_device(
        ctypes.byref(pp), float(dt), d_torques or None, d_wrench or None, int(batch), d_plant_state or None,
        d_init or None, d_sensors or None, d_plan_in or None, d_states or None, d_tq_records or None,
        d_plant_out or None, stream or None), None, "mpcqp_plant_step_wrench_device")


# ---- the host-side recomputation ------------------------------------------------------------------------
def _philox4(c, key):
    """Philox4x32-10: counter c (four ints), key (two ints) -> four output words as Python ints."""
    c0, c1, c2, c3 = (int(x) & 0xFFFFFFFF for x in c)
    k0, k1 = (int(x) & 0xFFFFFFFF for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _unit(w):
    return (float(w) + 0.5) * 2.0 ** -32


def _sym(w):
    return (float(w) + 0.5) * 2.0 ** -31 - 1.0


def disturbance_of(params, dirs, robot, episode, ticks):
    """What episode ``episode`` of robot ``robot`` is subjected to over its first ``ticks`` ticks, recomputed on
    the host with the device's arithmetic: a dict with ``load_force`` (the payload's weight, N), ``load_point``
    [3], ``bias_acc`` [3], ``bias_gyro`` [3] and ``pushes``, a list of dicts ``window``, ``start`` (the first
    active episode tick), ``stop`` (one past the last, cut at ``ticks``), ``force``, ``dir`` (the row of
    ``dirs``), ``vector`` [3] (the world-frame force) and ``point`` [3], for every push that starts before
    ``ticks``.  ``dirs`` may be None without pushes."""
    p, key = params, (params.seed[0], params.seed[1])
    robot, episode, ticks = int(robot), int(episode), int(ticks)
    w = _philox4((robot, episode, 1, 0), key)
    out = dict(load_force=(p.load_mass_max * _unit(w[0])) * p.gravity,
               load_point=np.array([p.load_point[i] * _sym(w[i + 1]) for i in range(3)]))
    w = _philox4((robot, episode, 1, 1), key)
    out["bias_acc"] = np.array([p.bias_acc * _sym(w[i]) for i in range(3)])
    w = _philox4((robot, episode, 1, 2), key)
    out["bias_gyro"] = np.array([p.bias_gyro * _sym(w[i]) for i in range(3)])
    pushes = []
    if p.push_interval > 0:
        dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 4)
        k = 0
        while p.push_start + k * p.push_interval < ticks:
            w = _philox4((robot, episode, 2, k), key)
            jitter = (w[0] * (p.push_interval - p.push_duration + 1)) >> 32
            start = p.push_start + k * p.push_interval + jitter
            if start < ticks:
                force = p.push_force[0] + (p.push_force[1] - p.push_force[0]) * _unit(w[1])
                di = (w[2] * p.dir_count) >> 32
                wp = _philox4((robot, episode, 3, k), key)
                pushes.append(dict(window=k, start=start, stop=min(start + p.push_duration, ticks), force=force,
                                   dir=di, vector=force * dirs[di, :3],
                                   point=np.array([p.push_point[i] * _sym(wp[i]) for i in range(3)])))
            k += 1
    out["pushes"] = pushes
    return out
