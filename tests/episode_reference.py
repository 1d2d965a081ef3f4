"""numpy restatement of the episode stage (csrc/mpcqp_episode.hip, include/mpcqp.h "episode stage"): the Philox
draw, the metrics, the phases of a restart and the command scripts, one robot at a time in the kernel's statement
order.  Everything is integer arithmetic, binary64 products and sums, and comparisons, so the device agrees
bitwise.  `step` works in place on a dict of arrays named as the fields of mpcqp_episode_buffers without the
d_ prefix (a missing or None entry is a NULL pointer) plus "episode_state"."""
from dataclasses import dataclass

import numpy as np

# include/mpcqp.h
PT_POS, PT_QUAT, PT_EULER, PT_LIN_VEL, PT_ANG_VEL, PT_CONTACTS, PT_STATUS, PT_SIZE = 0, 3, 7, 10, 13, 16, 47, 48
PN_SIZE, PI_SIZE, SN_JOINT_VEL, SN_SIZE, CM_SIZE, ST_EULER_D, ST_POS_D, ST_SIZE = 64, 20, 16, 36, 8, 21, 24, 64
ST_POS, ST_LIN_VEL = 3, 9
RESULT_DOUBLES, RESULT_STATUS_I32, RESULT_ITERS_I32, STATUS_SOLVED = 30, 56, 57, 1
END_FRESH, END_OUT_OF_REACH, END_FALLEN, END_BAD_TORQUE, END_ENVELOPE, END_TIMEOUT, END_COUNT = 0, 1, 2, 3, 4, 5, 6
POOL_INIT, POOL_EULER_D, POOL_POS_D, POOL_SIZE = 0, 20, 23, 28
SEG_TICK, SEG_CMD, SEG_SIZE = 0, 1, 8
ES_PHASE, ES_TICK, ES_EPISODE, ES_POOL, ES_SCRIPT, ES_SEG, ES_METRICS, ES_SIZE = 0, 1, 2, 3, 4, 5, 6, 24
EM_TILT2_MAX, EM_Z_MIN, EM_Z_MAX, EM_ENERGY, EM_TAU2, EM_ERR_V, EM_ITERS, EM_NOT_SOLVED = 0, 1, 2, 3, 4, 5, 8, 9
EM_LOW_CONTACT, EM_START, EM_END, EM_SIZE = 10, 11, 14, 17
EL_EPISODE, EL_POOL, EL_SCRIPT, EL_LENGTH, EL_REASON, EL_METRICS, EL_SIZE = 0, 1, 2, 3, 4, 5, 24
ET_EPISODES, ET_TICKS, ET_REASON, ET_SIZE = 0, 1, 2, 8

M32 = 0xFFFFFFFF


@dataclass
class Params:
    """mpcqp_episode_params"""
    dt: float = 0.0025
    tilt_max: float = 0.5
    height_min: float = 0.12
    height_max: float = 0.6
    seed: int = 0  # 64 bits: seed[0] the low word, seed[1] the high one
    max_ticks: int = 2000
    pool_count: int = 0
    script_count: int = 0
    script_segments: int = 0
    log_len: int = 4


def philox4x32(counter, key, rounds=10):
    """Philox4x32-10 (Salmon et al., SC'11) on four counter words and two key words."""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(rounds):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(seed, b, episode, pool_count, script_count):
    """(pool index, script index) of robot b's episode."""
    w = philox4x32((b, episode, 0, 0), (seed & M32, (seed >> 32) & M32))
    return (w[0] * max(int(pool_count), 0)) >> 32, (w[1] * max(int(script_count), 0)) >> 32


def _finite(x):
    return bool(np.isfinite(x))


def _end_reason(p, fresh, po, tilt2, z, tick):
    if fresh:
        return END_FRESH
    st = po[PT_STATUS]
    if st == 1.0:
        return END_OUT_OF_REACH
    if st == 2.0:
        return END_FALLEN
    if st == 3.0:
        return END_BAD_TORQUE
    pose_ok = all(_finite(po[i]) for i in range(PT_POS, PT_EULER + 3))  # pos, quat, euler are contiguous
    if tilt2 > p.tilt_max * p.tilt_max or z < p.height_min or z > p.height_max or not pose_ok:
        return END_ENVELOPE
    if tick + 1.0 >= float(p.max_ticks):
        return END_TIMEOUT
    return -1


def _segment(p, a, b, es, tick):
    """Writes the script's next segment into the cmd row if it starts at `tick`."""
    cmd, scripts = a.get("cmd"), a.get("scripts")
    if cmd is None or scripts is None:
        return
    seg = int(es[ES_SEG])
    if seg >= p.script_segments:
        return
    sg = scripts.reshape(p.script_count, p.script_segments, SEG_SIZE)[int(es[ES_SCRIPT]), seg]
    if sg[SEG_TICK] == tick:
        cmd[b, 0:7] = sg[SEG_CMD:SEG_CMD + 7]
        es[ES_SEG] = float(seg + 1)


def step(p, a, batch):
    """One tick of the stage on the arrays of `a`, in place."""
    with np.errstate(all="ignore"):
        for b in range(batch):
            _step_robot(p, a, b)


def _step_robot(p, a, b):
    f8 = np.float64
    es = a["episode_state"][b]
    m = es[ES_METRICS:ES_METRICS + EM_SIZE]
    po = a["plant_out"][b]
    tq, sn, cmd, res = a.get("joint_torques"), a.get("sensors"), a.get("cmd"), a.get("results")
    pool = a.get("pool") if p.pool_count > 0 else None
    roll, pitch, yaw = po[PT_EULER], po[PT_EULER + 1], po[PT_EULER + 2]
    tilt2 = roll * roll + pitch * pitch
    x, y, z = po[PT_POS], po[PT_POS + 1], po[PT_POS + 2]
    phase = es[ES_PHASE]

    if phase == 2.0:  # ---- priming ----
        for name in ("est_state", "plan_state", "cmd_state", "policy_state", "warm", "results", "counter"):
            if a.get(name) is not None:
                a[name][b] = 0
        pi = int(es[ES_POOL])
        if pool is not None and a.get("states") is not None:
            a["states"][b, ST_EULER_D:ST_EULER_D + 3] = pool[pi, POOL_EULER_D:POOL_EULER_D + 3]
            a["states"][b, ST_POS_D:ST_POS_D + 3] = pool[pi, POOL_POS_D:POOL_POS_D + 3]
        if a.get("est_state") is not None and a.get("states") is not None:
            # the estimator's first tick leaves root_pos and root_lin_vel as they are (A1CtrlStates::reset zeroes them)
            a["states"][b, ST_POS:ST_POS + 3] = 0.0
            a["states"][b, ST_LIN_VEL:ST_LIN_VEL + 3] = 0.0
        es[ES_SEG] = 0.0
        _segment(p, a, b, es, 0.0)
        m[:] = 0.0
        m[EM_TILT2_MAX] = tilt2
        m[EM_Z_MIN] = z
        m[EM_Z_MAX] = z
        m[EM_START:EM_START + 3] = (x, y, yaw)
        m[EM_END:EM_END + 3] = (x, y, yaw)
        m[np.isnan(m)] = np.nan
        es[ES_TICK] = 0.0
        es[ES_PHASE] = 1.0
        return

    fresh = phase == 0.0
    tick = es[ES_TICK]
    if not fresh:  # ---- this tick's metrics ----
        m[EM_TILT2_MAX] = tilt2 if tilt2 > m[EM_TILT2_MAX] else m[EM_TILT2_MAX]
        m[EM_Z_MIN] = z if z < m[EM_Z_MIN] else m[EM_Z_MIN]
        m[EM_Z_MAX] = z if z > m[EM_Z_MAX] else m[EM_Z_MAX]
        if tq is not None:
            t = tq[b].reshape(4, 3)
            t2 = [(t[l, 0] * t[l, 0] + t[l, 1] * t[l, 1]) + t[l, 2] * t[l, 2] for l in range(4)]
            m[EM_TAU2] = m[EM_TAU2] + ((t2[0] + t2[1]) + (t2[2] + t2[3]))
            if sn is not None:
                qd = sn[b, SN_JOINT_VEL:SN_JOINT_VEL + 12].reshape(4, 3)
                pw = [(t[l, 0] * qd[l, 0] + t[l, 1] * qd[l, 1]) + t[l, 2] * qd[l, 2] for l in range(4)]
                m[EM_ENERGY] = m[EM_ENERGY] + ((pw[0] + pw[1]) + (pw[2] + pw[3])) * f8(p.dt)
        # body-frame velocity R(quat)' v, R as in Eigen::Quaterniond::toRotationMatrix
        qw, qx, qy, qz = po[PT_QUAT:PT_QUAT + 4]
        tx, ty, tz = 2.0 * qx, 2.0 * qy, 2.0 * qz
        twx, twy, twz = tx * qw, ty * qw, tz * qw
        txx, txy, txz = tx * qx, ty * qx, tz * qx
        tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
        r0, r3, r6 = 1.0 - (tyy + tzz), txy + twz, txz - twy
        r1, r4, r7 = txy - twz, 1.0 - (txx + tzz), tyz + twx
        v0, v1, v2 = po[PT_LIN_VEL:PT_LIN_VEL + 3]
        vbx = (r0 * v0 + r3 * v1) + r6 * v2
        vby = (r1 * v0 + r4 * v1) + r7 * v2
        wz = po[PT_ANG_VEL + 2]
        cvx, cvy, cwz = (cmd[b, 0], cmd[b, 1], cmd[b, 5]) if cmd is not None else (f8(0.0), f8(0.0), f8(0.0))
        ex, ey, ew = vbx - cvx, vby - cvy, wz - cwz
        m[EM_ERR_V] = m[EM_ERR_V] + ex * ex
        m[EM_ERR_V + 1] = m[EM_ERR_V + 1] + ey * ey
        m[EM_ERR_V + 2] = m[EM_ERR_V + 2] + ew * ew
        if res is not None:
            ri = res[b].view(np.int32)
            m[EM_ITERS] = m[EM_ITERS] + f8(int(ri[RESULT_ITERS_I32]))
            m[EM_NOT_SOLVED] = m[EM_NOT_SOLVED] + (0.0 if ri[RESULT_STATUS_I32] == STATUS_SOLVED else 1.0)
        c = po[PT_CONTACTS:PT_CONTACTS + 4]
        nc = (c[0] + c[1]) + (c[2] + c[3])
        m[EM_LOW_CONTACT] = m[EM_LOW_CONTACT] + (1.0 if nc < 2.0 else 0.0)
        m[EM_END:EM_END + 3] = (x, y, yaw)
        # a NaN metric is stored as the one quiet NaN 0x7FF8000000000000 (np.nan): IEEE 754 leaves the sign and
        # payload of a NaN result open, and they do differ between this host and the device
        m[np.isnan(m)] = np.nan

    reason =_end_reason(p, fresh, po, tilt2, z, tick)
    if reason < 0:  # ---- the episode goes on: the next tick's command ----
        _segment(p, a, b, es, tick + 1.0)
        es[ES_TICK] = tick + 1.0
        return

    # ---- the episode ends ----
    episode = es[ES_EPISODE]
    tot = a.get("totals")
    if not fresh:
        length = tick + 1.0
        if a.get("log") is not None:
            row = a["log"].reshape(-1, p.log_len, EL_SIZE)[b, int(episode) % p.log_len]
            row[EL_EPISODE], row[EL_POOL], row[EL_SCRIPT] = episode, es[ES_POOL], es[ES_SCRIPT]
            row[EL_LENGTH], row[EL_REASON] = length, float(reason)
            row[EL_METRICS:EL_METRICS + EM_SIZE] = m
        if tot is not None:
            tot[b, ET_EPISODES] = tot[b, ET_EPISODES] + 1.0
            tot[b, ET_TICKS] = tot[b, ET_TICKS] + length
        episode = episode + 1.0
    if tot is not None:
        tot[b, ET_REASON + reason] = tot[b, ET_REASON + reason] + 1.0
    pi, si = draw(p.seed, b, int(episode), p.pool_count if pool is not None else 0,
                  p.script_count if a.get("scripts") is not None else 0)
    es[ES_EPISODE], es[ES_POOL], es[ES_SCRIPT] = episode, float(pi), float(si)
    a["plant_state"][b] = 0.0
    if tq is not None:
        tq[b] = 0.0
    if pool is not None and a.get("plant_init") is not None:
        a["plant_init"][b] = pool[pi, POOL_INIT:POOL_INIT + PI_SIZE]
    es[ES_PHASE] = 2.0
