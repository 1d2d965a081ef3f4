"""TEST INFRASTRUCTURE — numpy restatement of the disturbance stage (csrc/mpcqp_disturb.hip, include/mpcqp.h
"disturbance stage") and of the plant's wrench terms (mpcqp_plant_step_wrench_device).

The draws are integer arithmetic and exact or explicitly ordered binary64 products and sums, so the device agrees
bitwise.  `step` returns the rows of one call for B robots from the episode slots and the clean sensor rows.
`substep` / `WrenchPlant` are tests/plant_reference.py's with the external forces added in step 3; everything
else is that file's helpers, statement for statement."""
from dataclasses import dataclass, field

import numpy as np

import plant_reference as pr
from estimator_reference import fk, jac, mat_vec, quat_to_rot
from plant_reference import PN_INIT, PN_STATUS, STATUS_BAD_TORQUE, STATUS_HEIGHT, STATUS_REACH, cross, lu3_solve, mat_t_vec, quad_sum

# include/mpcqp.h
ES_PHASE, ES_TICK, ES_EPISODE, ES_SIZE = 0, 1, 2, 24
SN_QUAT, SN_JOINT_POS, SN_JOINT_VEL, SN_IMU_ACC, SN_IMU_ANG_VEL, SN_SIZE = 0, 4, 16, 28, 31, 36
PW_FORCE0, PW_POINT0, PW_FORCE1, PW_POINT1, PW_SIZE = 0, 3, 6, 9, 12
DO_PUSH_ACTIVE, DO_PUSH_WINDOW, DO_PUSH_FORCE, DO_PUSH_DIR, DO_PUSH_POINT, DO_LOAD_POINT = 0, 1, 2, 3, 4, 7
DO_LOAD_FORCE, DO_BIAS_ACC, DO_BIAS_GYRO, DO_SIZE = 10, 11, 14, 20
SQRT3 = 1.7320508075688772
M32 = np.uint64(0xFFFFFFFF)


@dataclass
class Params:
    """mpcqp_disturb_params; the defaults are mpcqp_disturb_default_params: everything off."""
    load_mass_max: float = 0.0
    gravity: float = 9.81
    load_point: list = field(default_factory=lambda: [0.0, 0.0, 0.0])
    bias_acc: float = 0.0
    bias_gyro: float = 0.0
    push_force: list = field(default_factory=lambda: [0.0, 0.0])
    push_point: list = field(default_factory=lambda: [0.0, 0.0, 0.0])
    sigma: list = field(default_factory=lambda: [0.0, 0.0, 0.0, 0.0])  # joint_pos, joint_vel, imu_acc, imu_ang_vel
    seed: int = 0  # 64 bits: seed[0] the low word, seed[1] the high one
    push_start: int = 0
    push_interval: int = 0
    push_duration: int = 1
    dir_count: int = 0


def philox4x32(c0, c1, c2, c3, seed):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of counter words (broadcast together) under the 64-bit key
    `seed` (or a pair of key words).  Returns four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3)))
    if isinstance(seed, tuple):
        k0, k1 = np.uint64(seed[0]), np.uint64(seed[1])
    else:
        k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 bits: no overflow of 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def unit(w):
    """(w + 0.5) 2^-32, in (0, 1); exact."""
    return (np.asarray(w).astype(np.float64) + 0.5) * 2.0 ** -32


def sym(w):
    """(w + 0.5) 2^-31 - 1, in (-1, 1); exact."""
    return (np.asarray(w).astype(np.float64) + 0.5) * 2.0 ** -31 - 1.0


def scaled(w, count):
    """(uint64(w) * count) >> 32"""
    return ((np.asarray(w, dtype=np.uint64) * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def normal(seed, robot, episode, j, tick):
    """z of value j at episode tick `tick`: ((u0 + u1) + (u2 + u3)) - 2, variance 1/3."""
    w = philox4x32(robot, episode, 16 + np.asarray(j), tick, seed)
    return ((unit(w[0]) + unit(w[1])) + (unit(w[2]) + unit(w[3]))) - 2.0


def push_window(p, robot, episode, k):
    """(jitter, magnitude, direction row) of window k."""
    w = philox4x32(robot, episode, 2, k, p.seed)
    return (scaled(w[0], p.push_interval - p.push_duration + 1),
            p.push_force[0] + (p.push_force[1] - p.push_force[0]) * unit(w[1]), scaled(w[2], p.dir_count))


def step(p, episode_state, sensors=None, dirs=None):
    """One call of mpcqp_disturb_device: (wrench [B, PW_SIZE], noisy [B, SN_SIZE] or None, out [B, DO_SIZE])."""
    es = np.asarray(episode_state, dtype=np.float64).reshape(-1, ES_SIZE)
    B = es.shape[0]
    robot = np.arange(B)
    run = es[:, ES_PHASE] == 1.0
    t = np.maximum(es[:, ES_TICK].astype(np.int32), 0).astype(np.int64)
    e = es[:, ES_EPISODE].astype(np.int32).astype(np.int64)
    wrench, out = np.zeros((B, PW_SIZE)), np.zeros((B, DO_SIZE))
    # once per episode
    w = philox4x32(robot, e, 1, 0, p.seed)
    weight = (p.load_mass_max * unit(w[0])) * p.gravity
    wrench[:, PW_FORCE1 + 2] = 0.0 - weight
    for i in range(3):
        wrench[:, PW_POINT1 + i] = p.load_point[i] * sym(w[i + 1])
    out[:, DO_LOAD_FORCE] = weight
    out[:, DO_LOAD_POINT:DO_LOAD_POINT + 3] = wrench[:, PW_POINT1:PW_POINT1 + 3]
    wa, wg = philox4x32(robot, e, 1, 1, p.seed), philox4x32(robot, e, 1, 2, p.seed)
    for i in range(3):
        out[:, DO_BIAS_ACC + i] = p.bias_acc * sym(wa[i])
        out[:, DO_BIAS_GYRO + i] = p.bias_gyro * sym(wg[i])
    # this tick's window
    if p.push_interval > 0:
        dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 4)
        inwin = t >= p.push_start
        r = np.where(inwin, t - p.push_start, 0)
        k = r // p.push_interval
        ph = r - k * p.push_interval
        jitter, mag, di = push_window(p, robot, e, k)
        on = inwin & (jitter <= ph) & (ph < jitter + p.push_duration)
        wp = philox4x32(robot, e, 3, k, p.seed)
        out[:, DO_PUSH_ACTIVE] = on
        out[:, DO_PUSH_WINDOW] = np.where(inwin, k, 0)
        out[:, DO_PUSH_FORCE] = np.where(inwin, mag, 0.0)
        out[:, DO_PUSH_DIR] = np.where(inwin, di, 0)
        for i in range(3):
            pt = p.push_point[i] * sym(wp[i])
            out[:, DO_PUSH_POINT + i] = np.where(inwin, pt, 0.0)
            wrench[:, PW_FORCE0 + i] = np.where(on, mag * dirs[di, i], 0.0)
            wrench[:, PW_POINT0 + i] = np.where(on, pt, 0.0)
    wrench[~run] = 0.0
    out[~run] = 0.0
    noisy = None
    if sensors is not None:
        sn = np.asarray(sensors, dtype=np.float64).reshape(B, SN_SIZE)
        noisy = sn.copy()
        bias = np.zeros((B, 30))
        bias[:, 24:27] = out[:, DO_BIAS_ACC:DO_BIAS_ACC + 3]
        bias[:, 27:30] = out[:, DO_BIAS_GYRO:DO_BIAS_GYRO + 3]
        sg = np.repeat(np.array(p.sigma, dtype=np.float64) * SQRT3, [12, 12, 3, 3])
        for j in range(30):
            d = bias[:, j] + sg[j] * normal(p.seed, robot, e, j, t)
            clean = sn[:, SN_JOINT_POS + j]
            noisy[:, SN_JOINT_POS + j] = np.where(run & (d != 0.0), clean + d, clean)
    return wrench, noisy, out


def pushes_of(p, robot, episode, ticks):
    """[(window, first active tick, one past the last)] of an episode's first `ticks` ticks, tick by tick from
    `step`'s rule."""
    got, cur = [], None
    for t in range(ticks):
        es = np.zeros((1, ES_SIZE))
        es[0, [ES_PHASE, ES_TICK, ES_EPISODE]] = 1.0, t, episode
        o = step_one(p, es, robot)
        if o[DO_PUSH_ACTIVE]:
            k = int(o[DO_PUSH_WINDOW])
            if cur is not None and cur[0] == k and cur[2] == t:
                cur[2] = t + 1
            else:
                cur = [k, t, t + 1]
                got.append(cur)
    return [tuple(c) for c in got]


def step_one(p, es_row, robot, dirs=None):
    """The output row of `step` for one robot index (the slot row is placed at that index)."""
    es = np.zeros((robot + 1, ES_SIZE))
    es[robot] = np.asarray(es_row).reshape(ES_SIZE)
    d = dirs if dirs is not None else np.tile([1.0, 0.0, 0.0, 0.0], (max(p.dir_count, 1), 1))
    return step(p, es, None, d)[2][robot]


# ---- the plant with a wrench row ----------------------------------------------------------------------------
def substep(p, s, h, tau, wrench):
    """plant_reference.substep with the wrench row [B, PW_SIZE] in step 3: F = quad_sum(f) + (F0 + F1) and
    R'M + (p0 x R'F0 + p1 x R'F1), with this substep's R, before - w x I w."""
    rho_opt, rho_fix = pr._geom(p)
    B = s["pos"].shape[0]
    F0, P0 = wrench[:, PW_FORCE0:PW_FORCE0 + 3], wrench[:, PW_POINT0:PW_POINT0 + 3]
    F1, P1 = wrench[:, PW_FORCE1:PW_FORCE1 + 3], wrench[:, PW_POINT1:PW_POINT1 + 3]
    with np.errstate(all="ignore"):
        R, p_b, J, reach, margin = pr.kinematics(p, s)
        Rl = R[:, None]
        g = lu3_solve(np.swapaxes(J, -1, -2), tau)
        f = -mat_vec(Rl, g)
        was = s["contact"]
        lift = was & (f[..., 2] < 0.0)
        margin = np.minimum(margin, np.min(np.where(was, np.abs(f[..., 2]), np.inf), 1))
        st = was & ~lift
        s["contact"] = st
        ft = np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1])
        lim = p.mu * f[..., 2]
        sc = np.where(ft > lim, lim / ft, 1.0)
        f = np.stack([f[..., 0] * sc, f[..., 1] * sc, f[..., 2]], -1)
        f = np.where(st[..., None], f, 0.0)
        Ij = np.array(p.joint_inertia, dtype=np.float64)
        bj = np.array(p.joint_damping, dtype=np.float64)
        s["qd"] = np.where(st[..., None], s["qd"], s["qd"] + h * (tau - bj * s["qd"]) / Ij)
        # 3. the wrench on the trunk: the legs, then the external forces
        r = s["foot"] - s["pos"][:, None]
        m = np.where(st[..., None], cross(r, f), 0.0)
        F, M = quad_sum(f), quad_sum(m)
        fe = F0 + F1
        F = np.where(fe == 0.0, F, F + fe)  # a zero term is skipped, not added: -0.0 + 0.0 would be +0.0
        ce = cross(P0, mat_t_vec(R, F0)) + cross(P1, mat_t_vec(R, F1))
        a = F / p.mass
        a[:, 2] = a[:, 2] + (-p.gravity)
        Ib = np.broadcast_to(np.array(p.inertia, dtype=np.float64).reshape(3, 3), (B, 3, 3))
        Iw = mat_vec(Ib, s["w"])
        rm = mat_t_vec(R, M)
        wd = lu3_solve(Ib, np.where(ce == 0.0, rm, rm + ce) - cross(s["w"], Iw))
        # 4. semi-implicit Euler
        s["v"] = s["v"] + h * a
        s["w"] = s["w"] + h * wd
        s["pos"] = s["pos"] + h * s["v"]
        qw, qx, qy, qz = (s["quat"][:, k] for k in range(4))
        w0, w1, w2 = (s["w"][:, k] for k in range(3))
        dq = np.stack([((-(qx * w0)) - qy * w1) - qz * w2, (qw * w0 + qy * w2) - qz * w1,
                       (qw * w1 + qz * w0) - qx * w2, (qw * w2 + qx * w1) - qy * w0], 1)
        quat = s["quat"] + (h * 0.5) * dq
        n = np.sqrt(((quat[:, 0] * quat[:, 0] + quat[:, 1] * quat[:, 1]) + quat[:, 2] * quat[:, 2])
                    + quat[:, 3] * quat[:, 3])
        s["quat"] = quat / n[:, None]
        s["acc"] = a
        # 5. swing legs: joints, feet, touchdown
        s["q"] = np.where(st[..., None], s["q"], s["q"] + h * s["qd"])
        R2 = quat_to_rot(s["quat"])[:, None]
        p2 = fk(s["q"], rho_opt, rho_fix)
        J2 = jac(s["q"], rho_opt, rho_fix)
        foot = s["pos"][:, None] + mat_vec(R2, p2)
        fv = s["v"][:, None] + mat_vec(R2, cross(s["w"][:, None], p2) + mat_vec(J2, s["qd"]))
        land = ~st & (foot[..., 2] <= 0.0) & (fv[..., 2] < 0.0)
        margin = np.minimum(margin, np.min(np.where(st, np.inf, np.minimum(np.abs(foot[..., 2]), np.abs(fv[..., 2]))),
                                           1))
        foot[..., 2] = np.where(land, 0.0, foot[..., 2])
        s["foot"] = np.where(st[..., None], s["foot"], foot)
        s["contact"] = st | land
    return f, reach, margin


class WrenchPlant(pr.Plant):
    """plant_reference.Plant whose ``step`` takes the wrench rows [B, PW_SIZE] (None: mpcqp_plant_step_device)."""

    def step(self, dt, tau, init=None, wrench=None):
        if wrench is None:
            return super().step(dt, tau, init)
        p, B = self.p, self.B
        tau = np.asarray(tau, dtype=np.float64).reshape(B, 4, 3)
        wrench = np.asarray(wrench, dtype=np.float64).reshape(B, PW_SIZE)
        frozen = self.slot[:, PN_STATUS] != 0.0
        bad = ~frozen & ~(np.all(np.isfinite(tau.reshape(B, 12)), 1) & np.all(np.isfinite(wrench), 1))
        fresh = self.slot[:, PN_INIT] == 0.0
        s0, m0 = pr.initial_state(p, init, B)
        s = self.unpack(self.slot)
        for k in pr._FIELDS:
            s[k] = np.where(fresh.reshape((B,) + (1,) * (s[k].ndim - 1)), s0[k], s[k])
        margin = np.where(fresh, m0, np.inf)
        f = np.zeros((B, 4, 3))
        reach = np.ones(B, dtype=bool)
        h = dt / p.substeps
        run = ~fresh
        tz = np.where(np.isfinite(tau), tau, 0.0)
        wz = np.where(np.isfinite(wrench), wrench, 0.0)
        for _ in range(p.substeps):
            s1 = {k: v.copy() for k, v in s.items()}
            f1, r1, m1 = substep(p, s1, h, tz, wz)
            for k in pr._FIELDS:
                s[k] = np.where(run.reshape((B,) + (1,) * (s[k].ndim - 1)), s1[k], s[k])
            f = np.where(run[:, None, None], f1, f)
            reach &= r1 | ~run
            margin = np.where(run, np.minimum(margin, m1), margin)
        R, p_b, J, r2, m2 = pr.kinematics(p, s)
        reach &= r2
        margin = np.minimum(margin, m2)
        with np.errstate(invalid="ignore"):
            low = reach & (s["pos"][:, 2] < p.min_height)
            margin = np.minimum(margin, np.abs(s["pos"][:, 2] - p.min_height))
        status = np.where(bad, STATUS_BAD_TORQUE, np.where(~reach, STATUS_REACH, np.where(low, STATUS_HEIGHT, 0)))
        status = np.where(frozen, self.slot[:, PN_STATUS], status).astype(np.float64)
        wrote = ~frozen & ~bad & reach
        out = pr.outputs(p, s, R, p_b, J, f, status)
        new = self.pack(s, status)
        self.slot = np.where(wrote[:, None], new, self.slot)
        only = ~frozen & ~bad & ~reach
        self.slot[only, PN_STATUS] = STATUS_REACH
        return out, wrote, np.where(frozen | bad, np.inf, margin)
