"""TEST INFRASTRUCTURE — numpy restatement of the plant stage on inclined ground (csrc/mpcqp_plant.hip with TERRAIN,
mpcqp_plant_step_terrain_device; include/mpcqp.h has the statement).

`substep` / `TerrainPlant` are tests/disturb_reference.py's (and with no wrench rows tests/plant_reference.py's) with
the four changes of the terrain row, in the statement order of the kernel: the fresh slot's contact rule, the ground
reaction, the touchdown rule and the fallen rule.  Everything else is those files' helpers, statement for statement.
The decision margin is extended by |fn|, |hgt(foot)| and |dot(n, v_foot)| at the three new decisions (and by
|hgt(pos) - min_height| at the fourth)."""
import numpy as np

import plant_reference as pr
from disturb_reference import PW_FORCE0, PW_FORCE1, PW_POINT0, PW_POINT1, PW_SIZE, WrenchPlant
from estimator_reference import fk, jac, mat_vec, quat_to_rot
from plant_reference import PN_INIT, PN_STATUS, STATUS_BAD_TORQUE, STATUS_HEIGHT, STATUS_REACH, cross, lu3_solve, mat_t_vec, quad_sum

# include/mpcqp.h MPCQP_TR_*, MPCQP_ES_POOL
TR_NORMAL, TR_OFFSET, TR_MU, TR_SIZE = 0, 3, 4, 8
ES_POOL, ES_SIZE = 3, 24


def dot(n, v):
    """(n0 v0 + n1 v1) + n2 v2 with n [B,3] against v [B,...,3]."""
    n = n.reshape((n.shape[0],) + (1,) * (v.ndim - 2) + (3,))
    return (n[..., 0] * v[..., 0] + n[..., 1] * v[..., 1]) + n[..., 2] * v[..., 2]


def hgt(n, d, p):
    """((n0 p0 + n1 p1) + n2 p2) - d"""
    return dot(n, p) - d.reshape((d.shape[0],) + (1,) * (p.ndim - 2))


def level_rows(B, mu):
    t = np.zeros((B, TR_SIZE))
    t[:, TR_NORMAL + 2] = 1.0
    t[:, TR_MU] = mu
    return t


def substep(p, s, h, tau, wrench, terrain):
    """disturb_reference.substep (wrench None: plant_reference.substep) on the ground of the rows terrain
    [B, TR_SIZE].  Returns the ground reactions, the reach flag, the decision margin and (ft_out, mu fn, clipped)
    [B,4] of the legs that stayed in stance (else NaN / False), for the friction tests."""
    rho_opt, rho_fix = pr._geom(p)
    B = s["pos"].shape[0]
    n, d, mu = terrain[:, TR_NORMAL:TR_NORMAL + 3], terrain[:, TR_OFFSET], terrain[:, TR_MU]
    nl = n[:, None]
    with np.errstate(all="ignore"):
        R, p_b, J, reach, margin = pr.kinematics(p, s)
        Rl = R[:, None]
        # 2. the ground reaction: the normal part decides, the tangential part is scaled onto the cone
        g = lu3_solve(np.swapaxes(J, -1, -2), tau)
        f = -mat_vec(Rl, g)
        was = s["contact"]
        fn = dot(n, f)
        lift = was & (fn < 0.0)
        margin = np.minimum(margin, np.min(np.where(was, np.abs(fn), np.inf), 1))
        st = was & ~lift
        s["contact"] = st
        t = f - fn[..., None] * nl
        ft = np.sqrt((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2])
        lim = mu[:, None] * fn
        sc = np.where(ft > lim, lim / ft, 1.0)
        f = fn[..., None] * nl + sc[..., None] * t
        f = np.where(st[..., None], f, 0.0)
        tout = f - dot(n, f)[..., None] * nl
        friction = (np.where(st, np.sqrt(np.sum(tout * tout, -1)), np.nan), np.where(st, lim, np.nan), st & (ft > lim))
        Ij = np.array(p.joint_inertia, dtype=np.float64)
        bj = np.array(p.joint_damping, dtype=np.float64)
        s["qd"] = np.where(st[..., None], s["qd"], s["qd"] + h * (tau - bj * s["qd"]) / Ij)
        # 3. the wrench on the trunk: the legs, then the external forces
        r = s["foot"] - s["pos"][:, None]
        m = np.where(st[..., None], cross(r, f), 0.0)
        F, M = quad_sum(f), quad_sum(m)
        rm = mat_t_vec(R, M)
        if wrench is not None:
            F0, P0 = wrench[:, PW_FORCE0:PW_FORCE0 + 3], wrench[:, PW_POINT0:PW_POINT0 + 3]
            F1, P1 = wrench[:, PW_FORCE1:PW_FORCE1 + 3], wrench[:, PW_POINT1:PW_POINT1 + 3]
            fe = F0 + F1
            F = np.where(fe == 0.0, F, F + fe)
            ce = cross(P0, mat_t_vec(R, F0)) + cross(P1, mat_t_vec(R, F1))
            rm = np.where(ce == 0.0, rm, rm + ce)
        a = F / p.mass
        a[:, 2] = a[:, 2] + (-p.gravity)
        Ib = np.broadcast_to(np.array(p.inertia, dtype=np.float64).reshape(3, 3), (B, 3, 3))
        Iw = mat_vec(Ib, s["w"])
        wd = lu3_solve(Ib, rm - cross(s["w"], Iw))
        # 4. semi-implicit Euler
        s["v"] = s["v"] + h * a
        s["w"] = s["w"] + h * wd
        s["pos"] = s["pos"] + h * s["v"]
        qw, qx, qy, qz = (s["quat"][:, k] for k in range(4))
        w0, w1, w2 = (s["w"][:, k] for k in range(3))
        dq = np.stack([((-(qx * w0)) - qy * w1) - qz * w2, (qw * w0 + qy * w2) - qz * w1,
                       (qw * w1 + qz * w0) - qx * w2, (qw * w2 + qx * w1) - qy * w0], 1)
        quat = s["quat"] + (h * 0.5) * dq
        nq = np.sqrt(((quat[:, 0] * quat[:, 0] + quat[:, 1] * quat[:, 1]) + quat[:, 2] * quat[:, 2])
                     + quat[:, 3] * quat[:, 3])
        s["quat"] = quat / nq[:, None]
        s["acc"] = a
        # 5. swing legs: joints, feet, touchdown on the plane
        s["q"] = np.where(st[..., None], s["q"], s["q"] + h * s["qd"])
        R2 = quat_to_rot(s["quat"])[:, None]
        p2 = fk(s["q"], rho_opt, rho_fix)
        J2 = jac(s["q"], rho_opt, rho_fix)
        foot = s["pos"][:, None] + mat_vec(R2, p2)
        fv = s["v"][:, None] + mat_vec(R2, cross(s["w"][:, None], p2) + mat_vec(J2, s["qd"]))
        hf, vn = hgt(n, d, foot), dot(n, fv)
        land = ~st & (hf <= 0.0) & (vn < 0.0)
        margin = np.minimum(margin, np.min(np.where(st, np.inf, np.minimum(np.abs(hf), np.abs(vn))), 1))
        foot = np.where(land[..., None], foot - hf[..., None] * nl, foot)
        s["foot"] = np.where(st[..., None], s["foot"], foot)
        s["contact"] = st | land
    return f, reach, margin, friction


def initial_state(p, init, B, terrain):
    """plant_reference.initial_state with the contact rule of the plane: held iff hgt(foot) <= 0, then put on it."""
    s, _ = pr.initial_state(p, init, B)
    rho_opt, rho_fix = pr._geom(p)
    n, d = terrain[:, TR_NORMAL:TR_NORMAL + 3], terrain[:, TR_OFFSET]
    with np.errstate(all="ignore"):
        foot = s["pos"][:, None] + mat_vec(quat_to_rot(s["quat"])[:, None], fk(s["q"], rho_opt, rho_fix))
        hf = hgt(n, d, foot)
        st = hf <= 0.0
        margin = np.min(np.abs(hf), 1)
        foot = np.where(st[..., None], foot - hf[..., None] * n[:, None], foot)
    s.update(foot=foot, contact=st)
    return s, margin


class TerrainPlant(WrenchPlant):
    """disturb_reference.WrenchPlant whose ``step`` takes the terrain table [P, TR_SIZE] and, optionally, the episode
    slot rows whose ES_POOL names each robot's row (None: robot b stands on row b).  ``terrain=None`` is
    WrenchPlant.step.  After a step ``friction`` holds, per substep, (ft_out, mu fn, clipped) [B,4]."""

    def step(self, dt, tau, init=None, wrench=None, terrain=None, episode_state=None):
        if terrain is None:
            return super().step(dt, tau, init, wrench=wrench)
        p, B = self.p, self.B
        tau = np.asarray(tau, dtype=np.float64).reshape(B, 4, 3)
        table = np.asarray(terrain, dtype=np.float64).reshape(-1, TR_SIZE)
        if episode_state is None:
            idx = np.arange(B, dtype=np.float64)
        else:
            idx = np.asarray(episode_state, dtype=np.float64).reshape(B, ES_SIZE)[:, ES_POOL]
        with np.errstate(invalid="ignore"):
            inside = (idx > -1.0) & (idx < float(table.shape[0]))
        rows = table[np.where(inside, idx, 0.0).astype(np.int64)]
        ok = inside & np.all(np.isfinite(rows[:, :TR_MU + 1]), 1)
        rows = np.where(ok[:, None], rows, level_rows(B, p.mu))  # (a bad robot writes nothing; keep its lanes finite)
        finite = np.all(np.isfinite(tau.reshape(B, 12)), 1) & ok
        wz = None
        if wrench is not None:
            wrench = np.asarray(wrench, dtype=np.float64).reshape(B, PW_SIZE)
            finite &= np.all(np.isfinite(wrench), 1)
            wz = np.where(np.isfinite(wrench), wrench, 0.0)
        frozen = self.slot[:, PN_STATUS] != 0.0
        bad = ~frozen & ~finite
        fresh = self.slot[:, PN_INIT] == 0.0
        s0, m0 = initial_state(p, init, B, rows)
        s = self.unpack(self.slot)
        for k in pr._FIELDS:
            s[k] = np.where(fresh.reshape((B,) + (1,) * (s[k].ndim - 1)), s0[k], s[k])
        margin = np.where(fresh, m0, np.inf)
        f = np.zeros((B, 4, 3))
        reach = np.ones(B, dtype=bool)
        h = dt / p.substeps
        run = ~fresh
        tz = np.where(np.isfinite(tau), tau, 0.0)
        self.friction = []
        for _ in range(p.substeps):
            s1 = {k: v.copy() for k, v in s.items()}
            f1, r1, m1, fr = substep(p, s1, h, tz, wz, rows)
            for k in pr._FIELDS:
                s[k] = np.where(run.reshape((B,) + (1,) * (s[k].ndim - 1)), s1[k], s[k])
            f = np.where(run[:, None, None], f1, f)
            reach &= r1 | ~run
            margin = np.where(run, np.minimum(margin, m1), margin)
            live = (run & ~frozen & ~bad)[:, None]
            self.friction.append((np.where(live, fr[0], np.nan), np.where(live, fr[1], np.nan), fr[2] & live))
        R, p_b, J, r2, m2 = pr.kinematics(p, s)
        reach &= r2
        margin = np.minimum(margin, m2)
        with np.errstate(invalid="ignore"):
            hp = hgt(rows[:, TR_NORMAL:TR_NORMAL + 3], rows[:, TR_OFFSET], s["pos"])
            low = reach & (hp < p.min_height)
            margin = np.minimum(margin, np.abs(hp - p.min_height))
        status = np.where(bad, STATUS_BAD_TORQUE, np.where(~reach, STATUS_REACH, np.where(low, STATUS_HEIGHT, 0)))
        status = np.where(frozen, self.slot[:, PN_STATUS], status).astype(np.float64)
        wrote = ~frozen & ~bad & reach
        out = pr.outputs(p, s, R, p_b, J, f, status)
        new = self.pack(s, status)
        self.slot = np.where(wrote[:, None], new, self.slot)
        only = ~frozen & ~bad & ~reach
        self.slot[only, PN_STATUS] = STATUS_REACH
        return out, wrote, np.where(frozen | bad, np.inf, margin)
