"""TEST INFRASTRUCTURE — numpy restatement of the plant stage on a bilinear height field (csrc/mpcqp_plant.hip with
GROUND == FIELD, mpcqp_plant_step_field_device; include/mpcqp.h has the statement).

`lookup` restates the statement's lookup; `substep` / `FieldPlant` are tests/terrain_reference.py's with every point's
own hgt and normal at the four places of the statement: the fresh slot's contact rule, the ground reaction (the normal
under the held foot), the touchdown rule and the fallen rule (the ground under the trunk).  Everything else is that
file's helpers, statement for statement.  The decision margin is the plane's (|fn|, |hgt(foot)|, |dot(n, v_foot)|,
|hgt(pos) - min_height|), extended by the distance of fu_raw and fv_raw to 0 and 1 at every lookup whose normal is
used: the fresh feet, the held feet and the swing feet.  (The trunk's normal enters hgt(pos) alone, whose margin to
min_height is its own.)"""
import numpy as np

import plant_reference as pr
from disturb_reference import PW_FORCE0, PW_FORCE1, PW_POINT0, PW_POINT1, PW_SIZE
from estimator_reference import fk, jac, mat_vec, quat_to_rot
from plant_reference import PN_INIT, PN_STATUS, STATUS_BAD_TORQUE, STATUS_HEIGHT, STATUS_REACH, cross, lu3_solve, mat_t_vec, quad_sum
from terrain_reference import ES_POOL, ES_SIZE, TerrainPlant

# include/mpcqp.h MPCQP_HF_*
HF_X0, HF_Y0, HF_CELL, HF_MU, HF_NX, HF_NY, HF_OFFSET, HF_SIZE = 0, 1, 2, 3, 4, 5, 6, 8


def _cell(u, n):
    c = np.floor(u)
    c = np.where(c > 0.0, c, 0.0)
    c = np.where(c < n - 2.0, c, n - 2.0)
    return c.astype(np.int64), u - c


def lookup(hdr, H, p):
    """hgt [B,...], n [B,...,3] and the edge margin [B,...] (the distance of fu_raw and fv_raw to 0 and 1, in cells) of
    the points p [B,...,3] over the tiles of the header rows hdr [B, HF_SIZE] in the heights array H."""
    r = hdr.reshape((hdr.shape[0],) + (1,) * (p.ndim - 2) + (HF_SIZE,))
    x0, y0, cell = r[..., HF_X0], r[..., HF_Y0], r[..., HF_CELL]
    nx, ny, off = r[..., HF_NX], r[..., HF_NY], r[..., HF_OFFSET].astype(np.int64)
    with np.errstate(all="ignore"):
        i, fu_raw = _cell((p[..., 0] - x0) / cell, nx)
        j, fv_raw = _cell((p[..., 1] - y0) / cell, ny)
        w = nx.astype(np.int64)
        at = off + j * w + i
        assert np.all((i >= 0) & (i <= w - 2) & (j >= 0) & (j <= ny.astype(np.int64) - 2))
        h00, h10, h01, h11 = H[at], H[at + 1], H[at + w], H[at + w + 1]
        fu = np.minimum(np.maximum(fu_raw, 0.0), 1.0)
        fv = np.minimum(np.maximum(fv_raw, 0.0), 1.0)
        a = h00 + fu * (h10 - h00)
        b = h01 + fu * (h11 - h01)
        h = a + fv * (b - a)
        gx = ((h10 - h00) + fv * ((h11 - h01) - (h10 - h00))) / cell
        gy = (b - a) / cell
        gx = np.where((fu_raw < 0.0) | (fu_raw > 1.0), 0.0, gx)
        gy = np.where((fv_raw < 0.0) | (fv_raw > 1.0), 0.0, gy)
        s = np.sqrt((gx * gx + gy * gy) + 1.0)
        n = np.stack([-gx / s, -gy / s, 1.0 / s], -1)
        edge = np.minimum(np.minimum(np.abs(fu_raw), np.abs(fu_raw - 1.0)),
                          np.minimum(np.abs(fv_raw), np.abs(fv_raw - 1.0)))
        return (p[..., 2] - h) * n[..., 2], n, edge


def dot(n, v):
    return (n[..., 0] * v[..., 0] + n[..., 1] * v[..., 1]) + n[..., 2] * v[..., 2]


def good_rows(table, idx, heights_len):
    """(header rows [B, HF_SIZE] of the indices idx [B] (doubles), good [B]): the device's rule for a bad row.  A bad
    robot gets a harmless 2x2 header at offset 0 (it writes nothing; this keeps its lanes inside the array)."""
    with np.errstate(invalid="ignore"):
        inside = (idx > -1.0) & (idx < float(table.shape[0]))
        rows = table[np.where(inside, idx, 0.0).astype(np.int64)]
        nx, ny, off = rows[:, HF_NX], rows[:, HF_NY], rows[:, HF_OFFSET]
        ok = inside & np.all(np.isfinite(rows[:, :HF_OFFSET + 1]), 1) & (rows[:, HF_CELL] > 0.0) & (nx >= 2.0) & \
            (ny >= 2.0) & (off >= 0.0) & (off + nx * ny <= float(heights_len))
    safe = np.zeros(HF_SIZE)
    safe[[HF_CELL, HF_NX, HF_NY]] = 1.0, 2.0, 2.0
    return np.where(ok[:, None], rows, safe), ok


def substep(p, s, h, tau, wrench, hdr, H):
    """terrain_reference.substep with the normal under each held foot and hgt / normal under each swing foot.  Returns
    the ground reactions, the reach flag, the decision margin and (ft_out, mu fn, clipped) [B,4]."""
    rho_opt, rho_fix = pr._geom(p)
    B = s["pos"].shape[0]
    mu = hdr[:, HF_MU]
    with np.errstate(all="ignore"):
        R, p_b, J, reach, margin = pr.kinematics(p, s)
        Rl = R[:, None]
        # 2. the ground reaction, with the normal under the held foot
        g = lu3_solve(np.swapaxes(J, -1, -2), tau)
        f = -mat_vec(Rl, g)
        was = s["contact"]
        _, nl, edge = lookup(hdr, H, s["foot"])
        fn = dot(nl, f)
        lift = was & (fn < 0.0)
        margin = np.minimum(margin, np.min(np.where(was, np.minimum(np.abs(fn), edge), np.inf), 1))
        st = was & ~lift
        s["contact"] = st
        t = f - fn[..., None] * nl
        ft = np.sqrt((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2])
        lim = mu[:, None] * fn
        sc = np.where(ft > lim, lim / ft, 1.0)
        f = fn[..., None] * nl + sc[..., None] * t
        f = np.where(st[..., None], f, 0.0)
        tout = f - dot(nl, f)[..., None] * nl
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
        # 5. swing legs: joints, feet, touchdown on the surface
        s["q"] = np.where(st[..., None], s["q"], s["q"] + h * s["qd"])
        R2 = quat_to_rot(s["quat"])[:, None]
        p2 = fk(s["q"], rho_opt, rho_fix)
        J2 = jac(s["q"], rho_opt, rho_fix)
        foot = s["pos"][:, None] + mat_vec(R2, p2)
        fv = s["v"][:, None] + mat_vec(R2, cross(s["w"][:, None], p2) + mat_vec(J2, s["qd"]))
        hf, ns, edge = lookup(hdr, H, foot)
        vn = dot(ns, fv)
        land = ~st & (hf <= 0.0) & (vn < 0.0)
        margin = np.minimum(margin, np.min(np.where(st, np.inf, np.minimum(np.minimum(np.abs(hf), np.abs(vn)), edge)), 1))
        foot = np.where(land[..., None], foot - hf[..., None] * ns, foot)
        s["foot"] = np.where(st[..., None], s["foot"], foot)
        s["contact"] = st | land
    return f, reach, margin, friction


def initial_state(p, init, B, hdr, H):
    """plant_reference.initial_state with the contact rule of the field: held iff hgt(foot) <= 0, then put on it."""
    s, _ = pr.initial_state(p, init, B)
    rho_opt, rho_fix = pr._geom(p)
    with np.errstate(all="ignore"):
        foot = s["pos"][:, None] + mat_vec(quat_to_rot(s["quat"])[:, None], fk(s["q"], rho_opt, rho_fix))
        hf, n, edge = lookup(hdr, H, foot)
        st = hf <= 0.0
        margin = np.min(np.minimum(np.abs(hf), edge), 1)
        foot = np.where(st[..., None], foot - hf[..., None] * n, foot)
    s.update(foot=foot, contact=st)
    return s, margin


class FieldPlant(TerrainPlant):
    """terrain_reference.TerrainPlant whose ``step`` takes the header table [P, HF_SIZE] and the heights array as
    ``field=(table, heights)``.  ``field=None`` is TerrainPlant.step."""

    def step(self, dt, tau, init=None, wrench=None, field=None, episode_state=None, terrain=None):
        if field is None:
            return super().step(dt, tau, init, wrench=wrench, terrain=terrain, episode_state=episode_state)
        p, B = self.p, self.B
        tau = np.asarray(tau, dtype=np.float64).reshape(B, 4, 3)
        table = np.asarray(field[0], dtype=np.float64).reshape(-1, HF_SIZE)
        H = np.asarray(field[1], dtype=np.float64).reshape(-1)
        if episode_state is None:
            idx = np.arange(B, dtype=np.float64)
        else:
            idx = np.asarray(episode_state, dtype=np.float64).reshape(B, ES_SIZE)[:, ES_POOL]
        hdr, ok = good_rows(table, idx, H.shape[0])
        finite = np.all(np.isfinite(tau.reshape(B, 12)), 1) & ok
        wz = None
        if wrench is not None:
            wrench = np.asarray(wrench, dtype=np.float64).reshape(B, PW_SIZE)
            finite &= np.all(np.isfinite(wrench), 1)
            wz = np.where(np.isfinite(wrench), wrench, 0.0)
        frozen = self.slot[:, PN_STATUS] != 0.0
        bad = ~frozen & ~finite
        fresh = self.slot[:, PN_INIT] == 0.0
        s0, m0 = initial_state(p, init, B, hdr, H)
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
            f1, r1, m1, fr = substep(p, s1, h, tz, wz, hdr, H)
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
            hp = lookup(hdr, H, s["pos"])[0]
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
