"""TEST INFRASTRUCTURE — a numpy restatement of the rigid-body plant stage (csrc/mpcqp_plant.hip,
mpcqp_plant_step_device), the checker of the kernel and the subject of tests/test_plant.py.

The model: a single rigid trunk, massless stance legs (a stance foot is held where it touched down and
the leg's joint torques act on the trunk as the ground reaction f = -R J^-T tau), joint-space swing legs
(each joint a free inertia driven by its torque; nothing of a swing leg acts on the trunk), flat ground
z = 0.  Left out: leg mass, the swing legs' reaction on the trunk, foot slip, terrain, joint limits, and
impact dynamics beyond zeroing the landing foot's velocity.

Every expression is explicit binary +, -, *, / in the statement order of the kernel, with arrays only
carrying robots [B] and legs [B,4] side by side; the leg kinematics are estimator_reference's fk / jac, so
the plant and the estimator agree on them.  The two sides differ only by their sin / cos / atan2 / acos /
asin / sqrt.
"""
from types import SimpleNamespace

import numpy as np

from estimator_reference import fk, jac, mat_vec, quat_to_euler, quat_to_rot, rot_z

# slot layout (include/mpcqp.h MPCQP_PN_*)
PN_INIT, PN_POS, PN_QUAT, PN_LIN_VEL, PN_ANG_VEL, PN_JOINT_POS, PN_JOINT_VEL = 0, 1, 4, 8, 11, 14, 26
PN_FOOT, PN_CONTACT, PN_ACC, PN_STATUS, PN_SIZE = 38, 50, 54, 57, 64
# init row (MPCQP_PI_*)
PI_POS, PI_QUAT, PI_JOINT_POS, PI_SIZE = 0, 3, 7, 20
# output row (MPCQP_PT_*)
PT_POS, PT_QUAT, PT_EULER, PT_LIN_VEL, PT_ANG_VEL, PT_CONTACTS, PT_GRF, PT_FOOT, PT_ACC, PT_STATUS = (
    0, 3, 7, 10, 13, 16, 20, 32, 44, 47)
PT_SIZE = 48
STATUS_OK, STATUS_REACH, STATUS_HEIGHT, STATUS_BAD_TORQUE = 0, 1, 2, 3

GO1_MASS = 13.0
GO1_INERTIA = (0.0168352186, 0.0, 0.0, 0.0, 0.0656071082, 0.0, 0.0, 0.0, 0.0742720659)


def default_params(**over):
    """mpcqp_plant_default_params, restated (tests/test_plant.py compares the two)."""
    ox = (0.1881, 0.1881, -0.1881, -0.1881)
    oy = (0.04675, -0.04675, 0.04675, -0.04675)
    mo = (0.08, -0.08, 0.08, -0.08)
    p = SimpleNamespace(
        rho_fix=[v for i in range(4) for v in (ox[i], oy[i], mo[i], 0.213, 0.213)], rho_opt=[0.0] * 12,
        mass=GO1_MASS, inertia=list(GO1_INERTIA), mu=0.6, gravity=9.81, joint_inertia=[0.03, 0.03, 0.01],
        joint_damping=[0.0, 0.0, 0.0], default_joint_pos=[0.0, 0.8, -1.6] * 4, min_height=0.05, substeps=4)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _geom(p):
    return (np.array(p.rho_opt, dtype=np.float64).reshape(1, 4, 3),
            np.array(p.rho_fix, dtype=np.float64).reshape(1, 4, 5))


# ---- the shared 3x3 solve (csrc/mpcqp_lu3.h): Eigen PartialPivLU<Matrix3d>(A).solve(b) -----------------
def lu3_solve(A, b):
    """A [...,3,3], b [...,3] -> x [...,3]; pivot on the first maximal |a_ik|, whole rows swapped."""
    a = [np.array(A[..., i, j], dtype=np.float64) for i in range(3) for j in range(3)]
    b = [np.array(b[..., i], dtype=np.float64) for i in range(3)]

    def swap_if(s, arr, i, j):
        t = arr[i]
        arr[i] = np.where(s, arr[j], arr[i])
        arr[j] = np.where(s, t, arr[j])

    with np.errstate(all="ignore"):
        m0, m1, m2 = np.abs(a[0]), np.abs(a[3]), np.abs(a[6])
        p1 = m1 > m0
        best = np.where(p1, m1, m0)
        p2 = m2 > best
        best = np.where(p2, m2, best)
        for j in range(3):
            swap_if(p2, a, j, 6 + j)
            swap_if(~p2 & p1, a, j, 3 + j)
        swap_if(p2, b, 0, 2)
        swap_if(~p2 & p1, b, 0, 1)
        nz = best != 0.0
        a[3] = np.where(nz, a[3] / a[0], a[3])
        a[6] = np.where(nz, a[6] / a[0], a[6])
        a[4] = a[4] - a[3] * a[1]
        a[5] = a[5] - a[3] * a[2]
        a[7] = a[7] - a[6] * a[1]
        a[8] = a[8] - a[6] * a[2]
        m1, m2 = np.abs(a[4]), np.abs(a[7])
        q = m2 > m1
        best = np.where(q, m2, m1)
        for j in range(3):
            swap_if(q, a, 3 + j, 6 + j)
        swap_if(q, b, 1, 2)
        a[7] = np.where(best != 0.0, a[7] / a[4], a[7])
        a[8] = a[8] - a[7] * a[5]
        y0 = b[0]
        y1 = b[1] - a[3] * y0
        y2 = (b[2] - a[6] * y0) - a[7] * y1
        x2 = y2 / a[8]
        x1 = (y1 - a[5] * x2) / a[4]
        x0 = ((y0 - a[1] * x1) - a[2] * x2) / a[0]
    return np.stack([x0, x1, x2], -1)


def mat_t_vec(R, v):
    """R' v, column by column: (R0k v0 + R1k v1) + R2k v2."""
    return np.stack([(R[..., 0, k] * v[..., 0] + R[..., 1, k] * v[..., 1]) + R[..., 2, k] * v[..., 2]
                     for k in range(3)], -1)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def quad_sum(x):
    """x [B,4,...] -> (l0 + l1) + (l2 + l3)."""
    return (x[:, 0] + x[:, 1]) + (x[:, 2] + x[:, 3])


# ---- leg inverse kinematics ----------------------------------------------------------------------------
def ik(p_b, rho_opt, rho_fix):
    """The analytic inverse of fk on the branch foot drop hh >= 0, knee angle negative.  Returns q [...,3],
    the reach flag and the reach margin min(y^2 + z^2 - dd^2, 1 - |c|)."""
    ox, oy, d, lt, lc = (rho_fix[..., k] for k in range(5))
    a0, a1, a2 = (rho_opt[..., k] for k in range(3))
    with np.errstate(all="ignore"):
        x, y, z = p_b[..., 0] - ox, p_b[..., 1] - oy, p_b[..., 2]
        dd, le = d + a1, lc - a2
        lce = np.sqrt(le * le + a0 * a0)
        phi = np.arctan2(a0, le)
        arg = (y * y + z * z) - dd * dd
        hh = np.sqrt(arg)
        q0 = np.arctan2(z, y) - np.arctan2(-hh, dd)
        c = (((x * x + hh * hh) - lt * lt) - lce * lce) / ((2.0 * lt) * lce)
        qk = -np.arccos(c)
        q1 = np.arctan2(-x, hh) - np.arctan2(lce * np.sin(qk), lt + lce * np.cos(qk))
        q2 = qk + phi
        ok = (arg >= 0.0) & (np.abs(c) <= 1.0)  # a NaN is out of reach
        margin = np.minimum(arg, 1.0 - np.abs(c))
    return np.stack([q0, q1, q2], -1), ok, margin


# ---- the model -----------------------------------------------------------------------------------------
_FIELDS = ("pos", "quat", "v", "w", "q", "qd", "foot", "contact", "acc")


def _zero_state(B):
    return dict(pos=np.zeros((B, 3)), quat=np.zeros((B, 4)), v=np.zeros((B, 3)), w=np.zeros((B, 3)),
                q=np.zeros((B, 4, 3)), qd=np.zeros((B, 4, 3)), foot=np.zeros((B, 4, 3)),
                contact=np.zeros((B, 4), dtype=bool), acc=np.zeros((B, 3)))


def kinematics(p, s):
    """Step 1: stance legs follow their held feet (q from IK, qd from the trunk's motion), swing feet follow
    their joints.  Updates s in place; returns R, p_b, J, the reach flag [B] and the reach margin [B]."""
    rho_opt, rho_fix = _geom(p)
    st = s["contact"]
    R = quat_to_rot(s["quat"])
    Rl = R[:, None]
    pb_held = mat_t_vec(Rl, s["foot"] - s["pos"][:, None])
    q_ik, ok, margin = ik(pb_held, rho_opt, rho_fix)
    s["q"] = np.where(st[..., None], q_ik, s["q"])
    J = jac(s["q"], rho_opt, rho_fix)
    p_b = fk(s["q"], rho_opt, rho_fix)
    with np.errstate(all="ignore"):
        rhs = (-mat_t_vec(Rl, s["v"][:, None])) - cross(s["w"][:, None], p_b)
        qd_st = lu3_solve(J, rhs)
    s["qd"] = np.where(st[..., None], qd_st, s["qd"])
    s["foot"] = np.where(st[..., None], s["foot"], s["pos"][:, None] + mat_vec(Rl, p_b))
    reach = np.all(ok | ~st, 1)
    return R, p_b, J, reach, np.min(np.where(st, margin, np.inf), 1)


def substep(p, s, h, tau):
    """Steps 1-5 for one substep of length h with the torque row tau [B,4,3] held.  Returns the ground
    reactions [B,4,3] (0 for a leg that exerts none), the reach flag and the decision margin [B]."""
    rho_opt, rho_fix = _geom(p)
    B = s["pos"].shape[0]
    with np.errstate(all="ignore"):
        R, p_b, J, reach, margin = kinematics(p, s)
        Rl = R[:, None]
        # 2. the ground reaction of a massless leg, f = -R J^-T tau, the inverse of tau = J^T (-f_grf)
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
        # 3. the wrench on the trunk
        r = s["foot"] - s["pos"][:, None]
        m = np.where(st[..., None], cross(r, f), 0.0)
        F, M = quad_sum(f), quad_sum(m)
        a = F / p.mass
        a[:, 2] = a[:, 2] + (-p.gravity)
        Ib = np.broadcast_to(np.array(p.inertia, dtype=np.float64).reshape(3, 3), (B, 3, 3))
        Iw = mat_vec(Ib, s["w"])
        wd = lu3_solve(Ib, mat_t_vec(R, M) - cross(s["w"], Iw))
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


def initial_state(p, init=None, B=None):
    """A fresh slot's first tick: the state from the init rows [B, PI_SIZE] (None: the defaults)."""
    rho_opt, rho_fix = _geom(p)
    if init is None:
        q = np.broadcast_to(np.array(p.default_joint_pos, dtype=np.float64).reshape(1, 4, 3), (B, 4, 3)).copy()
        z = -fk(q[:, 0], rho_opt[:, 0], rho_fix[:, 0])[:, 2]
        pos = np.stack([np.zeros(B), np.zeros(B), z], 1)
        quat = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (B, 1))
    else:
        init = np.asarray(init, dtype=np.float64).reshape(-1, PI_SIZE)
        B = init.shape[0]
        pos = init[:, PI_POS:PI_POS + 3].copy()
        quat = init[:, PI_QUAT:PI_QUAT + 4].copy()
        q = init[:, PI_JOINT_POS:PI_JOINT_POS + 12].reshape(B, 4, 3).copy()
    s = _zero_state(B)
    s.update(pos=pos, quat=quat, q=q)
    foot = pos[:, None] + mat_vec(quat_to_rot(quat)[:, None], fk(q, rho_opt, rho_fix))
    st = foot[..., 2] <= 0.0
    margin = np.min(np.abs(foot[..., 2]), 1)
    foot[..., 2] = np.where(st, 0.0, foot[..., 2])
    s.update(foot=foot, contact=st)
    return s, margin


def outputs(p, s, R, p_b, J, f, status):
    """The rows of one tick from the state after its closing kinematics pass."""
    B = s["pos"].shape[0]
    euler = quat_to_euler(s["quat"])
    g = np.array([0.0, 0.0, p.gravity])
    return dict(
        quat=s["quat"].copy(), joint_pos=s["q"].reshape(B, 12).copy(), joint_vel=s["qd"].reshape(B, 12).copy(),
        imu_acc=mat_t_vec(R, s["acc"] + g), imu_ang_vel=s["w"].copy(),
        foot_force=np.where(s["contact"], f[..., 2], 0.0), rot_z=rot_z(euler[:, 2]),
        root_euler=euler, root_pos=s["pos"].copy(), root_ang_vel=mat_vec(R, s["w"]), root_lin_vel=s["v"].copy(),
        root_rot_mat=R, foot_pos_abs=mat_vec(R[:, None], p_b), j_foot=J,
        contacts=s["contact"].copy(), grf=f.copy(), foot_world=s["foot"].copy(), acc=s["acc"].copy(),
        status=np.asarray(status, dtype=np.float64).copy())


class Plant:
    """B robots; ``step`` is one call of mpcqp_plant_step_device.  ``slot`` is the device slot image."""

    def __init__(self, p, B, slot=None):
        self.p, self.B = p, B
        self.slot = np.zeros((B, PN_SIZE)) if slot is None else np.array(slot, dtype=np.float64).reshape(B, PN_SIZE)

    @staticmethod
    def unpack(slot):
        B = slot.shape[0]
        return dict(pos=slot[:, PN_POS:PN_POS + 3].copy(), quat=slot[:, PN_QUAT:PN_QUAT + 4].copy(),
                    v=slot[:, PN_LIN_VEL:PN_LIN_VEL + 3].copy(), w=slot[:, PN_ANG_VEL:PN_ANG_VEL + 3].copy(),
                    q=slot[:, PN_JOINT_POS:PN_JOINT_POS + 12].reshape(B, 4, 3).copy(),
                    qd=slot[:, PN_JOINT_VEL:PN_JOINT_VEL + 12].reshape(B, 4, 3).copy(),
                    foot=slot[:, PN_FOOT:PN_FOOT + 12].reshape(B, 4, 3).copy(),
                    contact=slot[:, PN_CONTACT:PN_CONTACT + 4] != 0.0, acc=slot[:, PN_ACC:PN_ACC + 3].copy())

    @staticmethod
    def pack(s, status):
        B = s["pos"].shape[0]
        slot = np.zeros((B, PN_SIZE))
        slot[:, PN_INIT] = 1.0
        slot[:, PN_POS:PN_POS + 3] = s["pos"]
        slot[:, PN_QUAT:PN_QUAT + 4] = s["quat"]
        slot[:, PN_LIN_VEL:PN_LIN_VEL + 3] = s["v"]
        slot[:, PN_ANG_VEL:PN_ANG_VEL + 3] = s["w"]
        slot[:, PN_JOINT_POS:PN_JOINT_POS + 12] = s["q"].reshape(B, 12)
        slot[:, PN_JOINT_VEL:PN_JOINT_VEL + 12] = s["qd"].reshape(B, 12)
        slot[:, PN_FOOT:PN_FOOT + 12] = s["foot"].reshape(B, 12)
        slot[:, PN_CONTACT:PN_CONTACT + 4] = s["contact"].astype(np.float64)
        slot[:, PN_ACC:PN_ACC + 3] = s["acc"]
        slot[:, PN_STATUS] = status
        return slot

    def step(self, dt, tau, init=None):
        """One tick.  Returns (out, wrote, margin): the rows (outputs()), the robots [B] whose slot and rows
        the tick wrote (the others keep every double, apart from ``status`` of the output row for a
        non-finite torque row or a leg out of reach), and the smallest decision margin met [B]."""
        p, B = self.p, self.B
        tau = np.asarray(tau, dtype=np.float64).reshape(B, 4, 3)
        frozen = self.slot[:, PN_STATUS] != 0.0
        bad = ~frozen & ~np.all(np.isfinite(tau.reshape(B, 12)), 1)
        fresh = self.slot[:, PN_INIT] == 0.0
        s0, m0 = initial_state(p, init, B)
        s = self.unpack(self.slot)
        for k in _FIELDS:
            s[k] = np.where(fresh.reshape((B,) + (1,) * (s[k].ndim - 1)), s0[k], s[k])
        margin = np.where(fresh, m0, np.inf)
        f = np.zeros((B, 4, 3))
        reach = np.ones(B, dtype=bool)
        h = dt / p.substeps
        run = ~fresh
        tz = np.where(np.isfinite(tau), tau, 0.0)
        for _ in range(p.substeps):
            s1 = {k: v.copy() for k, v in s.items()}
            f1, r1, m1 = substep(p, s1, h, tz)
            for k in _FIELDS:
                s[k] = np.where(run.reshape((B,) + (1,) * (s[k].ndim - 1)), s1[k], s[k])
            f = np.where(run[:, None, None], f1, f)
            reach &= r1 | ~run
            margin = np.where(run, np.minimum(margin, m1), margin)
        R, p_b, J, r2, m2 = kinematics(p, s)
        reach &= r2
        margin = np.minimum(margin, m2)
        with np.errstate(invalid="ignore"):
            low = reach & (s["pos"][:, 2] < p.min_height)
            margin = np.minimum(margin, np.abs(s["pos"][:, 2] - p.min_height))
        status = np.where(bad, STATUS_BAD_TORQUE, np.where(~reach, STATUS_REACH, np.where(low, STATUS_HEIGHT, 0)))
        status = np.where(frozen, self.slot[:, PN_STATUS], status).astype(np.float64)
        wrote = ~frozen & ~bad & reach
        out = outputs(p, s, R, p_b, J, f, status)
        new = self.pack(s, status)
        self.slot = np.where(wrote[:, None], new, self.slot)
        only = ~frozen & ~bad & ~reach  # out of reach: the slot keeps its state and takes the status alone
        self.slot[only, PN_STATUS] = STATUS_REACH
        return out, wrote, np.where(frozen | bad, np.inf, margin)
