"""TEST INFRASTRUCTURE — a numpy restatement of the reference's state front end, the checker of
mpcqp_state_estimate_device (the reference itself cannot be compiled here: Eigen/ROS absent).

    pose callback   src/a1_cpp/src/GazeboA1ROS.cpp:242-289   frames (:265-269, Utils.cpp:7-33), legs (:272-285)
    IMU callback    src/a1_cpp/src/GazeboA1ROS.cpp:306       root_ang_vel = R imu_ang_vel
    A1BasicEKF      src/a1_cpp/src/A1BasicEKF.cpp:7-164      ctor, init_state, update_estimation

Frames and legs are explicit binary +, -, *, / element by element, in the order of Eigen's
Quaterniond::toRotationMatrix / AngleAxisd::toRotationMatrix / 3x3 products and of Utils::quat_to_euler,
with arrays only carrying the robots side by side.  fk and jac are written from the leg geometry
(legKinematics/A1Kinematics.cpp:39-130 holds the same functions as generated expressions); the kernel
uses the same grouping, so the two differ only by their sin / cos.

The filter is the reference's dense algebra: stored A, B, C, Q, R matrices, dense products, and both
solves through a column-pivoted Householder QR (the reference: fullPivHouseholderQr, :134-138).  Each
step reports cond_2(S) and the determinant the drift reset tests (:143).
"""
import numpy as np

EPS = np.finfo(np.float64).eps
NS, NM = 18, 28


# ---- a. frames --------------------------------------------------------------------------------------
def quat_to_rot(q):
    """Eigen::Quaterniond::toRotationMatrix for q [B,4] as w, x, y, z -> [B,3,3]."""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1.0 - (tyy + tzz)
    R[:, 0, 1] = txy - twz
    R[:, 0, 2] = txz + twy
    R[:, 1, 0] = txy + twz
    R[:, 1, 1] = 1.0 - (txx + tzz)
    R[:, 1, 2] = tyz - twx
    R[:, 2, 0] = txz - twy
    R[:, 2, 1] = tyz + twx
    R[:, 2, 2] = 1.0 - (txx + tyy)
    return R


def quat_to_euler(q):
    """Utils::quat_to_euler (Utils.cpp:7-33), q [B,4] as w, x, y, z -> roll, pitch, yaw [B,3]."""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    y_sqr = y * y
    t0 = 2.0 * (w * x + y * z)
    t1 = 1.0 - 2.0 * (x * x + y_sqr)
    t2 = 2.0 * (w * y - z * x)
    t2 = np.where(t2 > 1.0, 1.0, t2)
    t2 = np.where(t2 < -1.0, -1.0, t2)
    t3 = 2.0 * (w * z + x * y)
    t4 = 1.0 - 2.0 * (y_sqr + z * z)
    return np.stack([np.arctan2(t0, t1), np.arcsin(t2), np.arctan2(t3, t4)], 1)


def rot_z(yaw):
    """Eigen::AngleAxisd(yaw, UnitZ()).toRotationMatrix() -> [B,3,3]."""
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.zeros((yaw.shape[0], 3, 3))
    R[:, 0, 0] = c
    R[:, 0, 1] = -s
    R[:, 1, 0] = s
    R[:, 1, 1] = c
    R[:, 2, 2] = (1.0 - c) + c
    return R


def mat_vec(R, v):
    """Eigen 3x3 * 3-vector, row by row: (R0 v0 + R1 v1) + R2 v2.  R [...,3,3], v [...,3]."""
    return np.stack([(R[..., r, 0] * v[..., 0] + R[..., r, 1] * v[..., 1]) + R[..., r, 2] * v[..., 2]
                     for r in range(3)], -1)


# ---- b. legs ----------------------------------------------------------------------------------------
def _leg_terms(q, rho_opt, rho_fix):
    q0, q1, q2 = q[..., 0], q[..., 1], q[..., 2]
    ox, oy, d, lt, lc = (rho_fix[..., k] for k in range(5))
    a0, a1, a2 = (rho_opt[..., k] for k in range(3))
    s0, c0, s1, c1 = np.sin(q0), np.cos(q0), np.sin(q1), np.cos(q1)
    q12 = q1 + q2
    s12, c12 = np.sin(q12), np.cos(q12)
    dd, le = d + a1, lc - a2
    h2 = le * c12 + a0 * s12  # the calf's drop below the knee
    x2 = a0 * c12 - le * s12  # and its forward reach
    hh = lt * c1 + h2         # the foot's drop below the hip axis
    xx = x2 - lt * s1         # and its forward reach
    return ox, oy, dd, s0, c0, h2, x2, hh, xx


def fk(q, rho_opt, rho_fix):
    """Foot position in the body frame.  The hip sits at (ox, oy, 0) and turns about x by q0; the thigh
    hangs from a point dd = motor offset + rho_opt[1] along the hip's y axis and swings in the hip's x-z
    plane by q1, the calf (length lc - rho_opt[2], foot shifted rho_opt[0] along its normal) by q1 + q2.
    q [...,3], rho_opt [...,3], rho_fix [...,5] -> [...,3]."""
    ox, oy, dd, s0, c0, h2, x2, hh, xx = _leg_terms(q, rho_opt, rho_fix)
    return np.stack([ox + xx, oy + (dd * c0 + hh * s0), dd * s0 - hh * c0], -1)


def jac(q, rho_opt, rho_fix):
    """d fk / d q, [...,3,3] with J[i][j] = d p_i / d q_j."""
    ox, oy, dd, s0, c0, h2, x2, hh, xx = _leg_terms(q, rho_opt, rho_fix)
    J = np.zeros(q.shape[:-1] + (3, 3))
    J[..., 0, 1] = -hh
    J[..., 0, 2] = -h2
    J[..., 1, 0] = hh * c0 - dd * s0
    J[..., 1, 1] = xx * s0
    J[..., 1, 2] = x2 * s0
    J[..., 2, 0] = dd * c0 + hh * s0
    J[..., 2, 1] = -(xx * c0)
    J[..., 2, 2] = -(x2 * c0)
    return J


def front_end(p, quat, joint_pos, joint_vel, imu_ang_vel):
    """Steps a-c for B robots: GazeboA1ROS.cpp:265-285 and :306."""
    B = quat.shape[0]
    rho_fix = np.array(p.rho_fix).reshape(1, 4, 5)
    rho_opt = np.array(p.rho_opt).reshape(1, 4, 3)
    R = quat_to_rot(quat)
    euler = quat_to_euler(quat)
    q = joint_pos.reshape(B, 4, 3)
    qd = joint_vel.reshape(B, 4, 3)
    pos_rel = fk(q, rho_opt, rho_fix)
    J = jac(q, rho_opt, rho_fix)
    vel_rel = mat_vec(J, qd)
    Rl = R[:, None]
    return dict(root_rot_mat=R, root_euler=euler, rot_z=rot_z(euler[:, 2]), foot_pos_rel=pos_rel, j_foot=J,
                foot_vel_rel=vel_rel, foot_pos_abs=mat_vec(Rl, pos_rel), foot_vel_abs=mat_vec(Rl, vel_rel),
                root_ang_vel=mat_vec(R, imu_ang_vel))


# ---- d. the filter ----------------------------------------------------------------------------------
def make_C():
    """A1BasicEKF ctor (A1BasicEKF.cpp:11-17)."""
    C = np.zeros((NM, NS))
    eye3 = np.eye(3)
    for i in range(4):
        C[3 * i:3 * i + 3, 0:3] = -eye3
        C[3 * i:3 * i + 3, 6 + 3 * i:9 + 3 * i] = eye3
        C[12 + 3 * i:15 + 3 * i, 3:6] = eye3
        C[24 + i, 6 + 3 * i + 2] = 1.0
    return C


def skew(v):
    """Utils::skew (Utils.cpp:35-41), v [B,3] -> [B,3,3]."""
    S = np.zeros((v.shape[0], 3, 3))
    S[:, 0, 1], S[:, 0, 2] = -v[:, 2], v[:, 1]
    S[:, 1, 0], S[:, 1, 2] = v[:, 2], -v[:, 0]
    S[:, 2, 0], S[:, 2, 1] = -v[:, 1], v[:, 0]
    return S


def qr_solve(S, Y):
    """Solve S X = Y for a batch through a Householder QR with column pivoting (largest remaining column
    norm first).  S [B,n,n], Y [B,n,k]."""
    A, Y = S.copy(), Y.copy()
    B, n, _ = A.shape
    perm = np.tile(np.arange(n), (B, 1))
    rows = np.arange(B)
    for k in range(n):
        j = k + np.argmax((A[:, k:, k:] ** 2).sum(1), 1)
        ck, cj = A[rows, :, k].copy(), A[rows, :, j].copy()
        A[rows, :, k], A[rows, :, j] = cj, ck
        pk, pj = perm[rows, k].copy(), perm[rows, j].copy()
        perm[rows, k], perm[rows, j] = pj, pk
        v = A[:, k:, k].copy()
        alpha = -np.where(v[:, 0] >= 0.0, 1.0, -1.0) * np.sqrt((v * v).sum(1))
        v[:, 0] -= alpha
        beta = 2.0 / (v * v).sum(1)
        A[:, k:, k:] -= (beta[:, None] * v)[:, :, None] * np.einsum("bi,bij->bj", v, A[:, k:, k:])[:, None, :]
        Y[:, k:, :] -= (beta[:, None] * v)[:, :, None] * np.einsum("bi,bij->bj", v, Y[:, k:, :])[:, None, :]
    Z = np.zeros_like(Y)
    for i in range(n - 1, -1, -1):
        Z[:, i] = (Y[:, i] - np.einsum("bj,bjk->bk", A[:, i, i + 1:], Z[:, i + 1:])) / A[:, i, i, None]
    X = np.empty_like(Z)
    np.put_along_axis(X, perm[:, :, None], Z, 1)
    return X


def contact_weights(p, foot_force, movement_mode):
    """estimated_contacts (A1BasicEKF.cpp:79-86): std::min(std::max(f / 100, 0), 1), 1 when standing."""
    c = foot_force / (p.contact_force_scale - 0.0)
    c = np.where(c < 0.0, 0.0, c)
    c = np.where(1.0 < c, 1.0, c)
    return np.where((np.asarray(movement_mode) == 0)[:, None], 1.0, c)


def noise(p, dt, c):
    """Contact-scaled Q [B,18,18] and R [B,28,28] (A1BasicEKF.cpp:19-32, :44-54, :88-107)."""
    B = c.shape[0]
    Q = np.zeros((B, NS, NS))
    Rm = np.zeros((B, NM, NM))
    scale = 1.0 + (1.0 - c) * 1e3
    for k in range(3):
        Q[:, k, k] = p.process_noise_pimu * dt / 20.0
        Q[:, 3 + k, 3 + k] = p.process_noise_vimu * dt * 9.8 / 20.0
    for i in range(4):
        for k in range(3):
            Q[:, 6 + 3 * i + k, 6 + 3 * i + k] = scale[:, i] * dt * p.process_noise_pfoot
            Rm[:, 3 * i + k, 3 * i + k] = scale[:, i] * p.sensor_noise_pimu_rel_foot
            Rm[:, 12 + 3 * i + k, 12 + 3 * i + k] = scale[:, i] * p.sensor_noise_vimu_rel_foot
        Rm[:, 24 + i, 24 + i] = scale[:, i] * p.sensor_noise_zfoot if p.assume_flat_ground else p.height_noise_no_flat
    return Q, Rm


def predict_and_measure(p, dt, x, P, fe, imu_acc, imu_ang_vel, c):
    """Everything of update_estimation up to S (A1BasicEKF.cpp:72-131): xbar, Pbar, y - C xbar, S."""
    B = x.shape[0]
    A = np.eye(NS)
    A[0:3, 3:6] = dt * np.eye(3)
    Bm = np.zeros((NS, 3))
    Bm[3:6, 0:3] = dt * np.eye(3)
    C = make_C()
    R = fe["root_rot_mat"]
    u = mat_vec(R, imu_acc) + np.array([0.0, 0.0, -p.gravity])
    Q, Rm = noise(p, dt, c)
    xbar = x @ A.T + u @ Bm.T
    Pbar = A @ P @ A.T + Q
    y = np.zeros((B, NM))
    sk = skew(imu_ang_vel)
    for i in range(4):
        fk_pos = fe["foot_pos_rel"][:, i]
        y[:, 3 * i:3 * i + 3] = mat_vec(R, fk_pos)
        leg_v = -fe["foot_vel_rel"][:, i] - mat_vec(sk, fk_pos)
        ci = c[:, i, None]
        y[:, 12 + 3 * i:15 + 3 * i] = (1.0 - ci) * x[:, 3:6] + mat_vec(ci[:, :, None] * R, leg_v)
        y[:, 24 + i] = (1.0 - c[:, i]) * (x[:, 2] + fk_pos[:, 2]) + c[:, i] * 0.0
    S = C @ Pbar @ C.T + Rm
    S = 0.5 * (S + S.transpose(0, 2, 1))
    return xbar, Pbar, y - xbar @ C.T, S


def correct(xbar, Pbar, err, S):
    """x and P from the two QR solves (A1BasicEKF.cpp:133-140)."""
    C = make_C()
    B = xbar.shape[0]
    sol = qr_solve(S, np.concatenate([err[:, :, None], np.broadcast_to(C, (B, NM, NS))], 2))
    PCt = Pbar @ C.T
    x = xbar + np.einsum("bij,bj->bi", PCt, sol[:, :, 0])
    P = Pbar - PCt @ sol[:, :, 1:] @ Pbar
    return x, 0.5 * (P + P.transpose(0, 2, 1))


def drift_reset(p, P):
    """A1BasicEKF.cpp:143-147; returns P, the determinant as tested and the decision."""
    det = P[:, 0, 0] * P[:, 1, 1] - P[:, 1, 0] * P[:, 0, 1]
    reset = det > p.drift_threshold
    Pr = P.copy()
    Pr[:, 0:2, 2:] = 0.0
    Pr[:, 2:, 0:2] = 0.0
    Pr[:, 0:2, 0:2] = P[:, 0:2, 0:2] / p.drift_divisor
    return np.where(reset[:, None, None], Pr, P), det, reset


class Estimator:
    """GazeboA1ROS's callbacks + A1BasicEKF for B robots, one ``step`` per tick."""

    def __init__(self, p, B, x=None, P=None):
        self.p, self.B = p, B
        self.inited = x is not None
        self.x = np.zeros((B, NS)) if x is None else np.array(x, dtype=np.float64).reshape(B, NS)
        self.P = np.zeros((B, NS, NS)) if P is None else np.array(P, dtype=np.float64).reshape(B, NS, NS)

    def step(self, dt, quat, joint_pos, joint_vel, imu_acc, imu_ang_vel, foot_force, movement_mode, root_pos,
             root_lin_vel):
        p, B = self.p, self.B
        out = front_end(p, quat, joint_pos, joint_vel, imu_ang_vel)
        if not self.inited:
            # init_state (A1BasicEKF.cpp:55-68); root_pos / root_lin_vel stay the caller's
            self.inited = True
            self.P = np.broadcast_to(np.eye(NS) * p.init_cov, (B, NS, NS)).copy()
            self.x = np.zeros((B, NS))
            self.x[:, 2] = p.init_height
            for i in range(4):
                self.x[:, 6 + 3 * i:9 + 3 * i] = out["foot_pos_abs"][:, i] + self.x[:, 0:3]
            out.update(root_pos=np.array(root_pos, dtype=np.float64), root_lin_vel=np.array(root_lin_vel, dtype=np.float64),
                       contact_weights=np.zeros((B, 4)), det=np.zeros(B), reset=np.zeros(B, bool),
                       cond=np.ones(B), contacts=np.zeros((B, 4), bool))
        else:
            c = contact_weights(p, foot_force, movement_mode)
            xbar, Pbar, err, S = predict_and_measure(p, dt, self.x, self.P, out, imu_acc, imu_ang_vel, c)
            x, P = correct(xbar, Pbar, err, S)
            self.P, det, reset = drift_reset(p, P)
            self.x = x
            out.update(root_pos=x[:, 0:3].copy(), root_lin_vel=x[:, 3:6].copy(), contact_weights=c, det=det,
                       reset=reset, cond=np.linalg.cond(S), contacts=~(c < 0.5))
        out.update(x=self.x.copy(), P=self.P.copy(), diag_P=np.diagonal(self.P, axis1=1, axis2=2).copy())
        return out
