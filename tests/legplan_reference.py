"""TEST INFRASTRUCTURE — a numpy restatement of the reference's per-tick leg plan, the checker of
mpcqp_leg_plan_device (the reference itself cannot be compiled here: Eigen/ROS absent).

    A1RobotControl::update_plan               src/a1_cpp/src/A1RobotControl.cpp:148-202
    A1RobotControl::generate_swing_legs_ctrl  src/a1_cpp/src/A1RobotControl.cpp:204-287
    compute_grf, terrain adaptation           src/a1_cpp/src/A1RobotControl.cpp:335-376, :566-582
    MovingWindowFilter                        src/a1_cpp/src/utils/filter.hpp:14-63
    BezierUtils, pseudo_inverse, dihedral     src/a1_cpp/src/utils/Utils.cpp:44-107

Every compared quantity is built from explicit binary +, -, *, / in the reference's order, written
out element by element (arrays only carry the robots and legs side by side; no einsum, sum or dot on
the compared path), with np.fmod, np.sqrt and np.float32 where the reference has std::fmod,
std::sqrt and float.  One stated deviation, shared with the kernel: the Bezier powers are repeated
multiplications from 1.0 instead of std::pow (``bezier_pow`` keeps the pow form for the self-check).
The terrain fit keeps the reference's SVD semantics through np.linalg.pinv(W'W, rcond=3 eps).
"""
import numpy as np

EPS = np.finfo(np.float64).eps
BEZIER_COEF = (1.0, 4.0, 6.0, 4.0, 1.0)


class MovingWindowFilter:
    """filter.hpp MovingWindowFilter for an array of independent filters of one window size.
    ``calculate_average(x, mask)`` advances only the filters selected by mask."""

    def __init__(self, shape, window):
        self.window = int(window)
        self.sum = np.zeros(shape)
        self.correction = np.zeros(shape)
        self.ring = np.zeros(tuple(shape) + (self.window,))
        self.head = np.zeros(shape, dtype=np.int64)
        self.count = np.zeros(shape, dtype=np.int64)

    def _neumaier(self, value, mask):
        new_sum = self.sum + value
        big = np.abs(self.sum) >= np.abs(value)
        corr = np.where(big, self.correction + ((self.sum - new_sum) + value),
                        self.correction + ((value - new_sum) + self.sum))
        self.correction = np.where(mask, corr, self.correction)
        self.sum = np.where(mask, new_sum, self.sum)

    def calculate_average(self, value, mask=None):
        value = np.broadcast_to(np.asarray(value, dtype=np.float64), self.sum.shape)
        mask = np.ones(self.sum.shape, bool) if mask is None else np.broadcast_to(mask, self.sum.shape)
        front = np.take_along_axis(self.ring, self.head[..., None], -1)[..., 0]
        self._neumaier(-front, mask & (self.count >= self.window))  # pop_front of a full deque
        self._neumaier(value, mask)
        new_ring = self.ring.copy()
        np.put_along_axis(new_ring, self.head[..., None], value[..., None], -1)
        self.ring = np.where(mask[..., None], new_ring, self.ring)
        self.head = np.where(mask, (self.head + 1) % self.window, self.head)
        self.count = np.where(mask, np.minimum(self.count + 1, self.window), self.count)
        return (self.sum + self.correction) / float(self.window)


def bezier_mul(t, P):
    """bezier_curve (Utils.cpp:100-107) with t^i, (1-t)^k by repeated multiplication from 1.0."""
    u = 1.0 - t
    tp, up = [np.ones_like(t)], [np.ones_like(t)]
    for _ in range(4):
        tp.append(tp[-1] * t)
        up.append(up[-1] * u)
    y = np.zeros_like(t)
    for i in range(5):
        y = y + BEZIER_COEF[i] * tp[i] * up[4 - i] * P[i]
    return y


def bezier_pow(t, P):
    """bezier_curve as the reference writes it, with std::pow."""
    y = np.zeros_like(t)
    for i in range(5):
        y = y + BEZIER_COEF[i] * np.power(t, i) * np.power(1 - t, 4 - i) * P[i]
    return y


def _matT_vec(M, v):
    """M^T v for M [B,3,3] row-major, v [...,3] broadcast against B: Eigen's coefficient order."""
    return [(M[:, 0, k, None] * v[0] + M[:, 1, k, None] * v[1]) + M[:, 2, k, None] * v[2] for k in range(3)]


def _mat_vec(M, v):
    return [(M[:, k, 0, None] * v[0] + M[:, k, 1, None] * v[1]) + M[:, k, 2, None] * v[2] for k in range(3)]


class LegPlan:
    """B controllers side by side; a fresh object is A1CtrlStates::reset() + the A1RobotControl ctor.

    ``p`` is any object with mpcqp_plan_params' fields ([4][3] ones leg-major, flat or shaped)."""

    def __init__(self, p, batch):
        B = self.B = int(batch)
        self.dfp = np.asarray(p.default_foot_pos, dtype=np.float64).reshape(4, 3)
        self.kp = np.asarray(p.kp_foot, dtype=np.float64).reshape(4, 3)
        self.kd = np.asarray(p.kd_foot, dtype=np.float64).reshape(4, 3)
        self.speed = np.asarray(p.gait_counter_speed, dtype=np.float64).reshape(4)
        self.gc_init = np.asarray(p.gait_counter_init, dtype=np.float64).reshape(4)
        self.cpg, self.cps, self.control_dt = float(p.counter_per_gait), float(p.counter_per_swing), float(p.control_dt)
        self.force_low = float(p.foot_force_low)
        self.dx_lim, self.dy_lim = float(p.foot_delta_x_limit), float(p.foot_delta_y_limit)
        self.clr1, self.clr2 = float(p.swing_clearance1), float(p.swing_clearance2)
        self.terrain, self.adapt = bool(p.terrain), bool(p.use_terrain_adapt)
        self.counter = np.zeros(B, dtype=np.int64)
        self.gait_counter = np.broadcast_to(self.gc_init, (B, 4)).copy()  # reset() -> gait_counter_reset()
        self.early = np.zeros((B, 4), bool)
        self.foot_pos_start = np.zeros((B, 4, 3))
        self.rel_last = np.zeros((B, 4, 3))
        self.tgt_last = np.zeros((B, 4, 3))
        self.recent = np.zeros((B, 4, 3))
        self.contact_filter = MovingWindowFilter((B, 4, 3), 60)
        self.terrain_filter = MovingWindowFilter((B,), 100)

    def step(self, dt, root_lin_vel, root_lin_vel_d, root_rot_mat, root_pos, foot_pos_abs, root_euler_d,
             rot_z, foot_force, movement_mode):
        """One tick.  Arrays: root_* [B,3], root_rot_mat / rot_z [B,3,3], foot_pos_abs [B,4,3],
        foot_force [B,4], movement_mode [B].  Returns a dict of the reference's outputs (3-vectors as
        [B,4,3]); ``root_euler_d`` is the adapted copy."""
        B = self.B
        out = {}
        walk = np.broadcast_to(np.asarray(movement_mode) != 0, (B,))[:, None]
        # ---- update_plan :149-165
        self.counter = self.counter + 1
        stepped = np.fmod(self.gait_counter + self.speed, self.cpg)
        self.gait_counter = np.where(walk, stepped, self.gc_init)
        gc = self.gait_counter
        plan = np.where(walk, gc <= self.cps, True)
        # ---- Raibert :168-201
        v = [root_lin_vel[:, k, None] for k in range(3)]
        rel = _matT_vec(rot_z, v)  # [B,1] each
        vd = [root_lin_vel_d[:, k, None] for k in range(2)]
        kr = np.sqrt(np.abs(self.dfp[0, 2]) / 9.8)
        half_swing = ((self.cps / self.speed) * self.control_dt) / 2.0  # [4]
        dx = kr * (rel[0] - vd[0]) + half_swing * vd[0]
        dy = kr * (rel[1] - vd[1]) + half_swing * vd[1]
        dx = np.where(dx < -self.dx_lim, -self.dx_lim, dx)
        dx = np.where(dx > self.dx_lim, self.dx_lim, dx)
        dy = np.where(dy < -self.dy_lim, -self.dy_lim, dy)
        dy = np.where(dy > self.dy_lim, self.dy_lim, dy)
        trel = [self.dfp[:, 0] + dx, self.dfp[:, 1] + dy, np.broadcast_to(self.dfp[:, 2], (B, 4))]
        tabs = _mat_vec(root_rot_mat, trel)
        tworld = [tabs[k] + root_pos[:, k, None] for k in range(3)]
        # ---- generate_swing_legs_ctrl :223-253
        fabs = [foot_pos_abs[:, :, k] for k in range(3)]
        cur = _matT_vec(rot_z, fabs)
        stance = gc <= self.cps
        st32 = (gc - self.cps).astype(np.float32) / np.float32(self.cps)
        t = np.where(stance, np.float32(0.0), st32).astype(np.float32).astype(np.float64)
        tgt, fkin = [], []
        for k in range(3):
            self.foot_pos_start[:, :, k] = np.where(stance, cur[k], self.foot_pos_start[:, :, k])
            s, f = self.foot_pos_start[:, :, k], trel[k]
            P = [s, s, f, f, f]
            if k == 2:
                P[1] = P[1] + self.clr1
                P[2] = P[2] + self.clr2
            tgt.append(bezier_mul(t, P))
            vel_cur = (cur[k] - self.rel_last[:, :, k]) / dt
            vel_tgt = (tgt[k] - self.tgt_last[:, :, k]) / dt
            self.rel_last[:, :, k] = cur[k]
            self.tgt_last[:, :, k] = tgt[k]
            pos_err = tgt[k] - cur[k]
            vel_err = vel_tgt - vel_cur
            fkin.append(pos_err * self.kp[:, k] + vel_err * self.kd[:, k])
        # ---- contacts :259-282
        late = gc > self.cps * 1.5
        self.early = np.where(~late, False, self.early)
        self.early = np.where(~plan & late & (foot_force > self.force_low), True, self.early)
        contacts = plan | self.early
        avg = self.contact_filter.calculate_average(foot_pos_abs, contacts[:, :, None])
        self.recent = np.where(contacts[:, :, None], avg, self.recent)
        stack = lambda c: np.stack([np.broadcast_to(x, (B, 4)) for x in c], -1)
        out.update(foot_pos_target_rel=stack(trel), foot_pos_target_abs=stack(tabs),
                   foot_pos_target_world=stack(tworld),
                   foot_pos_cur=stack(cur), foot_pos_target=stack(tgt), foot_forces_kin=stack(fkin),
                   foot_pos_recent_contact=self.recent.copy(), gait_counter=gc.copy(),
                   plan_contacts=plan.astype(np.float64), early_contacts=self.early.astype(np.float64),
                   contacts=contacts.astype(np.float64), counter=self.counter.copy())
        # ---- compute_grf terrain adaptation :335-376
        euler_d = np.array(root_euler_d, dtype=np.float64, copy=True)
        a = np.zeros((B, 3))
        cos = np.zeros(B)
        angle = np.zeros(B)
        cond = np.zeros(B)
        if self.terrain:
            W = np.concatenate([np.ones((B, 4, 1)), self.recent[:, :, :2]], -1)  # :572-573
            z = self.recent[:, :, 2]
            WtW = np.matmul(W.transpose(0, 2, 1), W)
            a = np.matmul(np.matmul(np.linalg.pinv(WtW, rcond=3 * EPS), W.transpose(0, 2, 1)), z[:, :, None])[:, :, 0]
            with np.errstate(all="ignore"):
                cond = np.linalg.cond(WtW)
            n = np.stack([a[:, 1], a[:, 2], -np.ones(B)], -1)  # :580
            cos = np.abs(n[:, 2]) / (1.0 * np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]))
            raw = np.arccos(cos)
            high = root_pos[:, 2] > 0.1
            angle = np.where(high, self.terrain_filter.calculate_average(raw, high), 0.0)
            angle = np.clip(angle, -0.5, 0.5)
            f_r_diff = ((z[:, 0] + z[:, 1]) - z[:, 2]) - z[:, 3]
            if self.adapt:
                euler_d[:, 1] = np.where(f_r_diff > 0.05, -angle, angle)
            out.update(raw_angle=raw, f_r_diff=f_r_diff)
        out.update(plane=a, angle_cos=cos, terrain_pitch_angle=angle, cond=cond, root_euler_d=euler_d)
        return out
