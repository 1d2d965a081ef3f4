"""Numpy restatement of the joystick command block at the top of main_update
(src/a1_cpp/src/GazeboA1ROS.cpp:122-188; HardwareA1ROS.cpp:104-158 is the same block), batched over robots.

It states the reference, statement by statement and in its order, in binary64 with every product rounded
before it is added (numpy never contracts), so the device stage can be compared bitwise.  The members the
block keeps between ticks are attributes; ``root_euler_d`` and ``root_pos_d`` are a1_ctrl_states fields that
other code also writes (the terrain adaptation, A1RobotControl.cpp:376), so they are passed in and out.
"""
import numpy as np

# GazeboA1ROS.h:133, A1Params.h:16-17, GazeboA1ROS.cpp:180, Go1CtrlStates.hpp:279-281 and :304-305
DEFAULTS = dict(body_height_init=0.2, body_height_max=0.32, body_height_min=0.1, vel_lock_threshold=0.05,
                kp_linear=(100.0, 100.0, 300.0), kp_linear_lock_x=100.0, kp_linear_lock_y=100.0)


class CommandBlock:
    def __init__(self, B, **over):
        p = dict(DEFAULTS, **over)
        self.p = p
        self.body_height = np.full(B, p["body_height_init"])        # joy_cmd_body_height
        self.ctrl_state = np.zeros(B, dtype=np.int64)                # joy_cmd_ctrl_state
        self.prev_ctrl_state = np.zeros(B, dtype=np.int64)           # prev_joy_cmd_ctrl_state
        self.kp_linear = np.tile(np.asarray(p["kp_linear"], dtype=np.float64), (B, 1))

    def step(self, dt, vel, rate, request, root_pos, root_euler_d, root_pos_d):
        """One tick.  vel [B,3] joy_cmd_velx/y/z, rate [B,3] roll/pitch/yaw rate, request [B] bool,
        root_pos [B,3] as the previous tick's estimator left it.  Returns a dict of the a1_ctrl_states fields
        after the block (new arrays) and the request flags after it (all False, :146)."""
        p = self.p
        vel, rate = np.asarray(vel, dtype=np.float64), np.asarray(rate, dtype=np.float64)
        request = np.asarray(request, dtype=bool)
        euler_d, pos_d = np.array(root_euler_d, dtype=np.float64), np.array(root_pos_d, dtype=np.float64)
        # :124-130
        h = self.body_height + vel[:, 2] * dt
        h = np.where(h >= p["body_height_max"], p["body_height_max"], h)
        h = np.where(h <= p["body_height_min"], p["body_height_min"], h)
        self.body_height = h
        # :140-147
        self.prev_ctrl_state = self.ctrl_state.copy()
        self.ctrl_state = np.where(request, (self.ctrl_state + 1) % 2, self.ctrl_state)
        # :150-157
        lin_vel_d, ang_vel_d = vel.copy(), rate.copy()
        # :158-161
        for k in range(3):
            euler_d[:, k] = euler_d[:, k] + rate[:, k] * dt
        pos_d[:, 2] = h
        # :164-176
        walk = self.ctrl_state == 1
        leave = (self.ctrl_state == 0) & (self.prev_ctrl_state == 1)
        movement_mode = walk.astype(np.int64)
        pos_d[leave, 0:2] = root_pos[leave, 0:2]
        self.kp_linear[leave, 0] = p["kp_linear_lock_x"]
        self.kp_linear[leave, 1] = p["kp_linear_lock_y"]
        # :179-188 (Eigen's norm of a 2-vector: sqrt(x*x + y*y))
        moving = np.sqrt(vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1]) > p["vel_lock_threshold"]
        free, lock = walk & moving, walk & ~moving
        pos_d[free, 0:2] = root_pos[free, 0:2]
        self.kp_linear[free, 0:2] = 0.0
        self.kp_linear[lock, 0] = p["kp_linear_lock_x"]
        self.kp_linear[lock, 1] = p["kp_linear_lock_y"]
        return dict(root_lin_vel_d=lin_vel_d, root_ang_vel_d=ang_vel_d, root_euler_d=euler_d, root_pos_d=pos_d,
                    movement_mode=movement_mode, kp_linear=self.kp_linear.copy(), body_height=h.copy(),
                    ctrl_state=self.ctrl_state.copy(), prev_ctrl_state=self.prev_ctrl_state.copy(),
                    request=np.zeros_like(request))
