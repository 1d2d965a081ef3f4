"""Numpy restatement of the reference's Go1 RL controller (src/go1_rl_ctrl_cpp), the parity checker of the
device policy stage (mpcqp_policy_device).  Nothing of the product imports it.

    observation      observation/Go1Observation.hpp:143-170 (scale factors :52-63, clipObs_ :449)
    network          torch_eigen/TorchEigen.cpp (a TorchScript MLP on the CPU, float32), run from
                     Go1RLController.cpp:95-99 on obs.cast<float>()
    action, targets  Go1RLController.cpp:99-109 (clipAction_, actionScale_: Go1RLController.hpp; pose limits :36-37;
                     default_joint_pos: Go1CtrlStates.hpp:75-78)
    servo stand      Go1RLController.cpp:121-146
    gains            :79-86 (walk), :125-132 (servo)
    motor law        tau = Kp (q_target - q) - Kd dq, what the motor controller does with the LowCmd send_cmd fills
                     (q = target, dq = 0, tau = 0, :149-166)
    mode             MainGazebo.cpp:74-83: movement_mode 0 = advance_servo, otherwise advance
    decimation       parameters.yaml:9-11 (action_update_frequency 4 ms, deployment_frequency 2 ms) and the two
                     threads of MainGazebo.cpp:55-134, restated as a per-robot tick counter (PolicyBlock.step)

Everything but the network is binary64 with unfused multiplies and adds, left to right, as numpy evaluates the
expressions below.  The history stacks of updateHistory (Go1Observation.hpp:172-181) are dead code in the
reference and are not built.
"""
import numpy as np

NUM_DOF = 12
OBS_DIM, PROPRIO_DIM = 48, 36
# Go1CtrlStates.hpp:75-78
DEFAULT_JOINT_POS = np.array([0.1, 0.8, -1.5, -0.1, 0.8, -1.5, 0.1, 1.0, -1.5, -0.1, 1.0, -1.5])
# Go1Observation.hpp:52-63: linVel 2, angVel 0.25, gravity 1, command (2, 2, 0.25), dofPos 1, dofVel 0.05
OBS_SCALE = np.array([2.0] * 3 + [0.25] * 3 + [1.0] * 3 + [2.0, 2.0, 0.25] + [1.0] * 12 + [0.05] * 12)
CLIP_OBS = 100.0       # Go1Observation.hpp:449
CLIP_ACTION = 100.0    # Go1RLController.hpp clipAction_
ACTION_SCALE = 0.25    # Go1RLController.hpp actionScale_
# Go1RLController.cpp:36-37
POSE_LOWER = np.array([-0.9425, -0.4817, -2.6285] * 4)
POSE_UPPER = np.array([0.9425, 2.7855, -0.9320] * 4)
# :79-86
KP_WALK = np.array([20.0, 50.0, 50.0] * 4)
KD_WALK = np.array([1.0, 2.0, 2.0] * 4)
# :122-132
STAND_POS = np.array([0.1, 0.6, -1.3, -0.1, 0.6, -1.3, 0.1, 0.6, -1.3, -0.1, 0.6, -1.3])
KP_SERVO = np.array([20.0, 30.0, 60.0] * 2 + [20.0, 80.0, 140.0] * 2)
KD_SERVO = np.array([5.0, 8.0, 12.0] * 4)
SERVO_TICKS = 1000.0   # :139
HIDDEN = (512, 256, 128)


def default_params(**over):
    p = dict(obs_scale=OBS_SCALE.copy(), clip_obs=CLIP_OBS, clip_action=CLIP_ACTION, action_scale=ACTION_SCALE,
             default_joint_pos=DEFAULT_JOINT_POS.copy(), pose_lower=POSE_LOWER.copy(), pose_upper=POSE_UPPER.copy(),
             kp_walk=KP_WALK.copy(), kd_walk=KD_WALK.copy(), kp_servo=KP_SERVO.copy(), kd_servo=KD_SERVO.copy(),
             stand_pos=STAND_POS.copy(), servo_ticks=SERVO_TICKS, servo_clamp=0, decimation=1)
    for k, v in over.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def _rt_v(rot, v):
    """rot^T v for row-major rot [B,9], v [B,3] (or [3]): entry i is (R0i v0 + R1i v1) + R2i v2."""
    r = np.asarray(rot, dtype=np.float64).reshape(-1, 3, 3)
    v = np.broadcast_to(np.asarray(v, dtype=np.float64), (r.shape[0], 3))
    return np.stack([(r[:, 0, i] * v[:, 0] + r[:, 1, i] * v[:, 1]) + r[:, 2, i] * v[:, 2] for i in range(3)], axis=1)


def observation(p, rot_z, lin_vel, imu_ang_vel, rot, joy, joint_pos, joint_vel, prev_action):
    """The 48-wide float32 observation (Go1Observation.hpp:152-166, Go1RLController.cpp:95-96).  rot_z, rot
    [B,9] row-major; joy [B,3] = joy_cmd_velx, joy_cmd_vely, joy_cmd_yaw_rate."""
    q = np.asarray(joint_pos, dtype=np.float64).reshape(-1, 12)
    B = q.shape[0]
    ob = np.empty((B, PROPRIO_DIM))
    ob[:, 0:3] = _rt_v(rot_z, lin_vel)                                   # :152
    ob[:, 3:6] = np.asarray(imu_ang_vel, dtype=np.float64).reshape(B, 3)   # :153
    ob[:, 6:9] = _rt_v(rot, np.array([0.0, 0.0, -1.0]))                  # :154
    ob[:, 9:12] = np.asarray(joy, dtype=np.float64).reshape(B, 3)          # :155
    ob[:, 12:24] = q - p["default_joint_pos"]                            # :156
    ob[:, 24:36] = np.asarray(joint_vel, dtype=np.float64).reshape(B, 12)  # :157
    ob = ob * p["obs_scale"]                                             # :161-163
    ob = np.maximum(np.minimum(ob, p["clip_obs"]), -p["clip_obs"])       # :166
    full = np.empty((B, OBS_DIM), dtype=np.float32)
    full[:, :36] = ob.astype(np.float32)                                 # Go1RLController.cpp:96
    full[:, 36:] = np.asarray(prev_action, dtype=np.float64).reshape(B, 12).astype(np.float32)
    return full


def mlp_f64(weights, biases, x):
    """y = W3 elu(W2 elu(W1 elu(W0 x + b0) + b1) + b2) + b3 in binary64 (expm1) on the float32 weights: the
    yardstick.  weights[l] is [out][in] as torch.nn.Linear; x [B, 48] float32."""
    h = np.asarray(x, dtype=np.float64)
    n = len(weights)
    for l, (W, b) in enumerate(zip(weights, biases)):
        h = h @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        if l + 1 < n:
            h = np.where(h > 0.0, h, np.expm1(np.minimum(h, 0.0)))
    return h


def mlp_f64_layers(weights, biases, x):
    """Pre-activations of every layer, binary64 (for the exactness conditions of the integer test)."""
    h = np.asarray(x, dtype=np.float64)
    pre = []
    n = len(weights)
    for l, (W, b) in enumerate(zip(weights, biases)):
        h = h @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        pre.append(h)
        if l + 1 < n:
            h = np.where(h > 0.0, h, np.expm1(np.minimum(h, 0.0)))
    return pre


def mlp_torch(weights, biases, x):
    """The same network as torch evaluates it on the CPU in float32 (linear / elu): the reference's arithmetic,
    since TorchEigen::run runs the TorchScript module on the CPU."""
    import torch
    import torch.nn.functional as F
    h = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    n = len(weights)
    with torch.no_grad():
        for l, (W, b) in enumerate(zip(weights, biases)):
            h = F.linear(h, torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)),
                         torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)))
            if l + 1 < n:
                h = F.elu(h)
    return h.numpy()


def seeded_weights(seed, hidden=HIDDEN, gain=1.0):
    """float32 weights and biases, uniform +-gain / sqrt(fan_in) (torch.nn.Linear's default range)."""
    rng = np.random.default_rng(seed)
    dims = [OBS_DIM] + list(hidden) + [NUM_DOF]
    ws, bs = [], []
    for i, o in zip(dims[:-1], dims[1:]):
        a = gain / np.sqrt(i)
        ws.append(rng.uniform(-a, a, (o, i)).astype(np.float32))
        bs.append(rng.uniform(-a, a, (o,)).astype(np.float32))
    return ws, bs


def action_to_targets(p, raw):
    """Go1RLController.cpp:99-109: raw [B,12] network output -> (clipped action = prev_action, target poses)."""
    a = np.asarray(raw, dtype=np.float64)                                  # :99
    a = np.maximum(np.minimum(a, p["clip_action"]), -p["clip_action"])     # :102
    scaled = a * p["action_scale"]                                         # :106
    target = scaled + p["default_joint_pos"]                               # :107
    target = np.maximum(np.minimum(target, p["pose_upper"]), p["pose_lower"])  # :109
    return a, target


def servo_targets(p, servo_motion_time, joint_pos):
    """Go1RLController.cpp:136-142 for counters that :136 has already advanced.  The reference never clamps
    percent and never resets the counter; servo_clamp != 0 clamps percent to 1."""
    percent = np.asarray(servo_motion_time, dtype=np.float64) / p["servo_ticks"]   # :139
    if p["servo_clamp"]:
        percent = np.minimum(percent, 1.0)
    q = np.asarray(joint_pos, dtype=np.float64)
    pc = percent[..., None]
    return q * (1.0 - pc) + p["stand_pos"] * pc                            # :141


def gains(p, walk):
    """(Kp, Kd) [B,12] for the mode that ran: walk :79-86, servo :125-132."""
    w = np.asarray(walk, dtype=bool)[:, None]
    return np.where(w, p["kp_walk"], p["kp_servo"]), np.where(w, p["kd_walk"], p["kd_servo"])


def torque(kp, kd, target, joint_pos, joint_vel):
    """The motor law on the LowCmd of send_cmd (:155-163): Kp (q_target - q) + Kd (0 - dq) + 0."""
    return kp * (target - joint_pos) - kd * joint_vel


class PolicyBlock:
    """The members Go1RLController keeps between ticks, per robot, and the decimation schedule.

    A tick counter c starts at 0.  On a tick with c % decimation == 0 the robot runs advance (movement_mode
    1.0) or advance_servo (anything else) and stores the targets and the mode it ran; on every tick the
    torque comes from the stored targets, the stored mode's gains and this tick's q and dq; then c += 1."""

    def __init__(self, B, params=None):
        self.p = params if params is not None else default_params()
        self.B = B
        self.init = np.zeros(B)
        self.tick = np.zeros(B)
        self.servo_motion_time = np.zeros(B)      # Go1RLController.cpp:50
        self.mode = np.zeros(B)                   # the mode the last update ran, 0.0 / 1.0
        self.prev_action = np.zeros((B, 12))      # prevActionDouble_ (:34)
        self.target = np.zeros((B, 12))           # targetPoses_ (:35)

    def due(self):
        return np.fmod(self.tick, float(self.p["decimation"])) == 0.0

    def slot_rows(self):
        """[B, 28] as the device slot (include/mpcqp.h MPCQP_PS_*)."""
        return np.concatenate([self.init[:, None], self.tick[:, None], self.servo_motion_time[:, None],
                               self.mode[:, None], self.prev_action, self.target], axis=1)

    def step(self, movement_mode, joint_pos, joint_vel, raw, run=None):
        """One tick.  raw [B,12]: the network output for this tick's observation (used only by robots that
        update in walk mode).  run [B] bool: robots left out keep every member (not selected, or a
        non-finite input).  Returns raw as reported (0 unless the robot ran the network), the action, the
        targets, the torques, and the update flag."""
        p, B = self.p, self.B
        run = np.ones(B, bool) if run is None else np.asarray(run, bool)
        q = np.asarray(joint_pos, dtype=np.float64).reshape(B, 12)
        dq = np.asarray(joint_vel, dtype=np.float64).reshape(B, 12)
        upd = self.due() & run
        walk = np.asarray(movement_mode, dtype=np.float64) == 1.0
        uw, us = upd & walk, upd & ~walk
        act, tgt = action_to_targets(p, raw)
        self.prev_action[uw] = act[uw]
        self.target[uw] = tgt[uw]
        self.servo_motion_time[us] += 1.0                                   # :136
        self.target[us] = servo_targets(p, self.servo_motion_time, q)[us]
        self.mode[upd] = walk[upd].astype(np.float64)
        kp, kd = gains(p, self.mode == 1.0)
        tau = torque(kp, kd, self.target, q, dq)
        self.tick[run] += 1.0
        self.init[run] = 1.0
        raw_out = np.where(uw[:, None], np.asarray(raw, dtype=np.float64), 0.0)
        return dict(raw=raw_out, action=self.prev_action.copy(), target=self.target.copy(), tau=tau, updated=upd)
