"""tests/policy_reference.py (the numpy restatement of src/go1_rl_ctrl_cpp's controller) against literals worked
by hand from the cited lines, its decimation schedule, its two network evaluations against each other, and the
weight loader of mpcqp.policy.  No GPU."""
import os

import numpy as np
import pytest

import policy_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a checkout of the reference project beside this repository (or MPCQP_REFERENCE_DIR); absent = that test skips
REFERENCE_MODEL = os.path.join(os.environ.get("MPCQP_REFERENCE_DIR") or os.path.join(os.path.dirname(REPO), "reference"),
                               "src", "go1_rl_ctrl_cpp", "resource", "cpp_model.pt")
IDENT = np.eye(3).reshape(1, 9)


def test_constants():
    p = ref.default_params()
    # Go1Observation.hpp:52-63
    assert p["obs_scale"].tolist() == [2, 2, 2, .25, .25, .25, 1, 1, 1, 2, 2, .25] + [1] * 12 + [.05] * 12
    # Go1CtrlStates.hpp:75-78
    assert p["default_joint_pos"].tolist() == [.1, .8, -1.5, -.1, .8, -1.5, .1, 1., -1.5, -.1, 1., -1.5]
    # Go1RLController.cpp:36-37, :79-86, :122-132
    assert p["pose_lower"][:3].tolist() == [-0.9425, -0.4817, -2.6285] and p["pose_upper"][9:].tolist() == [0.9425, 2.7855, -0.9320]
    assert p["kp_walk"][3:6].tolist() == [20, 50, 50] and p["kd_walk"][:3].tolist() == [1, 2, 2]
    assert p["kp_servo"].tolist() == [20, 30, 60, 20, 30, 60, 20, 80, 140, 20, 80, 140]
    assert p["kd_servo"][6:9].tolist() == [5, 8, 12]
    assert p["stand_pos"].tolist() == [.1, .6, -1.3, -.1, .6, -1.3, .1, .6, -1.3, -.1, .6, -1.3]
    assert (p["clip_obs"], p["clip_action"], p["action_scale"], p["servo_ticks"]) == (100.0, 100.0, 0.25, 1000.0)
    assert (p["servo_clamp"], p["decimation"]) == (0, 1)


def test_observation_scales_and_frames():
    p = ref.default_params()
    # yaw by 90 degrees: root_rot_mat_z = [[0,-1,0],[1,0,0],[0,0,1]]; R^T v for v = (1, 2, 3) is (2, -1, 3)
    rz = np.array([[0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
    # root_rot_mat with third row (0.6, 0, 0.8): R^T (0,0,-1) = minus the third row
    rot = np.array([[0.8, 0.0, -0.6, 0.0, 1.0, 0.0, 0.6, 0.0, 0.8]])
    q = p["default_joint_pos"] + np.arange(12) * 0.125
    dq = np.arange(12) * 2.0
    prev = np.arange(12) * 0.5 - 1.0
    ob = ref.observation(p, rz, [[1.0, 2.0, 3.0]], [[4.0, -8.0, 12.0]], rot, [[0.5, -0.25, 2.0]], q, dq, prev)
    assert ob.dtype == np.float32 and ob.shape == (1, 48)
    assert ob[0, 0:3].tolist() == [4.0, -2.0, 6.0]        # x 2
    assert ob[0, 3:6].tolist() == [1.0, -2.0, 3.0]        # x 0.25
    assert ob[0, 6:9].tolist() == [np.float32(-0.6), 0.0, np.float32(-0.8)]
    assert ob[0, 9:12].tolist() == [1.0, -0.5, 0.5]       # x (2, 2, 0.25)
    assert np.array_equal(ob[0, 12:24], ((p["default_joint_pos"] + np.arange(12) * 0.125) - p["default_joint_pos"]).astype(np.float32))
    assert np.allclose(ob[0, 12:24], np.arange(12) * 0.125, atol=1e-7)
    assert np.array_equal(ob[0, 24:36], (np.arange(12) * 2.0 * 0.05).astype(np.float32))
    assert ob[0, 36:48].tolist() == (np.arange(12) * 0.5 - 1.0).tolist()


def test_observation_clip_both_sides():
    p = ref.default_params()
    dq = np.zeros(12)
    dq[0], dq[1], dq[2] = 2000.0, -2000.1, 1999.0   # x 0.05: 100 (reached exactly), -100.005 -> -100, 99.95
    ob = ref.observation(p, IDENT, [[60.0, -50.0, 49.0]], [[500.0, 0.0, -400.0]], IDENT, np.zeros((1, 3)),
                         p["default_joint_pos"], dq, np.full(12, 250.0))
    assert ob[0, 0:3].tolist() == [100.0, -100.0, 98.0]
    assert ob[0, 3:6].tolist() == [100.0, 0.0, -100.0]
    assert ob[0, 24:27].tolist() == [100.0, -100.0, np.float32(1999.0 * 0.05)]
    assert ob[0, 36] == 250.0   # the previous action is appended after the clip (Go1RLController.cpp:96)


def test_action_clip_and_pose_limits():
    p = ref.default_params()
    raw = np.zeros((1, 12))
    raw[0, 0] = 150.0     # clip 100 -> 25 + 0.1 -> upper limit 0.9425
    raw[0, 1] = -150.0    # clip -100 -> -25 + 0.8 -> lower limit -0.4817
    raw[0, 2] = 1.0       # 0.25 - 1.5 = -1.25, inside
    raw[0, 3] = 4.0       # 1.0 - 0.1 = 0.9, inside
    raw[0, 4] = 8.0       # 2.0 + 0.8 = 2.8 -> 2.7855
    raw[0, 5] = -5.0      # -1.25 - 1.5 = -2.75 -> -2.6285
    raw[0, 8] = 3.0       # 0.75 - 1.5 = -0.75 -> -0.932
    act, tgt = ref.action_to_targets(p, raw)
    assert act[0, :6].tolist() == [100.0, -100.0, 1.0, 4.0, 8.0, -5.0]
    assert tgt[0, :6].tolist() == [0.9425, -0.4817, -1.25, 1.0 + -0.1, 2.7855, -2.6285]
    assert tgt[0, 8] == -0.932 and tgt[0, 6] == 0.1 and tgt[0, 7] == 1.0


@pytest.mark.parametrize("clamp", [0, 1])
def test_servo_interpolation(clamp):
    p = ref.default_params(servo_clamp=clamp)
    q = np.full((1, 12), 0.5)
    blk = ref.PolicyBlock(1, p)
    seen = {}
    for t in range(1, 1501):
        o = blk.step([0.0], q, np.zeros((1, 12)), np.zeros((1, 12)))
        if t in (1, 1000, 1500):
            seen[t] = o
    assert blk.servo_motion_time[0] == 1500.0 and blk.tick[0] == 1500.0
    # tick 1: percent = 0.001 (:139-141)
    assert seen[1]["target"][0, 1] == 0.5 * (1 - 0.001) + 0.6 * 0.001
    assert seen[1]["target"][0, 3] == 0.5 * (1 - 0.001) + -0.1 * 0.001
    # tick 1000: percent = 1: the stand pose itself
    assert seen[1000]["target"][0].tolist() == (0.5 * 0.0 + p["stand_pos"] * 1.0).tolist()
    # tick 1500: the reference extrapolates (percent = 1.5); servo_clamp holds the stand pose
    want = p["stand_pos"] if clamp else 0.5 * (1 - 1.5) + p["stand_pos"] * 1.5
    assert seen[1500]["target"][0].tolist() == want.tolist()
    # the servo gains, front and rear (:125-132): tau = Kp (target - q) - Kd dq
    tau = blk.step([0.0], q, np.full((1, 12), 2.0), np.zeros((1, 12)))["tau"]
    assert tau[0, 2] == 60.0 * (blk.target[0, 2] - 0.5) - 12.0 * 2.0
    assert tau[0, 7] == 80.0 * (blk.target[0, 7] - 0.5) - 8.0 * 2.0
    assert not blk.prev_action.any()   # advance_servo leaves prevActionDouble_ alone


def test_walk_torque_and_prev_action():
    p = ref.default_params()
    blk = ref.PolicyBlock(2, p)
    raw = np.tile(np.arange(12) * 0.1, (2, 1))
    q = np.tile(p["default_joint_pos"], (2, 1))
    dq = np.ones((2, 12))
    o = blk.step([1.0, 0.0], q, dq, raw)
    assert o["updated"].tolist() == [True, True] and blk.mode.tolist() == [1.0, 0.0]
    # walk: target = 0.25 raw + default, Kp (20, 50, 50), Kd (1, 2, 2)
    assert o["tau"][0, 4] == 50.0 * ((0.4 * 0.25 + 0.8) - 0.8) - 2.0 * 1.0
    assert o["tau"][0, 3] == 20.0 * ((np.float64(0.1 * 3) * 0.25 + -0.1) - -0.1) - 1.0
    assert np.array_equal(blk.prev_action[0], raw[0]) and not blk.prev_action[1].any()
    assert np.array_equal(o["raw"][0], raw[0]) and not o["raw"][1].any()
    # a robot that is left out keeps everything
    before = blk.slot_rows().copy()
    blk.step([1.0, 1.0], q, dq, raw + 1.0, run=[False, True])
    after = blk.slot_rows()
    assert np.array_equal(before[0], after[0]) and not np.array_equal(before[1], after[1])


def test_decimation_schedule():
    p = ref.default_params(decimation=4)
    blk = ref.PolicyBlock(1, p)
    q = np.tile(p["default_joint_pos"], (1, 1))
    flags, targets, taus = [], [], []
    for t in range(10):
        raw = np.full((1, 12), 0.1 * (t + 1))
        o = blk.step([1.0], q + 0.01 * t, np.zeros((1, 12)), raw)
        flags.append(bool(o["updated"][0]))
        targets.append(o["target"][0, 1])
        taus.append(o["tau"][0, 1])
    assert flags == [True, False, False, False, True, False, False, False, True, False]
    t0, t4, t8 = 0.1 * 0.25 + 0.8, 0.5 * 0.25 + 0.8, 0.9 * 0.25 + 0.8
    assert targets == [t0] * 4 + [t4] * 4 + [t8] * 2
    assert len(set(taus)) == 10   # the torque follows this tick's q on every tick
    assert blk.tick[0] == 10.0
    # the mode is sampled on update ticks only: a switch to stand at tick 1 takes effect at tick 4
    blk = ref.PolicyBlock(1, p)
    modes = []
    for t in range(6):
        blk.step([1.0 if t == 0 else 0.0], q, np.zeros((1, 12)), np.zeros((1, 12)))
        modes.append(blk.mode[0])
    assert modes == [1.0, 1.0, 1.0, 1.0, 0.0, 0.0] and blk.servo_motion_time[0] == 1.0


def test_network_evaluations_agree():
    ws, bs = ref.seeded_weights(3)
    x = np.random.default_rng(4).normal(0.0, 1.0, (67, 48)).astype(np.float32)
    y64 = ref.mlp_f64(ws, bs, x)
    y32 = ref.mlp_torch(ws, bs, x)
    assert y32.dtype == np.float32 and y64.shape == y32.shape == (67, 12)
    err = np.max(np.abs(y32 - y64))
    assert 0.0 < err < 2e-6 * max(1.0, np.max(np.abs(y64)))   # float32 round-off over 4 layers, not a layout error
    # ELU's negative side is exercised
    pre = ref.mlp_f64_layers(ws, bs, x)
    assert (pre[0] < 0).any() and (pre[0] > 0).any()
    # a hand-sized network: 48 -> 32 -> 12 with one active input
    w0 = np.zeros((32, 48), np.float32); w0[0, 0], w0[1, 0] = 2.0, -1.0
    w1 = np.zeros((12, 32), np.float32); w1[0, 0], w1[0, 1] = 1.0, 1.0
    b0, b1 = np.zeros(32, np.float32), np.full(12, 0.5, np.float32)
    x1 = np.zeros((1, 48), np.float32); x1[0, 0] = 1.5
    assert ref.mlp_f64([w0, w1], [b0, b1], x1)[0, 0] == 3.0 + np.expm1(-1.5) + 0.5
    assert ref.mlp_f64([w0, w1], [b0, b1], x1)[0, 1] == 0.5


def test_load_policy_weights_npz_roundtrip(tmp_path):
    from mpcqp.policy import load_policy_weights
    ws, bs = ref.seeded_weights(11, hidden=(64, 32))
    path = tmp_path / "policy.npz"
    np.savez(path, **{f"w{l}": w for l, w in enumerate(ws)}, **{f"b{l}": b for l, b in enumerate(bs)})
    got_w, got_b = load_policy_weights(path)
    assert [w.shape for w in got_w] == [(64, 48), (32, 64), (12, 32)]
    assert all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(got_w, ws))
    assert all(np.array_equal(a, b) for a, b in zip(got_b, bs))
    # state_dict style names
    path2 = tmp_path / "sd.npz"
    np.savez(path2, **{f"actor.{2 * l}.weight": w for l, w in enumerate(ws)},
             **{f"actor.{2 * l}.bias": b for l, b in enumerate(bs)})
    got_w2, got_b2 = load_policy_weights(path2)
    assert all(np.array_equal(a, b) for a, b in zip(got_w2 + got_b2, ws + bs))


@pytest.mark.skipif(not os.path.exists(REFERENCE_MODEL), reason="the reference tree is not present")
def test_load_policy_weights_reads_the_reference_model():
    from mpcqp.policy import load_policy_weights
    ws, bs = load_policy_weights(REFERENCE_MODEL)
    assert [w.shape for w in ws] == [(512, 48), (256, 512), (128, 256), (12, 128)]
    assert [b.shape for b in bs] == [(512,), (256,), (128,), (12,)]
    assert all(w.dtype == np.float32 for w in ws + bs)
