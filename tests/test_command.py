"""The numpy restatement of the command block (tests/command_reference.py) on a hand-written script, against
literal expected values worked out from GazeboA1ROS.cpp:122-188 by hand; pack_commands and the slot view."""
import numpy as np

from mpcqp import _lib
from mpcqp.command import CMD_STATE_DTYPE, pack_commands

import command_reference as ref

DT = 0.5  # a coarse step, so every literal below is a short decimal


def _tick(blk, vel, rate, request, root_pos, euler_d, pos_d):
    out = blk.step(DT, np.array([vel], dtype=np.float64), np.array([rate], dtype=np.float64), np.array([request]),
                   np.array([root_pos], dtype=np.float64), euler_d, pos_d)
    return out, out["root_euler_d"], out["root_pos_d"]


def test_height_reaches_both_clamps():
    blk = ref.CommandBlock(1)
    e, p = np.zeros((1, 3)), np.zeros((1, 3))
    # 0.2 + 0.125 * 0.5 = 0.2625, + 0.0625 = 0.325 -> clamped to 0.32
    o, e, p = _tick(blk, [0, 0, 0.125], [0, 0, 0], False, [0, 0, 0], e, p)
    assert o["body_height"][0] == 0.2625 and p[0, 2] == 0.2625
    o, e, p = _tick(blk, [0, 0, 0.125], [0, 0, 0], False, [0, 0, 0], e, p)
    assert o["body_height"][0] == 0.32 and p[0, 2] == 0.32
    # 0.32 - 0.5 * 0.5 = 0.07 -> clamped to 0.1
    o, e, p = _tick(blk, [0, 0, -0.5], [0, 0, 0], False, [0, 0, 0], e, p)
    assert o["body_height"][0] == 0.1 and p[0, 2] == 0.1
    assert np.array_equal(o["root_lin_vel_d"][0], [0.0, 0.0, -0.5])


def test_toggle_lock_and_threshold():
    blk = ref.CommandBlock(1)
    e, p = np.array([[0.0, 0.25, 1.0]]), np.array([[7.0, 8.0, 9.0]])
    # tick 1, standing: nothing locks, root_pos_d[0:2] stays, euler_d integrates, kp_linear is the parameter
    o, e, p = _tick(blk, [0.0, 0.0, 0.0], [0.5, -0.5, 1.0], False, [1.0, 2.0, 0.3], e, p)
    assert o["movement_mode"][0] == 0 and (o["ctrl_state"][0], o["prev_ctrl_state"][0]) == (0, 0)
    assert np.array_equal(e[0], [0.25, 0.0, 1.5]) and np.array_equal(p[0], [7.0, 8.0, 0.2])
    assert np.array_equal(o["kp_linear"][0], [100.0, 100.0, 300.0])
    assert np.array_equal(o["root_ang_vel_d"][0], [0.5, -0.5, 1.0])
    # tick 2, request: walking, planar speed 0.5 > 0.05: position target follows root_pos, kp_linear[0:2] = 0
    o, e, p = _tick(blk, [0.3, 0.4, 0.0], [0, 0, 0], True, [1.5, 2.5, 0.3], e, p)
    assert o["movement_mode"][0] == 1 and (o["ctrl_state"][0], o["prev_ctrl_state"][0]) == (1, 0)
    assert not o["request"][0]
    assert np.array_equal(p[0], [1.5, 2.5, 0.2]) and np.array_equal(o["kp_linear"][0], [0.0, 0.0, 300.0])
    # tick 3, walking, speed 0.04 < 0.05: the lock values come back and the target stays where it was
    o, e, p = _tick(blk, [0.04, 0.0, 0.0], [0, 0, 0], False, [2.0, 3.0, 0.3], e, p)
    assert o["movement_mode"][0] == 1
    assert np.array_equal(p[0], [1.5, 2.5, 0.2]) and np.array_equal(o["kp_linear"][0], [100.0, 100.0, 300.0])
    # tick 4, walking and fast again, then tick 5 the request out of walking: the one-tick lock of :167-173
    o, e, p = _tick(blk, [0.0, -0.06, 0.0], [0, 0, 0], False, [2.5, 3.5, 0.3], e, p)
    assert np.array_equal(p[0], [2.5, 3.5, 0.2]) and np.array_equal(o["kp_linear"][0], [0.0, 0.0, 300.0])
    o, e, p = _tick(blk, [0.3, 0.4, 0.0], [0, 0, 0], True, [3.0, 4.0, 0.3], e, p)
    assert o["movement_mode"][0] == 0 and (o["ctrl_state"][0], o["prev_ctrl_state"][0]) == (0, 1)
    assert np.array_equal(p[0], [3.0, 4.0, 0.2]) and np.array_equal(o["kp_linear"][0], [100.0, 100.0, 300.0])
    # tick 6, standing: the lock happened for one instance only; speed is not looked at outside walking
    o, e, p = _tick(blk, [0.3, 0.4, 0.0], [0, 0, 0], False, [9.0, 9.0, 0.3], e, p)
    assert o["movement_mode"][0] == 0 and (o["ctrl_state"][0], o["prev_ctrl_state"][0]) == (0, 0)
    assert np.array_equal(p[0], [3.0, 4.0, 0.2]) and np.array_equal(o["kp_linear"][0], [100.0, 100.0, 300.0])
    assert np.array_equal(e[0], [0.25, 0.0, 1.5])


def test_rounded_norm_decides():
    """(0.03, 0.04): 0.03^2 + 0.04^2 rounds to 0.0025000000000000005, whose square root rounds to exactly the
    binary64 0.05, so `> 0.05` is false and the position stays locked; (0.04, 0.03) is the same sum."""
    blk = ref.CommandBlock(2)
    blk.ctrl_state[:] = 1
    vel = np.array([[0.03, 0.04, 0.0], [0.04, 0.03, 0.0]])
    assert np.all(np.sqrt(vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1]) == 0.05)
    o = blk.step(DT, vel, np.zeros((2, 3)), np.zeros(2, bool), np.ones((2, 3)), np.zeros((2, 3)), np.zeros((2, 3)))
    assert np.array_equal(o["kp_linear"][:, :2], np.full((2, 2), 100.0))
    assert np.array_equal(o["root_pos_d"][:, :2], np.zeros((2, 2)))


def test_two_consecutive_requests_toggle_twice():
    blk = ref.CommandBlock(1)
    z = np.zeros((1, 3))
    o = blk.step(DT, z, z, np.array([True]), z, z, z)
    assert o["movement_mode"][0] == 1
    o = blk.step(DT, z, z, np.array([True]), z, z, z)
    assert o["movement_mode"][0] == 0 and o["prev_ctrl_state"][0] == 1


def test_pack_commands_and_slot_view():
    rows = pack_commands([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]], [0, 5])
    assert rows.shape == (2, _lib.CM_SIZE) and rows.dtype == np.float64
    assert np.array_equal(rows[:, _lib.CM_VEL:_lib.CM_VEL + 3], [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    assert np.array_equal(rows[:, _lib.CM_RATE:_lib.CM_RATE + 3], [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]])
    assert np.array_equal(rows[:, _lib.CM_MODE_REQUEST], [0.0, 1.0]) and np.all(rows[:, 7] == 0.0)
    assert np.array_equal(pack_commands(np.zeros((3, 3)), np.zeros((3, 3)), 1)[:, _lib.CM_MODE_REQUEST], np.ones(3))
    slot = np.arange(2 * _lib.CS_SIZE, dtype=np.float64).reshape(2, _lib.CS_SIZE)
    v = slot.view(CMD_STATE_DTYPE).reshape(2)
    assert np.array_equal(v["init"], slot[:, _lib.CS_INIT])
    assert np.array_equal(v["body_height"], slot[:, _lib.CS_BODY_HEIGHT])
    assert np.array_equal(v["ctrl_state"], slot[:, _lib.CS_CTRL_STATE])
    assert np.array_equal(v["prev_ctrl_state"], slot[:, _lib.CS_PREV_CTRL_STATE])
    assert np.array_equal(v["kp_linear"], slot[:, _lib.CS_KP_LINEAR:_lib.CS_KP_LINEAR + 3])
    v["kp_linear"][1] = [9.0, 8.0, 7.0]
    assert np.array_equal(slot[1, 4:7], [9.0, 8.0, 7.0])  # a view, and back
