"""mpcqp_command_device on the GPU against the numpy restatement of GazeboA1ROS.cpp:122-188
(tests/command_reference.py), bitwise, over 40 ticks of a scripted command sequence per robot: every field the
stage writes, the whole slot, the consumed request, and that no other double of the rows moves."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib

import command_reference as ref

pytestmark = pytest.mark.gpu

DT = 0.0005
T = 40
PAD = 3  # rows past the batch, NaN-filled: the stage must not touch them
# planar speeds on both sides of the 0.05 threshold; (0.03, 0.04) and (0.04, 0.03) round to exactly 0.05
PLANAR = [(0.0, 0.0), (0.03, 0.04), (0.2, 0.1), (0.04, 0.03), (0.049, 0.0), (0.051, 0.0), (0.05, 0.0), (-0.3, 0.4),
          (0.0, -0.0501), (0.03, -0.03)]
REQUEST_TICKS = (3, 4, 12, 20, 27, 28, 29, 35)  # two and three consecutive ones among them
NAN_TICK = 17


def _script(B, seed):
    rng = np.random.default_rng(seed)
    t, b = np.arange(T)[:, None], np.arange(B)[None, :]
    vel = np.zeros((T, B, 3))
    pl = np.array(PLANAR)[(t + b) % len(PLANAR)]
    vel[:, :, 0:2] = pl
    # +0.02 m per tick for ten ticks (0.2 -> the 0.32 clamp), then -0.02 for sixteen (-> the 0.1 clamp), then small
    vz = np.where(t < 10, 40.0, np.where(t < 26, -40.0, 0.0)) * (1.0 + 0.1 * (b % 5))
    vel[:, :, 2] = vz + np.where(t >= 26, rng.normal(0.0, 0.3, (T, B)), 0.0)
    rate = rng.normal(0.0, 0.5, (T, B, 3))
    request = np.isin((t + (b % 4)) % T, REQUEST_TICKS)
    pos = rng.normal(0.0, 2.0, (T, B, 3))  # root_pos as the estimator leaves it, another one every tick
    return vel, rate, request, pos


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("B", [1, 67])
def test_command_stage_bitwise(B):
    vel, rate, request, pos = _script(B, seed=5 + B)
    nb = B // 2  # the robot whose command row is NaN on NAN_TICK
    cmd_rows = np.stack([mpcqp.pack_commands(vel[t], rate[t], request[t]) for t in range(T)])
    cmd_rows[NAN_TICK, nb, _lib.CM_VEL + 1] = np.nan
    rng = np.random.default_rng(77)
    nan = float("nan")

    def sentinel(width):  # distinct finite sentinels in the batch's rows, NaN past them
        a = np.full((B + PAD, width), nan)
        a[:B] = 1000.0 + rng.permutation(B * width).reshape(B, width)
        return a

    st0, pin0, cmd0 = sentinel(_lib.ST_SIZE), sentinel(_lib.PL_SIZE), sentinel(_lib.CM_SIZE)
    slot0 = np.full((B + PAD, mpcqp.command_state_size()), nan)
    slot0[:B] = 0.0
    cp = mpcqp.default_command_params()
    d_st, d_pin, d_cmd, d_slot = (torch.from_numpy(a.copy()).cuda() for a in (st0, pin0, cmd0, slot0))
    d_rows, d_pos = torch.from_numpy(cmd_rows).cuda(), torch.from_numpy(pos).cuda()
    hist = [torch.empty((T,) + tuple(d.shape), dtype=torch.float64, device="cuda") for d in (d_st, d_pin, d_cmd, d_slot)]
    after_write = torch.empty((T,) + tuple(d_cmd.shape), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for t in range(T):
        d_cmd[:B, :7] = d_rows[t][:, :7]  # the caller's write; the padding double keeps its sentinel
        d_st[:B, _lib.ST_POS:_lib.ST_POS + 3] = d_pos[t]
        after_write[t].copy_(d_cmd)
        mpcqp.command_device(cp, DT, d_cmd.data_ptr(), d_st.data_ptr(), d_pin.data_ptr(), B, d_slot.data_ptr(), s)
        for h, d in zip(hist, (d_st, d_pin, d_cmd, d_slot)):
            h[t].copy_(d)
    torch.cuda.synchronize()
    got_st, got_pin, got_cmd, got_slot = (h.cpu().numpy() for h in hist)
    written = after_write.cpu().numpy()

    blk = ref.CommandBlock(B)
    exp_st, exp_pin, exp_slot = st0.copy(), pin0.copy(), slot0.copy()
    E, P, A, V = _lib.ST_EULER_D, _lib.ST_POS_D, _lib.ST_ANG_VEL_D, _lib.ST_LIN_VEL_D
    for t in range(T):
        exp_st[:B, _lib.ST_POS:_lib.ST_POS + 3] = pos[t]
        skip = np.zeros(B, bool)
        skip[nb] = t == NAN_TICK
        keep = {k: getattr(blk, k).copy() for k in ("body_height", "ctrl_state", "prev_ctrl_state", "kp_linear")}
        v = np.where(skip[:, None], 0.0, vel[t])  # (the skipped robot's members are put back below)
        o = blk.step(DT, v, rate[t], request[t], pos[t], exp_st[:B, E:E + 3], exp_st[:B, P:P + 3])
        for k, old in keep.items():
            getattr(blk, k)[skip] = old[skip]
        run = ~skip
        exp_st[:B, E:E + 3][run] = o["root_euler_d"][run]
        exp_st[:B, P:P + 3][run] = o["root_pos_d"][run]
        exp_st[:B, A:A + 3][run] = o["root_ang_vel_d"][run]
        exp_st[:B, V:V + 3][run] = o["root_lin_vel_d"][run]
        exp_st[:B, V:V + 3][skip] = np.nan
        exp_pin[:B, _lib.PL_MOVEMENT_MODE][run] = o["movement_mode"][run].astype(np.float64)
        sl = exp_slot[:B].view(mpcqp.CMD_STATE_DTYPE).reshape(B)
        for i in np.flatnonzero(run):
            sl[i] = (1.0, blk.body_height[i], blk.ctrl_state[i], blk.prev_ctrl_state[i], blk.kp_linear[i], 0.0)
        exp_cmd = written[t].copy()
        exp_cmd[:B, _lib.CM_MODE_REQUEST][run] = 0.0
        for name, got, exp in (("states", got_st[t], exp_st), ("plan_in", got_pin[t], exp_pin),
                               ("cmd", got_cmd[t], exp_cmd), ("slot", got_slot[t], exp_slot)):
            bad = np.argwhere(_bits(got) != _bits(exp))
            assert bad.size == 0, f"tick {t} {name}: first differing (row, double) {bad[:5].tolist()}"
        assert np.all(got_cmd[t][:B, _lib.CM_MODE_REQUEST][run] == 0.0)
    # the script did what it is for: both clamps, both modes, both sides of the threshold, the NaN tick
    heights = got_slot[:, :B, _lib.CS_BODY_HEIGHT]
    assert (heights == cp.body_height_max).any() and (heights == cp.body_height_min).any()
    modes = got_pin[:, :B, _lib.PL_MOVEMENT_MODE]
    assert (modes == 1.0).any() and (modes == 0.0).any()
    kp = got_slot[:, :B, _lib.CS_KP_LINEAR]
    assert (kp[modes == 1.0] == 0.0).any() and (kp[modes == 1.0] == 100.0).any()
    assert np.all(np.isnan(got_st[NAN_TICK, nb, V:V + 3])) and not np.isnan(got_st[NAN_TICK + 1, nb, V:V + 3]).any()


def test_command_arguments():
    cp = mpcqp.default_command_params()
    L = mpcqp.load()
    import ctypes
    assert L.mpcqp_command_device(ctypes.byref(cp), DT, None, None, None, 0, None, None) == _lib.ERR_OK
    assert L.mpcqp_command_device(ctypes.byref(cp), DT, None, None, None, 1, None, None) == _lib.ERR_INVALID_ARG
    assert L.mpcqp_command_device(None, DT, None, None, None, 0, None, None) == _lib.ERR_INVALID_ARG
    assert mpcqp.command_state_size() == _lib.CS_SIZE
    assert (cp.body_height_init, cp.body_height_max, cp.body_height_min, cp.vel_lock_threshold) == (0.2, 0.32, 0.1, 0.05)
    assert list(cp.kp_linear) == [100.0, 100.0, 300.0] and (cp.kp_linear_lock_x, cp.kp_linear_lock_y) == (100.0, 100.0)
