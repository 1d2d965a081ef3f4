"""mpcqp_assemble_balance_device on the GPU: the MPCQP_BAL_* records are bitwise mpcqp/balance.py
assemble_balance (pure copies), with the gains' kp_linear and with the command slots' one."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib, balance

pytestmark = pytest.mark.gpu

B = 67
PAD = 2


def _inputs():
    s = mpcqp.synthetic_go1(B, seed=31, gait="mixed")
    rng = np.random.default_rng(32)
    s.root_euler_d = rng.normal(0.0, 0.1, (B, 3))
    s.root_pos_d = rng.normal(0.0, 1.0, (B, 3))
    s.robot_mass = rng.uniform(10.0, 15.0, B)
    rz = balance.rot_z(rng.uniform(-np.pi, np.pi, B))  # not the row's yaw: the record takes the plan row's matrix
    st = np.full((B + PAD, _lib.ST_SIZE), np.nan)
    st[:B] = mpcqp.pack_states(s)
    pin = np.full((B + PAD, _lib.PL_SIZE), np.nan)
    pin[:B] = mpcqp.pack_plan_inputs(rz, rng.uniform(0.0, 100.0, (B, 4)), 1)
    return s, rz, st, pin, rng


def _device(gains, st, pin, slot):
    d_st, d_pin = torch.from_numpy(st).cuda(), torch.from_numpy(pin).cuda()
    d_slot = torch.from_numpy(slot).cuda() if slot is not None else None
    d_rec = torch.full((B + PAD, _lib.BAL_SIZE), -7.0, dtype=torch.float64, device="cuda")
    mpcqp.assemble_balance_device(gains, d_st.data_ptr(), d_pin.data_ptr(), d_slot.data_ptr() if slot is not None else 0,
                                  B, d_rec.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_rec.cpu().numpy()
    assert np.all(got[B:] == -7.0)  # nothing past the batch
    for d, a in ((d_st, st), (d_pin, pin)):  # inputs are read only
        assert np.array_equal(d.cpu().numpy().view(np.int64), a.view(np.int64))
    return got[:B]


def _same(got, want):
    bad = np.argwhere(got.view(np.int64) != np.ascontiguousarray(want).view(np.int64))
    assert bad.size == 0, f"first differing (robot, double): {bad[:5].tolist()}"


def test_default_gains():
    g = mpcqp.default_balance_gains()
    assert np.array_equal(list(g.kp_linear), balance.GO1_KP_LINEAR) and np.array_equal(list(g.kd_linear), balance.GO1_KD_LINEAR)
    assert np.array_equal(list(g.kp_angular), balance.GO1_KP_ANGULAR)
    assert np.array_equal(list(g.kd_angular), balance.GO1_KD_ANGULAR)
    s, rz, st, pin, _ = _inputs()
    _same(_device(g, st, pin, None), balance.assemble_balance(s, mass=s.robot_mass, root_rot_mat_z=rz))


def test_other_gains_without_slot():
    kw = dict(kp_linear=[11.0, 12.0, 13.0], kd_linear=[21.0, 22.0, 23.0], kp_angular=[31.0, 32.0, 33.0],
              kd_angular=[41.0, 42.0, 43.0])
    s, rz, st, pin, _ = _inputs()
    want = balance.assemble_balance(s, mass=s.robot_mass, root_rot_mat_z=rz, **{k: np.array(v) for k, v in kw.items()})
    _same(_device(mpcqp.default_balance_gains(**kw), st, pin, None), want)


def test_kp_linear_from_command_slot():
    s, rz, st, pin, rng = _inputs()
    slot = np.full((B + PAD, mpcqp.command_state_size()), np.nan)
    slot[:B] = rng.normal(size=(B, _lib.CS_SIZE))
    kp = np.tile([100.0, 100.0, 300.0], (B, 1))
    kp[::3, 0:2] = 0.0  # robots walking with a planar speed command: the position lock is off
    kp[5] = [1.0, 2.0, 3.0]
    slot[:B, _lib.CS_KP_LINEAR:_lib.CS_KP_LINEAR + 3] = kp
    g = mpcqp.default_balance_gains(kp_linear=[-1.0, -2.0, -3.0])  # must not show up
    want = balance.assemble_balance(s, kp_linear=kp, mass=s.robot_mass, root_rot_mat_z=rz)
    got = _device(g, st, pin, slot)
    _same(got, want)
    assert np.all(got[::3, balance.BAL_KP_LIN:balance.BAL_KP_LIN + 2] == 0.0)
