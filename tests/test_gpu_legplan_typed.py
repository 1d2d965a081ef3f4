"""mpcqp_leg_plan_typed_device on the GPU: the terrain adaptation per robot (A1RobotControl.cpp:335 adapts the
terrain only under stance_leg_control_type == 1).  Over 130 ticks, past the terrain window of 100, with
terrain = 1: a type-1 robot is bitwise mpcqp_leg_plan_device with terrain = 1 and every other robot bitwise
the terrain = 0 run, in every row the stage writes and in the whole slot, the terrain filter included."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib

from test_gpu_legplan import DT, _sequence
from test_torques import torque_inputs

pytestmark = pytest.mark.gpu

B, T, PAD = 67, 130, 2


def _run(p, ticks, tq0, types):
    """One launch per tick on inputs uploaded once as [T][B][..]; (states, tq, out, slot) per tick, as bits."""
    nan = float("nan")
    states = np.full((T, B + PAD, _lib.ST_SIZE), nan)
    pin = np.full((T, B + PAD, _lib.PL_SIZE), nan)
    for t, (st, rz, force, mode) in enumerate(ticks):
        states[t, :B] = mpcqp.pack_states(st)
        pin[t, :B] = mpcqp.pack_plan_inputs(rz, force, mode)
    tq = np.full((T, B + PAD, _lib.TQ_SIZE), nan)
    tq[:, :B] = tq0
    d_states, d_in, d_tq = (torch.from_numpy(a).cuda() for a in (states, pin, tq))
    d_out = torch.full((T, B + PAD, _lib.PO_SIZE), nan, dtype=torch.float64, device="cuda")
    d_slot = torch.zeros((B + PAD, mpcqp.plan_state_size()), dtype=torch.float64, device="cuda")
    d_slot[B:] = nan
    d_hist = torch.empty((T,) + tuple(d_slot.shape), dtype=torch.float64, device="cuda")
    d_ty = None
    if types is not None:
        ty = np.full(B + PAD, 1, np.int32)  # (the rows past the batch would run the terrain block if read)
        ty[:B] = types
        d_ty = torch.from_numpy(ty).cuda()
    s = torch.cuda.current_stream().cuda_stream
    for t in range(T):
        if d_ty is None:
            mpcqp.leg_plan_device(p, DT, d_states[t].data_ptr(), d_in[t].data_ptr(), B, d_slot.data_ptr(),
                                  d_tq[t].data_ptr(), d_out[t].data_ptr(), s)
        else:
            mpcqp.leg_plan_typed_device(p, DT, d_states[t].data_ptr(), d_in[t].data_ptr(), B, d_slot.data_ptr(),
                                        d_tq[t].data_ptr(), d_out[t].data_ptr(), d_ty.data_ptr(), s)
        d_hist[t].copy_(d_slot)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy().view(np.int64), pin.view(np.int64))
    return tuple(d.cpu().numpy().view(np.int64) for d in (d_states, d_tq, d_out, d_hist))


def test_terrain_adaptation_per_robot():
    ticks = _sequence(B, T, 23)
    J, fkin, contacts, _ = torque_inputs(B, 4)
    tq0 = mpcqp.assemble_torque_records(J, fkin, contacts)
    rng = np.random.default_rng(24)
    types = rng.integers(0, 2, B).astype(np.int32)
    types[:3] = [1, 0, 2]  # 2: neither branch; the terrain block is the MPC branch's alone
    on = _run(mpcqp.default_plan_params(terrain=1), ticks, tq0, None)
    off = _run(mpcqp.default_plan_params(terrain=0), ticks, tq0, None)
    typed = _run(mpcqp.default_plan_params(terrain=1), ticks, tq0, types)
    null = _run(mpcqp.default_plan_params(terrain=1), ticks, tq0, np.ones(B, np.int32))
    mpc = np.concatenate([types == 1, np.zeros(PAD, bool)])
    rest = ~mpc
    for name, got, a, b, n in zip(("states", "tq_records", "plan_out", "slot"), typed, on, off, null):
        assert np.array_equal(n, a), f"{name}: every type 1 is the terrain = 1 run"
        assert np.array_equal(got[:, mpc], a[:, mpc]), f"{name}: type-1 robots differ from the terrain = 1 run"
        assert np.array_equal(got[:, rest], b[:, rest]), f"{name}: the other robots differ from the terrain = 0 run"
    # the two runs do differ where it matters: root_euler_d[1], the terrain filter, the plane of the output row
    e1 = _lib.ST_EULER_D + 1
    assert np.all((on[0][:, :B, e1] != off[0][:, :B, e1]).any(axis=0))
    assert np.all((on[3][-1, :B] != off[3][-1, :B]).any(axis=1))
    assert np.all((on[2][:, :B] != off[2][:, :B]).any(axis=(0, 2)))
