"""The six-stage mixed tick: command -> estimate -> plan -> assemble (MPC and balance) -> balance solve of the
type-0 robots -> warm MPC solve of the type-1 robots -> torque map, with per-robot control types that change
between ticks.  The fused ControlTick is bitwise the same stages called one by one, its graph replay bitwise
the eager tick, the first tick agrees with the CPU oracle per branch, and a ControlTick without the new
arguments is still the three-call tick."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib, balance
from mpcqp.records import RobotStates
from mpcqp.tick import ControlTick

from test_gpu_estimator import _tick_inputs
from test_torques import torque_inputs

pytestmark = pytest.mark.gpu

B, T = 67, 14  # 14 ticks: past the torque map's start-up counter of 10
SLOTS = ("warm", "plan_state", "est_state", "cmd_state")
ROWS = ("results", "torques", "counter", "states", "plan_in", "cmd", "records", "bal_records", "plan_out", "est_out")


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.int64 if a.dtype == np.float64 else a.dtype).copy()


def _inputs():
    states_t, seq, sensors, plan_in = _tick_inputs(B, T)
    rng = np.random.default_rng(61)
    vel = rng.normal(0.0, 0.05, (T, B, 3))        # planar speeds on both sides of the 0.05 lock threshold
    vel[:, :, 2] = rng.normal(0.0, 2.0, (T, B))   # the height moves by about a millimetre a tick
    rate = rng.normal(0.0, 0.2, (T, B, 3))
    request = np.zeros((T, B), bool)
    request[0] = np.arange(B) % 4 != 0            # three in four start walking on the first tick
    request[6, ::5] = True                        # and some toggle again later
    cmds = [mpcqp.pack_commands(vel[t], rate[t], request[t]) for t in range(T)]
    types = np.ones((T, B), np.int32)
    types[0:] = rng.integers(0, 2, B)
    types[4:] = rng.integers(0, 2, B)             # the types change on ticks 4 and 9
    types[9:] = rng.integers(0, 2, B)
    types[:, 7] = 2                               # neither branch: keeps its (zero) result row
    J, fkin, _, _ = torque_inputs(B, 3)
    tq = mpcqp.assemble_torque_records(J, fkin, states_t[0].contacts)
    return states_t, sensors, plan_in, cmds, types, tq


def _make():
    return ControlTick(B, plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                       command=mpcqp.default_command_params(), control_type="per_robot")


def _staged(k):
    """The stages ControlTick.step walks for the tick with a control type, one entry point at a time on the
    object's buffers."""
    s = torch.cuda.current_stream().cuda_stream
    ty = k.control_type.data_ptr()
    mpcqp.command_device(k.command, k.dt, k.cmd.data_ptr(), k.states.data_ptr(), k.plan_in.data_ptr(), B,
                         k.cmd_state.data_ptr(), s)
    mpcqp.state_estimate_device(k.estimator, k.dt, k.sensors.data_ptr(), k.plan_in.data_ptr(), k.states.data_ptr(), B,
                                k.est_state.data_ptr(), k.tq_records.data_ptr(), k.est_out.data_ptr(), s)
    mpcqp.leg_plan_typed_device(k.plan, k.dt, k.states.data_ptr(), k.plan_in.data_ptr(), B, k.plan_state.data_ptr(),
                                k.tq_records.data_ptr(), k.plan_out.data_ptr(), ty, s)
    mpcqp.assemble_records_device(10, k.states.data_ptr(), B, k.records.data_ptr(), s)
    mpcqp.assemble_balance_device(k.gains, k.states.data_ptr(), k.plan_in.data_ptr(), k.cmd_state.data_ptr(), B,
                                  k.bal_records.data_ptr(), s)
    k.solver.balance_solve_typed_device(k.balance, k.bal_records.data_ptr(), B, ty, 0, k.results.data_ptr(), s)
    k.solver.solve_warm_typed_device(k.records.data_ptr(), B, k.warm.data_ptr(), ty, 1, k.results.data_ptr(), 0, s)
    mpcqp.joint_torques_device(k.tq_records.data_ptr(), k.results.data_ptr(), B, k.counter.data_ptr(),
                               k.torques.data_ptr(), s)


def _drive(k, inputs, how):
    states_t, sensors, plan_in, cmds, types, tq = inputs
    k.tq_records.copy_(torch.from_numpy(tq))
    k.states.copy_(torch.from_numpy(mpcqp.pack_states(states_t[0])))  # the caller's fields, written once
    outs = []
    for t in range(T):
        k.sensors.copy_(torch.from_numpy(sensors[t]))
        k.plan_in[:, _lib.PL_FOOT_FORCE:_lib.PL_FOOT_FORCE + 4].copy_(
            torch.from_numpy(plan_in[t][:, _lib.PL_FOOT_FORCE:_lib.PL_FOOT_FORCE + 4]))
        k.cmd.copy_(torch.from_numpy(cmds[t]))
        k.control_type.copy_(torch.from_numpy(types[t]))
        if how == "graph":
            if k.graph is None:
                k.capture()
            k.replay()
        elif how == "eager":
            k.step()
        else:
            _staged(k)
        torch.cuda.synchronize()
        outs.append({name: _bits(getattr(k, name)) for name in ROWS + SLOTS})
    return outs


@pytest.fixture(scope="module")
def runs():
    inputs = _inputs()
    out = {}
    for how in ("eager", "staged", "graph"):
        k = _make()
        try:
            out[how] = _drive(k, inputs, how)
        finally:
            k.close()
    return inputs, out


@pytest.mark.parametrize("other", ["staged", "graph"])
def test_fused_tick_is_bitwise_the_stages_and_its_graph(runs, other):
    _, out = runs
    for t, (a, b) in enumerate(zip(out["eager"], out[other])):
        for name in ROWS + SLOTS:
            assert np.array_equal(a[name], b[name]), f"tick {t}: {name} of the eager tick and the {other} one differ"
    last = out["eager"][-1]
    assert last["counter"].min() == T and np.abs(last["torques"].view(np.float64)).max() > 0
    modes = np.stack([o["plan_in"].view(np.float64)[:, _lib.PL_MOVEMENT_MODE] for o in out["eager"]])
    assert (modes == 1.0).any() and (modes == 0.0).any()


def _unpack(st):
    g = lambda o, n: st[:, o:o + n].copy()  # noqa: E731
    return RobotStates(
        root_euler=g(_lib.ST_EULER, 3), root_pos=g(_lib.ST_POS, 3), root_ang_vel=g(_lib.ST_ANG_VEL, 3),
        root_lin_vel=g(_lib.ST_LIN_VEL, 3), root_rot_mat=g(_lib.ST_ROT, 9).reshape(-1, 3, 3),
        root_euler_d=g(_lib.ST_EULER_D, 3), root_pos_d=g(_lib.ST_POS_D, 3), root_ang_vel_d=g(_lib.ST_ANG_VEL_D, 3),
        root_lin_vel_d=g(_lib.ST_LIN_VEL_D, 3), foot_pos_abs=g(_lib.ST_FEET, 12).reshape(-1, 4, 3),
        contacts=g(_lib.ST_CONTACTS, 4) != 0.0, robot_mass=st[:, _lib.ST_MASS].copy(),
        trunk_inertia=g(_lib.ST_INERTIA, 9).reshape(-1, 3, 3), mu=st[:, _lib.ST_MU].copy(),
        fz_min=float(st[0, _lib.ST_FZMIN]), fz_max=float(st[0, _lib.ST_FZMAX]), mpc_dt=float(st[0, _lib.ST_DT]))


def test_first_tick_against_the_oracle(runs, oracle):
    inputs, out = runs
    types = inputs[4][0]
    first = out["eager"][0]
    st = first["states"].view(np.float64)
    s = _unpack(st)
    res = np.frombuffer(first["results"].tobytes(), dtype=mpcqp.RESULT_DTYPE)
    # type 0: the balance QP of records assembled on the host, bitwise
    rz = first["plan_in"].view(np.float64)[:, _lib.PL_ROT_Z:_lib.PL_ROT_Z + 9].reshape(B, 3, 3)
    kp = first["cmd_state"].view(np.float64)[:, _lib.CS_KP_LINEAR:_lib.CS_KP_LINEAR + 3]
    brec = balance.assemble_balance(s, kp_linear=kp, mass=s.robot_mass, root_rot_mat_z=rz)
    assert np.array_equal(brec.view(np.int64), first["bal_records"])
    qp = types == 0
    ref = oracle.balance_solve_batch(oracle.default_params(10), oracle.default_balance_params(), brec, 8)
    assert np.array_equal(res["status"][qp], ref["status"][qp]) and np.array_equal(res["iters"][qp], ref["iters"][qp])
    assert np.array_equal(res["u0"][qp].view(np.int64), ref["u0"][qp].view(np.int64))
    # type 1: the MPC of records assembled on the host, cold on the first tick
    mpc = types == 1
    rec = mpcqp.assemble_compute_grf(s, 10)
    ref = oracle.solve_batch(oracle.default_params(10), rec, nthreads=8)
    assert np.array_equal(res["status"][mpc], ref["status"][mpc])
    err = np.abs(res["u0"] - ref["u0"]).max(1) / np.maximum(np.abs(ref["u0"]).max(1), 1.0)
    print(f"[note] mixed tick 1: max u0 rel err of the MPC robots {err[mpc].max():.3e}")
    assert err[mpc].max() <= 1e-4
    # neither: the result row the buffer started with
    assert np.all(first["results"][types == 2] == 0)
    assert qp.sum() > 5 and mpc.sum() > 5


def test_tick_without_the_new_arguments_is_the_three_call_tick():
    states_t = _inputs()[0]
    J, fkin, contacts, _ = torque_inputs(B, 3)
    tq = torch.from_numpy(mpcqp.assemble_torque_records(J, fkin, contacts)).cuda()
    k = ControlTick(B)
    s = mpcqp.MpcQpSolver(mpcqp.default_params(10))
    try:
        assert not hasattr(k, "control_type") and not hasattr(k, "cmd") and not hasattr(k, "bal_records")
        f64 = dict(dtype=torch.float64, device="cuda")
        states = torch.zeros((B, _lib.ST_SIZE), **f64)
        records = torch.zeros((B, _lib.rec_size(10)), **f64)
        warm = torch.zeros((B, s.warm_state_size), **f64)
        results = torch.zeros((B, _lib.RESULT_DOUBLES), **f64)
        counter = torch.zeros((B,), dtype=torch.int32, device="cuda")
        torques = torch.zeros((B, 12), **f64)
        k.tq_records.copy_(tq)
        stream = torch.cuda.current_stream().cuda_stream
        for t in range(T):
            rows = torch.from_numpy(mpcqp.pack_states(states_t[t]))
            k.states.copy_(rows)
            states.copy_(rows)
            k.step()
            mpcqp.assemble_records_device(10, states.data_ptr(), B, records.data_ptr(), stream)
            s.solve_warm_device(records.data_ptr(), B, warm.data_ptr(), results.data_ptr(), 0, stream)
            mpcqp.joint_torques_device(tq.data_ptr(), results.data_ptr(), B, counter.data_ptr(), torques.data_ptr(),
                                       stream)
            torch.cuda.synchronize()
            for name, mine in (("results", results), ("torques", torques), ("counter", counter), ("warm", warm)):
                assert np.array_equal(_bits(getattr(k, name)), _bits(mine)), f"tick {t}: {name}"
    finally:
        k.close()
        s.close()
