"""ControlTick(plant=): the tick that closes its own loop.  The fused step is bitwise the staged C calls and the
captured graph's replays; a tick without plant= enqueues what it did before; and a tilted fleet under the
truth-fed MPC tick, replayed 400 times with no host write in between, meets the conditions the CPU model met."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib
from mpcqp.tick import ControlTick

import plant_reference as pr
from test_plant import DT, closed_loop_conditions, tilted_fleet

pytestmark = pytest.mark.gpu

B, T = 5, 24  # 24 ticks: past the torque map's nine zero-torque ticks
FULL = ("results", "torques", "counter", "states", "plan_in", "cmd", "records", "bal_records", "plan_out", "est_out",
        "sensors", "tq_records", "plant_out", "warm", "plan_state", "est_state", "cmd_state", "plant_state")
MPC = ("results", "torques", "counter", "states", "plan_in", "records", "tq_records", "plant_out", "warm",
       "plant_state")


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.int64 if a.dtype == np.float64 else a.dtype).copy()


def _caller_rows():
    """What the caller owns: the constants of the state rows and of the torque records."""
    st = mpcqp.synthetic_go1(B, seed=9, gait="stance")
    st.root_euler_d[:] = 0.0
    st.root_ang_vel_d[:] = 0.0
    st.root_lin_vel_d[:] = 0.0
    st.root_pos_d[:] = [0.0, 0.0, 0.29]
    tq = mpcqp.assemble_torque_records(np.zeros((B, 4, 3, 3)), np.zeros((B, 4, 3)), np.ones((B, 4), bool))
    return mpcqp.pack_states(st), tq


def _make(kind, plant=True):
    pp = mpcqp.default_plant_params() if plant else None
    if kind == "full":
        return ControlTick(B, plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                           command=mpcqp.default_command_params(), control_type="per_robot", dt=DT, plant=pp)
    return ControlTick(B, dt=DT, plant=pp)


def _staged(k, kind):
    """ControlTick.step's stages, one entry point at a time on the object's buffers."""
    s = torch.cuda.current_stream().cuda_stream
    if kind == "full":
        ty = k.control_type.data_ptr()
        mpcqp.command_device(k.command, k.dt, k.cmd.data_ptr(), k.states.data_ptr(), k.plan_in.data_ptr(), B,
                             k.cmd_state.data_ptr(), s)
        mpcqp.state_estimate_device(k.estimator, k.dt, k.sensors.data_ptr(), k.plan_in.data_ptr(), k.states.data_ptr(),
                                    B, k.est_state.data_ptr(), k.tq_records.data_ptr(), k.est_out.data_ptr(), s)
        mpcqp.leg_plan_typed_device(k.plan, k.dt, k.states.data_ptr(), k.plan_in.data_ptr(), B, k.plan_state.data_ptr(),
                                    k.tq_records.data_ptr(), k.plan_out.data_ptr(), ty, s)
        mpcqp.assemble_records_device(10, k.states.data_ptr(), B, k.records.data_ptr(), s)
        mpcqp.assemble_balance_device(k.gains, k.states.data_ptr(), k.plan_in.data_ptr(), k.cmd_state.data_ptr(), B,
                                      k.bal_records.data_ptr(), s)
        k.solver.balance_solve_typed_device(k.balance, k.bal_records.data_ptr(), B, ty, 0, k.results.data_ptr(), s)
        k.solver.solve_warm_typed_device(k.records.data_ptr(), B, k.warm.data_ptr(), ty, 1, k.results.data_ptr(), 0, s)
    else:
        mpcqp.assemble_records_device(10, k.states.data_ptr(), B, k.records.data_ptr(), s)
        k.solver.solve_warm_device(k.records.data_ptr(), B, k.warm.data_ptr(), k.results.data_ptr(), 0, s)
    mpcqp.joint_torques_device(k.tq_records.data_ptr(), k.results.data_ptr(), B, k.counter.data_ptr(),
                               k.torques.data_ptr(), s)
    if k.plant is not None:
        truth = kind != "full"
        mpcqp.plant_step_device(k.plant, k.dt, k.torques.data_ptr(), B, k.plant_state.data_ptr(), 0,
                                k.sensors.data_ptr() if kind == "full" else 0, k.plan_in.data_ptr(),
                                k.states.data_ptr() if truth else 0, k.tq_records.data_ptr() if truth else 0,
                                k.plant_out.data_ptr(), s)


def _drive(k, kind, how, names, fed=None):
    """T ticks; the host writes the commands and the control types only (and, for a tick without the plant,
    the sensor-level rows `fed` recorded from one with it).  Returns the rows at the start and after every tick."""
    rows, tq = _caller_rows()
    k.states.copy_(torch.from_numpy(rows))
    k.tq_records.copy_(torch.from_numpy(tq))
    if k.plant is not None:
        k.prime_plant()  # the slots and the rows of the start
        torch.cuda.synchronize()
    rng = np.random.default_rng(17)
    types = np.ones((T, B), np.int32)
    types[0:] = rng.integers(0, 2, B)
    types[8:] = rng.integers(0, 2, B)
    types[16:] = rng.integers(0, 2, B)
    outs = [{name: _bits(getattr(k, name)) for name in names}]
    for t in range(T):
        if kind == "full":
            request = np.zeros(B, bool)
            request[1::2] = t == 12  # two robots start walking half way
            k.cmd.copy_(torch.from_numpy(mpcqp.pack_commands(np.zeros((B, 3)), np.zeros((B, 3)), request)))
            k.control_type.copy_(torch.from_numpy(types[t]))
            if fed is not None:
                k.sensors.copy_(torch.from_numpy(fed[t][0]))
                k.plan_in[:, _lib.PL_FOOT_FORCE:_lib.PL_FOOT_FORCE + 4].copy_(torch.from_numpy(fed[t][1]))
        if how == "graph":
            if k.graph is None:
                k.capture()
            k.replay()
        elif how == "eager":
            k.step()
        else:
            _staged(k, kind)
        torch.cuda.synchronize()
        outs.append({name: _bits(getattr(k, name)) for name in names})
    return outs


_RUNS = {}


def _runs(kind):
    """The plant-closed tick of `kind` driven three ways, once per module."""
    if kind not in _RUNS:
        names = FULL if kind == "full" else MPC
        out = {}
        for how in ("eager", "staged", "graph"):
            k = _make(kind)
            try:
                out[how] = _drive(k, kind, how, names)
            finally:
                k.close()
        _RUNS[kind] = (names, out)
    return _RUNS[kind]


@pytest.mark.parametrize("other", ["staged", "graph"])
@pytest.mark.parametrize("kind", ["full", "mpc"])
def test_fused_tick_is_bitwise_the_stages_and_its_graph(kind, other):
    """8. over 24 ticks, with command + estimator + plan + per-robot types and MPC-only, truth-fed."""
    names, out = _runs(kind)
    for t, (a, b) in enumerate(zip(out["eager"], out[other])):
        for name in names:
            assert np.array_equal(a[name], b[name]), f"{kind} tick {t}: {name} of the eager tick and the {other} one differ"
    last = out["eager"][-1]
    po = last["plant_out"].view(np.float64)
    assert last["counter"].min() == T and np.abs(last["torques"].view(np.float64)).max() > 0
    assert np.all(last["plant_state"].view(np.float64)[:, _lib.PN_INIT] == 1.0)
    moved = po[:, _lib.PT_POS + 2] - out["eager"][0]["plant_out"].view(np.float64)[:, _lib.PT_POS + 2]
    print(f"[note] {kind} tick, {T} ticks: plant status {po[:, _lib.PT_STATUS]}, height change {moved}")
    assert np.all(moved != 0.0)  # the torques reached the plant and the plant moved


def test_tick_without_plant_enqueues_what_it_did():
    """8. a tick built without plant= is bitwise the stages of before on the same inputs: the sensor-level rows
    the plant produced in the closed run, fed from the host; and fed those, it computes the closed tick's torques."""
    _, out = _runs("full")
    closed = out["eager"]
    fed = [(o["sensors"].view(np.float64),
            o["plan_in"].view(np.float64)[:, _lib.PL_FOOT_FORCE:_lib.PL_FOOT_FORCE + 4].copy()) for o in closed[:-1]]
    keep = tuple(n for n in FULL if not n.startswith("plant"))
    got = {}
    for how in ("eager", "staged"):
        k = _make("full", plant=False)
        try:
            assert not hasattr(k, "plant_state") and not hasattr(k, "plant_out")
            got[how] = _drive(k, "full", how, keep, fed)
        finally:
            k.close()
    for t in range(1, T + 1):
        for name in keep:
            assert np.array_equal(got["eager"][t][name], got["staged"][t][name]), f"tick {t}: {name}"
        assert np.array_equal(got["eager"][t]["torques"], closed[t]["torques"]), f"tick {t}: torques"


def test_closed_loop_rollout_on_the_device():
    """9. test_plant's closed loop as a truth-fed MPC-only tick, graph-replayed 400 times with no host write in
    between; substeps 1 on the even robots and 4 on the odd ones (two ticks: substeps is a kernel argument).
    The conditions are measured over ticks 10 .. 400 (the torque map holds zero torques before); the height
    may sag during those, so dz is measured against the start and the largest on the way is printed."""
    init, rpy = tilted_fleet()
    n = init.shape[0]
    tilt0 = np.hypot(rpy[:, 0], rpy[:, 1])
    tilt1, fz, dz, sag = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    statuses, contacts = np.zeros((391, n), np.int32), np.zeros((400, n, 4))
    for substeps, idx in ((1, np.arange(0, n, 2)), (4, np.arange(1, n, 2))):
        b = len(idx)
        pp = mpcqp.default_plant_params(substeps=substeps)
        k = ControlTick(b, dt=DT, plant=pp, plant_init=init[idx])
        try:
            z = np.zeros((b, 3))
            st = mpcqp.RobotStates(  # the caller's rows: the desired values and the constants
                root_euler=z, root_pos=z, root_ang_vel=z, root_lin_vel=z, root_rot_mat=np.zeros((b, 3, 3)),
                root_euler_d=np.stack([z[:, 0], z[:, 0], rpy[idx, 2]], 1),
                root_pos_d=init[idx, pr.PI_POS:pr.PI_POS + 3], root_ang_vel_d=z, root_lin_vel_d=z,
                foot_pos_abs=np.zeros((b, 4, 3)), contacts=np.ones((b, 4), bool), mu=np.full(b, 0.3))
            k.states.copy_(torch.from_numpy(mpcqp.pack_states(st)))
            k.tq_records.copy_(torch.from_numpy(mpcqp.assemble_torque_records(
                np.zeros((b, 4, 3, 3)), np.zeros((b, 4, 3)), np.ones((b, 4), bool), torques_gravity=np.zeros(12))))
            k.prime_plant()  # the truth of the start, so the first solve sees the robot
            k.capture()
            mg = pp.mass * pp.gravity
            z0 = init[idx, pr.PI_POS + 2]
            for t in range(1, 401):
                k.replay()
                torch.cuda.synchronize()
                po = k.plant_out.cpu().numpy()
                assert np.all(po[:, _lib.PT_STATUS] == 0.0), f"tick {t}: plant status {po[:, _lib.PT_STATUS]}"
                contacts[t - 1, idx] = po[:, _lib.PT_CONTACTS:_lib.PT_CONTACTS + 4]
                sag[idx] = np.maximum(sag[idx], np.abs(po[:, _lib.PT_POS + 2] - z0))
                if t >= 10:
                    res = np.frombuffer(k.results.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE)
                    statuses[t - 10, idx] = res["status"]
            tilt1[idx] = np.hypot(po[:, _lib.PT_EULER], po[:, _lib.PT_EULER + 1])
            fz[idx] = po[:, _lib.PT_GRF + 2:_lib.PT_GRF + 12:3].sum(1) / mg
            dz[idx] = po[:, _lib.PT_POS + 2] - z0
        finally:
            k.close()
    print(f"[note] device closed loop: tilt ratio {np.round(tilt1 / tilt0, 4)} Fz/mg {np.round(fz, 5)} "
          f"dz at the end {np.round(dz, 6)} largest |dz| on the way {np.round(sag, 6)}")
    closed_loop_conditions(tilt0, tilt1, fz, dz, statuses, contacts == 1.0)
