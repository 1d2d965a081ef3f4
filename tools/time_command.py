"""Time of the command stage (mpcqp_command_device) and the balance assembly (mpcqp_assemble_balance_device)
beside the plan and assemble kernels, and of the graph-replayed control tick in four forms (HIP events, 3
warm-up runs, median of 20, all in one session):

  five_stage       estimate, plan, assemble, warm solve, torques, fed the command fields the command stage
                   produced, so every form solves the same problems
  six_stage        the same with the command stage
  per_robot_all1   control_type="per_robot", every type 1: the cost of the typed path (order_kernel's
                   selection, scale_kernel's type test, the second assembly and one empty balance launch)
  per_robot_half   control_type="per_robot", every other robot type 0

Each form also prints the quartiles and extremes of its 20 repetitions: the run-to-run spread a difference
between two forms has to exceed.  balance_kernel_half_ms is the typed balance solve of the half fleet
alone, which the mixed tick runs serially before the MPC solve on one stream.
usage: python tools/time_command.py [--batch 4096]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "go1-qp-mpc-controller_amd"), os.path.join(REPO, "tests")]
import mpcqp  # noqa: E402
from mpcqp import _lib  # noqa: E402
from mpcqp.records import synthetic_go1_ticks  # noqa: E402
from mpcqp.tick import ControlTick  # noqa: E402
from test_torques import torque_inputs  # noqa: E402  (synthetic Jacobians)
from time_estimator import STAND, WARMUP, RUNS, event_ms, median_ms, quat_zyx  # noqa: E402

CMD_FIELDS = slice(_lib.ST_EULER_D, _lib.ST_LIN_VEL_D + 3)  # what the command stage writes in the state row


def spread(times):
    t = sorted(times[WARMUP:])
    q = statistics.quantiles(t, n=4)
    return {"median_ms": statistics.median(t), "min_ms": t[0], "q1_ms": q[0], "q3_ms": q[2], "max_ms": t[-1]}


def paired_tick_ms(k, without, settle):
    """The graph-replayed tick `k` with and without the stages `without` (ControlTick.capture(without=): the same
    tick on the same buffers).  After `settle` replays of the full graph, each of WARMUP + RUNS repetitions
    snapshots every tensor of the tick, replays the graph without, restores the snapshot and replays the full one,
    so the two replays of a pair do the same work from the same slots but for the stages (the solver handle's
    launch-order hint is the one state not restored).  Returns the spread of the full tick's times, of the times
    without, and the median and extremes of the paired differences."""
    g_with, g_without = k.capture(), k.capture(without=without)
    for _ in range(settle):
        g_with.replay()
    tensors = [v for v in vars(k).values() if isinstance(v, torch.Tensor)]
    t_with, t_without, diff = [], [], []
    for _ in range(WARMUP + RUNS):
        snap = [t.clone() for t in tensors]
        t_without.append(event_ms(g_without.replay))
        for t, c in zip(tensors, snap):
            t.copy_(c)
        t_with.append(event_ms(g_with.replay))
        diff.append(t_with[-1] - t_without[-1])
    d = sorted(diff[WARMUP:])
    return spread(t_with), spread(t_without), {"median_ms": d[len(d) // 2], "min_ms": d[0], "max_ms": d[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    B = ap.parse_args().batch
    T = WARMUP + RUNS
    states = synthetic_go1_ticks(B, T, seed=3, gait="stance")
    rng = np.random.default_rng(4)
    st0 = torch.from_numpy(mpcqp.pack_states(states[0])).cuda()
    sns = [torch.from_numpy(mpcqp.pack_sensors(quat_zyx(s.root_euler), STAND + rng.uniform(-0.1, 0.1, (B, 12)),
                                               rng.normal(0.0, 0.05, (B, 12)),
                                               rng.normal(0.0, 0.1, (B, 3)) + np.array([0.0, 0.0, 9.81]),
                                               rng.normal(0.0, 0.1, (B, 3)))).cuda() for s in states]
    forces = [torch.from_numpy(rng.uniform(0.0, 60.0, (B, 4))).cuda() for _ in states]
    # every robot asks to walk on the first tick; planar speed commands on both sides of the lock threshold
    cmds = [torch.from_numpy(mpcqp.pack_commands(np.concatenate([rng.normal(0.0, 0.05, (B, 2)), np.zeros((B, 1))], 1),
                                                 rng.normal(0.0, 0.1, (B, 3)), i == 0)).cuda() for i in range(T)]
    J, fkin, contacts, _ = torque_inputs(B, 1)
    tq = torch.from_numpy(mpcqp.assemble_torque_records(J, fkin, contacts)).cuda()
    pp, pe, pc = mpcqp.default_plan_params(), mpcqp.default_estimator_params(), mpcqp.default_command_params()
    stream = torch.cuda.current_stream().cuda_stream
    out = {"batch": B, "warmup": WARMUP, "runs": RUNS}

    # the four launch-bound kernels alone, one launch between two events
    f64 = dict(dtype=torch.float64, device="cuda")
    cslot = torch.zeros((B, mpcqp.command_state_size()), **f64)
    pslot = torch.zeros((B, mpcqp.plan_state_size()), **f64)
    pout = torch.zeros((B, _lib.PO_SIZE), **f64)
    recs = torch.zeros((B, _lib.rec_size(10)), **f64)
    brecs = torch.zeros((B, _lib.BAL_SIZE), **f64)
    work, tqw, cmd = st0.clone(), tq.clone(), cmds[1].clone()
    pin = torch.from_numpy(mpcqp.pack_plan_inputs(np.tile(np.eye(3), (B, 1, 1)), forces[0].cpu().numpy(), 1)).cuda()
    gains = mpcqp.default_balance_gains()
    out["command_kernel_ms"] = median_ms(
        lambda: mpcqp.command_device(pc, pp.control_dt, cmd.data_ptr(), work.data_ptr(), pin.data_ptr(), B,
                                     cslot.data_ptr(), stream))
    out["assemble_balance_kernel_ms"] = median_ms(
        lambda: mpcqp.assemble_balance_device(gains, work.data_ptr(), pin.data_ptr(), cslot.data_ptr(), B,
                                              brecs.data_ptr(), stream))
    out["plan_kernel_ms"] = median_ms(
        lambda: mpcqp.leg_plan_device(pp, pp.control_dt, work.data_ptr(), pin.data_ptr(), B, pslot.data_ptr(),
                                      tqw.data_ptr(), pout.data_ptr(), stream))
    out["assemble_kernel_ms"] = median_ms(
        lambda: _lib.assemble_records_device(10, work.data_ptr(), B, recs.data_ptr(), stream))

    half = torch.from_numpy((np.arange(B) % 2).astype(np.int32)).cuda()

    def run_form(control_type, command, types=None, produced=None, keep=None):
        k = ControlTick(B, plan=pp, estimator=pe, command=pc if command else None, control_type=control_type)
        k.tq_records.copy_(tq)
        k.states.copy_(st0)
        if types is not None:
            k.control_type.copy_(types)
        k.capture()
        times = []
        for i in range(T):
            k.sensors.copy_(sns[i])
            k.plan_in[:, _lib.PL_FOOT_FORCE:_lib.PL_FOOT_FORCE + 4].copy_(forces[i])
            if command:
                k.cmd.copy_(cmds[i])
            else:
                k.states[:, CMD_FIELDS].copy_(produced[i][0])
                k.plan_in[:, _lib.PL_MOVEMENT_MODE].copy_(produced[i][1])
            times.append(event_ms(k.replay))
            if keep is not None:
                keep.append((k.states[:, CMD_FIELDS].clone(), k.plan_in[:, _lib.PL_MOVEMENT_MODE].clone()))
        if types is not None and control_type == "per_robot" and bool((types == 0).any()):
            bal = torch.zeros((B, _lib.RESULT_DOUBLES), **f64)
            out["balance_kernel_half_ms"] = median_ms(
                lambda: k.solver.balance_solve_typed_device(k.balance, k.bal_records.data_ptr(), B, types.data_ptr(), 0,
                                                            bal.data_ptr(), stream))
        k.close()
        return spread(times)

    produced = []
    out["tick_graph_six_stage"] = run_form(None, True, keep=produced)
    out["tick_graph_five_stage"] = run_form(None, False, produced=produced)
    out["tick_graph_per_robot_all1"] = run_form("per_robot", True)
    out["tick_graph_per_robot_half"] = run_form("per_robot", True, types=half)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
