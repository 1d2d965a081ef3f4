"""Time of the state front end (mpcqp_state_estimate_device) beside the plan and assemble kernels, and of
the graph-replayed control tick with and without it (HIP events, 3 warm-up runs, median of 20).

The four-stage tick (plan, assemble, solve, torques) is fed the state rows, plan rows and torque records
the five-stage tick's estimator produced, so both solve exactly the same problems and the difference is
the estimator stage.
usage: python tools/time_estimator.py [--batch 4096]"""
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

WARMUP, RUNS = 3, 20
STAND = np.tile([0.0, 0.8, -1.6], 4)


def event_ms(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def median_ms(fn, before=lambda i: None):
    times = []
    for i in range(WARMUP + RUNS):
        before(i)
        times.append(event_ms(fn))
    return statistics.median(times[WARMUP:])


def quat_zyx(e):
    cr, sr, cp, sp, cy, sy = (f(e[:, k] / 2) for k in range(3) for f in (np.cos, np.sin))
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy], -1)


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
    pins = [torch.from_numpy(mpcqp.pack_plan_inputs(np.zeros((B, 3, 3)), rng.uniform(0.0, 60.0, (B, 4)), 1)).cuda()
            for _ in states]
    J, fkin, contacts, _ = torque_inputs(B, 1)
    tq = torch.from_numpy(mpcqp.assemble_torque_records(J, fkin, contacts)).cuda()
    pp, pe = mpcqp.default_plan_params(), mpcqp.default_estimator_params()
    stream = torch.cuda.current_stream().cuda_stream
    out = {"batch": B, "warmup": WARMUP, "runs": RUNS}

    # the three kernels alone, one launch between two events (the estimator on initialized filters: the
    # warm-up launches include the init_state tick)
    f64 = dict(dtype=torch.float64, device="cuda")
    eslot = torch.zeros((B, mpcqp.estimator_state_size()), **f64)
    eout = torch.zeros((B, _lib.EO_SIZE), **f64)
    pslot = torch.zeros((B, mpcqp.plan_state_size()), **f64)
    pout = torch.zeros((B, _lib.PO_SIZE), **f64)
    recs = torch.zeros((B, _lib.rec_size(10)), **f64)
    work, pin, tqw = st0.clone(), pins[0].clone(), tq.clone()
    out["estimate_kernel_ms"] = median_ms(
        lambda: mpcqp.state_estimate_device(pe, pp.control_dt, sns[0].data_ptr(), pin.data_ptr(), work.data_ptr(), B,
                                            eslot.data_ptr(), tqw.data_ptr(), eout.data_ptr(), stream))
    out["plan_kernel_ms"] = median_ms(
        lambda: mpcqp.leg_plan_device(pp, pp.control_dt, work.data_ptr(), pin.data_ptr(), B, pslot.data_ptr(),
                                      tqw.data_ptr(), pout.data_ptr(), stream))
    out["assemble_kernel_ms"] = median_ms(
        lambda: _lib.assemble_records_device(10, work.data_ptr(), B, recs.data_ptr(), stream))

    # the graph-replayed five-stage tick; keep what the estimator wrote for the four-stage tick
    produced = []
    five = ControlTick(B, plan=pp, estimator=pe)
    five.tq_records.copy_(tq)
    five.states.copy_(st0)
    five.capture()
    times = []
    for i in range(T):
        five.sensors.copy_(sns[i])
        five.plan_in.copy_(pins[i])
        times.append(event_ms(five.replay))
        produced.append((five.states.clone(), five.plan_in.clone(), five.tq_records.clone()))
    out["tick_graph_five_stage_ms"] = statistics.median(times[WARMUP:])
    five.close()

    four = ControlTick(B, plan=pp)
    four.capture()

    def load_four(i):
        four.states.copy_(produced[i][0])
        four.plan_in.copy_(produced[i][1])
        four.tq_records.copy_(produced[i][2])

    out["tick_graph_four_stage_ms"] = median_ms(four.replay, load_four)
    four.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
