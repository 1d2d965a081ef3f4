"""Time of the leg-plan stage (mpcqp_leg_plan_device) beside the assemble kernel, and of the
graph-replayed control tick with and without it (HIP events, 3 warm-up runs, median of 20).

The tick without the plan is fed the state rows and torque records the tick with the plan produced, so
both solve exactly the same problems and the difference is the plan stage.
usage: python tools/time_legplan.py [--batch 4096]"""
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
from mpcqp.records import rot_zyx, synthetic_go1_ticks  # noqa: E402
from mpcqp.tick import ControlTick  # noqa: E402
from test_torques import torque_inputs  # noqa: E402  (synthetic Jacobians)

WARMUP, RUNS = 3, 20


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    B = ap.parse_args().batch
    T = WARMUP + RUNS
    states = synthetic_go1_ticks(B, T, seed=3, gait="stance")
    rng = np.random.default_rng(4)
    sts = [torch.from_numpy(mpcqp.pack_states(s)).cuda() for s in states]
    pins = [torch.from_numpy(mpcqp.pack_plan_inputs(rot_zyx(np.zeros(B), np.zeros(B), s.root_euler[:, 2]),
                                                    rng.uniform(0.0, 60.0, (B, 4)), 1)).cuda() for s in states]
    J, fkin, contacts, _ = torque_inputs(B, 1)
    tq = torch.from_numpy(mpcqp.assemble_torque_records(J, fkin, contacts)).cuda()
    p = mpcqp.default_plan_params()
    stream = torch.cuda.current_stream().cuda_stream
    out = {"batch": B, "warmup": WARMUP, "runs": RUNS}

    # the two kernels alone, one launch between two events
    f64 = dict(dtype=torch.float64, device="cuda")
    slot = torch.zeros((B, mpcqp.plan_state_size()), **f64)
    pout = torch.zeros((B, _lib.PO_SIZE), **f64)
    recs = torch.zeros((B, _lib.rec_size(10)), **f64)
    work = sts[0].clone()
    out["plan_kernel_ms"] = median_ms(
        lambda: mpcqp.leg_plan_device(p, p.control_dt, work.data_ptr(), pins[0].data_ptr(), B, slot.data_ptr(),
                                      tq.data_ptr(), pout.data_ptr(), stream))
    out["assemble_kernel_ms"] = median_ms(
        lambda: _lib.assemble_records_device(10, work.data_ptr(), B, recs.data_ptr(), stream))

    # the graph-replayed tick with the plan; keep what the plan wrote for the tick without it
    produced = []
    with_plan = ControlTick(B, plan=p)
    with_plan.tq_records.copy_(tq)
    with_plan.capture()

    def load_with(i):
        with_plan.states.copy_(sts[i])
        with_plan.plan_in.copy_(pins[i])

    times = []
    for i in range(T):
        load_with(i)
        times.append(event_ms(with_plan.replay))
        produced.append((with_plan.states.clone(), with_plan.tq_records.clone()))
    out["tick_graph_with_plan_ms"] = statistics.median(times[WARMUP:])
    with_plan.close()

    without = ControlTick(B)
    without.capture()

    def load_without(i):
        without.states.copy_(produced[i][0])
        without.tq_records.copy_(produced[i][1])

    out["tick_graph_without_plan_ms"] = median_ms(without.replay, load_without)
    without.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
