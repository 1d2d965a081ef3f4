"""Time of the plant stage (mpcqp_plant_step_device) beside the torque map and the plan kernel, and of the
graph-replayed control tick with and without it (HIP events, 3 warm-up runs, median of 20, all in one session):

  plant_kernel_substeps{1,4}_ms   one launch, a standing fleet under weight-bearing torques (every leg in
                                  stance: the inverse kinematics and three 3x3 solves per leg and substep)
  plant_kernel_swing_substeps4_ms the same fleet in free fall (every leg in swing)
  plant_kernel_{wrench,terrain,wrench_terrain}_substeps4_ms
                                  the other three instantiations on the standing fleet, in the same session: a zero
                                  wrench row, and a level terrain row per robot with the plant's mu (the same
                                  motion, so the four differ by their code alone)
  plant_kernel_slope_substeps4_ms the terrain instantiation with the fleet standing slope-parallel on planes of
                                  pitch and roll in +-0.2 rad
  plant_kernel_{terrain,field_level,field_rolling}_substeps{1,4}_ms   (--field) the field instantiation beside the
                                  plane one: a level terrain row, a level 33 x 25 tile per robot (the same motion,
                                  so the two differ by their code alone), and the fleet standing on one shared tile
                                  of rolling ground (3 cm amplitude, 5 cm cells) at random places and headings
  tick_graph_mpc_plant            ControlTick(plant=), MPC-only and truth-fed, closing its own loop
  tick_graph_mpc                  the same tick object captured without its last stage (what the tick enqueued
                                  before the stage existed).  Each repetition snapshots every buffer of the tick,
                                  replays this graph, restores the snapshot and replays the closed graph, so the
                                  two replays of a pair do the same work from the same slots but for the stage
                                  (the solver handle's launch-order hint is the one state not restored)
  tick_graph_full_plant / _full   the same pair for command + estimator + plan + MPC

The stage's share of the tick is the median of the 20 paired differences over the median tick without it;
each form also prints the quartiles and extremes of its 20 repetitions.
usage: python tools/time_plant.py [--batch 4096] [--kernels-only] [--flat-only] [--field]
(--kernels-only: the plant kernel's lines alone; --flat-only: without the terrain instantiations, for an A/B against a
library from before they existed, given by MPCQP_LIB; --field: the lines of the field instantiation alone)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "go1-qp-mpc-controller_amd"), os.path.join(REPO, "tests"),
                os.path.join(REPO, "tools")]
import mpcqp  # noqa: E402
from mpcqp import _lib  # noqa: E402
from mpcqp.tick import ControlTick  # noqa: E402
from rollout import DT, caller_rows, start_rows  # noqa: E402
from test_torques import torque_inputs  # noqa: E402  (synthetic Jacobians)
from time_command import paired_tick_ms  # noqa: E402
from time_estimator import RUNS, WARMUP, median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--flat-only", action="store_true")
    ap.add_argument("--field", action="store_true")
    args = ap.parse_args()
    B = args.batch
    f64 = dict(dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"batch": B, "warmup": WARMUP, "runs": RUNS}

    # ---- the kernel alone ----
    def plant_alone(substeps, stance, wrench=False, terrain=None, field=None):
        """terrain: None, "level" or "slope"; with either the launch goes through the terrain entry point.
        field: None, "level" or "rolling"; with either the launch goes through the field entry point."""
        pp = mpcqp.default_plant_params(substeps=substeps)
        slot = torch.zeros((B, mpcqp.plant_state_size()), **f64)
        rows = {n: torch.zeros((B, w), **f64) for n, w in (("sn", _lib.SN_SIZE), ("pl", _lib.PL_SIZE),
                                                           ("st", _lib.ST_SIZE), ("tq", _lib.TQ_SIZE),
                                                           ("po", _lib.PT_SIZE))}
        tau = torch.zeros((B, 12), **f64)
        init = None
        if not stance:
            pos = np.tile([0.0, 0.0, 100.0], (B, 1))
            init = torch.from_numpy(mpcqp.pack_plant_init(pos, np.tile([1.0, 0, 0, 0], (B, 1)),
                                                          np.tile(list(pp.default_joint_pos), (B, 1)))).cuda()

        wr = torch.zeros((B, mpcqp.disturb.PW_SIZE), **f64) if wrench else None
        tr = None
        if terrain is not None:
            rng = np.random.default_rng(5)
            a = 0.2 if terrain == "slope" else 0.0
            t_rows = mpcqp.terrain_from_slope(rng.uniform(-a, a, B), rng.uniform(-a, a, B), pp.mu)
            flat, _ = start_rows(B, list(pp.default_joint_pos)[:3], 0.0, 2)
            init = torch.from_numpy(mpcqp.place_on_terrain(flat, t_rows)[0]).cuda()
            tr = torch.from_numpy(t_rows).cuda()
        hf = None
        if field is not None:
            rng = np.random.default_rng(5)
            x = (-0.8 + 0.05 * np.arange(33))[None, :] + np.zeros((25, 1))
            y = (-0.6 + 0.05 * np.arange(25))[:, None] + np.zeros((1, 33))
            tile = 0.03 * np.sin(2 * np.pi * x / 0.9 + 0.4) * np.cos(2 * np.pi * y / 1.3 - 0.2)
            if field == "level":  # a tile of its own per robot, as every robot has a terrain row of its own
                f_rows, heights = mpcqp.pack_height_field([0.0 * tile] * B, -0.8, -0.6, 0.05, pp.mu)
            else:
                f_rows, heights = mpcqp.pack_height_field([tile], -0.8, -0.6, 0.05, pp.mu, share=np.zeros(B, int))
            flat, _ = start_rows(B, list(pp.default_joint_pos)[:3], 0.0, 2)
            if field == "rolling":
                flat[:, :2] = rng.uniform(-0.3, 0.3, (B, 2))
            init = torch.from_numpy(mpcqp.place_on_field(flat, f_rows, heights, np.arange(B), pp)[0]).cuda()
            hf = (torch.from_numpy(f_rows).cuda(), torch.from_numpy(heights).cuda())
        ptr = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
        out_rows = (rows["sn"].data_ptr(), rows["pl"].data_ptr(), rows["st"].data_ptr(), rows["tq"].data_ptr(),
                    rows["po"].data_ptr(), stream)

        def step():
            if hf is not None:
                mpcqp.plant_step_field_device(pp, DT, tau.data_ptr(), ptr(wr), hf[0].data_ptr(), B, hf[1].data_ptr(),
                                              hf[1].numel(), 0, B, slot.data_ptr(), ptr(init), *out_rows)
            elif tr is not None:
                mpcqp.plant_step_terrain_device(pp, DT, tau.data_ptr(), ptr(wr), tr.data_ptr(), B, 0, B,
                                                slot.data_ptr(), ptr(init), *out_rows)
            elif wr is not None:
                mpcqp.plant_step_wrench_device(pp, DT, tau.data_ptr(), wr.data_ptr(), B, slot.data_ptr(), ptr(init),
                                               *out_rows)
            else:
                mpcqp.plant_step_device(pp, DT, tau.data_ptr(), B, slot.data_ptr(), ptr(init), *out_rows)

        step()  # initialise
        torch.cuda.synchronize()
        if stance:  # tau = J^T (-R^T (0, 0, m g / 4)), held for the 23 timed ticks (R = 1 on level ground)
            J = rows["tq"][:, _lib.TQ_JFOOT:_lib.TQ_JFOOT + 36].reshape(B, 4, 3, 3)
            R = rows["st"][:, _lib.ST_ROT:_lib.ST_ROT + 9].reshape(B, 3, 3)
            fb = R[:, 2, :] * (pp.mass * pp.gravity / 4.0)  # R^T e_z
            tau.copy_((-torch.einsum("blji,bj->bli", J, fb)).reshape(B, 12))
        ms = median_ms(step)
        po = rows["po"].cpu().numpy()
        assert np.all(po[:, _lib.PT_STATUS] == 0.0)
        assert np.all(po[:, _lib.PT_CONTACTS:_lib.PT_CONTACTS + 4] == (1.0 if stance else 0.0))
        return ms

    if args.field:
        for n in (1, 4):
            out[f"plant_kernel_terrain_substeps{n}_ms"] = plant_alone(n, True, terrain="level")
            out[f"plant_kernel_field_level_substeps{n}_ms"] = plant_alone(n, True, field="level")
            out[f"plant_kernel_field_rolling_substeps{n}_ms"] = plant_alone(n, True, field="rolling")
            out[f"plant_kernel_wrench_terrain_substeps{n}_ms"] = plant_alone(n, True, wrench=True, terrain="level")
            out[f"plant_kernel_wrench_field_level_substeps{n}_ms"] = plant_alone(n, True, wrench=True, field="level")
        print(json.dumps(out))
        return
    out["plant_kernel_substeps1_ms"] = plant_alone(1, True)
    out["plant_kernel_substeps4_ms"] = plant_alone(4, True)
    out["plant_kernel_swing_substeps4_ms"] = plant_alone(4, False)
    out["plant_kernel_wrench_substeps4_ms"] = plant_alone(4, True, wrench=True)
    if not args.flat_only:
        out["plant_kernel_terrain_substeps4_ms"] = plant_alone(4, True, terrain="level")
        out["plant_kernel_wrench_terrain_substeps4_ms"] = plant_alone(4, True, wrench=True, terrain="level")
        out["plant_kernel_slope_substeps4_ms"] = plant_alone(4, True, terrain="slope")
    if args.kernels_only:
        print(json.dumps(out))
        return

    # ---- the two neighbours it shares its thread mapping with ----
    J, fkin, contacts, f_grf = torque_inputs(B, 1)
    tq = torch.from_numpy(mpcqp.assemble_torque_records(J, fkin, contacts)).cuda()
    res = np.zeros(B, dtype=mpcqp.RESULT_DTYPE)
    res["f_body"] = f_grf
    d_res = torch.from_numpy(res.view(np.float64).reshape(B, -1).copy()).cuda()
    counter = torch.full((B,), 100, dtype=torch.int32, device="cuda")
    tau = torch.zeros((B, 12), **f64)
    out["torque_kernel_ms"] = median_ms(
        lambda: mpcqp.joint_torques_device(tq.data_ptr(), d_res.data_ptr(), B, counter.data_ptr(), tau.data_ptr(), stream))
    plp = mpcqp.default_plan_params()
    st0 = torch.from_numpy(mpcqp.pack_states(mpcqp.synthetic_go1(B, seed=3, gait="stance"))).cuda()
    pin = torch.from_numpy(mpcqp.pack_plan_inputs(np.tile(np.eye(3), (B, 1, 1)), np.full((B, 4), 30.0), 1)).cuda()
    pslot = torch.zeros((B, mpcqp.plan_state_size()), **f64)
    pout = torch.zeros((B, _lib.PO_SIZE), **f64)
    out["plan_kernel_ms"] = median_ms(
        lambda: mpcqp.leg_plan_device(plp, plp.control_dt, st0.data_ptr(), pin.data_ptr(), B, pslot.data_ptr(),
                                      tq.data_ptr(), pout.data_ptr(), stream))

    # ---- the graph-replayed tick with and without the stage ----
    def pair(full):
        kw = dict(plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                  command=mpcqp.default_command_params()) if full else {}
        init, e = start_rows(B, [0.0, 0.8, -1.6], 0.05, 2)
        k = ControlTick(B, dt=DT, plant=mpcqp.default_plant_params(), plant_init=init, **kw)
        caller_rows(k, B, init[:, :3], e[:, 2], full)
        k.prime_plant()
        try:
            return paired_tick_ms(k, ("plant",), 12)  # past the torque map's zero-torque ticks
        finally:
            k.close()

    for name, full in (("mpc", False), ("full", True)):
        w, wo, d = pair(full)
        out[f"tick_graph_{name}_plant"], out[f"tick_graph_{name}"], out[f"tick_graph_{name}_paired_diff"] = w, wo, d
        out[f"plant_share_of_{name}_tick"] = d["median_ms"] / wo["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
