"""Time of the episode stage (mpcqp_episode_device) beside the plant kernel, and of the graph-replayed control tick
with and without it (HIP events, 3 warm-up runs, median of 20, all in one session):

  plant_kernel_substeps4_ms   the yardstick: one launch of the plant stage on a standing fleet
  episode_running_ms          (a) one launch, every robot running: metrics, end tests, the script test
  episode_restarting_ms       (b) one launch in which every robot restarts: max_ticks = 1 and half of the fleet one
                              tick ahead of the other, so each launch ends one half (log row, totals, draw, plant
                              slot, torque row and init row) and primes the other (every controller slot, the result
                              row and the counter zero-filled).  With the bytes one such launch moves this gives
                              the achieved rate.
  tick_graph_{mpc,full}_episode / tick_graph_{mpc,full}
                              the paired comparison of tools/time_plant.py: the same tick object captured with and
                              without its last stage; each repetition snapshots every buffer, replays one graph,
                              restores the snapshot and replays the other
usage: python tools/time_episode.py [--batch 4096]"""
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
from mpcqp import episode as me  # noqa: E402
from mpcqp.tick import ControlTick  # noqa: E402
from rollout import DT, caller_rows, episode_pool, full_stance  # noqa: E402
from time_command import paired_tick_ms  # noqa: E402
from time_estimator import RUNS, WARMUP, median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    B = ap.parse_args().batch
    T = WARMUP + RUNS
    f64 = dict(dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"batch": B, "warmup": WARMUP, "runs": RUNS}

    # ---- the yardstick: the plant kernel on a standing fleet, as tools/time_plant.py ----
    pp = mpcqp.default_plant_params(substeps=4)
    slot = torch.zeros((B, mpcqp.plant_state_size()), **f64)
    rows = {n: torch.zeros((B, w), **f64) for n, w in (("sn", _lib.SN_SIZE), ("pl", _lib.PL_SIZE), ("st", _lib.ST_SIZE),
                                                       ("tq", _lib.TQ_SIZE), ("po", _lib.PT_SIZE))}
    tau = torch.zeros((B, 12), **f64)

    def plant():
        mpcqp.plant_step_device(pp, DT, tau.data_ptr(), B, slot.data_ptr(), 0, rows["sn"].data_ptr(),
                                rows["pl"].data_ptr(), rows["st"].data_ptr(), rows["tq"].data_ptr(),
                                rows["po"].data_ptr(), stream)

    plant()
    torch.cuda.synchronize()
    J = rows["tq"][:, _lib.TQ_JFOOT:_lib.TQ_JFOOT + 36].reshape(B, 4, 3, 3)
    tau.copy_((-J[:, :, 2, :] * (pp.mass * pp.gravity / 4.0)).reshape(B, 12))
    out["plant_kernel_substeps4_ms"] = median_ms(plant)
    assert np.all(rows["po"].cpu().numpy()[:, _lib.PT_STATUS] == 0.0)

    # ---- the stage alone, on the plant's rows and slots of the tick's sizes ----
    solver = mpcqp.MpcQpSolver(_lib.default_params(10))
    sizes = dict(est_state=mpcqp.estimator_state_size(), plan_state=mpcqp.plan_state_size(),
                 cmd_state=mpcqp.command_state_size(), policy_state=mpcqp.policy_state_size(),
                 warm=solver.warm_state_size)
    solver.close()
    out["slot_doubles"] = sizes
    pool = torch.from_numpy(episode_pool(8, [0.0, 0.8, -1.6], 0.05, 3)).cuda()
    scripts = torch.from_numpy(mpcqp.pack_episode_scripts([[(0, (0, 0, 0), (0, 0, 0), False)]])).cuda()

    def stage(max_ticks):
        t = {n: torch.full((B, w), 1.0, **f64) for n, w in sizes.items()}
        t.update(es=torch.zeros((B, me.ES_SIZE), **f64), init=torch.zeros((B, _lib.PI_SIZE), **f64),
                 cmd=torch.zeros((B, _lib.CM_SIZE), **f64), res=torch.zeros((B, _lib.RESULT_DOUBLES), **f64),
                 st=torch.zeros((B, _lib.ST_SIZE), **f64), counter=torch.zeros((B,), dtype=torch.int32, device="cuda"),
                 log=torch.zeros((B, 4, me.EL_SIZE), **f64), tot=torch.zeros((B, me.ET_SIZE), **f64),
                 slot=slot.clone(), tau=tau.clone())
        ep = mpcqp.default_episode_params(max_ticks=max_ticks, pool_count=pool.shape[0], script_count=1,
                                          script_segments=1, seed=11)
        bf = mpcqp.episode_buffers(
            rows["po"].data_ptr(), t["slot"].data_ptr(), t["init"].data_ptr(), t["tau"].data_ptr(),
            rows["sn"].data_ptr(), t["cmd"].data_ptr(), t["res"].data_ptr(), pool.data_ptr(), scripts.data_ptr(),
            t["st"].data_ptr(), t["counter"].data_ptr(), t["log"].data_ptr(), t["tot"].data_ptr(),
            t["est_state"].data_ptr(), sizes["est_state"], t["plan_state"].data_ptr(), sizes["plan_state"],
            t["cmd_state"].data_ptr(), sizes["cmd_state"], t["policy_state"].data_ptr(), sizes["policy_state"],
            t["warm"].data_ptr(), sizes["warm"])
        return t, lambda: mpcqp.episode_device(ep, bf, B, t["es"].data_ptr(), stream)

    t, run = stage(1 << 30)
    run()
    run()  # fresh, priming: every robot runs from here on
    torch.cuda.synchronize()
    out["episode_running_ms"] = median_ms(run)
    es = t["es"].cpu().numpy()
    assert np.all(es[:, 0] == 1.0) and np.all(es[:, 1] == T)

    t, run = stage(1)
    t["es"][1::2, 0] = 2.0  # the odd robots one tick ahead: priming while the even ones end
    run()
    torch.cuda.synchronize()
    out["episode_restarting_ms"] = median_ms(run)
    tot = t["tot"].cpu().numpy()
    assert np.all(tot[:, 0] >= T // 2 - 1)  # episodes completed
    zeroed = sum(sizes.values()) + _lib.RESULT_DOUBLES
    priming = 8 * (zeroed + 12 + 2 * me.ES_SIZE + _lib.PT_SIZE + 8 + 6) + 4
    ending = 8 * (_lib.PN_SIZE + 12 + 2 * _lib.PI_SIZE + me.EL_SIZE + 2 * me.ET_SIZE + 2 * me.ES_SIZE + _lib.PT_SIZE +
                  12 + 12 + 3 + 1)
    out["bytes_per_priming_robot"], out["bytes_per_ending_robot"] = priming, ending
    moved = (B // 2) * (priming + ending)
    out["episode_restarting_bytes"] = moved
    out["episode_restarting_TB_per_s"] = moved / (out["episode_restarting_ms"] * 1e-3) / 1e12

    # ---- the graph-replayed tick with and without the stage ----
    def pair(full):
        kw = dict(plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                  command=mpcqp.default_command_params()) if full else {}
        q, h = full_stance() if full else ([0.0, 0.8, -1.6], None)
        k = ControlTick(B, dt=DT, plant=mpcqp.default_plant_params(), episode=mpcqp.default_episode_params(seed=5),
                        episode_pool=episode_pool(8, q, 0.05, 2, h), **kw)
        caller_rows(k, B, np.zeros((B, 3)), np.zeros(B), full)
        try:
            # the fresh and the priming tick, then past the torque map\'s zero-torque ticks
            return paired_tick_ms(k, ("episode",), 14)
        finally:
            k.close()

    for name, full in (("mpc", False), ("full", True)):
        w, wo, d = pair(full)
        out[f"tick_graph_{name}_episode"], out[f"tick_graph_{name}"], out[f"tick_graph_{name}_paired_diff"] = w, wo, d
        out[f"episode_share_of_{name}_tick"] = d["median_ms"] / wo["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
