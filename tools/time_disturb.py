"""Time of the disturbance stage (mpcqp_disturb_device) and of the plant kernel with a wrench row beside the plant and
the episode kernel, and of the graph-replayed control tick with and without the stage (HIP events, 3 warm-up runs,
median of 20, all in one session):

  plant_kernel_substeps4_ms    the yardsticks of tools/time_episode.py: one launch of the plant stage on a standing
  episode_running_ms           fleet, and one of the episode stage with every robot running
  disturb_all_ms               one launch, every robot running, pushes, load, biases and noise on: 13 Philox blocks
                               per lane, 36 doubles read and 68 written per robot
  disturb_wrench_only_ms       the truth-fed tick's call: no sensor rows, no output row
  disturb_off_ms               the default (all-off) params on the same buffers
  plant_wrench_substeps4_ms    the plant kernel's wrench instantiation under the rows disturb_all wrote
  plant_wrench_zero_substeps4_ms   the same under an all-zero wrench row
  tick_graph_{mpc,full}_disturb / tick_graph_{mpc,full}
                               the paired comparison of tools/time_episode.py: the same tick object captured with and
                               without the stage (without it the estimator reads the clean sensor row and the plant
                               runs without a wrench); each repetition snapshots every buffer, replays one graph,
                               restores the snapshot and replays the other
usage: python tools/time_disturb.py [--batch 4096]"""
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
from mpcqp import disturb as md  # noqa: E402
from mpcqp import episode as me  # noqa: E402
from mpcqp.tick import ControlTick  # noqa: E402
from rollout import DT, caller_rows, episode_pool, full_stance  # noqa: E402
from time_command import paired_tick_ms  # noqa: E402
from time_estimator import RUNS, WARMUP, median_ms  # noqa: E402


def all_on(**over):
    kw = dict(load_mass_max=3.0, load_point=[0.1, 0.05, 0.02], bias_acc=0.05, bias_gyro=0.01, push_force=[10.0, 40.0],
              push_point=[0.1, 0.05, 0.03], sigma=[0.002, 0.05, 0.05, 0.01], seed=11, push_start=0, push_interval=4,
              push_duration=2, dir_count=16)
    kw.update(over)
    return mpcqp.default_disturb_params(**kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    B = ap.parse_args().batch
    f64 = dict(dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    out = {"batch": B, "warmup": WARMUP, "runs": RUNS}

    # ---- the yardsticks: the plant kernel on a standing fleet and the episode kernel with every robot running ----
    pp = mpcqp.default_plant_params(substeps=4)
    slot = torch.zeros((B, mpcqp.plant_state_size()), **f64)
    rows = {n: torch.zeros((B, w), **f64) for n, w in (("sn", _lib.SN_SIZE), ("pl", _lib.PL_SIZE), ("st", _lib.ST_SIZE),
                                                       ("tq", _lib.TQ_SIZE), ("po", _lib.PT_SIZE))}
    tau = torch.zeros((B, 12), **f64)
    wrench = torch.zeros((B, md.PW_SIZE), **f64)

    def plant(w=0):
        args = (B, slot.data_ptr(), 0, rows["sn"].data_ptr(), rows["pl"].data_ptr(), rows["st"].data_ptr(),
                rows["tq"].data_ptr(), rows["po"].data_ptr(), stream)
        if w:
            mpcqp.plant_step_wrench_device(pp, DT, tau.data_ptr(), w, *args)
        else:
            mpcqp.plant_step_device(pp, DT, tau.data_ptr(), *args)

    plant()
    torch.cuda.synchronize()
    J = rows["tq"][:, _lib.TQ_JFOOT:_lib.TQ_JFOOT + 36].reshape(B, 4, 3, 3)
    tau.copy_((-J[:, :, 2, :] * (pp.mass * pp.gravity / 4.0)).reshape(B, 12))
    start = slot.clone()
    out["plant_kernel_substeps4_ms"] = median_ms(plant)
    assert np.all(rows["po"].cpu().numpy()[:, _lib.PT_STATUS] == 0.0)

    es = torch.zeros((B, me.ES_SIZE), **f64)
    tot, log = torch.zeros((B, me.ET_SIZE), **f64), torch.zeros((B, 4, me.EL_SIZE), **f64)
    init = torch.zeros((B, _lib.PI_SIZE), **f64)
    ep = mpcqp.default_episode_params(max_ticks=1 << 30, seed=11)
    s2, t2 = slot.clone(), tau.clone()  # the stage zero-fills these on the fresh robots' first tick
    ebf = mpcqp.episode_buffers(rows["po"].data_ptr(), s2.data_ptr(), init.data_ptr(), t2.data_ptr(),
                                rows["sn"].data_ptr(), d_log=log.data_ptr(), d_totals=tot.data_ptr())

    def episode():
        mpcqp.episode_device(ep, ebf, B, es.data_ptr(), stream)

    episode()
    episode()  # fresh, priming: every robot runs from here on
    torch.cuda.synchronize()
    out["episode_running_ms"] = median_ms(episode)
    assert np.all(es.cpu().numpy()[:, 0] == 1.0)

    # ---- the stage alone, on the running fleet's episode slots and sensor rows ----
    dirs = torch.from_numpy(mpcqp.pack_push_dirs(16)).cuda()
    noisy, dout = torch.zeros((B, _lib.SN_SIZE), **f64), torch.zeros((B, md.DO_SIZE), **f64)
    full_bf = mpcqp.disturb_buffers(es.data_ptr(), wrench.data_ptr(), rows["sn"].data_ptr(), noisy.data_ptr(),
                                    dirs.data_ptr(), dout.data_ptr())
    bare_bf = mpcqp.disturb_buffers(es.data_ptr(), wrench.data_ptr(), d_dirs=dirs.data_ptr())
    on, off = all_on(), mpcqp.default_disturb_params()
    out["disturb_wrench_only_ms"] = median_ms(lambda: mpcqp.disturb_device(on, bare_bf, B, stream))
    out["disturb_off_ms"] = median_ms(lambda: mpcqp.disturb_device(off, full_bf, B, stream))
    out["disturb_all_ms"] = median_ms(lambda: mpcqp.disturb_device(on, full_bf, B, stream))
    moved = 8 * B * (3 + _lib.SN_SIZE + md.PW_SIZE + _lib.SN_SIZE + md.DO_SIZE)
    out["disturb_all_bytes"] = moved
    out["disturb_all_TB_per_s"] = moved / (out["disturb_all_ms"] * 1e-3) / 1e12
    o = dout.cpu().numpy()
    out["disturb_all_pushed_share"] = float(o[:, md.DO_PUSH_ACTIVE].mean())
    assert o[:, md.DO_LOAD_FORCE].min() > 0.0 and not torch.equal(noisy, rows["sn"])

    # ---- the plant kernel with the wrench row, from the same standing state ----
    slot.copy_(start)
    out["plant_wrench_substeps4_ms"] = median_ms(lambda: plant(wrench.data_ptr()))
    out["plant_wrench_status_nonzero"] = int((rows["po"].cpu().numpy()[:, _lib.PT_STATUS] != 0.0).sum())
    slot.copy_(start)
    zero = torch.zeros_like(wrench)
    out["plant_wrench_zero_substeps4_ms"] = median_ms(lambda: plant(zero.data_ptr()))
    slot.copy_(start)
    out["plant_kernel_substeps4_again_ms"] = median_ms(plant)

    # ---- the graph-replayed tick with and without the stage ----
    def pair(full):
        kw = dict(plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                  command=mpcqp.default_command_params()) if full else {}
        q, h = full_stance() if full else ([0.0, 0.8, -1.6], None)
        k = ControlTick(B, dt=DT, plant=mpcqp.default_plant_params(), episode=mpcqp.default_episode_params(seed=5),
                        episode_pool=episode_pool(8, q, 0.05, 2, h), disturb=all_on(push_interval=200, push_duration=20),
                        disturb_dirs=mpcqp.pack_push_dirs(16), **kw)
        caller_rows(k, B, np.zeros((B, 3)), np.zeros(B), full)
        try:
            # the fresh and the priming tick, then past the torque map\'s zero-torque ticks
            return paired_tick_ms(k, ("disturb",), 14)
        finally:
            k.close()

    for name, full in (("mpc", False), ("full", True)):
        w, wo, d = pair(full)
        out[f"tick_graph_{name}_disturb"], out[f"tick_graph_{name}"], out[f"tick_graph_{name}_paired_diff"] = w, wo, d
        out[f"disturb_share_of_{name}_tick"] = d["median_ms"] / wo["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
