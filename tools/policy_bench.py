#!/usr/bin/env python3
"""Time the policy stage (mpcqp_policy_device) against the same computation written in torch.

  python tools/policy_bench.py [--batches 4096 65536] [--launches 50] [--warmup 10] [--out profiles/policy/bench.json]

Per batch size, all robots walking, decimation 1, seeded weights of the reference's widths (48-512-256-128-12):
  fused        one mpcqp_policy_device launch (observation, MLP, clip, targets, slot, torque)
  torch_eager  fp32 linear / elu plus the elementwise pre- and post-processing as torch ops on the same device:
               what a user would have without the stage
  torch_graph  the same, captured in a graph and replayed
Each is the median of --launches timings with device events after --warmup untimed ones.  The achieved fraction
of the f32 matrix peak counts 2 FLOP for each of the 189,952 weights per robot against 157 TFLOP/s.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go1-qp-mpc-controller_amd"))

HIDDEN = (512, 256, 128)
PEAK_F32_MATRIX = 157e12


def seeded_weights(seed):
    rng = np.random.default_rng(seed)
    dims = [48] + list(HIDDEN) + [12]
    ws, bs = [], []
    for i, o in zip(dims[:-1], dims[1:]):
        a = 1.0 / np.sqrt(i)
        ws.append(rng.uniform(-a, a, (o, i)).astype(np.float32))
        bs.append(rng.uniform(-a, a, (o,)).astype(np.float32))
    return ws, bs


def timed(torch, fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "policy", "bench.json"))
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F

    import mpcqp
    from mpcqp import _lib

    dev = "cuda:0"
    ws, bs = seeded_weights(0)
    pp = mpcqp.default_policy_params()
    flop_per_robot = 2 * sum(w.size for w in ws)
    results = []
    with mpcqp.Policy(ws, bs, pp) as pol:
        tw = [torch.from_numpy(w).to(dev) for w in ws]
        tb = [torch.from_numpy(b).to(dev) for b in bs]
        c64 = lambda a: torch.tensor(list(a), dtype=torch.float64, device=dev)
        scale, dflt = c64(pp.obs_scale), c64(pp.default_joint_pos)
        lo, hi, kp, kd = c64(pp.pose_lower), c64(pp.pose_upper), c64(pp.kp_walk), c64(pp.kd_walk)
        for B in args.batches:
            rng = np.random.default_rng(B)
            f64 = dict(dtype=torch.float64, device=dev)
            sn = torch.from_numpy(rng.normal(0, 1, (B, _lib.SN_SIZE))).to(dev)
            st = torch.from_numpy(rng.normal(0, 1, (B, _lib.ST_SIZE))).to(dev)
            pl = torch.from_numpy(rng.normal(0, 1, (B, _lib.PL_SIZE))).to(dev)
            cm = torch.from_numpy(rng.normal(0, 1, (B, _lib.CM_SIZE))).to(dev)
            pl[:, _lib.PL_MOVEMENT_MODE] = 1.0
            slot = torch.zeros((B, mpcqp.policy_state_size()), **f64)
            tau = torch.zeros((B, 12), **f64)
            stream = torch.cuda.current_stream().cuda_stream

            def fused():
                mpcqp.policy_device(pol, sn.data_ptr(), st.data_ptr(), pl.data_ptr(), cm.data_ptr(), B, slot.data_ptr(),
                                    tau.data_ptr(), 0, 0, 2, stream)

            prev = torch.zeros((B, 12), **f64)
            tau_t = torch.zeros((B, 12), **f64)

            def torch_tick():
                rz = pl[:, _lib.PL_ROT_Z:_lib.PL_ROT_Z + 9].view(B, 3, 3)
                rm = st[:, _lib.ST_ROT:_lib.ST_ROT + 9].view(B, 3, 3)
                q = sn[:, _lib.SN_JOINT_POS:_lib.SN_JOINT_POS + 12]
                dq = sn[:, _lib.SN_JOINT_VEL:_lib.SN_JOINT_VEL + 12]
                ob = torch.cat([
                    torch.einsum("bki,bk->bi", rz, st[:, _lib.ST_LIN_VEL:_lib.ST_LIN_VEL + 3]),
                    sn[:, _lib.SN_IMU_ANG_VEL:_lib.SN_IMU_ANG_VEL + 3], -rm[:, 2, :],
                    cm[:, _lib.CM_VEL:_lib.CM_VEL + 2], cm[:, _lib.CM_RATE + 2:_lib.CM_RATE + 3], q - dflt, dq], dim=1)
                ob = torch.clamp(ob * scale, -pp.clip_obs, pp.clip_obs)
                h = torch.cat([ob, prev], dim=1).to(torch.float32)
                for l in range(len(tw)):
                    h = F.linear(h, tw[l], tb[l])
                    if l + 1 < len(tw):
                        h = F.elu(h)
                act = torch.clamp(h.to(torch.float64), -pp.clip_action, pp.clip_action)
                prev.copy_(act)
                tgt = torch.minimum(torch.maximum(act * pp.action_scale + dflt, lo), hi)
                tau_t.copy_(kp * (tgt - q) - kd * dq)

            row = dict(batch=B, launches=args.launches, warmup=args.warmup)
            row["fused_ms"], row["fused_min_ms"] = timed(torch, fused, args.launches, args.warmup)
            row["torch_eager_ms"], row["torch_eager_min_ms"] = timed(torch, torch_tick, args.launches, args.warmup)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                torch_tick()
            row["torch_graph_ms"], row["torch_graph_min_ms"] = timed(torch, g.replay, args.launches, args.warmup)
            row["fused_tflops"] = flop_per_robot * B / (row["fused_ms"] * 1e-3) / 1e12
            row["fused_fraction_of_f32_matrix_peak"] = flop_per_robot * B / (row["fused_ms"] * 1e-3) / PEAK_F32_MATRIX
            row["fused_over_torch_graph"] = row["fused_ms"] / row["torch_graph_ms"]
            results.append(row)
            print(json.dumps(row), flush=True)
    doc = dict(what="mpcqp_policy_device vs torch fp32 linear/elu + elementwise, median ms of HIP-event timings",
               device=torch.cuda.get_device_name(0), hidden=list(HIDDEN), flop_per_robot=flop_per_robot,
               peak_f32_matrix_tflops=PEAK_F32_MATRIX / 1e12, results=results)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
