#!/usr/bin/env python3
"""Cost of one ADMM iteration of the product build, without instrumentation: fixed-work solves
(tools/iter_cost.py's settings: eps 0, adaptive rho off, so every robot runs exactly max_iter
iterations and one factorization) at two iteration counts, timed with HIP events on the solve's
stream.  The difference over the iteration difference is the batch's time per iteration (1/25 of a
termination check included); with every robot doing the same work the SIMD slots stay full, so
cycles per robot and iteration = that time x the shader clock x slots / batch.  Phase-timing builds
(-DMPCQP_PHASE_TIMING) are scheduled and spilled differently from the product; this is the figure to
compare two product libraries by (MPCQP_LIB).

  python tools/iter_time.py [--iters 100 200] [--batch 4096] [--reps 7] [--ghz 2.19] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go1-qp-mpc-controller_amd"))
import mpcqp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, nargs=2, default=[100, 200])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ghz", type=float, default=2.19, help="shader clock under this load (wave_phases.py shader_ghz)")
    ap.add_argument("--slots", type=int, default=1024, help="waves in flight: 256 CUs x 4 SIMDs x 1 wave")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    st = mpcqp.synthetic_go1(a.batch, seed=1000, gait="trot")
    recs = mpcqp.assemble_compute_grf(st, a.horizon)
    d_rec = torch.from_numpy(recs).cuda()
    d_res = torch.zeros((a.batch, mpcqp._lib.RESULT_DOUBLES), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream()
    ms = {}
    for it in a.iters:
        p = mpcqp.default_params(a.horizon, max_iter=it, eps_abs=0.0, eps_rel=0.0, adaptive_rho=0,
                                 eps_prim_inf=0.0, eps_dual_inf=0.0)
        with mpcqp.MpcQpSolver(p) as s:
            t = []
            for rep in range(a.reps + 2):  # two warm-up solves (the second has the launch-order hint's key)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                s.solve_device(d_rec.data_ptr(), a.batch, d_res.data_ptr(), 0, stream.cuda_stream)
                e1.record(stream)
                torch.cuda.synchronize()
                if rep >= 2:
                    t.append(e0.elapsed_time(e1))
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE)
        assert np.all(res["iters"] == it) and np.all(res["rho_updates"] == 0), "not a fixed-work solve"
        ms[it] = t
    lo, hi = a.iters
    per_iter_us = (np.median(ms[hi]) - np.median(ms[lo])) / (hi - lo) * 1e3
    out = {"lib": os.path.basename(mpcqp._lib.LIB_PATH), "batch": a.batch, "horizon": a.horizon,
           "ms": {str(k): [round(x, 4) for x in v] for k, v in ms.items()},
           "median_ms": {str(k): float(np.median(v)) for k, v in ms.items()},
           "batch_us_per_iteration": float(per_iter_us),
           "cycles_per_robot_iteration": float(per_iter_us * 1e-6 * a.ghz * 1e9 * a.slots / a.batch)}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
