#!/usr/bin/env python3
"""A/B of the launch-order hint (mpcqp_set_order_hint) on records that change every call: B robots
over T consecutive ticks of synthetic_go1_ticks (seed 31) at swing_ticks 5 and 40, solved cold
(mpcqp_solve_batch_device) and warm-started (mpcqp_solve_batch_warm_device), the hint off and on
alternated in one process on one handle.  Every tick is timed with HIP events on the solve's stream;
tick 0 (first call: no previous cost, cold warm slots) is dropped and a sequence's figure is the
median per-tick ms.  REPS repetitions per setting.

A path (cold, warm) earns the hint as its default only where the median with the hint beats the
median without it by more than the max - min spread of the hint-off repetitions.  bench.py's timed
loop re-solves one batch, where the hint is perfect: this tool measures what a controller gets.

  python tools/order_hint_ab.py [--batch 4096] [--ticks 40] [--reps 3] [--out FILE]
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
from mpcqp.records import synthetic_go1_ticks  # noqa: E402

RD = mpcqp._lib.RESULT_DOUBLES


def run_sequence(s, d_t, d_res, warm, hint):
    """Per-tick ms of one pass over the ticks (fresh warm slots), and the mean iterations of ticks 1.."""
    T, B = d_t.shape[0], d_t.shape[1]
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    s.set_order_hint(hint)
    d_w = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda") if warm else None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(T + 1)]
    torch.cuda.synchronize()
    ev[0].record(stream)
    for t in range(T):
        if warm:
            s.solve_warm_device(d_t[t].data_ptr(), B, d_w.data_ptr(), d_res[t].data_ptr(), 0, sp)
        else:
            s.solve_device(d_t[t].data_ptr(), B, d_res[t].data_ptr(), 0, sp)
        ev[t + 1].record(stream)
    torch.cuda.synchronize()
    ms = np.array([ev[t].elapsed_time(ev[t + 1]) for t in range(T)])
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE).reshape(T, B)
    return ms, float(res[1:]["iters"].mean()), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--swing", type=int, nargs="*", default=[5, 40])
    ap.add_argument("--split", type=int, default=0, help="mpcqp_debug_set_split (0 = auto)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    B, N, T = a.batch, a.horizon, a.ticks
    out = {"batch": B, "horizon": N, "ticks": T, "reps": a.reps, "split": a.split, "cases": []}
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        s.reserve(B)
        s.set_split(a.split)
        for swing in a.swing:
            ticks = synthetic_go1_ticks(B, T, seed=31, gait="trot", swing_ticks=swing)
            d_t = torch.from_numpy(np.stack([mpcqp.assemble_compute_grf(x, N) for x in ticks])).cuda()
            d_res = torch.zeros((T, B, RD), dtype=torch.float64, device="cuda")
            for warm in (False, True):
                run_sequence(s, d_t, d_res, warm, 0)  # warm-up of the process, untimed
                med = {0: [], 1: []}
                ref = None
                for _ in range(a.reps):
                    for hint in (0, 1):
                        ms, iters, res = run_sequence(s, d_t, d_res, warm, hint)
                        med[hint].append(float(np.median(ms[1:])))
                        if ref is None:
                            ref = res.tobytes()
                        elif res.tobytes() != ref:
                            raise SystemExit(f"swing {swing} warm {warm} hint {hint}: results differ")
                off, on = float(np.median(med[0])), float(np.median(med[1]))
                spread = max(med[0]) - min(med[0])
                case = {"swing_ticks": swing, "path": "warm" if warm else "cold", "mean_iters": iters,
                        "off_ms": med[0], "on_ms": med[1], "off_median_ms": off, "on_median_ms": on,
                        "off_spread_ms": spread, "gain_ms": off - on, "gain_pct": 100.0 * (off - on) / off,
                        "hint_wins": bool(off - on > spread)}
                out["cases"].append(case)
                print(json.dumps(case), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
