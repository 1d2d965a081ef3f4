#!/usr/bin/env python3
"""CPU-only list-scheduling simulation of wave_kernel's dispatch with and without the launch-order
hint (csrc/mpcqp_order.hip), from the oracle's iteration counts.

Model: 1024 SIMD slots, one robot per slot at a time, no migration; a robot costs
15k + 54k (1 + rho_updates) + 3.7k iters cycles (the budget of DESIGN 8); the batch is cut into
contiguous parts whose blocks the dispatcher takes round-robin; within a part the blocks go out in
the part's order; the next block goes to the slot that frees first.  Reported per workload: the
busy fraction in input order, and the span cut by the hint's key (contacts changed first, then the
previous call's clamped cost key, then batch index) and by a perfect key (this call's own cost).

  python tools/launch_order_sim.py [--batch 4096] [--ticks 11] [--threads 8]
"""
import argparse
import heapq
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "go1-qp-mpc-controller_amd"), os.path.join(REPO, "oracle")):
    sys.path.insert(0, p)

KEY_MAX, KEY_SHIFT, RHO_WEIGHT = 63, 3, 15  # csrc/mpcqp_internal.h


def cycles(res):
    return 15e3 + 54e3 * (1 + res["rho_updates"]) + 3.7e3 * res["iters"]


def key_of(res):
    return np.minimum((res["iters"] + RHO_WEIGHT * res["rho_updates"]) >> KEY_SHIFT, KEY_MAX)


def span(cost, orders, slots=1024):
    """orders: one index array per part; blocks are taken from the parts round-robin."""
    free = [0.0] * slots
    heapq.heapify(free)
    pos = [0] * len(orders)
    left = sum(len(o) for o in orders)
    end = 0.0
    while left:
        for i, o in enumerate(orders):
            if pos[i] < len(o):
                t = heapq.heappop(free) + cost[o[pos[i]]]
                heapq.heappush(free, t)
                end = max(end, t)
                pos[i] += 1
                left -= 1
    return end


def part_orders(B, parts, sort_key=None):
    bnd = [B * i // parts for i in range(parts + 1)]
    out = []
    for b0, b1 in zip(bnd[:-1], bnd[1:]):
        idx = np.arange(b0, b1)
        out.append(idx if sort_key is None else idx[np.argsort(sort_key[b0:b1], kind="stable")])
    return out


def evaluate(cost, hint_key, parts, slots=1024):
    B = len(cost)
    s_in = span(cost, part_orders(B, parts), slots)
    s_hint = span(cost, part_orders(B, parts, hint_key), slots)
    s_best = span(cost, part_orders(B, parts, -cost), slots)
    return {"busy_input": float(cost.sum() / (slots * s_in)), "cut_hint_pct": 100 * (1 - s_hint / s_in),
            "cut_perfect_pct": 100 * (1 - s_best / s_in), "busy_perfect": float(cost.sum() / (slots * s_best))}


def summarize(name, rows):
    cut = np.array([r["cut_hint_pct"] for r in rows])
    out = {"workload": name, "calls": len(rows), "busy_input": float(np.mean([r["busy_input"] for r in rows])),
           "cut_hint_pct_mean": float(cut.mean()), "cut_hint_pct_min": float(cut.min()),
           "cut_hint_pct_max": float(cut.max()),
           "cut_perfect_pct_mean": float(np.mean([r["cut_perfect_pct"] for r in rows]))}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=11)
    ap.add_argument("--parts", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--swing", type=int, nargs="*", default=[40, 5])
    a = ap.parse_args()
    import mpcqp.records as rec  # numpy only: no GPU library is loaded
    import pyoracle
    pyoracle.build()
    B, N = a.batch, a.horizon
    op = pyoracle.default_params(N)
    contacts = lambda r: (r[:, 39:43] != 0.0) @ np.array([1, 2, 4, 8])  # noqa: E731  (MPCQP_REC_CONTACTS)

    # the bench batch re-solved: the previous call solved the same problems
    recs = rec.assemble_compute_grf(rec.synthetic_go1(B, seed=1000, gait="trot"), N)
    res = pyoracle.solve_batch(op, recs, nthreads=a.threads)
    summarize("bench C2 batch re-solved", [evaluate(cycles(res), KEY_MAX - key_of(res), a.parts)])

    for swing in a.swing:
        ticks = rec.synthetic_go1_ticks(B, a.ticks + 1, seed=31, gait="trot", swing_ticks=swing)
        recs_t = np.stack([rec.assemble_compute_grf(s, N) for s in ticks])
        for warm in (False, True):
            if warm:
                rs = pyoracle.solve_sequence(op, recs_t, nthreads=a.threads)
            else:
                rs = [pyoracle.solve_batch(op, r, nthreads=a.threads) for r in recs_t]
            rows = []
            for t in range(1, len(recs_t)):
                changed = contacts(recs_t[t]) != contacts(recs_t[t - 1])
                hint = np.where(changed, 0, KEY_MAX + 1) + (KEY_MAX - key_of(rs[t - 1]))
                rows.append(evaluate(cycles(rs[t]), hint, a.parts))
            summarize(f"{'warm' if warm else 'cold'} ticks, swing_ticks {swing}", rows)


if __name__ == "__main__":
    main()
