#!/usr/bin/env python3
"""Bitwise A/B of two libmpcqp builds: `python tools/ab_bitwise.py dump OUT.npz` (libraries chosen with
MPCQP_LIB and MPCQP_DEBUG_LIB) solves C2 (4096 trot robots, N = 10), a C5 sample (2048 mixed-gait robots,
random mu), a C4 sample (1024 robots, N = 20) and 6 warm-started ticks of 512 robots, then small cases
at non-default OSQP settings (check / adapt_rho intervals, max_iter exits, adaptive rho off) on every
compiled wave variant, warm ticks, the two cross-check solvers, the balance kernel and NaN-input
records, and stores the raw result records and solutions; `python tools/ab_bitwise.py cmp A.npz B.npz`
reports which arrays differ."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go1-qp-mpc-controller_amd"))


# non-default settings: check 7 / adapt 10 out of step; no termination checks; adaptive rho off; an
# early max_iter exit under the default intervals
SETTINGS = [dict(check_termination=7, adaptive_rho_interval=10, max_iter=60, eps_abs=1e-9, eps_rel=1e-9),
            dict(check_termination=0, adaptive_rho_interval=10, max_iter=35, eps_abs=1e-9, eps_rel=1e-9),
            dict(adaptive_rho=0, check_termination=7, max_iter=30, eps_abs=1e-9, eps_rel=1e-9),
            dict(max_iter=10)]
# one horizon per compiled wave variant: Schur one round / three rounds (with hand-offs), stored Acl,
# no Acl four rounds, five rounds with two packed row-4 registers
HORIZONS = [(3, 64), (10, 64), (12, 32), (13, 32), (20, 32)]


def dump_settings(res):
    """The small cases: every array is keyed by what was solved."""
    import torch
    import mpcqp
    from mpcqp import balance as bal
    stream = torch.cuda.current_stream().cuda_stream

    def solve(params, recs, debug=False, path=None):
        B, N = recs.shape[0], params.horizon
        with mpcqp.MpcQpSolver(params, debug=debug) as s:
            if path is not None:
                s.set_solver(path)
            d_rec = torch.from_numpy(recs).cuda()
            d_res = torch.zeros((B, mpcqp._lib.RESULT_DOUBLES), dtype=torch.float64, device="cuda")
            d_sol = torch.zeros((B, 12 * N), dtype=torch.float64, device="cuda")
            s.solve_device(d_rec.data_ptr(), B, d_res.data_ptr(), d_sol.data_ptr(), stream)
            torch.cuda.synchronize()
            return d_res.cpu().numpy(), d_sol.cpu().numpy()

    for N, B in HORIZONS:  # wave path, cold
        recs = mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(B, seed=700 + N, gait="mixed", mixed_mu=True), N)
        for i, over in enumerate(SETTINGS):
            res[f"n{N}_s{i}_res"], res[f"n{N}_s{i}_sol"] = solve(mpcqp.default_params(N, **over), recs)
    T, B, N = 3, 64, 10  # wave path, warm
    ticks = mpcqp.records.synthetic_go1_ticks(B, T, seed=62, gait="trot", swing_ticks=3)
    for i, over in enumerate(SETTINGS[:2]):
        with mpcqp.MpcQpSolver(mpcqp.default_params(N, **over)) as s:
            d_state = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
            d_res = torch.zeros((B, mpcqp._lib.RESULT_DOUBLES), dtype=torch.float64, device="cuda")
            for t in range(T):
                d_rec = torch.from_numpy(mpcqp.assemble_compute_grf(ticks[t], N)).cuda()
                s.solve_warm_device(d_rec.data_ptr(), B, d_state.data_ptr(), d_res.data_ptr(), 0, stream)
                torch.cuda.synchronize()
                res[f"warm_s{i}_t{t}_res"] = d_res.cpu().numpy()
            res[f"warm_s{i}_state"] = d_state.cpu().numpy()
    for path, N in [(1, 10), (2, 10), (2, 20)]:  # debug library: dense K^-1, workgroup Riccati
        recs = mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(16, seed=800 + N, gait="mixed", mixed_mu=True), N)
        for name, over in [("def", {}), ("s0", SETTINGS[0])]:
            key = f"path{path}_n{N}_{name}"
            res[key + "_res"], res[key + "_sol"] = solve(mpcqp.default_params(N, **over), recs, debug=True, path=path)
    brecs = bal.assemble_balance(mpcqp.synthetic_go1(64, seed=2025, gait="mixed"))  # balance kernel
    bp = mpcqp._lib.default_balance_params()

    def balance(params, recs, key):
        with mpcqp.MpcQpSolver(params) as s:
            d_rec = torch.from_numpy(recs).cuda()
            d_res = torch.zeros((recs.shape[0], mpcqp._lib.RESULT_DOUBLES), dtype=torch.float64, device="cuda")
            s.balance_solve_device(bp, d_rec.data_ptr(), recs.shape[0], d_res.data_ptr(), stream)
            torch.cuda.synchronize()
            res[key] = d_res.cpu().numpy()

    balance(mpcqp.default_params(1), brecs, "bal_def_res")
    balance(mpcqp.default_params(1, max_iter=10), brecs, "bal_max10_res")
    # a NaN-input record among good ones
    recs = mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(8, seed=900, gait="mixed", mixed_mu=True), 10)
    recs[3, 5] = np.nan
    res["nan_wave_res"], res["nan_wave_sol"] = solve(mpcqp.default_params(10), recs)
    bnan = brecs[:8].copy()
    bnan[3, 5] = np.nan
    balance(mpcqp.default_params(1), bnan, "nan_bal_res")


def dump(out):
    import torch
    import mpcqp
    res = {}
    cases = [("c2", 10, mpcqp.synthetic_go1(4096, seed=1000, gait="trot")),
             ("c5", 10, mpcqp.synthetic_go1(2048, seed=5, gait="mixed", mixed_mu=True)),
             ("c4", 20, mpcqp.synthetic_go1(1024, seed=1000, gait="trot"))]
    stream = torch.cuda.current_stream().cuda_stream
    for name, N, st in cases:
        recs = mpcqp.assemble_compute_grf(st, N)
        B = recs.shape[0]
        with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
            d_rec = torch.from_numpy(recs).cuda()
            d_res = torch.zeros((B, mpcqp._lib.RESULT_DOUBLES), dtype=torch.float64, device="cuda")
            d_sol = torch.zeros((B, 12 * N), dtype=torch.float64, device="cuda")
            s.solve_device(d_rec.data_ptr(), B, d_res.data_ptr(), d_sol.data_ptr(), stream)
            torch.cuda.synchronize()
            res[name + "_res"] = d_res.cpu().numpy()
            res[name + "_sol"] = d_sol.cpu().numpy()
    T, B, N = 6, 512, 10
    ticks = mpcqp.records.synthetic_go1_ticks(B, T, seed=61, gait="trot", swing_ticks=3)
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        d_state = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
        d_res = torch.zeros((B, mpcqp._lib.RESULT_DOUBLES), dtype=torch.float64, device="cuda")
        for t in range(T):
            d_rec = torch.from_numpy(mpcqp.assemble_compute_grf(ticks[t], N)).cuda()
            s.solve_warm_device(d_rec.data_ptr(), B, d_state.data_ptr(), d_res.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            res[f"warm{t}_res"] = d_res.cpu().numpy()
        res["warm_state"] = d_state.cpu().numpy()
    dump_settings(res)
    np.savez(out, **res)
    print("dumped", out, sorted(res))


def cmp(a, b):
    A, B = np.load(a), np.load(b)
    bad = 0
    for k in sorted(set(A.files) | set(B.files)):
        same = k in A.files and k in B.files and A[k].tobytes() == B[k].tobytes()
        bad += not same
        print(f"{k:18s} {'bitwise equal' if same else 'DIFFERS'}")
    print("ALL EQUAL" if bad == 0 else f"{bad} arrays differ")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(1 if cmp(sys.argv[2], sys.argv[3]) else 0)
