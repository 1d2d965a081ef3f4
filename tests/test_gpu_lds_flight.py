"""The Schur-form KKT solve keeps its LDS reads in flight (mpcqp_schur.h schur_solve: the u phase's
columns of B are issued ahead of q, every round's q reads in one batch with counted waits).  What can
go wrong there is silent: a register read before its load has returned, a padding round's clamped
step, or the AMP instantiation of the info iteration taking another schedule.  So small batches at
every round count (N = 1, 3, 5, 8, 10: R = 1, 2, 3 with partial and full last rounds), mixed gaits
with random mu (feet off the ground, hand-offs to the Riccati form), cold and warm, and settings under
which every iteration is an info iteration and rho is adapted (hence refactorized) every few
iterations.  Gates against the CPU oracle: status and iterations equal, u0 within the cold-solve
sentinel of 1e-8."""
import numpy as np
import pytest
import torch

import mpcqp
from gpu_helpers import rel_err_u0, sentinel, solve_gpu

pytestmark = pytest.mark.gpu

HORIZONS = [1, 3, 5, 8, 10]
B = 64
SENTINEL = 1e-8
# every iteration an info iteration (checks, the AMP solve, schur_px), rho adapted every third
# iteration, a max_iter exit
INFO = dict(check_termination=1, adaptive_rho_interval=3, max_iter=40, eps_abs=1e-9, eps_rel=1e-9)


def _recs(N):
    return mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(B, seed=4100 + N, gait="mixed", mixed_mu=True), N)


def _check(oracle, N, over, label):
    recs = _recs(N)
    p = mpcqp.default_params(N, **over)
    with mpcqp.MpcQpSolver(p) as s:
        got, _, _ = solve_gpu(s, recs)
    ref = oracle.solve_batch(oracle.default_params(N, **over), recs, nthreads=8)
    assert np.all(np.isfinite(ref["u0"]))
    err = rel_err_u0(got["u0"], ref["u0"])
    print(f"[lds_flight] {label}: statuses {sorted(set(ref['status'].tolist()))}, iters "
          f"{int(ref['iters'].min())}..{int(ref['iters'].max())}, max u0 rel err {float(err.max()):.3e}")
    np.testing.assert_array_equal(got["status"], ref["status"], err_msg=label)
    np.testing.assert_array_equal(got["iters"], ref["iters"], err_msg=label)
    sentinel(err, SENTINEL, label)


@pytest.mark.parametrize("N", HORIZONS)
def test_cold_solves_match_oracle(oracle, N):
    _check(oracle, N, {}, f"lds_flight cold N={N}")


@pytest.mark.parametrize("N", HORIZONS)
def test_info_every_iteration_matches_oracle(oracle, N):
    _check(oracle, N, INFO, f"lds_flight info N={N}")


@pytest.mark.parametrize("N", [5, 10])
def test_warm_ticks_match_oracle(oracle, N):
    T = 2
    ticks = mpcqp.records.synthetic_go1_ticks(B, T, seed=4200 + N, gait="trot", swing_ticks=3)
    recs_t = np.stack([mpcqp.assemble_compute_grf(s, N) for s in ticks])
    out = np.zeros((T, B), dtype=mpcqp.RESULT_DTYPE)
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        d_state = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
        d_res = torch.zeros((B, mpcqp._lib.RESULT_DOUBLES), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for t in range(T):
            d_rec = torch.from_numpy(np.ascontiguousarray(recs_t[t])).cuda()
            s.solve_warm_device(d_rec.data_ptr(), B, d_state.data_ptr(), d_res.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            out[t] = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE)
    ref = oracle.solve_sequence(oracle.default_params(N), recs_t, nthreads=8)
    for t in range(T):
        label = f"lds_flight warm N={N} tick {t}"
        err = rel_err_u0(out[t]["u0"], ref[t]["u0"])
        print(f"[lds_flight] {label}: iters {int(ref[t]['iters'].min())}..{int(ref[t]['iters'].max())}, "
              f"max u0 rel err {float(err.max()):.3e}")
        np.testing.assert_array_equal(out[t]["status"], ref[t]["status"], err_msg=label)
        np.testing.assert_array_equal(out[t]["iters"], ref[t]["iters"], err_msg=label)
        sentinel(err, SENTINEL, label)
