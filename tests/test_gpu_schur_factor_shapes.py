"""The Schur factorization at every shape of its tile code (mpcqp_schur.h schur_factor,
schur_gj_tiles).  The tiles are cut by the horizon at compile time, so what can go wrong does so at
one horizon and not at its neighbour: a pad row or column of the last tile taken for a real one, a
short last pivot tile, a table of the S build that overruns the factorization scratch at a short
horizon.  The horizons are those at which the shape changes (6N unknowns in 16x16 tiles):

  N   6N  tiles  last pivot tile        N   6N  tiles  last pivot tile
  1    6    1    short                  6   36    3    four rows
  2   12    1    short                  8   48    3    full
  3   18    2    two rows              10   60    4    twelve rows
  5   30    2    short

Per horizon 64 trot robots and 64 mixed-gait robots with random mu, solved cold, against the CPU
oracle: status, iterations and rho_updates equal on every robot, u0 within the 1e-8 sentinel of the
Schur parity tests (test_gpu_lds_flight, test_gpu_degenerate), the screen's hand-off counter inside
the host restatement's prediction (degenerate_cases.gram_ratio).  The seeds were chosen on the CPU so
that the oracle alone refactorizes: at least a quarter of every batch has rho_updates >= 2 in the
oracle's results (0.33 .. 0.95 with these seeds), which is asserted on the oracle's output.  Plus a
batch of one robot, and a warm sequence of three ticks across a contact change at N = 10 (contacts
enter the bounds only, so both later ticks take the update_P branch, which refactorizes with an
inherited rho and, where a row's kind changed, a new rho vector)."""
import numpy as np
import pytest
import torch

import mpcqp
from degenerate_cases import SCHUR_GRAM_TOL, gram_ratio
from gpu_helpers import rel_err_u0, sentinel, solve_gpu

pytestmark = pytest.mark.gpu

HORIZONS = [1, 2, 3, 5, 6, 8, 10]
B = 64
SENTINEL = 1e-8
GAITS = [("trot", False), ("mixed", True)]


def _recs(N, gait, mixed_mu, batch=B):
    return mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(batch, seed=5100 + N, gait=gait, mixed_mu=mixed_mu), N)


def _compare(got, ref, label):
    np.testing.assert_array_equal(got["status"], ref["status"], err_msg=label)
    np.testing.assert_array_equal(got["iters"], ref["iters"], err_msg=label)
    np.testing.assert_array_equal(got["rho_updates"], ref["rho_updates"], err_msg=label)
    err = rel_err_u0(got["u0"], ref["u0"])
    assert np.all(err <= 1e-4), label
    sentinel(err, SENTINEL, label)


@pytest.mark.parametrize("gait,mixed_mu", GAITS)
@pytest.mark.parametrize("N", HORIZONS)
def test_cold_batches_match_oracle(oracle, N, gait, mixed_mu):
    label = f"schur_factor shapes N={N} {gait}"
    recs = _recs(N, gait, mixed_mu)
    ref = oracle.solve_batch(oracle.default_params(N), recs, nthreads=8)
    assert np.all(np.isfinite(ref["u0"]))
    refact = float(np.mean(ref["rho_updates"] >= 2))
    print(f"[schur_factor] {label}: oracle iters {int(ref['iters'].min())}..{int(ref['iters'].max())}, "
          f"rho_updates >= 2 on {refact:.2f} of the batch")
    assert refact >= 0.25, "the batch must refactorize (oracle's results)"
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        got, _, _ = solve_gpu(s, recs)
        counts = s.handoff_counts()
    g = gram_ratio(recs, N)
    must, may = int(np.sum(g < SCHUR_GRAM_TOL / 1.01)), int(np.sum(g < SCHUR_GRAM_TOL * 1.01))
    print(f"[schur_factor] {label}: hand-off counts {tuple(counts)}, screen prediction {must}..{may}")
    assert must <= counts[0] <= may
    _compare(got, ref, label)


@pytest.mark.parametrize("N", [3, 10])
def test_a_batch_of_one(oracle, N):
    recs = _recs(N, "trot", False)[5:6]
    ref = oracle.solve_batch(oracle.default_params(N), recs, nthreads=1)
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        got, _, _ = solve_gpu(s, recs)
    _compare(got, ref, f"schur_factor one robot N={N}")


def test_warm_ticks_across_a_contact_change(oracle):
    """Trot with the stance pair switched every second tick and a per-robot phase: between ticks 0, 1
    and 2 every robot changes its contacts once (the bounds and the rho vector of the rows whose kind
    changed) and keeps them once; both are update_P ticks, as H's zero pattern and mu stay."""
    T, N = 3, 10
    ticks = mpcqp.records.synthetic_go1_ticks(B, T, seed=5210, gait="trot", swing_ticks=2)
    change = np.stack([np.any(ticks[t].contacts != ticks[t - 1].contacts, axis=1) for t in range(1, T)])
    assert np.all(change.sum(axis=0) == 1) and change[0].any() and change[1].any()
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
        print(f"[schur_factor] warm tick {t}: oracle iters {int(ref[t]['iters'].min())}..{int(ref[t]['iters'].max())}, "
              f"rho_updates up to {int(ref[t]['rho_updates'].max())}")
        _compare(out[t], ref[t], f"schur_factor warm N={N} tick {t}")
