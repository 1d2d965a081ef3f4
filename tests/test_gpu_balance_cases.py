"""balance_kernel (csrc/mpcqp_balance.hip) against the CPU oracle over the cases of tests/balance_cases.py: every
OSQP setting and balance parameter set that takes the kernel down another path, the batch sizes around its
64-thread block, every contact mask, and its structural claims (a lane's result does not depend on its wave
neighbours; the host wrapper's staging regrows and is reused).  Every field of the result record is compared
(balance_cases.assert_full_parity).  Results always land in a buffer with CANARY_ROWS more rows than the batch,
filled with a finite pattern that must come back bitwise unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import balance_cases as bc
import mpcqp
from mpcqp import balance as bal

pytestmark = pytest.mark.gpu

L = mpcqp._lib
RD = L.RESULT_DOUBLES
CANARY_ROWS = 3


def _canary(rows=CANARY_ROWS):
    return 1.0e3 + 0.5 * np.arange(rows * RD, dtype=np.float64).reshape(rows, RD)


def _structured(rows_u64):
    return np.frombuffer(np.ascontiguousarray(rows_u64).tobytes(), dtype=mpcqp.RESULT_DTYPE)


def run_gpu(recs, settings=None, balance=None, solver=None):
    """One mpcqp_balance_solve_device of exactly len(recs) record rows into a result buffer with canary rows
    behind the batch; returns the result rows as uint64 [B][RD] (for bitwise comparisons) after checking the
    canaries."""
    recs = np.ascontiguousarray(recs, dtype=np.float64).reshape(-1, bal.BAL_SIZE)
    B = recs.shape[0]
    bp = L.default_balance_params(**(balance or {}))
    own = solver is None
    s = mpcqp.MpcQpSolver(mpcqp.default_params(1, **(settings or {}))) if own else solver
    try:
        d_rec = torch.from_numpy(recs).cuda()
        d_res = torch.from_numpy(np.concatenate([np.zeros((B, RD)), _canary()])).cuda()
        s.balance_solve_device(bp, d_rec.data_ptr(), B, d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = d_res.cpu().numpy().view(np.uint64)
    finally:
        if own:
            s.close()
    assert np.array_equal(out[B:], _canary().view(np.uint64)), "a row past the batch was written"
    return out[:B].copy()


def solve(recs, settings=None, balance=None):
    return _structured(run_gpu(recs, settings, balance))


@pytest.mark.parametrize("name", [n for n, _ in bc.SETTINGS])
def test_settings_matrix(oracle, name):
    """130 robots (two blocks and a lane pair) under each OSQP setting, default balance parameters."""
    got = solve(bc.records(bc.B_GPU), settings=bc.SETTINGS_BY_NAME[name])
    bc.assert_full_parity(got, bc.reference(oracle, name, "default"), f"settings {name}")


@pytest.mark.parametrize("name", [n for n, _ in bc.BALANCE])
def test_balance_params_matrix(oracle, name):
    """130 robots under each balance parameter set, default settings; r < 0 makes the QP non-convex."""
    ref = bc.reference(oracle, "default", name)
    got = solve(bc.records(bc.B_GPU), balance=bc.BALANCE_BY_NAME[name])
    bc.assert_full_parity(got, ref, f"balance {name}")
    if bc.BALANCE_BY_NAME[name].get("r", 0.0) < 0:
        assert np.any(ref["status"] == L.STATUS_NON_CVX), "the comparison is vacuous: no NON_CVX robot"
        assert np.any(got["status"] == L.STATUS_NON_CVX)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 128, 129])
def test_batch_edges(oracle, B):
    """Batches that end just before, on and just after a block boundary; run_gpu checks the rows behind."""
    bc.assert_full_parity(solve(bc.records(B)), bc.reference(oracle, B=B), f"batch {B}")


def test_contact_masks(oracle):
    """One robot under each of the 16 contact masks.  A swing leg's force is as small on the device as in the
    oracle; with no foot down every bound is [0, 0] and the solve leaves at the first check."""
    recs = bc.mask_records()
    ref = oracle.balance_solve_batch(*bc.oracle_args(oracle), recs)
    got = solve(recs)
    bc.assert_full_parity(got, ref, "contact masks")
    assert np.all(ref["status"] == L.STATUS_SOLVED)
    for b in range(16):
        swing = np.repeat(bc.contact_mask(b) == 0, 3)
        if swing.any():
            worst = np.abs(ref["u0"][b][swing]).max()
            assert np.abs(got["u0"][b][swing]).max() <= worst + 1e-9 * max(np.abs(ref["u0"][b]).max(), 1.0)
    assert got["iters"][0] == mpcqp.default_params(1).check_termination == 25


def test_lane_independence(oracle):
    """No cross-lane operation: the 64 robots of block 0 under adaptive_rho=0 (exits from 25 over a few hundred
    to 4000 iterations, a NaN and an infinite record and all-swing robots among them) give bitwise the same rows
    in order, under a fixed permutation, and each alone."""
    settings = bc.SETTINGS_BY_NAME["no_adaptive_rho"]
    recs = bc.records(bc.B_GPU)[:64]
    ref = bc.reference(oracle, "no_adaptive_rho")[:64]
    base = run_gpu(recs, settings)
    bc.assert_full_parity(_structured(base), ref, "lane independence, in order")
    perm = np.random.default_rng(64).permutation(64)
    assert not np.array_equal(perm, np.arange(64))
    shuffled = run_gpu(recs[perm], settings)
    undone = np.empty_like(shuffled)
    undone[perm] = shuffled
    assert np.array_equal(undone, base), f"rows {np.flatnonzero((undone != base).any(1))} depend on their lane"
    longest = int(np.argmax(ref["iters"]))
    short = int(np.argmin(np.where(ref["iters"] > 25, ref["iters"], 1 << 30)))
    with mpcqp.MpcQpSolver(mpcqp.default_params(1, **settings)) as s:
        for b in (0, 63, longest, short):
            alone = run_gpu(recs[b:b + 1], solver=s)
            assert np.array_equal(alone[0], base[b]), f"robot {b} alone differs from robot {b} in its block"


def test_host_wrapper_regrows(oracle):
    """mpcqp_balance_solve_host on one handle with batches of 5, 70 and 3: its device staging grows, grows again
    and then stays larger than the batch.  Each result is bitwise the device path's for the same records, and
    the host rows past the batch stay as they were."""
    pool = bc.records(bc.B_GPU)
    parts = [pool[16:21], pool[30:100], pool[100:103]]
    dp = ctypes.POINTER(ctypes.c_double)
    bp = L.default_balance_params()
    with mpcqp.MpcQpSolver(mpcqp.default_params(1)) as s:
        for recs in parts:
            n = recs.shape[0]
            recs = np.ascontiguousarray(recs)
            out = np.concatenate([np.zeros((n, RD)), _canary()])
            L.check(s._L.mpcqp_balance_solve_host(s._h, ctypes.byref(bp), recs.ctypes.data_as(dp), n, out.ctypes.data),
                    s._h, "mpcqp_balance_solve_host", s._L)
            assert np.array_equal(out[n:].view(np.uint64), _canary().view(np.uint64))
            dev = run_gpu(recs, solver=s)
            assert np.array_equal(out[:n].view(np.uint64), dev), f"host batch of {n} differs from the device path"
    whole = bc.reference(oracle)
    bc.assert_full_parity(_structured(dev), whole[100:103], "host wrapper, last batch")
