"""The Riccati form of the wave kernel (wave_kernel<N, 0>, csrc/mpcqp_wave.hip and mpcqp_wave_riccati.h) at
every horizon 1..20, against the CPU oracle.

The form is shaped by N at compile time: two factor layouts (stored Acl for N <= 12, packed Gp without Acl for
N >= 13), R = (N + 3) / 4 register rounds of four steps whose last round is partial when N is no multiple of 4
(the clamped step indices, the kvr / vvr masks, the aslot clamp, the chain prefetch conditions), and special
cases at N = 1, 2.  Whole batches reach it at N >= 11 on their own; at N <= 10 the handle carries the
gravity-weight lever: q_weights[12] = -1 makes launch_wave's schur_ok() choose KS = 0 for the whole batch while
the QP stays that of the default weights (state 12 is the constant gravity state; tests/test_riccati_lever.py
pins this bitwise on the oracle).  The oracle always runs with the default weights.

Gates (tests/test_gpu_riccati.py, tests/test_gpu_parity.py): u0, f_body and the full-horizon solution within
1e-4, status identical, iterations within 25 on every robot and identical on at least 0.75 of a batch (the gate
for batches this small; the measured fraction goes to the sentinel log), rho_updates equal where the iterations
are."""
import functools

import numpy as np
import pytest
import torch

import mpcqp
import pyoracle
from degenerate_cases import SCHUR_GRAM_TOL, degenerate, gram_ratio
from gpu_helpers import note, rel_err_u0, sentinel, solve_gpu
from test_gpu_lds_flight import INFO
from test_gpu_riccati import ITER_TOL, TOL_P1, _check_p1_riccati, _edge_states

pytestmark = pytest.mark.gpu

B = 32
MIN_EQ = 0.75
ACL_MAXN = 12  # csrc/mpcqp_wave_riccati.h: stored Acl up to here, the packed layout beyond
LEVER = dict(q_weights=pyoracle.GO1_Q[:12] + [-1.0])

# Regression sentinels on the worst u0 error against the oracle, one per factor layout: the first power of ten
# at least 10x above the worst value measured over this file's batches (profiles/riccati_horizons/measured.jsonl;
# every horizon met every gate at its first run, with identical iteration counts on every robot).
SENT_ACL = 1e-9    # stored Acl, N = 1..12: worst 2.5e-11 (cold N = 6; cold N = 1..12 between 7.7e-13 and 2.5e-11)
SENT_NOACL = 1e-9  # packed Gp, N = 13..20: worst 6.9e-11 (warm N = 13, tick 2; cold worst 5.9e-11 at N = 15)


def _sent(N):
    return SENT_ACL if N <= ACL_MAXN else SENT_NOACL


def _over(N, lever=None):
    """The handle's overrides: the lever wherever the Schur form would serve the horizon."""
    return LEVER if (N <= 10 if lever is None else lever) else {}


def _tag(N):
    return f"N={N} lever" if N <= 10 else f"N={N}"


@functools.lru_cache(maxsize=None)
def _recs(N):
    """The horizon's batch, shared by the tests: a test that plants something copies it first."""
    return mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(B, seed=5000 + N, gait="mixed", mixed_mu=True), N)


def _check(oracle, N, recs, label, over=None, sent=True, **params):
    """The extended helper on a handle with `over` (default: the lever at N <= 10), the oracle on the defaults."""
    over = _over(N) if over is None else over
    with mpcqp.MpcQpSolver(mpcqp.default_params(N, **over, **params)) as s:
        out = _check_p1_riccati(oracle, s, recs, label, min_iter_equal=MIN_EQ, sent=_sent(N) if sent else None,
                                oracle_params=oracle.default_params(N, **params))
        return out + (s.handoff_counts(),)


@pytest.mark.parametrize("N", range(1, 21))
def test_cold_every_horizon(oracle, N):
    got, ref, _, counts = _check(oracle, N, _recs(N), f"horizons cold {_tag(N)}")
    assert counts == (0, 0, 0)
    assert np.all(ref["status"] == mpcqp._lib.STATUS_SOLVED) and ref["rho_updates"].max() >= 1


@pytest.mark.parametrize("N", [2, 5, 10])
def test_lever_reaches_the_riccati_form(oracle, N):
    """A robot with collinear feet, which the host restatement of scale_kernel's screen flags, in the batch: the
    default handle runs the Schur form and hands it over (counted); the lever handle runs wave_solve<N, 0>
    from the start, which never counts.  Without this the N <= 10 tests could pass on the Schur form."""
    recs = _recs(N).copy()
    recs[6] = degenerate(recs[4:8], N)[2]
    assert gram_ratio(recs[6:7], N)[0] < SCHUR_GRAM_TOL / 1.01
    *_, schur = _check(oracle, N, recs, f"horizons planted N={N} default", over={}, sent=False)
    *_, lever = _check(oracle, N, recs, f"horizons planted N={N} lever")
    print(f"hand-off counts N={N}: default weights {schur}, lever {lever}")
    assert schur[0] >= 1
    assert lever == (0, 0, 0)


@pytest.mark.parametrize("N", range(1, 11))
def test_riccati_against_schur(N):
    """The two forms on the same records: same QP, different rounding."""
    recs = _recs(N)
    out = []
    for over in ({}, LEVER):
        with mpcqp.MpcQpSolver(mpcqp.default_params(N, **over)) as s:
            out.append(solve_gpu(s, recs)[0])
    schur, ric = out
    np.testing.assert_array_equal(ric["status"], schur["status"])
    di = np.abs(ric["iters"].astype(int) - schur["iters"].astype(int))
    assert di.max() <= ITER_TOL, f"iteration drift {di.max()}"
    err = rel_err_u0(ric["u0"], schur["u0"])
    note(f"riccati horizons vs schur N={N}", max_rel_err_u0=float(err.max()), max_iter_drift=int(di.max()))
    assert np.all(err <= TOL_P1), f"worst {err.max()}"
    assert ric["u0"].tobytes() != schur["u0"].tobytes(), "bitwise equal: both handles ran the same form"


@pytest.mark.parametrize("N", [7, 11, 13, 19])
def test_edge_cases_at_partial_rounds(oracle, N):
    recs = mpcqp.assemble_compute_grf(_edge_states(), N)
    got, _, err, _ = _check(oracle, N, recs, f"horizons edge {_tag(N)}", sent=False)
    note(f"riccati horizons edge {_tag(N)}", max_rel_err_u0=float(err.max()))
    assert np.all(np.abs(got["u0"][0]) <= 1e-6), "all-swing robot must get zero forces"


@pytest.mark.parametrize("N", [6, 13, 18])
def test_info_every_iteration(oracle, N):
    """Every iteration an info iteration, rho adapted (the factorization rerun) every third, a max_iter exit."""
    got, ref, _, _ = _check(oracle, N, _recs(N), f"horizons info {_tag(N)}", **INFO)
    assert np.all(ref["iters"] == INFO["max_iter"]) and ref["rho_updates"].max() >= 2


@pytest.mark.parametrize("N", [3, 9, 11, 14, 17])
def test_trace_close_to_oracle(oracle, N):
    """Check trace (iter, pri_res, dua_res, rho): same check iterations, residuals to 1e-6."""
    recs = mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(4, seed=5100 + N, gait="trot"), N)
    with mpcqp.MpcQpSolver(mpcqp.default_params(N, **_over(N))) as s:
        _, _, tr = solve_gpu(s, recs, trace=True)
        assert s.handoff_counts() == (0, 0, 0)
    op = oracle.default_params(N)
    for b in range(4):
        _, _, otr = oracle.solve(op, recs[b], trace=True)
        g = tr[b][~np.isnan(tr[b][:, 0])]
        k = min(len(g), len(otr))
        assert k >= 1 and abs(len(g) - len(otr)) <= 1
        for (it, pr, du, rho), o in zip(g[:k], otr[:k]):
            assert it == o[0]
            assert abs(pr - o[2]) <= 1e-6 * max(abs(o[2]), 1e-9)
            assert abs(du - o[3]) <= 1e-6 * max(abs(o[3]), 1e-9)


@pytest.mark.parametrize("N", [6, 11, 13, 18])
def test_warm_ticks(oracle, N):
    """Three warm-started ticks with a change of the contact pattern inside, per tick against the oracle's
    persistent solvers.  (Contacts enter the bounds only: every tick after the first is an osqp_update_P tick.
    tests/test_gpu_warm_slot.py has the re-init ticks.)"""
    T = 3
    ticks = mpcqp.records.synthetic_go1_ticks(B, T, seed=5200 + N, gait="trot", swing_ticks=3)
    recs_t = np.stack([mpcqp.assemble_compute_grf(s, N) for s in ticks])
    contacts = recs_t[:, :, mpcqp._lib.REC_CONTACTS:mpcqp._lib.REC_CONTACTS + 4] != 0.0
    assert (contacts[1:] != contacts[:-1]).any(), "the ticks' contact sets must differ"
    out = np.zeros((T, B), dtype=mpcqp.RESULT_DTYPE)
    with mpcqp.MpcQpSolver(mpcqp.default_params(N, **_over(N))) as s:
        d_state = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
        d_res = torch.zeros((B, mpcqp._lib.RESULT_DOUBLES), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for t in range(T):
            d_rec = torch.from_numpy(np.ascontiguousarray(recs_t[t])).cuda()
            s.solve_warm_device(d_rec.data_ptr(), B, d_state.data_ptr(), d_res.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            out[t] = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE)
            assert s.handoff_counts() == (0, 0, 0)
    ref = oracle.solve_sequence(oracle.default_params(N), recs_t, nthreads=8)
    for t in range(T):
        label = f"riccati horizons warm {_tag(N)} tick {t}"
        got, r = out[t], ref[t]
        np.testing.assert_array_equal(got["status"], r["status"], err_msg=label)
        di = np.abs(got["iters"].astype(int) - r["iters"].astype(int))
        err = rel_err_u0(got["u0"], r["u0"])
        fb = np.max(np.abs(got["f_body"] - r["f_body"]), axis=1) / np.maximum(np.max(np.abs(r["f_body"]), axis=1), 1)
        note(label, iter_equal_fraction=float(np.mean(di == 0)), max_iter_drift=int(di.max()),
             iters=[int(r["iters"].min()), int(r["iters"].max())])
        assert di.max() <= ITER_TOL, f"{label}: iteration drift {di.max()}"
        assert np.mean(di == 0) >= MIN_EQ, f"{label}: only {np.mean(di == 0):.2f} identical iteration counts"
        assert np.all(err <= TOL_P1) and np.all(fb <= TOL_P1), f"{label}: worst u0 {err.max()}, f_body {fb.max()}"
        sentinel(err, _sent(N), label)


@pytest.mark.parametrize("N", [4, 15])
def test_nan_record_flagged(N):
    recs = mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(4, seed=1), N)
    recs[1, 7] = np.nan if N == 4 else np.inf
    with mpcqp.MpcQpSolver(mpcqp.default_params(N, **_over(N))) as s:
        got, _, _ = solve_gpu(s, recs)
    assert got["status"][1] == mpcqp._lib.STATUS_NAN_INPUT
    assert got["nan_legs"][1] == 0xF and np.all(got["f_body"][1] == 0)
    assert np.all(got["status"][[0, 2, 3]] == mpcqp._lib.STATUS_SOLVED)


@pytest.mark.parametrize("N", [9, 13])
def test_batch_of_one(oracle, N):
    _check(oracle, N, _recs(N)[3:4], f"horizons one robot {_tag(N)}")
