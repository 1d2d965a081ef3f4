"""The balance kernel's cases (tests/balance_cases.py) on the CPU: the case builder plants what it says, the
CPU oracle reaches every exit the device comparison is meant to cover, and the oracle itself is trustworthy
under each setting (a setting changes the path to the optimum, not the optimum)."""
import numpy as np

import balance_cases as bc
import mpcqp
from mpcqp import balance as bal

L = mpcqp._lib
B = bc.B_GPU


def _finite(n=B):
    ok = np.ones(n, bool)
    ok[[b for b in bc.NONFINITE if b < n]] = False
    return ok


def test_case_builder():
    """All 16 contact masks in every 16 consecutive robots; the planted robots where the helper says; the wrap
    robots beyond +-1.5 * 3.1415926 and brought back by 2 * 3.1415926, the near-wrap robots inside by 1e-9."""
    recs = bc.records(B)
    assert recs.shape == (B, bal.BAL_SIZE)
    masks = (recs[:, bal.BAL_CONTACTS:bal.BAL_CONTACTS + 4] != 0) @ [1, 2, 4, 8]  # as the kernel reads a flag
    np.testing.assert_array_equal(masks, np.arange(B) % 16)
    for b0 in range(0, B - 15):
        assert set(masks[b0:b0 + 16]) == set(range(16))
    bad = ~np.isfinite(recs)
    where = {(int(b), int(k)) for b, k in zip(*np.nonzero(bad))}
    assert where == {(bc.NAN_ROBOT, bc.NAN_FIELD), (bc.INF_ROBOT, bc.INF_FIELD), (bc.PAD_ROBOT, bal.BAL_SIZE - 1)}
    assert np.isnan(recs[bc.NAN_ROBOT, bc.NAN_FIELD]) and np.isinf(recs[bc.INF_ROBOT, bc.INF_FIELD])
    assert bc.NAN_FIELD != bc.INF_FIELD and bc.INF_FIELD == bal.BAL_SIZE - 2
    raw, err = bc.yaw_error(recs)
    lim = 1.5 * bc.WRAP
    assert raw[bc.YAW_WRAP_DOWN] > lim and err[bc.YAW_WRAP_DOWN] == 3.0 - 2 * bc.WRAP + 3.0
    assert raw[bc.YAW_WRAP_UP] < -lim and err[bc.YAW_WRAP_UP] == -3.0 + 2 * bc.WRAP - 3.0
    assert lim - 1e-8 < raw[bc.NEAR_WRAP_POS] <= lim and err[bc.NEAR_WRAP_POS] == raw[bc.NEAR_WRAP_POS]
    assert -lim <= raw[bc.NEAR_WRAP_NEG] < -lim + 1e-8 and err[bc.NEAR_WRAP_NEG] == raw[bc.NEAR_WRAP_NEG]
    wraps = np.abs(raw) > lim
    assert set(np.flatnonzero(wraps)) == {bc.YAW_WRAP_DOWN, bc.YAW_WRAP_UP}  # no synthetic robot wraps by chance
    # a smaller batch holds the planted robots it has room for, and the same rows
    np.testing.assert_array_equal(bc.records(65)[:64], bc.records(64))
    assert np.isfinite(bc.records(63)[:, :bal.BAL_SIZE - 1]).sum(1).min() < bal.BAL_SIZE - 1  # NAN_ROBOT
    m16 = bc.mask_records()
    assert np.array_equal((m16[:, bal.BAL_CONTACTS:bal.BAL_CONTACTS + 4] != 0) @ [1, 2, 4, 8], np.arange(16))
    rest = np.delete(m16, np.s_[bal.BAL_CONTACTS:bal.BAL_CONTACTS + 4], axis=1)
    assert np.all(rest == rest[0])


def test_settings_pass_validation(oracle):
    """Every SETTINGS entry is inside what mpcqp_create accepts (params_valid of csrc/mpcqp_capi.cpp)."""
    for name, over in bc.SETTINGS:
        p = bc.oracle_args(oracle, over)[0]
        assert p.max_iter >= 1 and p.scaling >= 0 and p.check_termination >= 0, name
        assert not p.adaptive_rho or p.adaptive_rho_interval > 0, name
        assert p.rho > 0 and p.sigma > 0 and 0 < p.alpha < 2 and p.eps_abs >= 0 and p.eps_rel >= 0, name
        assert p.scaled_termination == 0, name
    assert len(dict(bc.SETTINGS)) == len(bc.SETTINGS) == 22 and len(dict(bc.BALANCE)) == len(bc.BALANCE) == 9


def test_reachability_statuses(oracle):
    """Over the runs the device tests compare (every SETTINGS entry with default balance parameters, every
    BALANCE entry with default settings, 130 robots, seed 4) the oracle shows every exit.  Counted at seed 4:
    SOLVED in every run but max_iter=1; SOLVED_INACCURATE 34 (adaptive_rho=0), 40 (max_iter=50), 18 (eps 1e-9 /
    200 iterations); MAX_ITER_REACHED 128 (max_iter=1), 116 (max_iter=24, 25, 26), 55 (eps 1e-9 / 200); NON_CVX
    17 at r=-1 (all after iteration 0) and 105 at r=-1e3 (4 at iteration 0 from the setup factorization, 101
    later; 95 of the 105 through a residual above OSQP_INFTY, which reports a NaN objective, the others from
    the factorization inside adapt_rho); NAN_INPUT 2 in every run."""
    seen, ncvx0, ncvx_later, nan_obj, ncvx_adapt = set(), 0, 0, 0, 0
    for s, b in [(s, "default") for s, _ in bc.SETTINGS] + [("default", b) for b, _ in bc.BALANCE]:
        r = bc.reference(oracle, s, b)
        seen |= set(r["status"].tolist())
        ncvx0 += int(((r["status"] == L.STATUS_NON_CVX) & (r["iters"] == 0)).sum())
        ncvx_later += int(((r["status"] == L.STATUS_NON_CVX) & (r["iters"] > 0)).sum())
        nan_obj += int(np.isnan(r["obj_val"]).sum())
        # a NON_CVX after iteration 0 whose objective is not NaN came from the factorization inside adapt_rho
        ncvx_adapt += int(((r["status"] == L.STATUS_NON_CVX) & (r["iters"] > 0) & ~np.isnan(r["obj_val"])).sum())
        assert np.array_equal(np.flatnonzero(r["status"] == L.STATUS_NAN_INPUT), sorted(bc.NONFINITE)), (s, b)
    assert {L.STATUS_SOLVED, L.STATUS_SOLVED_INACCURATE, L.STATUS_MAX_ITER_REACHED, L.STATUS_NON_CVX,
            L.STATUS_NAN_INPUT} <= seen
    assert ncvx0 > 0 and ncvx_later > 0 and nan_obj > 0 and ncvx_adapt > 0
    for b in ("r-1", "r-1e3"):
        assert np.any(bc.reference(oracle, "default", b)["status"] == L.STATUS_NON_CVX)
    # the padding double is not read: that robot solves
    assert bc.reference(oracle)["status"][bc.PAD_ROBOT] == L.STATUS_SOLVED


def test_reachability_no_adaptive_rho(oracle):
    """adaptive_rho=0 at seed 4: 94 SOLVED, 34 SOLVED_INACCURATE; 25 iterations for the all-swing robots, then
    from 475 up to all 4000."""
    r = bc.reference(oracle, "no_adaptive_rho")
    it = r["iters"][_finite()]
    assert np.any(r["status"] == L.STATUS_SOLVED) and np.any(r["status"] == L.STATUS_SOLVED_INACCURATE)
    assert np.all(r["rho_updates"] == 0)
    assert it.max() == 4000 and np.any((it >= 200) & (it <= 1000)) and np.any((it > 1000) & (it < 4000))
    # the block the lane-independence test permutes has the whole spread, beside non-finite and all-swing robots
    blk = r["iters"][:64][_finite(64)]
    assert blk.max() == 4000 and np.any((blk >= 200) & (blk <= 1000)) and blk.min() == 25


def test_reachability_check_termination_0(oracle):
    """check_termination=0: no check before the post-loop one, 4000 iterations on every finite robot."""
    r = bc.reference(oracle, "check0")
    assert np.all(r["iters"][_finite()] == 4000) and np.all(r["iters"][~_finite()] == 0)


def test_reachability_adapt_between_checks(oracle):
    """check_termination=7 with adaptive_rho_interval=10 runs adapt_rho on iterations that are no check
    iterations (10, 20, 30, ...), which need an update_info of their own; with the interval at 25 (the
    check_termination=7 run) only 175, 350, ... coincide.  At seed 4 the rho_updates of 66 robots differ."""
    a, b = bc.reference(oracle, "check7"), bc.reference(oracle, "check7_rho10")
    assert np.any(a["rho_updates"] != b["rho_updates"])
    assert np.any(b["rho_updates"] > 0)


def test_reachability_default_spread(oracle):
    """Default settings: one 64-robot block holds exits from iteration 25 to at least 100 (seed 4: block 0 has
    25 x5, 50 x3, 75 x21, 100 x28, 125 x4, 150 x1; block 1 has 25 to 125)."""
    r = bc.reference(oracle)
    blk = r["iters"][:64][_finite(64)]
    assert blk.min() <= 25 and blk.max() >= 100
    assert len(set(blk.tolist())) >= 4


GUARD_B = 96
GUARD = dict(eps_abs=1e-10, eps_rel=1e-10, max_iter=200000)
GUARD_BOUND = 1.2e-4  # ten times the largest difference measured (scaling=0, 1.17e-5)


def test_oracle_guard(oracle):
    """The oracle under each setting that can converge, run to eps 1e-10 / 200000 iterations on 96 robots,
    finds the default-settings u0 (difference relative to max(|u0|, 1) of the robot).  Measured at seed 4, from
    the oracle alone: scaling=3 7.1e-11; scaling=0 1.17e-5 (the worst); check_termination=0 5.9e-6; the others
    1.2e-6 to 4.0e-6 (sigma=1e-3 4.0e-6, rho=1e-3 3.7e-6).  The bound is ten times the worst.

    adaptive_rho=0 keeps rho = 0.1, and 10 of the 94 finite robots are still MAX_ITER_REACHED after all 200000
    iterations: they cannot converge within the budget and are not held to the optimum.  The 84 that reach
    SOLVED are (2.0e-8 at the worst).  Every other setting must solve every finite robot."""
    recs = bc.records(GUARD_B)
    ok = _finite(GUARD_B)
    base = oracle.balance_solve_batch(*bc.oracle_args(oracle, GUARD), recs, 8)
    assert np.all(base["status"][ok] == L.STATUS_SOLVED)
    scale = np.maximum(np.abs(base["u0"][ok]).max(1), 1.0)
    worst = {}
    for name, over in bc.SETTINGS:
        if "max_iter" in over:
            continue
        r = oracle.balance_solve_batch(*bc.oracle_args(oracle, {**over, **GUARD}), recs, 8)
        solved = r["status"][ok] == L.STATUS_SOLVED
        if name == "no_adaptive_rho":
            out = r[ok][~solved]
            assert np.all(out["status"] == L.STATUS_MAX_ITER_REACHED) and np.all(out["iters"] == GUARD["max_iter"])
            assert 4 * solved.sum() >= 3 * ok.sum()  # a condition on the batch: 84 of 94 at seed 4
        else:
            assert solved.all(), name
        e = (np.abs(r["u0"][ok] - base["u0"][ok]).max(1) / scale)[solved]
        worst[name] = float(e.max())
        print(f"[oracle guard] {name}: worst relative u0 difference {worst[name]:.3e} over {int(solved.sum())} robots")
    for name, w in worst.items():
        assert w <= GUARD_BOUND, f"{name}: {w:.3e}"
