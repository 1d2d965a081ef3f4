"""The OSQP rules of csrc/mpcqp_osqp.h, run on the CPU (no GPU needed).

tests/cpp/osqp_rules_host.cpp is built twice with the host compiler, plain and with the address and
undefined-behaviour sanitizers, and both programs must print the same rows.  The expectations are
OSQP 0.6's own rules restated here (iter % interval for the schedule, the constants of constants.h,
the status precedence of check_termination) and, for the schedule, the CPU oracle's trace."""
import math
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpp", "osqp_rules_host.cpp")
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]

SOLVED, SOLVED_INACC, PINF_INACC, DINF_INACC = 1, 2, 3, 4
MAX_ITER, PINF, DINF, NON_CVX, NAN_INPUT, UNSOLVED = -2, -3, -4, -7, -100, -10
INF = 1e30
RHO_MIN, RHO_MAX, RHO_TOL, RHO_EQ = 1e-6, 1e6, 1e-4, 1e3


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    cxx = shutil.which("c++")
    assert cxx, "the host C++ compiler (c++) is needed"
    out = tmp_path_factory.mktemp("osqp_rules")
    plain, san = str(out / "osqp_rules_host"), str(out / "osqp_rules_host_san")
    subprocess.run([cxx, *CXXFLAGS, SRC, "-o", plain], check=True)
    # (the sanitizer runtimes linked statically: the program is run as it is, whatever else the
    # environment preloads into it)
    subprocess.run([cxx, *CXXFLAGS, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", SRC, "-o", san], check=True)

    def run(rule, *args):
        argv = [rule] + [a.hex() if isinstance(a, float) else str(int(a)) for a in args]
        outs = [subprocess.run([exe] + argv, check=True, capture_output=True, text=True).stdout for exe in (plain, san)]
        assert outs[0] == outs[1], f"sanitizer build prints other rows for {argv}"
        return [ln.split() for ln in outs[0].splitlines()]

    return run


_f = float.fromhex  # the program prints doubles with %a


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


# ---- schedule ------------------------------------------------------------------------------------------
# (check_termination, adaptive_rho, interval, max_iter, eps, oracle trace iterations, status, iters, rho_updates)
SCHEDULE_CASES = [
    (7, 1, 10, 60, 1e-9, list(range(7, 60, 7)), MAX_ITER, 60, 2),
    (25, 1, 25, 60, 1e-9, [25, 50], MAX_ITER, 60, 1),
    (0, 1, 10, 35, 1e-9, [], MAX_ITER, 35, 1),
    (7, 0, 25, 30, 1e-9, [7, 14, 21, 28], MAX_ITER, 30, 0),
    (5, 1, 25, 10, 1e-3, [5, 10], MAX_ITER, 10, 0),
]


@pytest.fixture(scope="module")
def test_mpc_record(oracle):
    return oracle.assemble_test_mpc(10)


@pytest.mark.parametrize("case", SCHEDULE_CASES, ids=lambda c: f"check{c[0]}_adapt{c[1]}x{c[2]}_max{c[3]}")
def test_schedule_matches_oracle_trace(rules, oracle, test_mpc_record, case):
    ct, ar, interval, max_iter, eps, trace_iters, status, iters, rho_updates = case
    rec, q, r = test_mpc_record
    p = oracle.default_params(10, q=list(q), r=list(r), check_termination=ct, adaptive_rho=ar,
                              adaptive_rho_interval=interval, max_iter=max_iter, eps_abs=eps, eps_rel=eps)
    res, _, trace = oracle.solve(p, rec, trace=True)
    # the oracle run the table in the issue was taken from
    assert [e[0] for e in trace] == trace_iters
    assert (int(res["status"]), int(res["iters"]), int(res["rho_updates"])) == (status, iters, rho_updates)

    rows = rules("schedule", ct, ar, interval, max_iter)
    walk = [[int(x) for x in row[1:]] for row in rows if row[0] == "walk"]
    every = [[int(x) for x in row[1:]] for row in rows if row[0] == "every"]
    plain = [int(row[1]) for row in rows if row[0] == "walk_plain"]
    # OSQP's rule: iter % interval == 0, and the last iteration
    want = []
    for it in range(1, max_iter + 1):
        ck = int(ct > 0 and it % ct == 0)
        ad = int(ar > 0 and interval > 0 and it % interval == 0)
        last = int(it == max_iter)
        if ck or ad or last:
            want.append([it, ck, ad, last, 1])
    assert walk == want  # runs of plain iterations never skip or split an update_info iteration
    assert every == want
    assert plain == [max_iter - len(want)]
    assert [row[0] for row in walk if row[1]] == trace_iters  # is_check iterations = the oracle's trace
    assert sum(row[1] for row in walk) == len(trace)


# ---- status ----------------------------------------------------------------------------------------------
def test_status_precedence(rules):
    rows = [[int(x) for x in row] for row in rules("status")]
    assert len(rows) == 32 and len({tuple(r[:5]) for r in rows}) == 32
    for prim_ok, dual_ok, prim_inf, dual_inf, approx, st in rows:
        if prim_ok and dual_ok:
            want = SOLVED_INACC if approx else SOLVED
        elif prim_inf:
            want = PINF_INACC if approx else PINF
        elif dual_inf:
            want = DINF_INACC if approx else DINF
        else:
            want = UNSOLVED
        assert st == want


def _check(rules, approx, pri, prim_norm, dua, dual_norm, cinv=1.0, prim_ret=0, dual_ret=0,
           eps=(1e-3, 1e-2, 1e-4, 1e-5)):
    (row,) = rules("check", *eps, approx, pri, prim_norm, dua, dual_norm, cinv, prim_ret, dual_ret)
    return int(row[0]), int(row[1]), _f(row[2]), int(row[3]), _f(row[4])


def test_check_skeleton(rules):
    eps_abs, eps_rel, eps_pinf, eps_dinf = 1e-3, 1e-2, 1e-4, 1e-5
    # both residuals under eps_abs + eps_rel * norm: solved, no certificate test runs
    assert _check(rules, 0, 1e-3, 1.0, 1e-3, 1.0) == (SOLVED, 0, 0.0, 0, 0.0)
    # a failing residual test runs its own certificate test, and only that one, with its own eps
    assert _check(rules, 0, 1.0, 1.0, 1e-3, 1.0) == (UNSOLVED, 1, eps_pinf, 0, 0.0)
    assert _check(rules, 0, 1e-3, 1.0, 1.0, 1.0) == (UNSOLVED, 0, 0.0, 1, eps_dinf)
    assert _check(rules, 0, 1.0, 1.0, 1.0, 1.0, prim_ret=1, dual_ret=1) == (PINF, 1, eps_pinf, 1, eps_dinf)
    assert _check(rules, 0, 1.0, 1.0, 1.0, 1.0, dual_ret=1) == (DINF, 1, eps_pinf, 1, eps_dinf)
    assert _check(rules, 0, 1e-3, 1.0, 1.0, 1.0, dual_ret=1)[0] == DINF
    # the tolerance is strict, and it is eps_abs + eps_rel * norm with the dual norm and residual unscaled by cinv
    tol = eps_abs + eps_rel * 3.0
    assert _check(rules, 0, tol, 3.0, 0.0, 0.0)[0] == UNSOLVED
    assert _check(rules, 0, math.nextafter(tol, 0.0), 3.0, 0.0, 0.0)[0] == SOLVED
    cinv = 0.25
    tol = eps_abs + eps_rel * (cinv * 8.0)
    assert _check(rules, 0, 0.0, 0.0, tol / cinv, 8.0, cinv=cinv)[0] == UNSOLVED
    assert _check(rules, 0, 0.0, 0.0, math.nextafter(tol, 0.0) / cinv, 8.0, cinv=cinv)[0] == SOLVED
    # approximate: all four eps x 10
    assert _check(rules, 1, 5e-3, 0.0, 5e-3, 0.0) == (SOLVED_INACC, 0, 0.0, 0, 0.0)
    assert _check(rules, 0, 5e-3, 0.0, 5e-3, 0.0)[0] == UNSOLVED
    assert _check(rules, 1, 0.0, 0.0, 5e-2, 3.0)[0] == SOLVED_INACC  # 5e-2 < 1e-2 + 1e-1 * 3
    assert _check(rules, 1, 1.0, 1.0, 1.0, 1.0, prim_ret=1) == (PINF_INACC, 1, eps_pinf * 10, 1, eps_dinf * 10)
    assert _check(rules, 1, 1.0, 1.0, 1.0, 1.0, dual_ret=1)[0] == DINF_INACC
    # NON_CVX guard: a residual above OSQP_INFTY, before anything else
    big = math.nextafter(INF, math.inf)
    assert _check(rules, 0, big, 1.0, 0.0, 1.0, prim_ret=1) == (NON_CVX, 0, 0.0, 0, 0.0)
    assert _check(rules, 1, 0.0, 1.0, big, 1.0, dual_ret=1) == (NON_CVX, 0, 0.0, 0, 0.0)
    assert _check(rules, 0, 0.0, 1.0, 1.5 * INF, 1.0, cinv=0.5)[0] == UNSOLVED  # dua_res = cinv * norm, under it
    assert _check(rules, 0, INF, 1.0, 0.0, 1.0)[0] == UNSOLVED  # at the bound: not above it


def test_tolerance(rules):
    for eps_abs, eps_rel, norm in [(1e-3, 1e-3, 7.25), (1e-9, 1e-9, 1234.5), (0.0, 0.1, 3.0)]:
        (row,) = rules("tolerance", eps_abs, eps_rel, norm)
        assert _f(row[0]) == eps_abs + eps_rel * norm  # (the test programs are built without contraction)


def _info(rules, is_check, is_adapt, last, rho, tol, norms, st_exact, st_approx):
    (row,) = rules("info", is_check, is_adapt, last, rho, tol, *norms, st_exact, st_approx)
    return dict(status=int(row[0]), refactor=int(row[1]), rho=_f(row[2]), rho_updates=int(row[3]),
                exact_calls=int(row[4]), approx_calls=int(row[5]), rho_at_approx=_f(row[6]))


def test_info_iteration(rules):
    still = (1.0, 1.0, 1.0, 1.0)    # estimate = rho
    moves = (100.0, 1.0, 1.0, 1.0)  # estimate = 10 rho
    # an adapt-only iteration does not check; rho moves and asks for a refactorization
    r = _info(rules, 0, 1, 0, 0.1, 5.0, moves, SOLVED, SOLVED)
    assert (r["status"], r["exact_calls"], r["approx_calls"]) == (UNSOLVED, 0, 0)
    assert r["refactor"] == 1 and r["rho_updates"] == 1 and r["rho"] == pytest.approx(1.0, rel=1e-12)
    r = _info(rules, 0, 1, 0, 0.1, 5.0, still, SOLVED, SOLVED)
    assert (r["refactor"], r["rho_updates"], r["rho"]) == (0, 0, 0.1)
    # a check iteration that terminates does not adapt
    r = _info(rules, 1, 1, 0, 0.1, 5.0, moves, SOLVED, UNSOLVED)
    assert (r["status"], r["exact_calls"], r["approx_calls"], r["rho_updates"], r["rho"]) == (SOLVED, 1, 0, 0, 0.1)
    # one that goes on adapts, if it is an adapt iteration
    r = _info(rules, 1, 1, 0, 0.1, 5.0, moves, UNSOLVED, SOLVED)
    assert (r["status"], r["exact_calls"], r["approx_calls"], r["rho_updates"], r["refactor"]) == (UNSOLVED, 1, 0, 1, 1)
    r = _info(rules, 1, 0, 0, 0.1, 5.0, moves, UNSOLVED, SOLVED)
    assert (r["status"], r["rho_updates"], r["refactor"], r["rho"]) == (UNSOLVED, 0, 0, 0.1)
    # the last iteration checks even when it is no check iteration; adapt_rho runs before the approximate
    # check (no refactorization: nothing follows); then MAX_ITER_REACHED
    r = _info(rules, 0, 1, 1, 0.1, 5.0, moves, UNSOLVED, UNSOLVED)
    assert (r["status"], r["exact_calls"], r["approx_calls"]) == (MAX_ITER, 1, 1)
    assert (r["rho_updates"], r["refactor"]) == (1, 0) and r["rho_at_approx"] == r["rho"] != 0.1
    r = _info(rules, 0, 0, 1, 0.1, 5.0, moves, UNSOLVED, SOLVED_INACC)
    assert (r["status"], r["exact_calls"], r["approx_calls"], r["rho_updates"]) == (SOLVED_INACC, 1, 1, 0)
    r = _info(rules, 1, 1, 1, 0.1, 5.0, moves, PINF, SOLVED_INACC)
    assert (r["status"], r["exact_calls"], r["approx_calls"], r["rho_updates"]) == (PINF, 1, 0, 0)
    # no update_info duty at all: nothing happens
    r = _info(rules, 0, 0, 0, 0.1, 5.0, moves, SOLVED, SOLVED)
    assert (r["status"], r["exact_calls"], r["approx_calls"], r["rho_updates"]) == (UNSOLVED, 0, 0, 0)


# ---- rho ---------------------------------------------------------------------------------------------------
def test_rho_estimate_and_clamp(rules):
    def est(*a):
        (row,) = rules("rho_estimate", *a)
        return _f(row[0])

    div_tol = 1.0 / INF
    rho, pri, pn, dua, dn = 0.1, 3.0, 7.0, 0.5, 11.0
    want = rho * math.sqrt((pri / (pn + div_tol)) / ((dua / (dn + div_tol)) + div_tol))
    assert est(rho, pri, pn, dua, dn) == want
    assert est(0.1, 0.0, 1.0, 1.0, 1.0) == RHO_MIN   # estimate 0: clamped up
    assert est(0.1, 1e-30, 1.0, 1.0, 1.0) == RHO_MIN
    assert est(0.1, 1.0, 1.0, 0.0, 1.0) == RHO_MAX   # dual residual 0: sqrt(1 / DIV_TOL) rho, clamped down
    assert est(1.0, 1e20, 1.0, 1.0, 1.0) == RHO_MAX
    assert est(1.0, 1.0, 1.0, 1.0, 1.0) == 1.0


def test_rho_moved_is_strict(rules):
    def moved(e, rho, tol):
        (row,) = rules("rho_moved", e, rho, tol)
        return int(row[0])

    rho, tol = 0.1, 5.0
    up, down = rho * tol, rho / tol
    assert moved(up, rho, tol) == 0 and moved(down, rho, tol) == 0
    assert moved(math.nextafter(up, math.inf), rho, tol) == 1
    assert moved(math.nextafter(down, 0.0), rho, tol) == 1
    assert moved(math.nextafter(up, 0.0), rho, tol) == 0
    assert moved(math.nextafter(down, math.inf), rho, tol) == 0
    assert moved(rho, rho, tol) == 0


def test_row_kind(rules):
    def row(l, u, rho=0.1):
        (r,) = rules("row", l, u, rho)
        return int(r[0]), _f(r[1])

    edge = INF * 1e-4  # OSQP_INFTY * MIN_SCALING
    above, below = math.nextafter(edge, math.inf), math.nextafter(edge, 0.0)
    assert row(-above, above) == (-1, RHO_MIN)            # loose: both bounds past the edge
    assert row(-edge, above) == (0, 0.1)                  # at the edge is finite: inequality
    assert row(-above, edge) == (0, 0.1)
    assert row(-above, below) == (0, 0.1)
    assert row(-INF, 0.0) == (0, 0.1) and row(0.0, INF) == (0, 0.1)
    assert row(-INF, INF) == (-1, RHO_MIN)
    assert row(0.0, 0.0) == (1, RHO_EQ * 0.1)             # equality
    assert row(2.0, 2.0 + math.nextafter(RHO_TOL, 0.0) / 2) == (1, RHO_EQ * 0.1)
    assert row(0.0, math.nextafter(RHO_TOL, 0.0)) == (1, RHO_EQ * 0.1)
    assert row(0.0, RHO_TOL) == (0, 0.1)                  # u - l < RHO_TOL is strict
    assert row(0.0, 180.0, 0.7) == (0, 0.7)
    assert row(0.0, 0.0, 2.5) == (1, RHO_EQ * 2.5)


# ---- rays --------------------------------------------------------------------------------------------------
def test_polar_project(rules):
    def proj(dy, l, u):
        (r,) = rules("polar", dy, l, u)
        return _f(r[0])

    for dy in (-2.5, 0.0, 3.5):
        assert proj(dy, -INF, INF) == 0.0               # free row: the polar cone is {0}
        assert proj(dy, 0.0, INF) == min(dy, 0.0)       # only a lower bound: dy <= 0
        assert proj(dy, -INF, 0.0) == max(dy, 0.0)      # only an upper bound: dy >= 0
        assert proj(dy, 0.0, 180.0) == dy               # both finite: unchanged
    edge = INF * 1e-4
    assert proj(3.5, 0.0, edge) == 3.5                  # a bound at the edge counts as finite
    assert proj(3.5, 0.0, math.nextafter(edge, math.inf)) == 0.0


def test_dual_ray_violates(rules):
    def viol(v, l, u, thr):
        (r,) = rules("ray", v, l, u, thr)
        return int(r[0])

    thr = 1e-3
    hi, lo = math.nextafter(thr, math.inf), math.nextafter(thr, 0.0)
    # finite upper bound: (A dx)_i must not exceed thr; finite lower bound: not fall below -thr
    assert viol(hi, 0.0, 180.0, thr) == 1 and viol(thr, 0.0, 180.0, thr) == 0 and viol(lo, 0.0, 180.0, thr) == 0
    assert viol(-hi, 0.0, 180.0, thr) == 1 and viol(-thr, 0.0, 180.0, thr) == 0
    # an infinite bound lets the ray go that way
    assert viol(5.0, 0.0, INF, thr) == 0 and viol(-5.0, 0.0, INF, thr) == 1
    assert viol(-5.0, -INF, 0.0, thr) == 0 and viol(5.0, -INF, 0.0, thr) == 1
    assert viol(5.0, -INF, INF, thr) == 0 and viol(-5.0, -INF, INF, thr) == 0
    edge = INF * 1e-4
    assert viol(5.0, 0.0, edge, thr) == 0 and viol(5.0, 0.0, math.nextafter(edge, 0.0), thr) == 1


# ---- epilogue ------------------------------------------------------------------------------------------------
def test_epilogue_by_status(rules):
    scaled, cinv = 12.5, 0.125
    rows = {int(r[0]): (int(r[1]), _f(r[2])) for r in rules("epilogue", scaled, cinv)}
    want = {
        SOLVED: (1, scaled * cinv), SOLVED_INACC: (1, scaled * cinv), MAX_ITER: (1, scaled * cinv),
        UNSOLVED: (1, scaled * cinv), NAN_INPUT: (1, scaled * cinv),
        PINF: (0, INF), PINF_INACC: (0, INF), DINF: (0, -INF), DINF_INACC: (0, -INF), NON_CVX: (0, math.nan),
    }
    assert set(rows) == set(want)  # every status code of include/mpcqp.h
    for st, (sol, obj) in want.items():
        assert rows[st][0] == sol and _same(rows[st][1], obj), st


def test_status_codes_cover_header():
    """The list above is include/mpcqp.h's."""
    import re
    text = open(os.path.join(REPO, "include", "mpcqp.h")).read()
    codes = {int(v) for v in re.findall(r"MPCQP_STATUS_\w+ = (-?\d+)", text)}
    assert codes == {SOLVED, SOLVED_INACC, PINF_INACC, DINF_INACC, MAX_ITER, PINF, DINF, NON_CVX, NAN_INPUT, UNSOLVED}


def test_nan_input_result(rules):
    rows = rules("nan_result", 0.1)
    assert len(rows) == 13
    for u0, fb in rows[:12]:
        assert math.isnan(_f(u0)) and _f(fb) == 0.0
    obj, pri, dua, rho, status, iters, rho_updates, nan_legs = rows[12]
    assert math.isnan(_f(obj)) and math.isnan(_f(pri)) and math.isnan(_f(dua)) and _f(rho) == 0.1
    assert (int(status), int(iters), int(rho_updates), int(nan_legs)) == (NAN_INPUT, 0, 0, 0xF)
