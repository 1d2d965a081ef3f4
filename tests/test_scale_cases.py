"""CPU checks of tests/scale_cases.py: the numpy restatement of scale_kernel's pass logic against the oracle's
scale_data on every frozen case (which also checks, without a GPU, that a bound-decided pass cannot change the result
beyond rounding), the census of the paths the cases take at every horizon, the margins that keep the kernel's own
decisions from differing from the predicted ones, and that the cases move D and E where they are meant to."""
from collections import Counter

import numpy as np
import pytest

import mpcqp
import scale_cases as sc

PLAIN = tuple(f for f in sc.PATH_FAMILIES if f not in sc.LATE_FAMILIES)


def _families(N):
    return [f for f, n in sc.CASES if n == N]


def test_case_list():
    assert len(sc.CASES) == len(set(sc.CASES)) == len(sc.PATH_FAMILIES) * 20 + len(sc.SCALING_FAMILIES) * 8
    assert set(sc.CPU_SPREAD) == set(sc.FAMILIES) == set(sc.FAMILY_PATHS)
    assert {sc.FAMILIES[f][3] for f in sc.SCALING_FAMILIES} == {0, 1, 2, 3, 15}
    assert all(sc.FAMILIES[f][3] == 10 for f in sc.PATH_FAMILIES)
    assert max(sc.CPU_SPREAD.values()) < 1e-14  # so every device gate is the project's 1e-13


@pytest.mark.parametrize("N", sc.HORIZONS)
def test_restatement_matches_oracle(oracle, N):
    """D, E, c, q~ of the restatement against scale_data, within twice the spread recorded per family or, where
    that is less, 1e-14 (a few dozen ulp, for another BLAS's summation order of B'QB; a tenth of the device gate)."""
    for f in _families(N):
        worst = 0.0
        for (img, _), ref in zip(sc.model(f, N), sc.oracle(f, N)):
            worst = max(worst, max(sc.image_error(img, ref).values()))
        print(f"N={N} {f}: {worst:.3g}")
        assert worst <= max(2.0 * sc.CPU_SPREAD[f], 1e-14), (f, worst)


@pytest.mark.parametrize("N", sc.HORIZONS)
def test_census(N):
    """Every path of the pass logic is reached at every horizon, every family reaches what the module says it does,
    the hand-over at a pass >= 1 happens where the module says, and every decision holds with a relative margin of
    MARGIN, as does the distance of every limit_scaling argument from 1e-4 and 1e4."""
    reached = set()
    late = {}
    for f in _families(N):
        mine = set()
        for img, cen in sc.model(f, N):
            assert cen["margin"] >= sc.MARGIN, (f, cen["margin"])
            assert cen["thr_dist"] >= sc.MARGIN, (f, cen["thr_dist"])
            p = sc.paths(img, cen)
            mine |= p
            if "late_switch" in p:
                late.setdefault(f, []).append(cen["switch_pass"])
            assert cen["bound_passes"] + cen["exact_passes"] == cen["scaling"] or cen["fixed_pass"] is not None
            assert (cen["exact_passes"] > 0) == (cen["switch_pass"] is not None)
            assert cen["ub_used"] == (cen["scaling"] > 0 and not f.startswith("neg_")) and not (
                cen["fallback"] and not cen["ub_used"])
        assert sc.FAMILY_PATHS[f] <= mine, (f, mine)
        if f in sc.PATH_FAMILIES:
            reached |= mine
    assert set(sc.PATHS) <= reached, set(sc.PATHS) - reached
    assert {f: tuple(v) for f, v in late.items()} == sc.LATE_SWITCH[N]
    assert not set(late) & set(PLAIN) and not set(late) & set(sc.SCALING_FAMILIES)


@pytest.mark.parametrize("N", sc.HORIZONS)
def test_cases_move_D_and_E(oracle, N):
    """On the oracle: the identity families are exactly the identity (that is what the Go1 weights exercise), r1e4
    moves where the module says, and every other family moves D or E by more than 1e-3 (on some robot; x 1e2 leaves
    a few robots of the shortest horizons at the identity)."""
    for f in _families(N):
        refs = sc.oracle(f, N)
        moved = [max(np.max(np.abs(r["D"] - 1.0)), np.max(np.abs(r["E"] - 1.0))) for r in refs]
        if f in sc.IDENTITY_FAMILIES:
            assert max(moved) == 0.0, f
        elif f == "r1e4":
            assert (max(moved) > 1e-3) == (N in sc.R1E4_MOVES), (f, max(moved))
        else:
            assert max(moved) > 1e-3, (f, max(moved))
        if sc.FAMILIES[f][3] == 0:
            assert all(r["c"] == 1.0 for r in refs)


@pytest.mark.parametrize("draw,frozen", [(931, sc._LATE_A), (3591, sc._LATE_B)])
def test_late_switch_cases_come_from_the_search(draw, frozen):
    hits = list(sc.late_switch_search(2, seed=1, budget=draw + 1, first=draw))
    assert len(hits) == 1
    d, qe, re_, mu, sw = hits[0]
    assert (d, qe, re_, mu) == (draw,) + frozen and sw == 1


def test_census_of_the_heavy_weight_device_test():
    """What tests/test_gpu_scale_image.py's heavy-weight cases run (its docstring): on most robots the first-pass
    fallback and then ten bound-decided passes with a D that moves, on the others a switch to the exact passes at
    pass 0 by ok2 alone; no fixed point, no hand-over at a later pass; the 1e4 clamp in the second and third."""
    want = {(10, 1e4, 1e4): (50, 14, False), (10, 1e6, 1.0): (63, 1, True), (20, 1e5, 1e3): (49, 15, True)}
    for (N, qs, rs), (n_bound, n_switch, clamp) in want.items():
        recs = mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(64, seed=7, gait="trot"), N)
        out = sc.run_model(recs, N, [w * qs for w in sc.GO1_Q], [w * rs for w in sc.GO1_R], 10)
        kinds = Counter(frozenset(sc.paths(img, cen)) - {"clamp_1e4"} for img, cen in out)
        assert kinds == {frozenset({"fallback", "bound_all_nonunit"}): n_bound,
                         frozenset({"fallback", "switch0_ok2_alone"}): n_switch}
        assert all(("clamp_1e4" in sc.paths(img, cen)) == clamp for img, cen in out)
        assert min(cen["margin"] for _, cen in out) >= sc.MARGIN
        assert min(cen["thr_dist"] for _, cen in out) >= sc.MARGIN
