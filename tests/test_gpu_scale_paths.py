"""scale_kernel alone (the debug library's mpcqp_debug_scale_image_device, no solve) on the frozen cases of
tests/scale_cases.py: inputs on which the Ruiz passes move D and E, through every path of the pass logic that
scale_cases.PATHS names (the census tests/test_scale_cases.py checks on the CPU; with and without the SPD upper
bound, i.e. with a negative weight the kernel looks at) at every horizon, i.e. every launch shape of the kernel;
every `scaling` setting; the warm branches (osqp_update_P with a previous scaling that is not the identity, re-init)
from slots encoded from the oracle's solver state; and the rows the kernel must leave alone.

Reference: the oracle's scale_data (pyoracle.scale_image / WarmSolver.step_image).  Gates per family
(scale_cases.gate): the larger of tests/test_gpu_scale_image.py's 1e-13 (D, E, c relative, q~ relative to max|q~|)
and ten times the spread the two CPU computations of the same family show; the branch, the flags and everything the
kernel does not compute bitwise.  The image has 56N + 3 doubles per robot; the buffer is prefilled with NaN and has
one row more than the batch, which, like a cold image's raw-gradient block, must still be NaN afterwards."""
import numpy as np
import pytest
import torch

import mpcqp
import pyoracle
import scale_cases as sc
import warm_slot
from degenerate_cases import SCHUR_GRAM_TOL, gram_ratio
from gpu_helpers import note
from mpcqp import _lib as L

pytestmark = pytest.mark.gpu

WARM_HORIZONS = (1, 5, 7, 10, 11, 16, 17, 20)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _image(solver, recs, slots=None):
    """The kernel's image rows [B][56N + 3] for recs (and warm slots [B][slot], left as they are: a copy goes to the
    device), after the checks of what must stay NaN."""
    N = solver.params.horizon
    recs = np.array(recs, dtype=np.float64)  # (a writable copy: the frozen records are read-only)
    B, size = recs.shape[0], solver.scale_image_size
    assert size == 56 * N + 3
    d_rec = torch.from_numpy(recs).cuda()
    d_img = torch.full((B + 1, size), float("nan"), dtype=torch.float64, device="cuda")
    d_state = None
    if slots is not None:
        assert slots.shape == (B, solver.warm_state_size)
        d_state = torch.from_numpy(np.ascontiguousarray(slots)).cuda()
    solver.scale_image_device(d_rec.data_ptr(), B, d_state.data_ptr() if d_state is not None else 0,
                              d_img.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    img = d_img.cpu().numpy()
    assert np.all(np.isnan(img[B])), "written past the last robot's 56N + 3 doubles"
    return img[:B]


def _split(img, N):
    n, m = 12 * N, 20 * N
    return {"D": img[:, :n], "E": img[:, n:n + m], "q": img[:, n + m:2 * n + m], "qn": img[:, 2 * n + m:3 * n + m],
            "c": img[:, 3 * n + m], "mode": img[:, 3 * n + m + 1], "degen": img[:, 3 * n + m + 2]}


def _check_degen(g, recs, N):
    """The screen's flag as in tests/test_gpu_degenerate.py: gram_ratio's prediction at the Schur horizons (ratios
    within 1 % of the threshold may go either way), no screen beyond them."""
    flag = g["degen"]
    assert np.all((flag == 0.0) | (flag == 1.0))
    if N <= 10:
        ratio = gram_ratio(recs, N)
        must, may = ratio < SCHUR_GRAM_TOL / 1.01, ratio < SCHUR_GRAM_TOL * 1.01
        assert np.all(flag[must] == 1.0) and not np.any(flag[~may] == 1.0)
    else:
        assert np.all(_bits(flag) == 0)


def _errors(g, b, ref, q=None):
    got = {"D": g["D"][b], "E": g["E"][b], "c": g["c"][b], "q": g["q"][b] if q is None else q}
    return sc.image_error(got, ref)


def _worst(errs):
    return {k: max(e[k] for e in errs) for k in ("D", "E", "c", "q")}


@pytest.mark.parametrize("family,N", sc.CASES, ids=[f"{f}-N{N}" for f, N in sc.CASES])
def test_cold_image_on_the_frozen_cases(oracle, family, N):
    """Every family at every horizon (the scaling families at the horizons of each launch shape)."""
    recs = sc.records(family, N)
    scaling = sc.FAMILIES[family][3]
    with mpcqp.MpcQpSolver(sc.device_params(family, N), debug=True) as s:
        assert s.params.scaling == scaling
        g = _split(_image(s, recs), N)
        # (the raw gradient is written for warm slots only: fresh, all-zero slots are a cold start that has it)
        fresh = _split(_image(s, recs, np.zeros((sc.ROBOTS, s.warm_state_size))), N) if scaling == 0 else None
    assert np.all(_bits(g["mode"]) == 0)
    assert np.all(np.isnan(g["qn"]))
    _check_degen(g, recs, N)
    refs = sc.oracle(family, N)
    worst = _worst([_errors(g, b, refs[b]) for b in range(sc.ROBOTS)])
    note(f"scale paths cold {family} N={N}", family=family, N=N, gate=sc.gate(family), **worst)
    assert max(worst.values()) <= sc.gate(family), worst
    if scaling == 0:
        one = _bits(np.ones(1))[0]
        assert np.all(_bits(g["D"]) == one) and np.all(_bits(g["E"]) == one) and np.all(_bits(g["c"]) == one)
        assert np.all(_bits(fresh["mode"]) == 0)
        assert np.array_equal(_bits(g["q"]), _bits(fresh["qn"]))  # q~ is the raw gradient
        assert np.array_equal(_bits(g["q"]), _bits(fresh["q"]))


def _warm_sequence(N, variant):
    """([4][8][rec], q, r): a trot whose every other robot changes its friction coefficient at tick 2."""
    ticks = mpcqp.records.synthetic_go1_ticks(sc.ROBOTS, 4, seed=4300 + N, gait="trot", swing_ticks=2)
    recs_t = np.stack([mpcqp.assemble_compute_grf(s, N) for s in ticks])
    base_mu, new_mu = (0.3, 0.5) if variant == "qr1e4" else (2.0, 2.5)
    recs_t[:, :, L.REC_MU] = base_mu
    recs_t[2:, ::2, L.REC_MU] = new_mu
    q, r, _, _ = sc.family_params("qr1e4" if variant == "qr1e4" else "go1")
    return recs_t, q, r


def _oracle_ticks(op, recs_t):
    """The oracle's persistent solvers over the ticks: (the solver state before each tick, the image each tick's
    ADMM starts from)."""
    T, B = recs_t.shape[:2]
    before = [[None] * B for _ in range(T)]
    refs = [[None] * B for _ in range(T)]
    for b in range(B):
        w = pyoracle.WarmSolver(op)
        for t in range(T):
            before[t][b] = w.state()
            refs[t][b] = w.step_image(recs_t[t, b])[1]
        w.close()
    return before, refs


@pytest.mark.parametrize("variant", ["qr1e4", "mu2"])
@pytest.mark.parametrize("N", WARM_HORIZONS)
def test_warm_branches_from_encoded_slots(oracle, N, variant):
    """Per tick, fresh slots encoded from the oracle's state after the tick before (no GPU solve): the branch
    bitwise, D, E, c and the warm q~ = c (D qn) against the data the oracle's tick starts from.  The update_P robots
    unscale by a previous D, E, c that is not the identity (weights x 1e4; mu = 2 with the Go1 weights).  The
    oracle's iteration limit is cut to one check interval: the scaled data and the branch depend on the records
    and the previous scaling alone, not on the iterates."""
    recs_t, q, r = _warm_sequence(N, variant)
    op = pyoracle.default_params(N, q=q, r=r, max_iter=25)
    before, refs = _oracle_ticks(op, recs_t)
    family = "qr1e4" if variant == "qr1e4" else "mu2"
    modes, errs = set(), []
    with mpcqp.MpcQpSolver(mpcqp.default_params(N, q_weights=q, r_weights=r), debug=True) as s:
        for t in range(recs_t.shape[0]):
            slots = np.stack([warm_slot.encode(before[t][b], N) for b in range(sc.ROBOTS)])
            g = _split(_image(s, recs_t[t], slots), N)
            _check_degen(g, recs_t[t], N)
            for b in range(sc.ROBOTS):
                ref = refs[t][b]
                assert g["mode"][b] == float(ref["mode"]), (t, b)
                assert ref["mode"] == (0 if t == 0 else 2 if (t == 2 and b % 2 == 0) else 1), (t, b)
                modes.add(ref["mode"])
                if ref["mode"] == 1:
                    prev = before[t][b]
                    assert np.any(prev["D"] != 1.0) or np.any(prev["E"] != 1.0)
                warm_q = g["q"][b] if ref["mode"] == 0 else (g["qn"][b] * g["D"][b]) * g["c"][b]
                errs.append(_errors(g, b, ref, q=warm_q))
    worst = _worst(errs)
    note(f"scale paths warm {variant} N={N}", family=family, N=N, gate=sc.gate(family), **worst)
    assert modes == {0, 1, 2}
    assert max(worst.values()) <= sc.gate(family), worst


def test_warm_tick_with_scaling_off(oracle):
    """scaling = 0 with warm slots at N = 10: no Ruiz pass runs, but the column pass still has to compare H's zero
    pattern with the slot's to decide the branch.  Two robots of tests/warm_slot.py's pattern sequence (mu unchanged
    throughout): the pitched pose after the level one (a changed pattern: re-init) and the rolled pose after the
    pitched one (the same pattern: update_P)."""
    N = 10
    seq, q, r = warm_slot.pattern_sequence(N)
    op = pyoracle.default_params(N, q=list(q), r=list(r), scaling=0, max_iter=25)
    before, refs = _oracle_ticks(op, seq[:3])
    recs = np.stack([seq[1, 0], seq[2, 0]])
    slots = np.stack([warm_slot.encode(before[1][0], N), warm_slot.encode(before[2][0], N)])
    with mpcqp.MpcQpSolver(mpcqp.default_params(N, q_weights=list(q), r_weights=list(r), scaling=0), debug=True) as s:
        g = _split(_image(s, recs, slots), N)
    want = [refs[1][0], refs[2][0]]
    assert [w["mode"] for w in want] == [2, 1]
    assert g["mode"].tolist() == [2.0, 1.0]
    one = _bits(np.ones(1))[0]
    assert np.all(_bits(g["D"]) == one) and np.all(_bits(g["E"]) == one) and np.all(_bits(g["c"]) == one)
    errs = [_errors(g, b, want[b], q=(g["qn"][b] * g["D"][b]) * g["c"][b]) for b in range(2)]
    worst = _worst(errs)
    note("scale paths warm scaling=0 N=10", family="s0_pattern", N=N, gate=sc.GATE, **worst)
    assert max(worst.values()) <= sc.GATE, worst


@pytest.mark.parametrize("N", [5, 10, 16, 20])
def test_a_non_finite_record_leaves_its_row_and_the_others_alone(N):
    """One NaN in one record of the batch: that robot's image row is still the prefill, and the other seven rows are
    bitwise the rows of the same batch without it (weights x 1e4: rows the passes work on)."""
    recs = sc.records("qr1e4", N)
    bad = recs.copy()
    bad[3, L.REC_X0 + 7] = np.nan
    with mpcqp.MpcQpSolver(sc.device_params("qr1e4", N), debug=True) as s:
        clean = _image(s, recs)
        got = _image(s, bad)
    assert np.all(np.isnan(got[3]))
    keep = np.arange(sc.ROBOTS) != 3
    assert np.array_equal(_bits(got[keep]), _bits(clean[keep]))
    assert np.all(np.isfinite(_split(clean, N)["D"]))
