"""The oracle's solver-state accessor, the slot restatement of tests/warm_slot.py, and the conditions the device tests
(tests/test_gpu_warm_slot.py) rely on, checked on the oracle alone at every horizon: that the sequences reach every
branch that consumes a warm slot, the re-init by a changed zero pattern of H (with mu unchanged) among them."""
import numpy as np
import pytest

import warm_slot as ws
from mpcqp import _lib


def _same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("N", [1, 6, 10, 13])
def test_accessor_is_consistent_with_the_step(oracle, N):
    recs = ws.trot_sequence(N)
    w = oracle.WarmSolver(oracle.default_params(N))
    assert w.state() == {"initialized": False}
    for t in range(ws.TROT_T - 1):
        res, sol = w.step(recs[t, 0])
        st = w.state()
        assert st["initialized"] and st["last_mode"] == (0 if t == 0 else 2 if t == 2 else 1)
        assert (st["D"] * st["x"]).tobytes() == sol.tobytes()  # ws_extract's product
        assert st["rho"] == res["rho"] and st["mu"] == recs[t, 0, _lib.REC_MU]
        assert not st["pzero"][np.tril_indices(12 * N, -1)].any()
        _same_state(st, w.state())  # reading changes nothing
    bad = recs[1, 0].copy()
    bad[7] = np.nan
    res, _ = w.step(bad)
    assert res["status"] == _lib.STATUS_NAN_INPUT
    _same_state(st, w.state())  # a non-finite record leaves the solver as it was, last_mode included
    res2, sol2 = w.step(recs[3, 0])
    ref = oracle.WarmSolver(oracle.default_params(N))
    for t in range(ws.TROT_T):
        r_ref, s_ref = ref.step(recs[t, 0])
    assert sol2.tobytes() == s_ref.tobytes() and res2.tobytes() == r_ref.tobytes()  # ... and the accessor did too
    w.reset()
    assert w.state() == {"initialized": False}
    w.close()
    ref.close()


def test_accessor_reports_the_constraint_matrix(oracle):
    """ak0 / ak1 are E A D of the rows' two entries, pzero the zeros of the dense P's upper triangle."""
    N = 3
    recs, q, r = ws.pattern_sequence(N)
    op = ws.oracle_params(N, q, r)
    w = oracle.WarmSolver(op)
    w.step(recs[0, 0])
    st = w.state()
    P, _, _, _, A = oracle.build_qp(op, recs[0, 0])
    assert np.array_equal(st["pzero"], np.triu(P == 0.0))
    At = st["E"][:, None] * A * st["D"][None, :]
    for i in range(20 * N):
        f, k5 = i // 5, i % 5
        assert st["ak1"][i] == At[i, 3 * f + 2] != 0.0
        assert st["ak0"][i] == (At[i, 3 * f + (k5 >> 1)] if k5 < 4 else 0.0)
        assert np.count_nonzero(At[i]) == (2 if k5 < 4 else 1)
    w.close()


@pytest.mark.parametrize("N", range(1, 21))
def test_layout_and_round_trip(N):
    w = ws.layout(N)
    assert (w.FLAG, w.RHO, w.C, w.MU, w.D) == (0, 1, 2, 3, 4)
    assert w.SIZE == 4 + 2 * 12 * N + 3 * 20 * N + 2 * 20 * N + 12 * N + w.MW * 12 * N
    assert w.SIZE == _lib.load().mpcqp_warm_state_size(N)
    rng = np.random.Generator(np.random.PCG64(N))
    n, m = w.n, w.m
    st = {"initialized": True, "rho": 0.37, "c": 1.5, "mu": 0.45}
    st.update({k: rng.normal(size=n if k in ("D", "q", "x") else m) for k in ws.FIELDS})
    st["pzero"] = np.triu(rng.random((n, n)) < 0.3)
    st["pzero"][0, 0] = st["pzero"][n - 1, n - 1] = st["pzero"][0, n - 1] = True  # first and last bit of the mask
    slot = ws.encode(st, N)
    assert slot.shape == (w.SIZE,)
    got = ws.decode(slot, N)
    assert got["flag"] == 1.0 and got["mask_extra"] == 0
    for k in st:
        assert np.array_equal(got[k], st[k]), k
    assert ws.encode(got, N).tobytes() == slot.tobytes()
    # the documented position of one bit: H[ri][j] at bit ri & 63 of word ri >> 6 of column j
    ri, j = n - 1, n - 1
    word = slot[w.MASK + w.MW * j + (ri >> 6):][:1].view(np.uint64)[0]
    assert (int(word) >> (ri & 63)) & 1
    junk = slot.copy()
    junk[w.MASK + w.MW - 1:][:1].view(np.uint64)[0] |= np.uint64(1) << np.uint64(63)
    assert ws.decode(junk, N)["mask_extra"] == (1 if n % 64 else 0)
    assert not ws.encode({"initialized": False}, N).any()


@pytest.mark.parametrize("N", range(1, 21))
def test_trot_sequence_reaches_every_branch(oracle, N):
    run = ws.oracle_trot(N)
    assert np.all(run.res["status"] == ws.SOLVED)
    modes = ws.modes_of(run)
    assert np.all(modes[0] == 0) and set(modes[1:].ravel()) == {1, 2}
    changed = np.zeros(modes.shape, dtype=bool)
    changed[2, ::4] = True
    assert np.array_equal(modes == 2, changed)  # only the mu change re-initializes: contacts enter the bounds only
    recs = ws.trot_sequence(N)
    contacts = recs[:, :, _lib.REC_CONTACTS:_lib.REC_CONTACTS + 4] != 0.0
    assert (contacts[1:] != contacts[:-1]).any(axis=(1, 2)).all()
    assert run.res["rho_updates"].max() >= 2
    assert 25 <= run.res["iters"].min() and run.res["iters"].max() <= 275


@pytest.mark.parametrize("N", range(1, 21))
def test_pattern_sequence_reinitializes_by_pattern(oracle, N):
    run = ws.oracle_pattern(N)
    recs, _, _ = ws.pattern_sequence(N)
    assert np.all(run.res["status"] == ws.SOLVED)
    assert np.all(recs[:, 0, _lib.REC_MU] == recs[0, 0, _lib.REC_MU])
    modes = ws.modes_of(run)[:, 0].tolist()
    zeros = [ws.upper_zeros(s[0]["pzero"]) for s in run.states]
    print(f"N={N}: modes {modes}, upper zeros {zeros}")
    assert modes[0] == 0 and 2 in modes[1:] and 1 in modes[1:]
    n = 12 * N
    assert len(set(zeros)) >= 3
    # the partly sparse tick: the pitched pose is dense, the y = 0 foot sparse, both together in between
    dense, sparse, partly = (zeros[ws.PATTERN_TICKS.index(k)] for k in ("pitch", "foot_y0", "pitch+foot_y0"))
    assert dense < partly < sparse
    full = max(zeros)
    if N in (2, 6, 10, 17):
        assert modes == ws.PATTERN_MODES
    if N == 10:
        assert zeros == ws.PATTERN_ZEROS_N10
    # the mask's words: at these horizons the pattern sets bits in every word of some column
    if n > 64:
        last = run.states[zeros.index(full)][0]["pzero"]
        assert all(last[64 * wd:64 * (wd + 1)].any() for wd in range((n + 63) // 64))
