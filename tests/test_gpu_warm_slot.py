"""The warm-start slot on the device (WarmLayout<N>, csrc/mpcqp_wave_common.h): what scale_kernel and wave_kernel leave in
it after every tick, against the state of the oracle's persistent solver (pyoracle.WarmSolver.state()), at every horizon
1..20 and on both forms of the solve (the Schur form at N <= 10, the Riccati form above and, at N <= 10, through the
gravity-weight lever of tests/test_gpu_riccati_horizons.py).

Two sequences (tests/warm_slot.py; their conditions are asserted on the oracle in tests/test_warm_slot.py): a trot whose
contacts change every tick and whose friction coefficient changes on every fourth robot (branches 0, 1 and the re-init
by mu), and test_mpc's stance through poses and foot positions that change the zero pattern of H's upper triangle with
mu unchanged (the re-init decided by the mask compare alone, a partly sparse H among the ticks).  On top of these: ticks
that alternate between the forms on the same slots, ticks started from the oracle's state encoded into fresh slots
(reading a slot apart from writing it; with one mask bit flipped, the mask compare word by word), a robot's placement in
the batch, a zeroed slot, a non-finite record, and the heavy-weights sequence of tests/test_gpu_conditioning.py.

Gates: the branch, the mask (every bit), FLAG, MU and the canary rows around the slot buffer bitwise; D, E, c within
1e-13 relative and q~ within 1e-13 of max|q~| (tests/test_gpu_scale_image.py's gates); A~ within 3e-13 relative (the
product of an exact entry of A with E and D, each within 1e-13); result.rho, the solution D x and u0 bitwise against the
slot; the unscaled iterates D x, z / E, E y / c and the full solution within 1e-4 max(|ref|_inf, 1) on the robots whose
iteration and rho-update counts equal the oracle's so far (at least 0.75 of a batch).  Regression sentinels per form and
quantity by the rule of tests/test_gpu_riccati_horizons.py: the first power of ten at least 10x the worst value
measured (profiles/warm_slot/measured.jsonl)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mpcqp
import warm_slot as ws
from gpu_helpers import note, sentinel, solve_gpu

pytestmark = pytest.mark.gpu

L = mpcqp._lib
TOL = 1e-13      # D, E, c, q~
TOL_AK = 3e-13   # A~ = (A E) D
TOL_P1 = 1e-4    # iterates and solution
MIN_EQ = 0.75
CANARY = -1.2345678901234567e300
NAN_TICK, NAN_ROBOT = 2, 5

CASES = [(N, False) for N in range(1, 21)] + [(N, True) for N in range(1, 11)]
CASE_IDS = [f"N{N}-{'lever' if lever else 'default'}" for N, lever in CASES]
SEQS = ("trot", "pattern")

# Regression sentinels on the worst error against the oracle over this file's runs, per form and quantity (x, z, y: the
# unscaled iterates relative to max(|ref|_inf, 1); sol: the full-horizon solution likewise; rho relative).
# Measured (every robot iterated like the oracle at every horizon, equal fraction 1.0 throughout):
#   Schur form    x 1.03e-9, z 1.03e-9, y 1.22e-9, sol 1.03e-9, rho 5.2e-9
#   Riccati form  x 1.03e-9, z 1.03e-9, y 2.02e-9, sol 1.03e-9, rho 7.0e-9
# (the scaling part sits at rounding: D 1.0e-15, E 1.3e-15, c 1.8e-15, q~ 2.9e-15, A~ 1.4e-15)
SENT = {
    "schur": {"x": 1e-7, "z": 1e-7, "y": 1e-7, "sol": 1e-7, "rho": 1e-7},
    "riccati": {"x": 1e-7, "z": 1e-7, "y": 1e-7, "sol": 1e-7, "rho": 1e-7},
}


def _form(N, lever):
    return "riccati" if (lever or N > 10) else "schur"


def _sent(table, form, k):
    """("both": a sequence that ran on both forms)"""
    return max(table[f][k] for f in (("schur", "riccati") if form == "both" else (form,)))


def _params(N, lever, q=None, r=None, scale=1.0):
    p0 = mpcqp.default_params(N)
    qq = [w * scale for w in (p0.q_weights if q is None else q)]
    if lever:
        qq[12] = -1.0
    return mpcqp.default_params(N, q_weights=qq, r_weights=list(p0.r_weights if r is None else r))


def _sequence(seq, N):
    """(records [T][B][rec], q, r, the oracle's run)"""
    if seq == "trot":
        return ws.trot_sequence(N), None, None, ws.oracle_trot(N)
    recs, q, r = ws.pattern_sequence(N)
    return recs, q, r, ws.oracle_pattern(N)


def run_ticks(N, levers, recs_t, q=None, r=None, slots0=None, scale=1.0, between=None, shadow=False):
    """One warm-started solve per tick on the same slots, tick t on the handle with lever levers[t].  The slot buffer
    has a canary row before and after the batch.  Per tick: the branch scale_kernel takes (the debug library's image,
    on a clone of the slots), results, solutions, the slots after the solve, whether the canaries survived, the
    hand-off counts.  between(t, interior slots tensor) runs before tick t's solve; slots0 [B][SIZE], or [T][B][SIZE]
    to start every tick from given slots.  shadow: the Riccati form's results of each tick from a clone of the same
    slots (out.shadow)."""
    T, B = recs_t.shape[:2]
    w = ws.layout(N)
    n, m = w.n, w.m
    out = SimpleNamespace(res=np.zeros((T, B), dtype=mpcqp.RESULT_DTYPE), sol=np.zeros((T, B, n)),
                          slots=np.zeros((T, B, w.SIZE)), modes=np.full((T, B), np.nan), canary=[], handoffs=[],
                          shadow=np.zeros((T, B), dtype=mpcqp.RESULT_DTYPE))
    stream = torch.cuda.current_stream().cuda_stream
    per_tick = slots0 is not None and np.ndim(slots0) == 3
    if per_tick:
        slots_t, slots0 = slots0, slots0[0]
        between = lambda t, inner: inner.copy_(torch.from_numpy(np.ascontiguousarray(slots_t[t])))  # noqa: E731
    handles = {lv: (mpcqp.MpcQpSolver(_params(N, lv, q, r, scale)), mpcqp.MpcQpSolver(_params(N, lv, q, r, scale), debug=True))
               for lv in set(levers)}
    shadow_solver = mpcqp.MpcQpSolver(_params(N, True, q, r, scale)) if shadow else None
    try:
        assert next(iter(handles.values()))[0].warm_state_size == w.SIZE
        buf = torch.full((B + 2, w.SIZE), CANARY, dtype=torch.float64, device="cuda")
        buf[1:B + 1] = 0.0 if slots0 is None else torch.from_numpy(np.ascontiguousarray(slots0)).cuda()
        inner = buf[1:B + 1]
        assert inner.data_ptr() == buf.data_ptr() + 8 * w.SIZE and inner.is_contiguous()
        d_res = torch.zeros((B, L.RESULT_DOUBLES), dtype=torch.float64, device="cuda")
        for t in range(T):
            s, dbg = handles[levers[t]]
            if between is not None:
                between(t, inner)
            d_rec = torch.from_numpy(np.array(recs_t[t], dtype=np.float64)).cuda()  # (a copy: the sequences are read-only)
            d_img = torch.full((B, dbg.scale_image_size), float("nan"), dtype=torch.float64, device="cuda")
            clone = inner.clone()  # (the pass records H's pattern in the slot: a copy)
            dbg.scale_image_device(d_rec.data_ptr(), B, clone.data_ptr(), d_img.data_ptr(), stream)
            d_sol = torch.full((B, n), float("nan"), dtype=torch.float64, device="cuda")
            if shadow:
                clone2 = inner.clone()
                shadow_solver.solve_warm_device(d_rec.data_ptr(), B, clone2.data_ptr(), d_res.data_ptr(), 0, stream)
                torch.cuda.synchronize()
                out.shadow[t] = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE)
            s.solve_warm_device(d_rec.data_ptr(), B, inner.data_ptr(), d_res.data_ptr(), d_sol.data_ptr(), stream)
            torch.cuda.synchronize()
            out.handoffs.append(s.handoff_counts())
            out.modes[t] = d_img.cpu().numpy()[:, 3 * n + m + 1]
            out.res[t] = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE)
            out.sol[t] = d_sol.cpu().numpy()
            h = buf.cpu().numpy()
            out.slots[t] = h[1:B + 1]
            out.canary.append(bool(np.all(h[[0, B + 1]].view(np.uint64) == np.float64(CANARY).view(np.uint64))))
    finally:
        for pair in handles.values():
            for s in pair:
                s.close()
        if shadow_solver is not None:
            shadow_solver.close()
    return out


@functools.lru_cache(maxsize=None)
def _run(seq, N, lever):
    recs, q, r, _ = _sequence(seq, N)
    return run_ticks(N, [lever] * recs.shape[0], recs, q, r)


def _relmax(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# ---- the checks, each over every robot and tick of a run -------------------------------------------------------------
def check_mode_mask(g, o, recs_t, label):
    T, B = recs_t.shape[:2]
    N = g.sol.shape[2] // 12
    assert all(g.canary), f"{label}: a canary row around the slot buffer changed"
    for t in range(T):
        for b in range(B):
            if o.res[t, b]["status"] == L.STATUS_NAN_INPUT:
                continue
            st, d = o.states[t][b], ws.decode(g.slots[t, b], N)
            assert g.modes[t, b] == st["last_mode"], f"{label} tick {t} robot {b}: branch {g.modes[t, b]} != {st['last_mode']}"
            bad = np.argwhere(d["pzero"] != st["pzero"])
            assert bad.size == 0, f"{label} tick {t} robot {b}: {len(bad)} mask bits differ, first (ri, j) = {bad[0]}"
            assert d["mask_extra"] == 0, f"{label} tick {t} robot {b}: bits set past 12N"
            assert d["flag"] == 1.0
            assert np.float64(d["mu"]).tobytes() == np.float64(recs_t[t, b, L.REC_MU]).tobytes()


def check_scaling(g, o, label):
    T, B = g.res.shape
    N = g.sol.shape[2] // 12
    worst = dict.fromkeys(("D", "E", "c", "q", "ak"), 0.0)
    for t in range(T):
        for b in range(B):
            if o.res[t, b]["status"] == L.STATUS_NAN_INPUT:
                continue
            st, d = o.states[t][b], ws.decode(g.slots[t, b], N)
            e = {"D": _relmax(d["D"], st["D"]), "E": _relmax(d["E"], st["E"]), "c": abs(d["c"] - st["c"]) / abs(st["c"]),
                 "q": float(np.max(np.abs(d["q"] - st["q"])) / max(np.max(np.abs(st["q"])), 1e-300)),
                 "ak": max(_relmax(d["ak0"], st["ak0"]), _relmax(d["ak1"], st["ak1"]))}
            for k, v in e.items():
                assert v <= (TOL_AK if k == "ak" else TOL), f"{label} tick {t} robot {b}: {k} off by {v:.3g}"
                worst[k] = max(worst[k], v)
    return worst


def check_bitwise(g, label):
    T, B = g.res.shape
    N = g.sol.shape[2] // 12
    for t in range(T):
        for b in range(B):
            if g.res[t, b]["status"] == L.STATUS_NAN_INPUT:
                continue
            d = ws.decode(g.slots[t, b], N)
            where = f"{label} tick {t} robot {b}"
            assert np.float64(g.res[t, b]["rho"]).tobytes() == np.float64(d["rho"]).tobytes(), f"{where}: rho"
            assert g.sol[t, b].tobytes() == (d["D"] * d["x"]).tobytes(), f"{where}: solution != D x"
            assert g.res[t, b]["u0"].tobytes() == g.sol[t, b, :12].tobytes(), f"{where}: u0 != solution[:12]"


def check_iterates(g, o, label, form):
    """A robot whose iteration or rho-update count differs from the oracle's is left out from that tick on (its
    iterates are another trajectory's); rho has the sentinel only.  Returns (worst errors per quantity, the robots
    still equal to the oracle)."""
    T, B = g.res.shape
    N = g.sol.shape[2] // 12
    eq = np.ones(B, dtype=bool)
    worst = dict.fromkeys(("x", "z", "y", "sol", "rho"), 0.0)
    for t in range(T):
        np.testing.assert_array_equal(g.res[t]["status"], o.res[t]["status"], err_msg=f"{label} tick {t}")
        eq &= (g.res[t]["iters"] == o.res[t]["iters"]) & (g.res[t]["rho_updates"] == o.res[t]["rho_updates"])
        note(f"{label} tick {t}", equal_fraction=float(eq.mean()))
        assert eq.mean() >= MIN_EQ, f"{label} tick {t}: only {eq.mean():.2f} of the batch iterate like the oracle"
        for b in np.nonzero(eq)[0]:
            if o.res[t, b]["status"] == L.STATUS_NAN_INPUT:
                continue
            ref, got = ws.unscaled(o.states[t][b]), ws.unscaled(ws.decode(g.slots[t, b], N))
            e = {k: float(np.max(np.abs(got[k] - ref[k])) / max(np.max(np.abs(ref[k])), 1.0)) for k in ("x", "z", "y")}
            e["sol"] = float(np.max(np.abs(g.sol[t, b] - o.sol[t, b])) / max(np.max(np.abs(o.sol[t, b])), 1.0))
            e["rho"] = abs(got["rho"] - ref["rho"]) / ref["rho"]
            for k, v in e.items():
                if k != "rho":
                    assert v <= TOL_P1, f"{label} tick {t} robot {b}: {k} off by {v:.3g}"
                worst[k] = max(worst[k], v)
    for k, v in worst.items():
        sentinel(np.array([v]), _sent(SENT, form, k), f"{label} {form} {k}")
    return worst, eq


def check_all(g, o, recs_t, label, form):
    check_mode_mask(g, o, recs_t, label)
    check_scaling(g, o, label)
    check_bitwise(g, label)
    return check_iterates(g, o, label, form)


def _slice(o, a, b):
    return SimpleNamespace(res=o.res[a:b], sol=o.sol[a:b], states=o.states[a:b])


# ---- a-d: every horizon, both forms, both sequences ------------------------------------------------------------------
@pytest.mark.parametrize("seq", SEQS)
@pytest.mark.parametrize("N,lever", CASES, ids=CASE_IDS)
def test_mode_and_mask(oracle, N, lever, seq):
    recs, _, _, o = _sequence(seq, N)
    g = _run(seq, N, lever)
    check_mode_mask(g, o, recs, f"slot {seq} {CASE_IDS[CASES.index((N, lever))]}")
    modes = set(ws.modes_of(o).ravel())
    assert modes == {0, 1, 2}


@pytest.mark.parametrize("seq", SEQS)
@pytest.mark.parametrize("N,lever", CASES, ids=CASE_IDS)
def test_scaling_fields(oracle, N, lever, seq):
    _, _, _, o = _sequence(seq, N)
    label = f"slot {seq} {CASE_IDS[CASES.index((N, lever))]}"
    worst = check_scaling(_run(seq, N, lever), o, label)
    note(f"{label} scaling", **worst)


@pytest.mark.parametrize("seq", SEQS)
@pytest.mark.parametrize("N,lever", CASES, ids=CASE_IDS)
def test_slot_is_what_the_solve_returned(N, lever, seq):
    check_bitwise(_run(seq, N, lever), f"slot {seq} {CASE_IDS[CASES.index((N, lever))]}")


@pytest.mark.parametrize("seq", SEQS)
@pytest.mark.parametrize("N,lever", CASES, ids=CASE_IDS)
def test_iterates_against_oracle(oracle, N, lever, seq):
    _, _, _, o = _sequence(seq, N)
    g = _run(seq, N, lever)
    label = f"slot {seq} {CASE_IDS[CASES.index((N, lever))]}"
    worst, eq = check_iterates(g, o, label, _form(N, lever))
    note(f"{label} iterates", handoffs=[list(c) for c in g.handoffs], equal_fraction=float(eq.mean()), **worst)
    if lever or N > 10:
        assert all(c == (0, 0, 0) for c in g.handoffs)


@pytest.mark.parametrize("N,lever", CASES, ids=CASE_IDS)
def test_nan_record_keeps_the_slot(oracle, N, lever):
    """A non-finite record at tick 2 in robot 5: its slot stays bitwise what tick 1 left, its next tick continues from
    there, and its neighbours are not disturbed."""
    recs = ws.trot_sequence(N).copy()
    recs[NAN_TICK, NAN_ROBOT, 7] = np.nan
    clean = ws.oracle_trot(N)
    one = ws.oracle_run(ws.oracle_params(N), recs, robots=[NAN_ROBOT])
    o = SimpleNamespace(res=clean.res.copy(), sol=clean.sol.copy(), states=[list(row) for row in clean.states])
    for t in range(recs.shape[0]):
        o.res[t, NAN_ROBOT], o.sol[t, NAN_ROBOT], o.states[t][NAN_ROBOT] = one.res[t, NAN_ROBOT], one.sol[t, NAN_ROBOT], one.states[t][NAN_ROBOT]
    assert o.res[NAN_TICK, NAN_ROBOT]["status"] == L.STATUS_NAN_INPUT
    g = run_ticks(N, [lever] * recs.shape[0], recs)
    label = f"slot nan {CASE_IDS[CASES.index((N, lever))]}"
    assert g.res[NAN_TICK, NAN_ROBOT]["status"] == L.STATUS_NAN_INPUT
    assert np.all(np.isnan(g.sol[NAN_TICK, NAN_ROBOT]))
    assert g.slots[NAN_TICK, NAN_ROBOT].tobytes() == g.slots[NAN_TICK - 1, NAN_ROBOT].tobytes()
    assert g.slots[NAN_TICK, NAN_ROBOT, 0] == 1.0
    check_all(g, o, recs, label, _form(N, lever))


# ---- e: the slot does not depend on the form that wrote it --------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 5, 10])
def test_slot_is_form_independent(oracle, N):
    """Tick 0 on the default handle (Schur form), tick 1 on the lever handle (Riccati form) on the same slots, tick 2
    on the default handle again: what every hand-off inside a sequence relies on."""
    recs = ws.trot_sequence(N)[:3]
    g = run_ticks(N, [False, True, False], recs)
    same = _run("trot", N, False)
    assert g.res[0].tobytes() == same.res[0].tobytes() and g.slots[0].tobytes() == same.slots[0].tobytes()
    assert g.res[1]["u0"].tobytes() != same.res[1]["u0"].tobytes(), "bitwise equal: tick 1 ran the same form"
    check_all(g, _slice(ws.oracle_trot(N), 0, 3), recs, f"slot forms N={N}", "both")


# ---- f: reading a slot, apart from writing it ---------------------------------------------------------------------------
@pytest.mark.parametrize("seq", SEQS)
@pytest.mark.parametrize("N", [3, 10, 13])
def test_transplant(oracle, N, seq):
    """The oracle's state after tick t, encoded into fresh slots; the device's tick t + 1 from them."""
    recs, q, r, o = _sequence(seq, N)
    T, B = recs.shape[:2]
    for t in range(T - 1):
        slots0 = np.stack([ws.encode(o.states[t][b], N) for b in range(B)])
        g = run_ticks(N, [False], recs[t + 1:t + 2], q, r, slots0=slots0)
        check_all(g, _slice(o, t + 1, t + 2), recs[t + 1:t + 2], f"slot transplant {seq} N={N} tick {t + 1}", _form(N, False))


@pytest.mark.parametrize("N", [5, 6, 11, 17, 20])
def test_one_mask_bit_in_any_word_decides(oracle, N):
    """The mask compare reads every word of a column: the oracle's state after tick 0 of the trot transplanted with
    one bit flipped (an entry recorded as zero that H does not have), in each word of the last column in turn and at
    the last bit of the mask, turns tick 1 from osqp_update_P into the re-init; the unflipped robots between them
    stay with osqp_update_P.  Afterwards the slot holds H's own pattern again."""
    recs, o = ws.trot_sequence(N), ws.oracle_trot(N)
    w = ws.layout(N)
    n = w.n
    flips = [(min(64 * k + 3, n - 1), n - 1) for k in range(w.MW)] + [(n - 1, n - 1), (0, 0)]  # (ri, j), ri <= j
    B = 2 * len(flips)
    states = [dict(o.states[0][b]) for b in range(B)]
    for i, (ri, j) in enumerate(flips):
        assert not states[2 * i]["pzero"][ri, j], "the entry must be a non-zero of H"
        states[2 * i]["pzero"] = states[2 * i]["pzero"].copy()
        states[2 * i]["pzero"][ri, j] = True
    g = run_ticks(N, [False], recs[1:2, :B], slots0=np.stack([ws.encode(s, N) for s in states]))
    assert np.all(ws.modes_of(o)[1, :B] == 1)
    assert g.modes[0].tolist() == [2.0, 1.0] * len(flips)
    assert np.all(g.res[0]["status"] == ws.SOLVED)
    for b in range(B):
        d = ws.decode(g.slots[0, b], N)
        assert np.array_equal(d["pzero"], o.states[1][b]["pzero"]) and d["mask_extra"] == 0
    check_bitwise(g, f"slot mask bit N={N}")
    keep = np.arange(1, B, 2)  # the unflipped robots are plain transplants
    sub = SimpleNamespace(res=g.res[:, keep], sol=g.sol[:, keep], slots=g.slots[:, keep], modes=g.modes[:, keep],
                          canary=g.canary, handoffs=g.handoffs)
    ref = SimpleNamespace(res=o.res[1:2, keep], sol=o.sol[1:2, keep], states=[[o.states[1][b] for b in keep]])
    check_all(sub, ref, recs[1:2, keep], f"slot mask bit N={N}", _form(N, False))


# ---- g: placement ---------------------------------------------------------------------------------------------------
PLACED = 4  # (a robot whose mu changes at tick 2: branches 0, 1, 2 over the three ticks)


@pytest.mark.parametrize("N", [10, 13])
def test_placement(N):
    """A robot's slots and results over three ticks do not depend on where in which batch it is solved."""
    recs = ws.trot_sequence(N)[:3]
    full = _run("trot", N, False)
    again = run_ticks(N, [False] * 3, recs)
    alone = run_ticks(N, [False] * 3, recs[:, PLACED:PLACED + 1])
    idx = np.r_[np.arange(64) % recs.shape[1], PLACED]
    last = run_ticks(N, [False] * 3, recs[:, idx])
    assert again.res.tobytes() == full.res[:3].tobytes() and again.sol.tobytes() == full.sol[:3].tobytes()
    assert again.slots.tobytes() == full.slots[:3].tobytes()
    for name, run, i in (("a batch of 1", alone, 0), ("index 64 of a batch of 65", last, 64)):
        for t in range(3):
            assert run.res[t, i].tobytes() == full.res[t, PLACED].tobytes(), f"{name}: result of tick {t}"
            assert run.sol[t, i].tobytes() == full.sol[t, PLACED].tobytes(), f"{name}: solution of tick {t}"
            assert run.slots[t, i].tobytes() == full.slots[t, PLACED].tobytes(), f"{name}: slot after tick {t}"
        assert all(run.canary)
    assert ws.modes_of(ws.oracle_trot(N))[:3, PLACED].tolist() == [0, 1, 2]


@pytest.mark.parametrize("N", [10, 13])
def test_zeroed_slot_is_a_cold_solve(N):
    """Zeroing one robot's slot before tick 2 makes that tick bitwise the cold kernel's for it; its neighbours stay
    warm, bitwise as in the undisturbed run."""
    recs = ws.trot_sequence(N)[:3]
    full = _run("trot", N, False)

    def zero(t, slots):
        if t == 2:
            slots[PLACED] = 0.0
    g = run_ticks(N, [False] * 3, recs, between=zero)
    with mpcqp.MpcQpSolver(_params(N, False)) as s:
        cold, cold_sol, _ = solve_gpu(s, recs[2, PLACED:PLACED + 1].copy())
    assert g.modes[2, PLACED] == 0
    assert g.res[2, PLACED].tobytes() == cold[0].tobytes() and g.sol[2, PLACED].tobytes() == cold_sol[0].tobytes()
    others = np.arange(recs.shape[1]) != PLACED
    assert np.all(g.modes[2, others] != 0)
    assert g.res[2, others].tobytes() == full.res[2, others].tobytes()
    assert g.slots[2, others].tobytes() == full.slots[2, others].tobytes()
    assert g.res[2, PLACED].tobytes() != full.res[2, PLACED].tobytes()


# ---- h: heavy weights (state weights x100, four feet down), where warm ticks sit above the cold solves' error ----------
# Sentinels by the rule above, per run (chained from the device's own slots / every tick from the oracle's state) and
# quantity, over handed-over and other robots together (profiles/warm_slot/heavy_weights.md has them apart).
# Measured: chained u0 8.5e-11, x 5.8e-10, z 5.8e-10, y 2.5e-10, rho 3.0e-8; transplanted u0 4.9e-11, x 2.7e-10,
# z 2.8e-10, y 2.3e-10, rho 3.2e-9 (its worst tick is the cold tick 0; the transplanted warm ticks sit at 1e-11).
SENT_HEAVY = {
    "chained": {"u0": 1e-9, "x": 1e-8, "z": 1e-8, "y": 1e-8, "rho": 1e-6},
    "transplanted": {"u0": 1e-9, "x": 1e-8, "z": 1e-8, "y": 1e-8, "rho": 1e-7},
}


def _heavy_errors(g, o, N):
    """[T][B] errors per quantity against the oracle (u0, x, z, y relative to max(|ref|_inf, 1), rho relative)."""
    T, B = g.res.shape
    e = {k: np.zeros((T, B)) for k in ("u0", "x", "z", "y", "rho")}
    for t in range(T):
        for b in range(B):
            ref, got = ws.unscaled(o.states[t][b]), ws.unscaled(ws.decode(g.slots[t, b], N))
            for k in ("x", "z", "y"):
                e[k][t, b] = np.max(np.abs(got[k] - ref[k])) / max(np.max(np.abs(ref[k])), 1.0)
            e["rho"][t, b] = abs(got["rho"] - ref["rho"]) / ref["rho"]
            e["u0"][t, b] = np.max(np.abs(g.res[t, b]["u0"] - o.res[t, b]["u0"])) / max(np.max(np.abs(o.res[t, b]["u0"])), 1.0)
    return e


def test_heavy_weights_slot_errors_by_tick(oracle):
    """tests/test_gpu_conditioning.py::test_heavy_weights_warm_ticks's sequence with the slot open: per tick the u0, x,
    z, y and rho errors against the oracle, for the robots the Schur form handed to the Riccati form and for the
    others, chained from the device's own slots and from the oracle's state of the tick before.  A robot counts as
    handed over when its result is bitwise the Riccati form's from the same slot.  With $MPCQP_SENTINEL_LOG set, the
    table goes to heavy_weights_table.md next to the log (profiles/warm_slot/heavy_weights.md has it, with a reading:
    no tick loses digits any more, 8.5e-11 in u0 chained and 5e-12 from the oracle's state)."""
    import os
    N, T, B = 10, 6, 48
    ticks = mpcqp.records.synthetic_go1_ticks(B, T, seed=7200, gait="trot", swing_ticks=3)
    recs = np.stack([mpcqp.assemble_compute_grf(s, N) for s in ticks])
    recs[:, :, L.REC_CONTACTS:L.REC_CONTACTS + 4] = 1.0  # four feet down
    p = _params(N, False, scale=100.0)
    o = ws.oracle_run(oracle.default_params(N, q=list(p.q_weights), r=list(p.r_weights)), recs)
    chained = run_ticks(N, [False] * T, recs, scale=100.0, shadow=True)
    slots_t = np.stack([np.zeros((B, ws.layout(N).SIZE))] +
                       [np.stack([ws.encode(o.states[t][b], N) for b in range(B)]) for t in range(T - 1)])
    planted = run_ticks(N, [False] * T, recs, scale=100.0, slots0=slots_t, shadow=True)
    lines = ["| run | tick | robots | count | iters equal | u0 | x | z | y | rho |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name, g in (("chained", chained), ("transplanted", planted)):
        label = f"slot heavy x100 {name}"
        check_mode_mask(g, o, recs, label)
        note(f"{label} scaling", **check_scaling(g, o, label))
        check_bitwise(g, label)
        handed = np.array([[g.res[t, b]["u0"].tobytes() == g.shadow[t, b]["u0"].tobytes() for b in range(B)] for t in range(T)])
        counts = np.array([c[1] + c[2] for c in g.handoffs])
        assert np.array_equal(handed.sum(1), counts), f"{label}: {handed.sum(1)} robots look handed over, {counts} counted"
        err = _heavy_errors(g, o, N)
        for t in range(T):
            np.testing.assert_array_equal(g.res[t]["status"], o.res[t]["status"], err_msg=f"{label} tick {t}")
            same = g.res[t]["iters"] == o.res[t]["iters"]
            assert np.mean(same) >= 0.97, f"{label} tick {t}"
            assert np.all(err["u0"][t] <= TOL_P1), f"{label} tick {t}: u0 off by {err['u0'][t].max():.3g}"
            for who, sel in (("handed over", handed[t]), ("Schur form", ~handed[t])):
                if sel.any():
                    worst = {k: float(v[t, sel].max()) for k, v in err.items()}
                    note(f"{label} tick {t} {who}", count=int(sel.sum()), iters_equal=float(np.mean(same[sel])), **worst)
                    lines.append(f"| {name} | {t} | {who} | {int(sel.sum())} | {np.mean(same[sel]):.2f} | " +
                                 " | ".join(f"{worst[k]:.1e}" for k in ("u0", "x", "z", "y", "rho")) + " |")
        for k, v in err.items():
            sentinel(v, SENT_HEAVY[name][k], f"{label} {k}")
        if name == "chained":
            sentinel(err["u0"][1:], 1e-6, "slot heavy x100 chained warm ticks u0 (the conditioning test's sentinel)")
            assert counts.sum() > 0
    log = os.environ.get("MPCQP_SENTINEL_LOG")
    if log:
        with open(os.path.join(os.path.dirname(log), "heavy_weights_table.md"), "w") as f:
            f.write("\n".join(lines) + "\n")
