"""The solves that select robots by control type (mpcqp_solve_batch_warm_typed_device,
mpcqp_balance_solve_typed_device): a selected robot's result row, solution row and warm slot are bitwise those
of the unselecting call on the same batch; of a robot that is not selected nothing is written (result and
solution buffers start as a NaN pattern no solve writes, warm slots as a previous tick left them); the
hand-off counters count the selected robots alone; and a robot that goes MPC -> QP -> MPC ends bitwise where
the gather / scatter path through mpcqp_copy_warm_slots_device puts it."""
import functools

import numpy as np
import pytest
import torch

import mpcqp
from degenerate_cases import SCHUR_GRAM_TOL, degenerate, gram_ratio
from mpcqp import balance as bal
from mpcqp.records import synthetic_go1_ticks

pytestmark = pytest.mark.gpu

B = 67
RD = mpcqp._lib.RESULT_DOUBLES
FILL = np.int64(0x7FF8DEAD0000BEEF)  # a NaN with a payload the kernels never produce


def _filled(shape):
    t = torch.empty(shape, dtype=torch.float64, device="cuda")
    t.view(torch.int64).fill_(int(FILL))
    return t


def _u64(t):
    return t.cpu().numpy().view(np.uint64).copy()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _records(N):
    """Three consecutive ticks of a trotting fleet whose stance pair switches every second tick."""
    return tuple(mpcqp.assemble_compute_grf(s, N) for s in synthetic_go1_ticks(B, 3, seed=40 + N, swing_ticks=2))


def _types(case, seed):
    if case == "all0":
        return np.zeros(B, np.int32)
    if case == "all1":
        return np.ones(B, np.int32)
    ty = np.random.default_rng(seed).integers(0, 2, B).astype(np.int32)
    ty[0], ty[B - 1] = 0, 1  # the robot that resets the hand-off counters is not selected
    return ty


def _warm(s, recs, slots, ty=None, want=1, res=None, sol=None):
    """One warm solve of the whole batch (ty None: mpcqp_solve_batch_warm_device) into FILL-ed buffers."""
    n = recs.shape[0]
    d_rec = torch.from_numpy(np.ascontiguousarray(recs)).cuda()
    res = _filled((n, RD)) if res is None else res
    sol = _filled((n, s.n)) if sol is None else sol
    if ty is None:
        s.solve_warm_device(d_rec.data_ptr(), n, slots.data_ptr(), res.data_ptr(), sol.data_ptr(), _stream())
    else:
        d_ty = torch.from_numpy(np.ascontiguousarray(ty, dtype=np.int32)).cuda()
        s.solve_warm_typed_device(d_rec.data_ptr(), n, slots.data_ptr(), d_ty.data_ptr(), want, res.data_ptr(),
                                  sol.data_ptr(), _stream())
    torch.cuda.synchronize()
    return _u64(res), _u64(sol)


@functools.lru_cache(maxsize=None)
def _reference(N):
    """Ticks 0 and 1 of the whole batch through mpcqp_solve_batch_warm_device from zero slots: per tick
    (results, solution, slots after).  Computed once per horizon and never modified."""
    out = []
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        slots = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
        for t in range(2):
            res, sol = _warm(s, _records(N)[t], slots)
            assert not np.any(res == np.uint64(FILL)) and not np.any(sol == np.uint64(FILL))
            out.append((res, sol, _u64(slots)))
    for a in out:
        for x in a:
            x.setflags(write=False)
    return tuple(out)


CASES = [(10, c, h, p) for c in ("random", "all0", "all1") for h in (1, 0) for p in (1, 3)] + [(20, "random", 1, 3)]


@pytest.mark.parametrize("N,case,hint,parts", CASES)
def test_typed_warm_solve(N, case, hint, parts):
    (_, _, slots0), (res1, sol1, slots1) = _reference(N)
    ty = _types(case, seed=3 * N + hint + parts)
    sel = ty == 1
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        s.set_split(parts)
        s.set_order_hint(hint)
        slots = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
        _warm(s, _records(N)[0], slots)  # tick 0, everyone: fills the slots and the handle's launch-order state
        assert np.array_equal(_u64(slots), slots0)
        res, sol = _warm(s, _records(N)[1], slots, ty, 1)
        order = s.launch_order()
        after = _u64(slots)
    assert np.array_equal(res[sel], res1[sel]), "selected robots: results"
    assert np.array_equal(sol[sel], sol1[sel]), "selected robots: solution"
    assert np.array_equal(after[sel], slots1[sel]), "selected robots: warm slots"
    assert np.all(res[~sel] == np.uint64(FILL)), "a result row of a robot that is not selected was written"
    assert np.all(sol[~sel] == np.uint64(FILL)), "a solution row of a robot that is not selected was written"
    assert np.array_equal(after[~sel], slots0[~sel]), "a warm slot of a robot that is not selected was written"
    # the launch order, per part: with the hint the selected robots, each once, then the empty places; without
    # it the identity with holes
    bnd = [B * i // parts for i in range(parts + 1)]
    for b0, b1 in zip(bnd[:-1], bnd[1:]):
        part = order[b0:b1]
        k = int(sel[b0:b1].sum())
        if hint:
            assert np.array_equal(np.sort(part[:k]), b0 + np.flatnonzero(sel[b0:b1])) and np.all(part[k:] == -1)
        else:
            assert np.array_equal(part, np.where(sel[b0:b1], np.arange(b0, b1), -1))


def test_launch_order_state_of_unselected_robots_is_kept():
    """The stored cost key and contact mask of a robot a typed call leaves out are those of its last solve: the
    next call's launch order is the rule of csrc/mpcqp_order.hip applied, per robot, to the records and results
    of the call that last solved it."""
    from test_gpu_order_hint import _assert_order
    N = 10
    recs = _records(N)
    ty = _types("random", seed=13)
    sel = ty == 1
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        s.set_split(1)
        s.set_order_hint(1)
        slots = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
        res0, sol0 = _warm(s, recs[0], slots)
        c0 = s.handoff_counts()
        res1, sol1 = _warm(s, recs[1], slots, ty, 1)
        c1 = s.handoff_counts()
        _warm(s, recs[2], slots)
        order = s.launch_order()
    last_recs = np.where(sel[:, None], recs[1], recs[0])
    last_res = np.where(sel[:, None], res1, res0)
    masks = lambda r: (r[:, mpcqp._lib.REC_CONTACTS:mpcqp._lib.REC_CONTACTS + 4] != 0.0)  # noqa: E731
    assert (masks(recs[0]) != masks(recs[1])).any(axis=1)[~sel].any(), "the ticks' contact sets must differ"
    _assert_order(order, recs[2], last_recs, (last_res, None, tuple(a + b for a, b in zip(c0, c1))), 1)


def test_mode_switch_matches_gather_scatter():
    """Three ticks, the types drawn anew each tick.  The reference keeps its member solver untouched on QP
    ticks (A1RobotControl.cpp:377-444); the path that did this so far gathers the MPC robots' slots into a
    compact buffer, solves, and scatters them back (tests/cpp/test_mode_switch_gpu.cpp checks it on the
    host path).  The typed solve leaves every slot bitwise where that path leaves it."""
    N = 10
    rng = np.random.default_rng(8)
    types = [rng.integers(0, 2, B).astype(np.int32) for _ in range(3)]
    types[0][:4], types[1][:4], types[2][:4] = [1, 1, 0, 1], [0, 1, 1, 0], [1, 1, 1, 0]  # robot 0: MPC, QP, MPC
    recs = _records(N)
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        slots = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
        typed = [_warm(s, recs[t], slots, types[t], 1) for t in range(3)]
        typed_slots = _u64(slots)
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        W = s.warm_state_size
        full = torch.zeros((B, W), dtype=torch.float64, device="cuda")
        for t in range(3):
            idx = np.flatnonzero(types[t] == 1).astype(np.int32)
            d_idx = torch.from_numpy(idx).cuda()
            compact = torch.zeros((len(idx), W), dtype=torch.float64, device="cuda")
            mpcqp._lib.copy_warm_slots_device(N, full.data_ptr(), d_idx.data_ptr(), compact.data_ptr(), 0, len(idx),
                                              _stream())
            res, sol = _warm(s, recs[t][idx], compact)
            mpcqp._lib.copy_warm_slots_device(N, compact.data_ptr(), 0, full.data_ptr(), d_idx.data_ptr(), len(idx),
                                              _stream())
            torch.cuda.synchronize()
            assert np.array_equal(typed[t][0][idx], res) and np.array_equal(typed[t][1][idx], sol), f"tick {t}"
            rest = types[t] != 1
            assert np.all(typed[t][0][rest] == np.uint64(FILL)) and np.all(typed[t][1][rest] == np.uint64(FILL))
        assert np.array_equal(typed_slots, _u64(full))
    # robot 0 skipped the middle tick: its slot is that of an all-MPC run of ticks 0 and 2 only
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        one = torch.zeros((1, s.warm_state_size), dtype=torch.float64, device="cuda")
        _warm(s, recs[0][:1], one)
        res, sol = _warm(s, recs[2][:1], one)
        assert np.array_equal(typed_slots[0], _u64(one)[0])
        assert np.array_equal(typed[2][0][0], res[0]) and np.array_equal(typed[2][1][0], sol[0])


@pytest.mark.parametrize("parts", [1, 3])
def test_typed_handoff_counts(parts):
    """Degenerate feet (tests/degenerate_cases.py): scale_kernel flags exactly the robots whose Gram pivot ratio
    is below the threshold, and wave_kernel counts each it hands to the Riccati form.  A typed call counts the
    selected robots alone."""
    N = 10
    recs = degenerate(_records(N)[0], N)
    g = gram_ratio(recs, N)
    flagged = g < SCHUR_GRAM_TOL
    assert not np.any((g > SCHUR_GRAM_TOL / 1.01) & (g < SCHUR_GRAM_TOL * 1.01)), "a ratio too near the threshold"
    ty = _types("random", seed=21)
    sel = ty == 1
    assert 0 < flagged[sel].sum() < flagged.sum()
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        s.set_split(parts)
        slots = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
        res_t, _ = _warm(s, recs, slots, ty, 1)
        typed = s.handoff_counts()
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        s.set_split(parts)
        slots = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
        res_w, _ = _warm(s, recs, slots)
        whole = s.handoff_counts()
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        idx = np.flatnonzero(sel)
        slots = torch.zeros((len(idx), s.warm_state_size), dtype=torch.float64, device="cuda")
        _warm(s, recs[idx], slots)
        alone = s.handoff_counts()
    print(f"hand-off counts: typed {typed}, selected robots alone {alone}, whole batch {whole}, "
          f"host prediction {int(flagged[sel].sum())} of {int(flagged.sum())}")
    assert whole[0] == flagged.sum()
    assert typed[0] == flagged[sel].sum()
    assert typed == alone
    assert np.array_equal(res_t[sel], res_w[sel])


def _row_bits(structured):
    return np.ascontiguousarray(structured).view(np.uint64).reshape(len(structured), RD)


@pytest.mark.parametrize("case", ["random", "all0", "all1"])
def test_typed_balance_solve(oracle, case):
    recs = bal.assemble_balance(mpcqp.synthetic_go1(B, seed=17, gait="mixed"))
    ty = _types(case, seed=5)
    sel = ty == 0
    d_rec = torch.from_numpy(recs).cuda()
    d_ty = torch.from_numpy(ty).cuda()
    bp = mpcqp.default_balance_params()
    with mpcqp.MpcQpSolver(mpcqp.default_params(10)) as s:
        whole, typed, null = _filled((B, RD)), _filled((B, RD)), _filled((B, RD))
        s.balance_solve_device(bp, d_rec.data_ptr(), B, whole.data_ptr(), _stream())
        s.balance_solve_typed_device(bp, d_rec.data_ptr(), B, d_ty.data_ptr(), 0, typed.data_ptr(), _stream())
        s.balance_solve_typed_device(bp, d_rec.data_ptr(), B, 0, 0, null.data_ptr(), _stream())
        torch.cuda.synchronize()
    whole, typed, null = _u64(whole), _u64(typed), _u64(null)
    assert np.array_equal(null, whole)
    assert np.array_equal(typed[sel], whole[sel])
    assert np.all(typed[~sel] == np.uint64(FILL))
    ref = oracle.balance_solve_batch(oracle.default_params(10), oracle.default_balance_params(), recs, 8)
    got = np.frombuffer(typed.tobytes(), dtype=mpcqp.RESULT_DTYPE)
    k = int(sel.sum())
    for f in mpcqp.RESULT_DTYPE.names:
        a, r = np.ascontiguousarray(got[f][sel]), np.ascontiguousarray(ref[f][sel]).astype(got[f].dtype)
        differ = (a.view(np.uint8).reshape(k, -1) != r.view(np.uint8).reshape(k, -1)).any(axis=1) if k else np.zeros(0)
        print(f"balance rows vs oracle, {f}: {int(differ.sum())} of {k} rows differ")
    for f in mpcqp.RESULT_DTYPE.names:
        a, r = np.ascontiguousarray(got[f][sel]), np.ascontiguousarray(ref[f][sel]).astype(got[f].dtype)
        assert np.array_equal(a.view(np.uint8), r.view(np.uint8)), f"selected rows vs the oracle: {f}"


def test_single_unselected_robot_writes_nothing():
    N = 10
    rec = _records(N)[0][:1]
    ty = np.array([0], np.int32)
    with mpcqp.MpcQpSolver(mpcqp.default_params(N)) as s:
        for hint in (1, 0):
            s.set_order_hint(hint)
            slots = _filled((1, s.warm_state_size))
            res, sol = _warm(s, rec, slots, ty, 1)  # (a failed call raises: MPCQP_OK)
            assert np.all(res == np.uint64(FILL)) and np.all(sol == np.uint64(FILL))
            assert np.all(_u64(slots) == np.uint64(FILL))
            assert s.handoff_counts() == (0, 0, 0)
        out = _filled((1, RD))
        d_rec = torch.from_numpy(bal.assemble_balance(mpcqp.synthetic_go1(1, seed=1))).cuda()
        d_ty = torch.from_numpy(np.array([1], np.int32)).cuda()
        s.balance_solve_typed_device(mpcqp.default_balance_params(), d_rec.data_ptr(), 1, d_ty.data_ptr(), 0,
                                     out.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert np.all(_u64(out) == np.uint64(FILL))
