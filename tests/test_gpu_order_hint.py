"""The wave path's launch-order hint (mpcqp_set_order_hint, csrc/mpcqp_order.hip): a solve that
dispatches its robots by the previous call's cost gives bitwise the results of one that dispatches
them in input order — results, full solutions, hand-off counts and warm slots — and the order is the
documented one: per batch part, robots whose contact mask changed since the previous call first,
then descending cost key, then batch index; the identity on a handle's first call and after the
batch size or the split changed.  Result buffers start as a NaN pattern no solve writes, so a robot
that no block solved shows."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mpcqp  # noqa: E402
from degenerate_cases import degenerate  # noqa: E402
from mpcqp.records import synthetic_go1_ticks  # noqa: E402

pytestmark = pytest.mark.gpu

RD = mpcqp._lib.RESULT_DOUBLES
C0 = mpcqp._lib.REC_CONTACTS
FILL = np.int64(0x7FF8DEAD0000BEEF)  # a NaN with a payload the kernels never produce
# csrc/mpcqp_internal.h order_cost / order_key
KEY_MAX, KEY_SHIFT, RHO_WEIGHT, COST_MAX = 63, 3, 15, 1 << 20


def _filled(shape):
    t = torch.empty(shape, dtype=torch.float64, device="cuda")
    t.view(torch.int64).fill_(int(FILL))
    return t


def _u64(t):
    return t.cpu().numpy().view(np.uint64).copy()


def _solve(s, recs, state=None):
    """One solve on the current stream: (results, solution, hand-off counts, launch order)."""
    B = recs.shape[0]
    d_rec = torch.from_numpy(np.ascontiguousarray(recs)).cuda()
    res, sol = _filled((B, RD)), _filled((B, s.n))
    stream = torch.cuda.current_stream().cuda_stream
    if state is None:
        s.solve_device(d_rec.data_ptr(), B, res.data_ptr(), sol.data_ptr(), stream)
    else:
        s.solve_warm_device(d_rec.data_ptr(), B, state.data_ptr(), res.data_ptr(), sol.data_ptr(), stream)
    torch.cuda.synchronize()
    return _u64(res), _u64(sol), s.handoff_counts(), s.launch_order()


def _assert_solved(out):
    res, sol = out[0], out[1]
    assert not np.any(res == np.uint64(FILL)), "a result row was not written"
    assert not np.any(sol == np.uint64(FILL)), "a solution row was not written"


def _assert_same(got, ref, what):
    _assert_solved(got)
    _assert_solved(ref)
    assert np.array_equal(got[0], ref[0]), f"{what}: results"
    assert np.array_equal(got[1], ref[1]), f"{what}: solution"
    assert got[2] == ref[2], f"{what}: hand-off counts"


def _masks(recs):
    return ((recs[:, C0:C0 + 4] != 0.0) * np.array([1, 2, 4, 8])).sum(axis=1)


def _keys(res_u64):
    r = np.frombuffer(res_u64.tobytes(), dtype=mpcqp.RESULT_DTYPE)
    cost = np.clip(r["iters"], 0, COST_MAX).astype(np.int64) + RHO_WEIGHT * np.clip(r["rho_updates"], 0, COST_MAX)
    return np.minimum(cost >> KEY_SHIFT, KEY_MAX)


def _bounds(B, parts):
    parts = max(1, min(parts, B))
    return [B * i // parts for i in range(parts + 1)]


def _expected_order(recs, prev_recs, prev_res, parts):
    """The rule of csrc/mpcqp_order.hip applied to the previous call's records and results."""
    changed = _masks(recs) != _masks(prev_recs)
    sort_key = np.where(changed, 0, KEY_MAX + 1) + (KEY_MAX - _keys(prev_res))
    bnd = _bounds(recs.shape[0], parts)
    out = []
    for b0, b1 in zip(bnd[:-1], bnd[1:]):
        out.append(b0 + np.argsort(sort_key[b0:b1], kind="stable"))
    return np.concatenate(out).astype(np.int32)


def _assert_order(order, recs, prev_recs, prev_out, parts):
    """`order` is the rule's order given the previous call's records and output.  A robot the Schur
    form handed over after iterating (hand-off counts 1 and 2) cost more than its results show, its
    Riccati solve and the Schur iterations before it: at most that many robots may stand ahead of
    the place their results give them, inside their own contacts-changed group, and the others'
    order among themselves is exactly the rule's."""
    want = _expected_order(recs, prev_recs, prev_out[0], parts)
    late = prev_out[2][1] + prev_out[2][2]
    if late == 0 or np.array_equal(order, want):
        assert np.array_equal(order, want)
        return
    _assert_partwise_permutation(order, recs.shape[0], parts)
    changed = _masks(recs) != _masks(prev_recs)
    promoted = set()
    a, b = list(order), list(want)
    while a != b:
        i = next(k for k in range(len(a)) if a[k] != b[k])
        g = a[i]  # stands earlier than its results say: a robot whose real cost is higher
        assert b.index(g) > i and changed[g] == changed[b[i]], f"robot {g} is out of order"
        promoted.add(g)
        a.remove(g)
        b.remove(g)
        assert len(promoted) <= late, "more robots out of the results' order than late hand-offs"


def _assert_partwise_permutation(order, B, parts):
    bnd = _bounds(B, parts)
    assert order.shape == (B,)
    for b0, b1 in zip(bnd[:-1], bnd[1:]):
        assert np.array_equal(np.sort(order[b0:b1]), np.arange(b0, b1))


def _odd_batch(horizon, B, seed):
    """Mixed-gait robots with one non-finite record and one with exactly rank-deficient feet (all four
    at the body origin: the Schur form hands it to the Riccati form)."""
    recs = mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(B, seed=seed, gait="mixed", mixed_mu=True), horizon)
    if B > 8:
        recs[5, mpcqp._lib.REC_X0 + 3] = np.nan
        recs[7:8] = degenerate(recs[7:8], horizon)
    return recs


def _handles(params):
    on, off = mpcqp.MpcQpSolver(params), mpcqp.MpcQpSolver(params)
    on.set_order_hint(1)
    off.set_order_hint(0)
    return on, off


def _twice(params, recs, parts):
    """The same records solved twice on one handle with the hint, against a handle without it."""
    B = recs.shape[0]
    on, off = _handles(params)
    with on, off:
        on.set_split(parts)
        off.set_split(parts)
        ref = _solve(off, recs)
        assert np.array_equal(ref[3], np.arange(B))
        one = _solve(on, recs)
        _assert_same(one, ref, "call 1")
        assert np.array_equal(one[3], np.arange(B)), "the first call's order is the identity"
        two = _solve(on, recs)
        _assert_same(two, ref, "call 2")
        _assert_partwise_permutation(two[3], B, parts)
        _assert_order(two[3], recs, recs, one, parts)
    return ref, two


@pytest.mark.parametrize("parts", [1, 2, 3])
def test_same_records_twice(parts):
    recs = _odd_batch(10, 67, seed=11)
    ref, two = _twice(mpcqp.default_params(10), recs, parts)
    r = np.frombuffer(ref[0].tobytes(), dtype=mpcqp.RESULT_DTYPE)
    assert r["status"][5] == mpcqp._lib.STATUS_NAN_INPUT and ref[2][0] == 1  # the odd robots are in
    assert ref[2][1] + ref[2][2] == 0  # (no late hand-off: the order is exactly the results' rule)
    assert len(np.unique(_keys(ref[0]))) > 3 and not np.array_equal(two[3], np.arange(67))


@pytest.mark.parametrize("parts", [1, 3])
def test_keys_beyond_the_clamp(parts):
    # nothing converges to 1e-9 in 600 iterations: every finite robot's cost is past the clamp
    p = mpcqp.default_params(10, eps_abs=1e-9, eps_rel=1e-9, max_iter=600)
    recs = _odd_batch(10, 67, seed=12)
    ref, _ = _twice(p, recs, parts)
    r = np.frombuffer(ref[0].tobytes(), dtype=mpcqp.RESULT_DTYPE)
    assert np.sum(r["iters"] == 600) > 30
    assert np.max(r["iters"] + RHO_WEIGHT * r["rho_updates"]) >> KEY_SHIFT > KEY_MAX


@pytest.mark.parametrize("horizon,batch,parts", [(10, 1, 1), (10, 3, 3), (10, 1500, 1), (20, 33, 1)])
def test_edge_sizes_and_sort_loop(horizon, batch, parts):
    # one robot; one robot per part; more robots than the sort's workgroup has threads; Riccati kernel
    _twice(mpcqp.default_params(horizon), _odd_batch(horizon, batch, seed=13), parts)


def test_stale_state_gives_identity():
    p = mpcqp.default_params(10)
    sizes = [67, 41, 67]
    on, off = _handles(p)
    with on, off:
        for i, B in enumerate(sizes):
            recs = _odd_batch(10, B, seed=20 + i)
            got = _solve(on, recs)
            _assert_same(got, _solve(off, recs), f"call {i}")
            assert np.array_equal(got[3], np.arange(B)), f"call {i}: the batch size changed"
        # the same size under another split is another layout
        on.set_split(2)
        off.set_split(2)
        got = _solve(on, recs)
        _assert_same(got, _solve(off, recs), "split changed")
        assert np.array_equal(got[3], np.arange(sizes[-1]))
        # and back to one part: part 1's layout of the split call must not be trusted later
        on.set_split(1)
        off.set_split(1)
        prev = _solve(on, recs)
        assert np.array_equal(prev[3], np.arange(sizes[-1]))
        on.set_split(2)
        off.set_split(2)
        got = _solve(on, recs)
        _assert_same(got, _solve(off, recs), "split changed back")
        assert np.array_equal(got[3], np.arange(sizes[-1]))


def _tick_records(horizon=10):
    return [mpcqp.assemble_compute_grf(s, horizon) for s in synthetic_go1_ticks(67, 4, seed=31, swing_ticks=2)]


@pytest.mark.parametrize("parts", [1, 2])
def test_cold_ticks(parts):
    ticks = _tick_records()
    on, off = _handles(mpcqp.default_params(10))
    with on, off:
        on.set_split(parts)
        off.set_split(parts)
        prev = None
        n_changed = 0
        for t, recs in enumerate(ticks):
            got = _solve(on, recs)
            _assert_same(got, _solve(off, recs), f"tick {t}")
            if prev is not None:
                _assert_order(got[3], recs, prev[0], prev[1], parts)
                changed = _masks(recs) != _masks(prev[0])
                bnd = _bounds(67, parts)
                for b0, b1 in zip(bnd[:-1], bnd[1:]):  # the changed robots lead their part
                    k = int(changed[b0:b1].sum())
                    assert changed[got[3][b0:b0 + k]].all() and not changed[got[3][b0 + k:b1]].any()
                    n_changed += k
            prev = (recs, got)
    assert 0 < n_changed < 3 * 67


def test_warm_ticks():
    ticks = _tick_records()
    on, off = _handles(mpcqp.default_params(10))
    with on, off:
        st_on = torch.zeros((67, on.warm_state_size), dtype=torch.float64, device="cuda")
        st_off = torch.zeros_like(st_on)
        prev = None
        for t, recs in enumerate(ticks):
            got = _solve(on, recs, st_on)
            _assert_same(got, _solve(off, recs, st_off), f"tick {t}")
            assert np.array_equal(_u64(st_on), _u64(st_off)), f"tick {t}: warm slots"
            if prev is not None:
                _assert_order(got[3], recs, prev[0], prev[1], 1)
            prev = (recs, got)


def test_captured_solve_follows_the_hint():
    ticks = _tick_records()[:3]
    B = 67
    on, off = _handles(mpcqp.default_params(10))
    with on, off:
        on.reserve(B)
        d_rec = torch.from_numpy(ticks[0]).cuda()
        res, sol = _filled((B, RD)), _filled((B, on.n))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # (capture launches nothing)
            on.solve_device(d_rec.data_ptr(), B, res.data_ptr(), sol.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
        orders, prev = [], None
        for t, recs in enumerate(ticks):
            d_rec.copy_(torch.from_numpy(recs))
            res.view(torch.int64).fill_(int(FILL))
            sol.view(torch.int64).fill_(int(FILL))
            g.replay()
            torch.cuda.synchronize()
            got = (_u64(res), _u64(sol), on.handoff_counts(), on.launch_order())
            _assert_same(got, _solve(off, recs), f"replay {t}")
            if prev is None:
                assert np.array_equal(got[3], np.arange(B))
            else:
                _assert_order(got[3], recs, prev[0], prev[1], 1)
            orders.append(got[3])
            prev = (recs, got)
    assert np.array_equal(orders[0], np.arange(B))
    assert not np.array_equal(orders[1], orders[0]) and not np.array_equal(orders[2], orders[1])
