"""The episode stage on the CPU: tests/episode_reference.py (Philox, draws, metrics, phases, scripts) against known
answers and hand-made cases, the ABI of the library against it, and the pool rows of the device tests under
tests/plant_reference.py.  No device."""
import ctypes
import re

import numpy as np
import pytest

import mpcqp
from mpcqp import _lib
from mpcqp import episode as me

import episode_cases as ec
import episode_reference as ep
import plant_reference as pr

DT = 0.0025


def test_philox_known_answers():
    """Philox4x32-10, the published vectors (Random123 kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{w:08x}" for w in ep.philox4x32(ctr, key)) == want


@pytest.mark.parametrize("count", [1, 3, 7])
def test_draws_stay_in_range_and_hit_every_index(count):
    seen_p, seen_s = set(), set()
    for i in range(2000):
        pi, si = ep.draw(0xDEADBEEF12345678, i % 50, i // 50, count, count)
        assert 0 <= pi < count and 0 <= si < count
        seen_p.add(pi)
        seen_s.add(si)
    assert seen_p == set(range(count)) and seen_s == set(range(count))
    assert ep.draw(5, 3, 9, 0, 0) == (0, 0)  # no pool, no scripts


def test_layouts_and_params_agree_with_the_library_and_the_header():
    L = _lib.load()
    assert L.mpcqp_episode_params_size() == ctypes.sizeof(mpcqp.EpisodeParams)
    assert L.mpcqp_episode_buffers_size() == ctypes.sizeof(mpcqp.EpisodeBuffers)
    assert mpcqp.episode_state_size() == ep.ES_SIZE == me.ES_SIZE
    p, r = mpcqp.default_episode_params(), ep.Params()
    for k in ("dt", "tilt_max", "height_min", "height_max", "max_ticks", "pool_count", "script_count",
              "script_segments", "log_len"):
        assert getattr(p, k) == getattr(r, k), k
    q = mpcqp.default_episode_params(seed=0x1234ABCD5678EF01, max_ticks=7)
    assert (q.seed[0], q.seed[1], q.max_ticks) == (0x5678EF01, 0x1234ABCD, 7)
    hdr = open(_lib.PKG_ROOT + "/../include/mpcqp.h").read()
    names = {"EP_END_FRESH": ep.END_FRESH, "EP_END_OUT_OF_REACH": ep.END_OUT_OF_REACH, "EP_END_FALLEN": ep.END_FALLEN,
             "EP_END_BAD_TORQUE": ep.END_BAD_TORQUE, "EP_END_ENVELOPE": ep.END_ENVELOPE,
             "EP_END_TIMEOUT": ep.END_TIMEOUT, "EP_END_COUNT": ep.END_COUNT, "EP_POOL_INIT": ep.POOL_INIT,
             "EP_POOL_EULER_D": ep.POOL_EULER_D, "EP_POOL_POS_D": ep.POOL_POS_D, "EP_POOL_SIZE": ep.POOL_SIZE,
             "EP_SEG_TICK": ep.SEG_TICK, "EP_SEG_CMD": ep.SEG_CMD, "EP_SEG_SIZE": ep.SEG_SIZE,
             "ES_PHASE": ep.ES_PHASE, "ES_TICK": ep.ES_TICK, "ES_EPISODE": ep.ES_EPISODE, "ES_POOL": ep.ES_POOL,
             "ES_SCRIPT": ep.ES_SCRIPT, "ES_SEG": ep.ES_SEG, "ES_METRICS": ep.ES_METRICS, "ES_SIZE": ep.ES_SIZE,
             "EM_TILT2_MAX": ep.EM_TILT2_MAX, "EM_Z_MIN": ep.EM_Z_MIN, "EM_Z_MAX": ep.EM_Z_MAX,
             "EM_ENERGY": ep.EM_ENERGY, "EM_TAU2": ep.EM_TAU2, "EM_ERR_V": ep.EM_ERR_V, "EM_ITERS": ep.EM_ITERS,
             "EM_NOT_SOLVED": ep.EM_NOT_SOLVED, "EM_LOW_CONTACT": ep.EM_LOW_CONTACT, "EM_START": ep.EM_START,
             "EM_END": ep.EM_END, "EM_SIZE": ep.EM_SIZE, "EL_EPISODE": ep.EL_EPISODE, "EL_POOL": ep.EL_POOL,
             "EL_SCRIPT": ep.EL_SCRIPT, "EL_LENGTH": ep.EL_LENGTH, "EL_REASON": ep.EL_REASON,
             "EL_METRICS": ep.EL_METRICS, "EL_SIZE": ep.EL_SIZE, "ET_EPISODES": ep.ET_EPISODES,
             "ET_TICKS": ep.ET_TICKS, "ET_REASON": ep.ET_REASON, "ET_SIZE": ep.ET_SIZE}
    for name, value in names.items():
        assert re.search(rf"^#define MPCQP_{name} {value}\s", hdr, flags=re.M), name
    for name in ("POOL_INIT", "POOL_EULER_D", "POOL_POS_D", "POOL_SIZE", "SEG_TICK", "SEG_CMD", "SEG_SIZE", "EL_SIZE",
                 "ET_SIZE", "END_COUNT"):
        assert getattr(me, name) == getattr(ep, name), name
    # the numpy dtypes are the rows
    for dt, base in ((mpcqp.EPISODE_STATE_DTYPE, ep.ES_METRICS), (mpcqp.EPISODE_LOG_DTYPE, ep.EL_METRICS)):
        for field, at in (("tilt2_max", ep.EM_TILT2_MAX), ("energy", ep.EM_ENERGY), ("err_v", ep.EM_ERR_V),
                          ("low_contact", ep.EM_LOW_CONTACT), ("start", ep.EM_START), ("end", ep.EM_END)):
            assert dt.fields[field][1] == 8 * (base + at), field
    assert mpcqp.EPISODE_LOG_DTYPE.fields["reason"][1] == 8 * ep.EL_REASON
    assert mpcqp.EPISODE_TOTALS_DTYPE.fields["reason"][1] == 8 * ep.ET_REASON
    assert ep.RESULT_DOUBLES == _lib.RESULT_DOUBLES
    assert mpcqp.RESULT_DTYPE.fields["status"][1] == 4 * ep.RESULT_STATUS_I32
    assert mpcqp.RESULT_DTYPE.fields["iters"][1] == 4 * ep.RESULT_ITERS_I32


def test_invalid_arguments_need_no_device():
    L = _lib.load()
    call = L.mpcqp_episode_device
    p = mpcqp.default_episode_params()
    ok = mpcqp.episode_buffers(64, 128)
    assert call(None, ctypes.byref(ok), 1, 16, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), None, 1, 16, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), ctypes.byref(ok), -1, 16, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), ctypes.byref(ok), 1, None, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), ctypes.byref(mpcqp.episode_buffers(0, 128)), 1, 16, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), ctypes.byref(mpcqp.episode_buffers(64, 0)), 1, 16, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), ctypes.byref(mpcqp.episode_buffers(64, 136)), 1, 16, None) == _lib.ERR_INVALID_ARG
    for bad in (dict(max_ticks=0), dict(dt=0.0), dict(pool_count=-1)):
        q = mpcqp.default_episode_params(**bad)
        assert call(ctypes.byref(q), ctypes.byref(ok), 1, 16, None) == _lib.ERR_INVALID_ARG, bad
    assert call(ctypes.byref(p), ctypes.byref(mpcqp.episode_buffers(64, 128, d_scripts=256)), 1, 16,
                None) == _lib.ERR_INVALID_ARG  # scripts without their counts
    q = mpcqp.default_episode_params(log_len=0)
    assert call(ctypes.byref(q), ctypes.byref(mpcqp.episode_buffers(64, 128, d_log=256)), 1, 16,
                None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), ctypes.byref(mpcqp.episode_buffers(64, 128, d_warm=256, warm_size=-1)), 1, 16,
                None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), ctypes.byref(ok), 0, None, None) == _lib.ERR_OK


def test_pack_helpers():
    row, z = ec.start_row([0.0, 0.8, -1.6])
    pool = mpcqp.pack_episode_pool([row, row], [[0, 0, 0.5], [0, 0, 0]], [[0, 0, z], [1, 2, z]])
    assert pool.shape == (2, ep.POOL_SIZE) and np.array_equal(pool[0, :20], row)
    assert np.array_equal(pool[1, ep.POOL_POS_D:ep.POOL_POS_D + 3], [1, 2, z]) and pool[0, ep.POOL_EULER_D + 2] == 0.5
    sc = mpcqp.pack_episode_scripts([[(0, (0, 0, 0), (0, 0, 0), False), (40, (0.3, 0, 0), (0, 0, 0.1), True)],
                                     [(0, (0, 0, 0), (0, 0, 0), False)]])
    assert sc.shape == (2, 2, ep.SEG_SIZE)
    assert np.array_equal(sc[0, 1], [40, 0.3, 0, 0, 0, 0, 0.1, 1.0]) and sc[1, 1, 0] == -1.0
    with pytest.raises(ValueError):
        mpcqp.pack_episode_scripts([[(5, (0, 0, 0), (0, 0, 0), False), (5, (0, 0, 0), (0, 0, 0), False)]])


def _run(name, B, missing=(), sizes=ec.SIZES, scripts=True):
    """A teacher-forced case on the restatement; yields (tick, arrays before, arrays after)."""
    p, events, T = ec.case_params(name, B)
    ar = ec.Arena(B, p, sizes, missing)
    h = ar.fill(ec.default_pool(p.pool_count), ec.default_scripts() if scripts else None)
    v = ar.views(h)
    v["cmd"][:] = ec.cmd_rows(B, 1)
    for t in range(T):
        for k, rows in ec.hand_rows(B, t, 3, events).items():
            v[k][:] = rows
        before = h.copy()
        ep.step(p, ar.stage_arrays(h), B)
        yield t, ar.views(before), ar.views(h.copy()), ar, p


def _log(v, p):
    return v["log"].reshape(-1, p.log_len, ep.EL_SIZE)


def test_every_end_reason_ends_an_episode_in_the_order_of_the_reasons():
    B = 16
    for t, _, v, ar, p in _run("each_reason", B):
        if t == 4:
            at4 = v["episode_state"][:, ep.ES_PHASE].copy()
            log4 = _log(v, p)[:, 0].copy()
        last = v
    # tick 0 the fresh end, tick 1 priming, ticks 2 .. 4 episode ticks 0 .. 2, tick 5 would be the time-out
    kinds = ("status1", "status2", "status3", "tilt", "low", "high", "all", None)
    want = {"status1": 1, "status2": 2, "status3": 3, "tilt": 4, "low": 4, "high": 4, "all": 1}
    for b in range(B):
        k = kinds[b % 8]
        if k is None:
            assert at4[b] == 1.0  # still running at tick 4
            assert _log(last, p)[b, 0, ep.EL_REASON] == ep.END_TIMEOUT and _log(last, p)[b, 0, ep.EL_LENGTH] == 4.0
        else:
            assert at4[b] == 2.0 and log4[b, ep.EL_REASON] == want[k] and log4[b, ep.EL_LENGTH] == 3.0, (b, k)
    tot = last["totals"]
    assert np.all(tot[:, ep.ET_REASON + ep.END_FRESH] == 1.0)  # the fresh start, once, and no log row for it
    assert np.array_equal(tot[:, ep.ET_REASON + 1:ep.ET_REASON + 6].sum(1), tot[:, ep.ET_EPISODES])
    assert np.all(tot[:, ep.ET_EPISODES] >= 1.0)


def test_fresh_start_draws_and_primes():
    B = 5
    runs = list(_run("none_end", B))
    _, before, v0, ar, p = runs[0]
    es = v0["episode_state"]
    assert np.all(es[:, ep.ES_PHASE] == 2.0) and np.all(es[:, ep.ES_EPISODE] == 0.0)
    pool = v0["pool"]
    for b in range(B):
        pi, si = ep.draw(p.seed, b, 0, p.pool_count, p.script_count)
        assert (es[b, ep.ES_POOL], es[b, ep.ES_SCRIPT]) == (pi, si)
        assert np.array_equal(v0["plant_init"][b], pool[pi, :20])
    assert not v0["plant_state"].any() and not v0["joint_torques"].any()
    assert np.array_equal(v0["log"], before["log"]) and not v0["totals"][:, ep.ET_EPISODES].any()
    for name in ec.SLOTS + ("results", "states"):  # untouched until the priming tick
        assert np.array_equal(v0[name], before[name]), name
    _, before, v1, _, _ = runs[1]
    for name in ec.SLOTS + ("results",):
        assert not v1[name].any(), name
    assert not v1["counter"][:B].any() and np.array_equal(v1["counter"][B:], before["counter"][B:])
    for b in range(B):
        pi = int(es[b, ep.ES_POOL])
        assert np.array_equal(v1["states"][b, ep.ST_EULER_D:ep.ST_EULER_D + 3], pool[pi, 20:23])
        assert np.array_equal(v1["states"][b, ep.ST_POS_D:ep.ST_POS_D + 3], pool[pi, 23:26])
    keep = np.ones(ep.ST_SIZE, bool)
    keep[ep.ST_EULER_D:ep.ST_POS_D + 3] = False
    keep[ep.ST_POS:ep.ST_POS + 3] = keep[ep.ST_LIN_VEL:ep.ST_LIN_VEL + 3] = False  # zeroed: an estimator slot is given
    assert not v1["states"][:, ep.ST_POS:ep.ST_POS + 3].any() and not v1["states"][:, ep.ST_LIN_VEL:ep.ST_LIN_VEL + 3].any()
    assert np.array_equal(v1["states"][:, keep], before["states"][:, keep])
    assert np.all(v1["episode_state"][:, ep.ES_PHASE] == 1.0) and not v1["episode_state"][:, ep.ES_TICK].any()
    assert np.array_equal(v1["episode_state"][:, ep.ES_METRICS + ep.EM_START], v1["plant_out"][:, ep.PT_POS])
    # and nobody ends afterwards
    _, _, last, _, _ = runs[-1]
    assert np.all(last["episode_state"][:, ep.ES_TICK] == len(runs) - 2)
    assert not last["totals"][:, ep.ET_EPISODES].any() and np.array_equal(last["log"], before["log"])


def test_metrics_are_the_sums_of_the_rows():
    """The accumulated metrics against direct numpy over the hand-written rows (to rounding)."""
    B = 3
    p, events, T = ec.case_params("none_end", B)
    rows = [ec.hand_rows(B, t, 3, events) for t in range(T)]
    *_, (_, _, v, _, _) = _run("none_end", B, scripts=False)
    m = v["episode_state"][:, ep.ES_METRICS:ep.ES_METRICS + ep.EM_SIZE]
    run = rows[2:]  # tick 0 fresh, tick 1 priming
    cm = ec.cmd_rows(B, 1)
    tau = np.array([r["joint_torques"] for r in run])
    qd = np.array([r["sensors"][:, ep.SN_JOINT_VEL:ep.SN_JOINT_VEL + 12] for r in run])
    po = np.array([r["plant_out"] for r in run])
    np.testing.assert_allclose(m[:, ep.EM_TAU2], (tau ** 2).sum((0, 2)), rtol=1e-13)
    np.testing.assert_allclose(m[:, ep.EM_ENERGY], (tau * qd).sum((0, 2)) * p.dt, rtol=1e-12, atol=1e-15)
    import estimator_reference as er
    R = er.quat_to_rot(po[..., ep.PT_QUAT:ep.PT_QUAT + 4].reshape(-1, 4)).reshape(len(run), B, 3, 3)
    vb = np.einsum("tbji,tbj->tbi", R, po[..., ep.PT_LIN_VEL:ep.PT_LIN_VEL + 3])
    np.testing.assert_allclose(m[:, ep.EM_ERR_V], ((vb[..., 0] - cm[:, 0]) ** 2).sum(0), rtol=1e-12)
    np.testing.assert_allclose(m[:, ep.EM_ERR_V + 1], ((vb[..., 1] - cm[:, 1]) ** 2).sum(0), rtol=1e-12)
    np.testing.assert_allclose(m[:, ep.EM_ERR_V + 2], ((po[..., ep.PT_ANG_VEL + 2] - cm[:, 5]) ** 2).sum(0), rtol=1e-12)
    ri = np.array([r["results"].view(np.int32).reshape(B, -1) for r in run])
    assert np.array_equal(m[:, ep.EM_ITERS], ri[..., ep.RESULT_ITERS_I32].sum(0))
    assert np.array_equal(m[:, ep.EM_NOT_SOLVED], (ri[..., ep.RESULT_STATUS_I32] != 1).sum(0))
    assert np.array_equal(m[:, ep.EM_LOW_CONTACT], (po[..., ep.PT_CONTACTS:ep.PT_CONTACTS + 4].sum(-1) < 2).sum(0))
    allpo = np.array([r["plant_out"] for r in rows[1:]])  # the start included
    assert np.array_equal(m[:, ep.EM_Z_MIN], allpo[..., ep.PT_POS + 2].min(0))
    assert np.array_equal(m[:, ep.EM_Z_MAX], allpo[..., ep.PT_POS + 2].max(0))
    assert np.array_equal(m[:, ep.EM_START + 2], rows[1]["plant_out"][:, ep.PT_EULER + 2])
    assert np.array_equal(m[:, ep.EM_END], rows[-1]["plant_out"][:, ep.PT_POS])


def test_log_ring_wraps():
    """log_len = 2, max_ticks = 3: episode e lands in row e % 2, the third overwrites the first."""
    B = 2
    seen = {}
    for t, _, v, ar, p in _run("ring", B):
        log = _log(v, p)
        for b in range(B):
            e = int(v["totals"][b, ep.ET_EPISODES])
            if e and (b, e - 1) not in seen:
                seen[b, e - 1] = t
                row = log[b, (e - 1) % 2]
                assert row[ep.EL_EPISODE] == e - 1 and row[ep.EL_LENGTH] == 3.0 and row[ep.EL_REASON] == ep.END_TIMEOUT
                pi, si = ep.draw(p.seed, b, e - 1, p.pool_count, p.script_count)
                assert (row[ep.EL_POOL], row[ep.EL_SCRIPT]) == (pi, si)
    # episode e: priming at tick 1 + 4 e, three ticks, the end at tick 4 + 4 e
    assert seen == {(b, e): 4 + 4 * e for b in range(B) for e in range(3)}
    assert np.array_equal(log[:, 0, ep.EL_EPISODE], [2.0, 2.0]) and np.array_equal(log[:, 1, ep.EL_EPISODE], [1.0, 1.0])
    assert np.all(v["totals"][:, ep.ET_TICKS] == 9.0) and np.all(v["totals"][:, ep.ET_REASON + ep.END_TIMEOUT] == 3.0)


def test_script_segments_are_written_at_their_ticks_and_reissued_after_a_restart():
    """max_ticks = 6: the cmd row before episode tick k holds the script's segment in force at k; script 0 starts
    at tick 0 (written by the priming tick), script 1 at tick 1 (until then the row keeps what it had)."""
    B = 12
    p, _, _ = ec.case_params("none_end", B)
    p.max_ticks = 6
    ar = ec.Arena(B, p)
    sc = ec.default_scripts()
    h = ar.fill(ec.default_pool(3), sc)
    v = ar.views(h)
    v["cmd"][:] = ec.cmd_rows(B, 1)
    used = set()
    for t in range(2 + 8 * 3):
        for k, rows in ec.hand_rows(B, t, 3, {}).items():
            v[k][:] = rows
        prev = v["cmd"].copy()
        ep.step(p, ar.stage_arrays(h), B)
        es = v["episode_state"]
        for b in range(B):
            if es[b, ep.ES_PHASE] != 1.0:
                assert np.array_equal(v["cmd"][b], prev[b])  # an ending tick writes no command
                continue
            si, k = int(es[b, ep.ES_SCRIPT]), int(es[b, ep.ES_TICK])  # the command now there is for episode tick k
            used.add(si)
            starts = [s for s in range(3) if sc[si, s, 0] == k]
            if starts:
                assert np.array_equal(v["cmd"][b, :7], sc[si, starts[0], 1:]), (t, b)
                assert es[b, ep.ES_SEG] == starts[0] + 1
            else:
                assert np.array_equal(v["cmd"][b], prev[b]), (t, b)
    assert used == {0, 1} and np.all(v["totals"][:, ep.ET_EPISODES] >= 2.0)


@pytest.mark.parametrize("missing", ec.OPTIONAL)
def test_a_missing_buffer_is_skipped(missing):
    """Each optional buffer absent in turn: its memory keeps the canary, and the rest goes on."""
    for t, before, v, ar, p in _run("each_reason", 9, missing=(missing,)):
        assert np.array_equal(v[missing], before[missing])
    assert np.all(v["episode_state"][:, ep.ES_EPISODE] >= 1.0)
    if missing != "totals":
        assert np.all(v["totals"][:, ep.ET_EPISODES] >= 1.0)


def test_pool_rows_of_the_device_test_behave_as_described():
    """The two pool rows of tests/test_gpu_tick_episode.py under zero torques and min_height 0.25: the 0.29 m
    stance keeps status 0, the crouch (trunk under 0.25 m) has status 2 after its first integrating tick at the
    latest and is frozen from then on."""
    stance, zs = ec.start_row([0.0, 0.8, -1.6])
    crouch, zc = ec.start_row([0.0, 1.2, -2.4])
    assert 0.28 < zs < 0.30 and zc < 0.25
    p = pr.default_params(min_height=0.25)
    init = np.stack([stance, crouch])
    pl = pr.Plant(p, 2)
    out, _, _ = pl.step(DT, np.zeros((2, 12)), init)
    assert out["status"][0] == 0.0
    out, wrote, _ = pl.step(DT, np.zeros((2, 12)), init)
    assert out["status"][0] == 0.0 and out["status"][1] == 2.0 and wrote[0]
    frozen = out["root_pos"][1].copy()
    for _ in range(6):
        out, wrote, _ = pl.step(DT, np.zeros((2, 12)), init)
        assert out["status"][0] == 0.0 and out["root_pos"][0, 2] > 0.25
        assert not wrote[1] and np.array_equal(out["root_pos"][1], frozen)
