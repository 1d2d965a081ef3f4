"""mpcqp_episode_device alone, teacher-forced: the host writes the plant_out, torque, sensor, cmd and result rows
by hand tick by tick (no plant and no solve run), and after every tick every double of every buffer the stage may
write, and of the guard gaps between the buffers, is compared bitwise with tests/episode_reference.py.  Every
buffer starts as a canary pattern: exactly the restarting robots' rows become zero, nothing else changes."""
import numpy as np
import pytest
import torch

import mpcqp

import episode_cases as ec
import episode_reference as ep

pytestmark = pytest.mark.gpu

BATCHES = (1, 5, 67)  # one robot, a partial wave, more than one workgroup and not a multiple of 16


def _device_params(p):
    return mpcqp.default_episode_params(dt=p.dt, tilt_max=p.tilt_max, height_min=p.height_min,
                                        height_max=p.height_max, seed=p.seed, max_ticks=p.max_ticks,
                                        pool_count=p.pool_count, script_count=p.script_count,
                                        script_segments=p.script_segments, log_len=p.log_len)


def _buffers(ar, d):
    base = d.data_ptr()
    at = lambda name: 0 if name in ar.missing else base + 8 * ar.at[name][0]
    size = lambda name: ar.sizes[name]
    return mpcqp.episode_buffers(
        at("plant_out"), at("plant_state"), at("plant_init"), at("joint_torques"), at("sensors"), at("cmd"),
        at("results"), at("pool"), at("scripts"), at("states"), at("counter"), at("log"), at("totals"),
        at("est_state"), size("est_state"), at("plan_state"), size("plan_state"), at("cmd_state"), size("cmd_state"),
        at("policy_state"), size("policy_state"), at("warm"), size("warm"))


def _check_rows(ar, B, before, after, tick):
    """Exactly the restarting robots' rows are zero; no other robot's double changed."""
    phase0 = before["episode_state"][:, ep.ES_PHASE]
    phase1 = after["episode_state"][:, ep.ES_PHASE]
    primed = phase0 == 2.0
    ended = (phase0 != 2.0) & (phase1 == 2.0)
    for names, who in ((ec.SLOTS + ("results",), primed), (("plant_state", "joint_torques"), ended)):
        for name in names:
            if name in ar.missing:
                continue
            assert not after[name][who].any(), f"tick {tick}: {name} of a restarting robot is not zero"
            assert np.array_equal(after[name][~who].view(np.int64), before[name][~who].view(np.int64)), \
                f"tick {tick}: {name} of a robot that does not restart changed"
    if "counter" not in ar.missing:
        assert not after["counter"][:B][primed].any()
        assert np.array_equal(after["counter"][:B][~primed], before["counter"][:B][~primed])
        assert np.array_equal(after["counter"][B:], before["counter"][B:])


def _drive(name, B, missing=(), sizes=ec.SIZES):
    p, events, T = ec.case_params(name, B)
    ar = ec.Arena(B, p, sizes, missing)
    h = ar.fill(ec.default_pool(p.pool_count), ec.default_scripts())
    v = ar.views(h)
    v["cmd"][:] = ec.cmd_rows(B, 1)
    d = torch.from_numpy(h.copy()).cuda()
    assert d.data_ptr() % 16 == 0
    dp, bf = _device_params(p), _buffers(ar, d)
    stream = torch.cuda.current_stream().cuda_stream
    es_ptr = d.data_ptr() + 8 * ar.at["episode_state"][0]
    for t in range(T):
        for k, rows in ec.hand_rows(B, t, 3, events).items():
            v[k][:] = rows
            off, n, _ = ar.at[k]
            d[off:off + n].copy_(torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)))
        before = h.copy()
        ep.step(p, ar.stage_arrays(h), B)
        mpcqp.episode_device(dp, bf, B, es_ptr, stream)
        torch.cuda.synchronize()
        got = d.cpu().numpy()
        gv = ar.views(got)
        for k in v:
            assert np.array_equal(gv[k].view(np.int64) if k != "counter" else gv[k],
                                  v[k].view(np.int64) if k != "counter" else v[k]), f"{name} B={B} tick {t}: {k} differs"
        assert np.array_equal(ar.guards(got).view(np.int64), ar.guards(before).view(np.int64)), f"tick {t}: a guard gap changed"
        assert np.array_equal(got.view(np.int64), h.view(np.int64))
        _check_rows(ar, B, ar.views(before), gv, t)
    return ar.views(got), p


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", ec.CASES)
def test_stage_is_bitwise_the_restatement(name, B):
    """No robot ends; every robot ends on one tick; two robots of a wave end while their quad neighbours run on;
    each end reason (and all at once) and the fresh start; non-finite pose entries; log_len 2 over three
    episodes."""
    v, p = _drive(name, B)
    tot = v["totals"]
    assert np.all(tot[:, ep.ET_REASON + ep.END_FRESH] == 1.0)
    if name == "none_end":
        assert not tot[:, ep.ET_EPISODES].any() and np.all(v["episode_state"][:, ep.ES_PHASE] == 1.0)
    if name == "all_end":
        assert np.all(tot[:, ep.ET_REASON + ep.END_FALLEN] == 1.0)
    if name == "two_of_a_wave" and B > 3:
        assert np.array_equal(np.flatnonzero(tot[:, ep.ET_EPISODES]), [1, 3])
    if name == "each_reason" and B >= 8:
        assert np.all(tot[:, ep.ET_REASON:ep.ET_REASON + ep.END_COUNT].sum(0) > 0)  # every reason was met
    if name == "non_finite":
        assert np.all(tot[:, ep.ET_REASON + ep.END_ENVELOPE] >= 1.0)
    if name == "ring":
        assert np.all(tot[:, ep.ET_EPISODES] == 3.0)
        assert np.all(v["log"].reshape(B, 2, ep.EL_SIZE)[:, 0, ep.EL_EPISODE] == 2.0)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("missing", ec.OPTIONAL)
def test_each_optional_pointer_null(missing, B):
    _drive("each_reason", B, missing=(missing,))


@pytest.mark.parametrize("B", BATCHES)
def test_odd_warm_row_size(B):
    """A warm slot of an odd number of doubles: its rows start at odd offsets and are cleared with 8-byte stores."""
    sizes = dict(ec.SIZES, warm=1235)
    _drive("each_reason", B, sizes=sizes)
    _drive("ring", B, sizes=dict(ec.SIZES, warm=3, policy_state=2, cmd_state=130))
