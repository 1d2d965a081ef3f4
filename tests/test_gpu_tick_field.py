"""ControlTick(field=): the plant stage of the tick on a bilinear height field.  The fused step is bitwise the staged
C calls and the captured graph's replays; the tick captured without the option is the tick built without it; the fleet
of tests/test_field.py under the truth-fed MPC tick, replayed 400 times, meets the conditions and the gates the CPU
model met; and with the episode stage every robot stands on the tile of its episode's pool row."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib
from mpcqp.tick import ControlTick

import episode_reference as ep
import plant_reference as pr
import test_gpu_tick_plant as tp
from test_field import field_conditions, field_fleet
from test_terrain import flat_stance

pytestmark = pytest.mark.gpu

DT, B, T = tp.DT, tp.B, tp.T


def _ground():
    """The first five robots of the closed-loop fleet: two on rolling ground, two on the step, one on the ramp."""
    rows, heights, init, euler = field_fleet()
    return rows[:B], heights, init[:B], euler[:B]


def _make(kind, field=True):
    rows, heights, init, euler = _ground()
    kw = dict(dt=DT, plant=mpcqp.default_plant_params(), plant_init=init, field=(rows, heights) if field else None)
    if kind == "full":
        k = ControlTick(B, plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                        command=mpcqp.default_command_params(), control_type="per_robot", **kw)
    else:
        k = ControlTick(B, **kw)
    st, tq = tp._caller_rows()
    k.states.copy_(torch.from_numpy(st))
    k.states[:, _lib.ST_EULER_D:_lib.ST_EULER_D + 3].copy_(torch.from_numpy(euler))
    k.states[:, _lib.ST_POS_D:_lib.ST_POS_D + 3].copy_(torch.from_numpy(init[:, :3].copy()))
    k.tq_records.copy_(torch.from_numpy(tq))
    return k


def _plant_call(k, kind):
    s = torch.cuda.current_stream().cuda_stream
    truth = kind != "full"
    mpcqp.plant_step_field_device(k.plant, k.dt, k.torques.data_ptr(), 0, k.field.data_ptr(), k.field.shape[0],
                                  k.heights.data_ptr(), k.heights.numel(), 0, B, k.plant_state.data_ptr(),
                                  k.plant_init.data_ptr(), k.sensors.data_ptr() if kind == "full" else 0,
                                  k.plan_in.data_ptr(), k.states.data_ptr() if truth else 0,
                                  k.tq_records.data_ptr() if truth else 0, k.plant_out.data_ptr(), s)


def _staged(k, kind):
    """tests/test_gpu_tick_plant.py's staged controller calls, then the field entry point."""
    plant, k.plant = k.plant, None  # (its _staged ends with the flat plant call of a tick that has one)
    try:
        tp._staged(k, kind)
    finally:
        k.plant = plant
    _plant_call(k, kind)


def _drive(k, kind, step, names, prime=True):
    """T ticks of `step`; ``prime``: the plant stage alone first, so the first solve sees the robot (without it the
    first tick's own plant stage initialises the slots)."""
    if prime:
        k.prime_plant()
    torch.cuda.synchronize()
    rng = np.random.default_rng(17)
    outs = [{name: tp._bits(getattr(k, name)) for name in names}]
    for t in range(T):
        if kind == "full":
            request = np.zeros(B, bool)
            request[1::2] = t == 12
            k.cmd.copy_(torch.from_numpy(mpcqp.pack_commands(np.zeros((B, 3)), np.zeros((B, 3)), request)))
            if t % 8 == 0:
                k.control_type.copy_(torch.from_numpy(rng.integers(0, 2, B).astype(np.int32)))
        step()
        torch.cuda.synchronize()
        outs.append({name: tp._bits(getattr(k, name)) for name in names})
    return outs


_RUNS = {}


def _runs(kind):
    if kind not in _RUNS:
        names = (tp.FULL if kind == "full" else tp.MPC) + ("field", "heights")
        out = {}
        for how in ("eager", "staged", "graph", "flat"):
            k = _make(kind)
            try:
                if how == "graph":
                    k.capture()
                    step = k.replay
                elif how == "flat":
                    g = k.capture(without=("field",))
                    assert k.graph is None and k.stages(without=("field",)) == k.stages()
                    step = g.replay
                else:
                    step = k.step if how == "eager" else (lambda k=k: _staged(k, kind))
                out[how] = _drive(k, kind, step, names, prime=how != "flat")
            finally:
                k.close()
        k = _make(kind, field=False)
        try:
            assert not hasattr(k, "field") and not hasattr(k, "heights")
            k.capture()
            out["built_flat"] = _drive(k, kind, k.replay, names[:-2], prime=False)
        finally:
            k.close()
        _RUNS[kind] = (names, out)
    return _RUNS[kind]


@pytest.mark.parametrize("other", ["staged", "graph"])
@pytest.mark.parametrize("kind", ["mpc", "full"])
def test_fused_tick_is_bitwise_the_stages_and_its_graph(kind, other):
    names, out = _runs(kind)
    for t, (a, b) in enumerate(zip(out["eager"], out[other])):
        for name in names:
            assert np.array_equal(a[name], b[name]), f"{kind} tick {t}: {name} of the eager tick and the {other} one differ"
    last = out["eager"][-1]
    po = last["plant_out"].view(np.float64)
    rows, heights = _ground()[:2]
    held = po[:, _lib.PT_CONTACTS:_lib.PT_CONTACTS + 4] == 1.0
    h = mpcqp.field_lookup(rows, heights, np.arange(B), po[:, _lib.PT_FOOT:_lib.PT_FOOT + 12].reshape(B, 4, 3))[0]
    print(f"[note] {kind} tick on the field, {T} ticks: plant status {po[:, _lib.PT_STATUS]}, held feet {held.sum()}, "
          f"|hgt| of held feet {np.abs(h[held]).max():.3e}")
    assert last["counter"].min() == T and np.abs(last["torques"].view(np.float64)).max() > 0
    assert held.any()
    if kind == "mpc":  # the standing fleet: no foot has landed anew
        assert held.all() and np.abs(h[held]).max() <= 1e-12
    # the ground is not the flat one: the same tick captured without the option moves differently
    assert not np.array_equal(last["plant_out"], out["flat"][-1]["plant_out"])


@pytest.mark.parametrize("kind", ["mpc", "full"])
def test_capture_without_field_is_the_tick_built_without_it(kind):
    names, out = _runs(kind)
    for t, (a, b) in enumerate(zip(out["flat"], out["built_flat"])):
        for name in names[:-2]:
            assert np.array_equal(a[name], b[name]), f"{kind} tick {t}: {name}"


def test_field_option_is_checked():
    rows, heights = _ground()[:2]
    pp = mpcqp.default_plant_params()
    with pytest.raises(ValueError, match="needs plant="):
        ControlTick(B, dt=DT, field=(rows, heights))
    with pytest.raises(ValueError, match="rows"):
        ControlTick(B, dt=DT, plant=pp, field=(rows[:3], heights))
    with pytest.raises(ValueError, match="exclude"):
        ControlTick(B, dt=DT, plant=pp, field=(rows, heights), terrain=mpcqp.terrain_from_slope(np.zeros(B), 0.0, 0.6))
    flat, _ = flat_stance(2, 1)
    pool = mpcqp.pack_episode_pool(flat, np.zeros((2, 3)), flat[:, :3])
    with pytest.raises(ValueError, match="rows"):
        ControlTick(B, dt=DT, plant=pp, episode=mpcqp.default_episode_params(), episode_pool=pool, field=(rows, heights))


def test_closed_loop_on_the_field_on_the_device():
    """tests/test_field.py's closed loop as a truth-fed MPC-only tick, graph-replayed 400 times with no host write in
    between; substeps 1 on the even robots and 4 on the odd ones (two ticks: substeps is a kernel argument)."""
    rows, heights, init, euler_d = field_fleet()
    n = init.shape[0]
    status, contacts = np.zeros((400, n)), np.zeros((400, n, 4), bool)
    solve, foot, quat = np.zeros((400, n), np.int32), np.zeros((400, n, 4, 3)), np.zeros((400, n, 4))
    grf, pos = np.zeros((n, 4, 3)), np.zeros((n, 3))
    for substeps, idx in ((1, np.arange(0, n, 2)), (4, np.arange(1, n, 2))):
        b = len(idx)
        pp = mpcqp.default_plant_params(substeps=substeps)
        k = ControlTick(b, dt=DT, plant=pp, plant_init=init[idx], field=(rows[idx], heights))
        try:
            z = np.zeros((b, 3))
            st = mpcqp.RobotStates(
                root_euler=z, root_pos=z, root_ang_vel=z, root_lin_vel=z, root_rot_mat=np.zeros((b, 3, 3)),
                root_euler_d=euler_d[idx], root_pos_d=init[idx, pr.PI_POS:pr.PI_POS + 3], root_ang_vel_d=z,
                root_lin_vel_d=z, foot_pos_abs=np.zeros((b, 4, 3)), contacts=np.ones((b, 4), bool), mu=np.full(b, 0.3))
            k.states.copy_(torch.from_numpy(mpcqp.pack_states(st)))
            k.tq_records.copy_(torch.from_numpy(mpcqp.assemble_torque_records(
                np.zeros((b, 4, 3, 3)), np.zeros((b, 4, 3)), np.ones((b, 4), bool), torques_gravity=np.zeros(12))))
            k.prime_plant()
            k.capture()
            for t in range(400):
                k.replay()
                torch.cuda.synchronize()
                po = k.plant_out.cpu().numpy()
                status[t, idx] = po[:, _lib.PT_STATUS]
                contacts[t, idx] = po[:, _lib.PT_CONTACTS:_lib.PT_CONTACTS + 4] == 1.0
                foot[t, idx] = po[:, _lib.PT_FOOT:_lib.PT_FOOT + 12].reshape(b, 4, 3)
                quat[t, idx] = po[:, _lib.PT_QUAT:_lib.PT_QUAT + 4]
                solve[t, idx] = np.frombuffer(k.results.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE)["status"]
            grf[idx] = po[:, _lib.PT_GRF:_lib.PT_GRF + 12].reshape(b, 4, 3)
            pos[idx] = po[:, _lib.PT_POS:_lib.PT_POS + 3]
        finally:
            k.close()
    pp = mpcqp.default_plant_params()
    field_conditions(rows, heights, init[:, :3], status, contacts, solve, grf, pos, foot, quat, pp.mass, pp.gravity)


def test_each_robot_stands_on_the_tile_of_its_pool_row():
    """16 robots, a four-row pool (rolling, step, ramp, stairs) with the header table parallel to it, 60 replays at
    max_ticks 17: whenever a robot's plant tick ran, its held feet lie on the tile its episode slot named before that
    tick, and every logged episode names the row its ticks ran on."""
    n, T2 = 16, 60
    rows, heights, init, euler = field_fleet()
    pick = [0, 2, 4, 5]
    rows, init, euler = rows[pick], init[pick], euler[pick]
    assert len(set(rows[:, _lib.HF_OFFSET])) == 4
    pool = mpcqp.pack_episode_pool(init, euler, init[:, :3])
    k = ControlTick(n, dt=DT, plant=mpcqp.default_plant_params(), episode=mpcqp.default_episode_params(max_ticks=17, seed=5),
                    episode_pool=pool, field=(rows, heights))
    try:
        st, tq = tp._caller_rows()
        k.states.copy_(torch.from_numpy(np.tile(st[:1], (n, 1))))
        k.tq_records.copy_(torch.from_numpy(np.tile(tq[:1], (n, 1))))
        k.capture()
        used, worst, held_ticks = [], 0.0, 0
        for t in range(T2):
            es = k.episode_state.cpu().numpy()
            k.replay()
            torch.cuda.synchronize()
            po = k.plant_out.cpu().numpy()
            row = es[:, ep.ES_POOL].astype(int)
            held = (po[:, _lib.PT_CONTACTS:_lib.PT_CONTACTS + 4] == 1.0) & (po[:, _lib.PT_STATUS:_lib.PT_STATUS + 1] == 0.0)
            h = np.abs(mpcqp.field_lookup(rows, heights, row, po[:, _lib.PT_FOOT:_lib.PT_FOOT + 12].reshape(n, 4, 3))[0])
            if t >= 2:  # (tick 1 draws and tick 2 primes)
                assert np.all(held.sum(1) >= 1), f"tick {t}"
                worst = max(worst, float(h[held].max()))
                held_ticks += int(held.sum())
            used.append((es[:, ep.ES_PHASE].copy(), es[:, ep.ES_EPISODE].copy(), row))
        log = k.episode_log.cpu().numpy().reshape(n, -1, ep.EL_SIZE)
    finally:
        k.close()
    print(f"[note] four-row pool: held feet |hgt| {worst:.3e} over {held_ticks} leg-ticks; rows drawn "
          f"{np.bincount(np.concatenate([u[2] for u in used[2:]]), minlength=4).tolist()}")
    assert worst <= 1e-12
    rows_seen = set()
    for b in range(n):
        for entry in log[b][log[b][:, ep.EL_LENGTH] > 0]:
            ran = [u[2][b] for u in used if u[0][b] == 1.0 and u[1][b] == entry[ep.EL_EPISODE]]
            assert ran and all(r == int(entry[ep.EL_POOL]) for r in ran), (b, entry[:5])
            rows_seen.add(int(entry[ep.EL_POOL]))
    assert rows_seen == {0, 1, 2, 3}
