"""Inclined ground and per-robot friction on the CPU: the header's defines and the new entry's argument checks,
pack_terrain / terrain_from_slope / place_on_terrain, tests/terrain_reference.py against tests/plant_reference.py on a
level row, the inputs of the device's parity test, and the model in closed loop under the oracle's MPC on eight
slopes, with enough friction and with too little.  No device."""
import ctypes
import re

import numpy as np
import pytest

import mpcqp
from mpcqp import _lib

import estimator_reference as er
import plant_reference as pr
import terrain_reference as tr
from test_disturb import DT, mixed_init, wrench_rows
from test_plant import truth_states

PARITY_TICKS = 30
# the seeds of tests/test_gpu_plant_terrain.py::test_teacher_forced_parity, per (B, substeps): (init, inputs);
# test_parity_inputs_exclude_nothing holds them to the margin the device test relies on
PARITY_SEEDS = {(B, n): (300 + B, 13 * B + n) for B in (1, 5, 67) for n in (1, 4)}


def terrain_rows(rng, B):
    """Random terrain rows: slopes in +-0.25 rad, offsets +-0.05, mu 0.1 .. 0.9; every fourth row level (its own
    offset and mu), every eighth the flat ground itself."""
    pitch, roll = rng.uniform(-0.25, 0.25, B), rng.uniform(-0.25, 0.25, B)
    pitch[3::4] = roll[3::4] = 0.0
    t = mpcqp.terrain_from_slope(pitch, roll, rng.uniform(0.1, 0.9, B))
    t[:, tr.TR_OFFSET] = rng.uniform(-0.05, 0.05, B)
    t[7::8, tr.TR_OFFSET] = 0.0
    return t


def parity_inputs(B, substeps):
    """(init rows, torques [T,B,12], wrench rows per tick (None: a NULL pointer), terrain rows [B, TR_SIZE]).  The
    starts are tests/test_disturb.py's mixed ones, rotated onto each robot's plane with their heights kept."""
    s_init, s_in = PARITY_SEEDS[(B, substeps)]
    rng = np.random.Generator(np.random.PCG64(s_in))
    tau = rng.uniform(-8.0, 8.0, (PARITY_TICKS, B, 12))
    wr = [None if t % 5 == 2 else wrench_rows(rng, B) for t in range(PARITY_TICKS)]
    terrain = terrain_rows(rng, B)
    init, _ = mpcqp.place_on_terrain(mixed_init(B, s_init), terrain, lower=False)
    return init, tau, wr, terrain


def shuffled_pool(B, terrain, seed=3):
    """A hand-made episode slot whose MPCQP_ES_POOL is a permutation, and the table that gives robot b the row
    terrain[b] through it (two spare rows in front, so no robot's index is its own)."""
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(B) + 2
    table = np.zeros((B + 2, tr.TR_SIZE))
    table[:2] = tr.level_rows(2, 0.6)
    table[perm] = terrain
    es = np.full((B, tr.ES_SIZE), 3.5)
    es[:, tr.ES_POOL] = perm
    return es, table


def test_defines_agree_with_the_header():
    hdr = open(_lib.PKG_ROOT + "/../include/mpcqp.h").read()
    for name in ("TR_NORMAL", "TR_OFFSET", "TR_MU", "TR_SIZE"):
        assert re.search(rf"^#define MPCQP_{name} {getattr(tr, name)}\s", hdr, flags=re.M), name
        assert getattr(_lib, name) == getattr(tr, name), name
    assert re.search(rf"^#define MPCQP_ES_POOL {tr.ES_POOL}\s", hdr, flags=re.M)
    assert re.search(rf"^#define MPCQP_ES_SIZE {tr.ES_SIZE}\s", hdr, flags=re.M)


def test_invalid_arguments_need_no_device():
    L = _lib.load()
    p = ctypes.byref(mpcqp.default_plant_params())
    call = L.mpcqp_plant_step_terrain_device
    rest = (None,) * 7
    bad = _lib.ERR_INVALID_ARG
    assert call(None, DT, 8, None, 8, 1, None, 1, 8, *rest) == bad
    assert call(p, 0.0, 8, None, 8, 1, None, 1, 8, *rest) == bad
    assert call(p, float("nan"), 8, None, 8, 1, None, 1, 8, *rest) == bad
    assert call(p, DT, None, None, 8, 1, None, 1, 8, *rest) == bad
    assert call(p, DT, 8, None, 8, 1, None, 1, None, *rest) == bad
    assert call(p, DT, 8, None, 8, 1, None, -1, 8, *rest) == bad
    for n in (0, 17):
        q = ctypes.byref(mpcqp.default_plant_params(substeps=n))
        assert call(q, DT, 8, None, 8, 1, None, 1, 8, *rest) == bad
    # the table: no rows, or fewer rows than robots without an episode slot to choose them
    assert call(p, DT, 8, None, 8, 0, None, 1, 8, *rest) == bad
    assert call(p, DT, 8, None, 8, 0, 8, 1, 8, *rest) == bad
    assert call(p, DT, 8, None, 8, 4, None, 5, 8, *rest) == bad
    assert call(p, DT, None, None, 8, 4, None, 0, None, *rest) == _lib.ERR_OK
    assert call(p, DT, None, None, None, 0, None, 0, None, *rest) == _lib.ERR_OK


def test_pack_terrain_and_slopes():
    t = mpcqp.pack_terrain([[0.0, 0.0, 2.0], [0.3, -0.1, 1.0]], [0.0, 0.25], 0.5)
    assert t.shape == (2, tr.TR_SIZE) and not t[:, 5:].any()
    np.testing.assert_allclose(np.linalg.norm(t[:, :3], axis=1), 1.0, rtol=1e-15)
    assert np.array_equal(t[0, :5], [0.0, 0.0, 1.0, 0.0, 0.5]) and t[1, tr.TR_OFFSET] == 0.25
    for normal, offset, mu in (([0.0, 1.0, 0.0], 0.0, 0.5), ([0.1, 0.0, -1.0], 0.0, 0.5), ([0.0, np.nan, 1.0], 0.0, 0.5),
                               ([0.0, 0.0, 1.0], np.inf, 0.5), ([0.0, 0.0, 1.0], 0.0, np.nan), ([0.0, 0.0, 1.0], 0.0, -0.1)):
        with pytest.raises(ValueError):
            mpcqp.pack_terrain([normal], offset, mu)
    pitch, roll = np.array([0.0, 0.2, -0.1, 0.0, 0.15]), np.array([0.0, 0.0, 0.0, 0.1, 0.15])
    point = np.array([0.3, -0.2, 0.1])
    s = mpcqp.terrain_from_slope(pitch, roll, 0.6, point)
    np.testing.assert_allclose(np.linalg.norm(s[:, :3], axis=1), 1.0, rtol=1e-15)
    assert np.array_equal(s[0, :3], [0.0, 0.0, 1.0]) and np.all(s[:, tr.TR_MU] == 0.6)
    np.testing.assert_allclose(mpcqp.terrain_height(s, np.tile(point, (5, 1))), 0.0, atol=1e-16)
    for k in range(5):  # n = R_y(pitch) R_x(roll) e_z
        Ry = mpcqp.records.rot_zyx(np.zeros(1), pitch[k:k + 1], np.zeros(1))[0]
        Rx = mpcqp.records.rot_zyx(roll[k:k + 1], np.zeros(1), np.zeros(1))[0]
        np.testing.assert_allclose(s[k, :3], Ry @ Rx @ [0.0, 0.0, 1.0], atol=1e-15)


def flat_stance(B, seed):
    """The default stance on z = 0 at a random yaw: init rows [B, PI_SIZE]."""
    p = pr.default_params()
    ro, rf = pr._geom(p)
    yaw = np.random.Generator(np.random.PCG64(seed)).uniform(-np.pi, np.pi, B)
    q = np.tile(np.array(p.default_joint_pos), (B, 1))
    z0 = -er.fk(q.reshape(B, 4, 3), ro, rf)[:, 0, 2]
    quat = np.stack([np.cos(yaw / 2), np.zeros(B), np.zeros(B), np.sin(yaw / 2)], 1)
    return mpcqp.pack_plant_init(np.stack([np.zeros(B), np.zeros(B), z0], 1), quat, q), yaw


SLOPES = np.array([(0.0, 0.0), (0.1, 0.0), (-0.1, 0.0), (0.2, 0.0), (-0.2, 0.0), (0.0, 0.1), (0.0, -0.2), (0.15, 0.15)])


def slope_fleet(mu):
    """The closed-loop fleet: (terrain rows, init rows, slope-parallel euler) of eight robots at a random yaw on the
    eight slopes, shared with the device twin."""
    terrain = mpcqp.terrain_from_slope(SLOPES[:, 0], SLOPES[:, 1], mu)
    init, euler = mpcqp.place_on_terrain(flat_stance(len(SLOPES), 5)[0], terrain)
    return terrain, init, euler


def feet_of(init):
    p = pr.default_params()
    ro, rf = pr._geom(p)
    B = init.shape[0]
    q = init[:, pr.PI_JOINT_POS:pr.PI_JOINT_POS + 12].reshape(B, 4, 3)
    return init[:, None, :3] + er.mat_vec(er.quat_to_rot(init[:, pr.PI_QUAT:pr.PI_QUAT + 4])[:, None], er.fk(q, ro, rf))


def test_place_on_terrain():
    B = 24
    rng = np.random.Generator(np.random.PCG64(2))
    terrain = mpcqp.terrain_from_slope(rng.uniform(-0.25, 0.25, B), rng.uniform(-0.25, 0.25, B), 0.6,
                                       rng.uniform(-0.5, 0.5, (B, 3)))
    terrain[0] = tr.level_rows(1, 0.6)
    flat, yaw = flat_stance(B, 7)
    init, euler = mpcqp.place_on_terrain(flat, terrain)
    h = mpcqp.terrain_height(terrain, feet_of(init))
    print(f"[note] placed feet: hgt {h.min():.3e} .. {h.max():.3e}")
    assert np.all(h <= 0.0) and np.all(h >= -1e-15)
    np.testing.assert_allclose(np.linalg.norm(init[:, 3:7], axis=1), 1.0, rtol=1e-15)
    np.testing.assert_allclose(euler, er.quat_to_euler(init[:, 3:7]), atol=1e-14)
    assert np.array_equal(init[:, 7:], flat[:, 7:])
    # slope-parallel: the body's z axis is the normal, and a level row leaves the yaw
    np.testing.assert_allclose(er.quat_to_rot(init[:, 3:7])[:, :, 2], terrain[:, :3], atol=1e-14)
    assert abs(euler[0, 2] - yaw[0]) <= 1e-14 and np.all(np.abs(euler[0, :2]) <= 1e-16)
    # every foot starts held, and lower=False keeps the heights of the start
    plant = tr.TerrainPlant(pr.default_params(), B)
    o = plant.step(DT, np.zeros((B, 12)), init, terrain=terrain)[0]
    assert o["contacts"].all()
    lifted = flat.copy()
    lifted[:, pr.PI_POS + 2] += 0.02
    kept, _ = mpcqp.place_on_terrain(lifted, terrain, lower=False)
    np.testing.assert_allclose(mpcqp.terrain_height(terrain, feet_of(kept)), 0.02, atol=1e-15)


@pytest.mark.parametrize("substeps", [1, 4])
def test_level_row_is_plant_reference(substeps):
    """n = (0, 0, 1), d = 0, mu = pp.mu: the algebra makes the two equal up to the sign of zeros."""
    B, T = 12, 12
    init = mixed_init(B, 31)
    rng = np.random.Generator(np.random.PCG64(8))
    p = pr.default_params(substeps=substeps)
    a, b = pr.Plant(p, B), tr.TerrainPlant(p, B)
    level = tr.level_rows(B, p.mu)
    worst, stance, swing = 0.0, 0, 0
    for t in range(T):
        tau = rng.uniform(-8.0, 8.0, (B, 12))
        oa, wa, ma = a.step(DT, tau, init)
        ob, wb, mb = b.step(DT, tau, init, terrain=level)
        assert np.array_equal(oa["status"], ob["status"]) and np.array_equal(oa["contacts"], ob["contacts"]), f"tick {t}"
        assert np.array_equal(wa, wb)
        pairs = [(a.slot, b.slot)] + [(np.asarray(oa[k], dtype=np.float64), np.asarray(ob[k], dtype=np.float64)) for k in oa]
        for x, y in pairs:
            x, y = x.reshape(B, -1)[wa], y.reshape(B, -1)[wa]
            ratio = np.abs(y - x) / np.maximum(1.0, np.abs(x))
            worst = max(worst, float(ratio.max()))
            assert np.all(ratio <= 1e-12), f"tick {t}: off by {ratio.max():.3e}"
        stance += int(oa["contacts"].sum())
        swing += int((~oa["contacts"]).sum())
    print(f"[note] level row against plant_reference, substeps {substeps}: worst difference {worst:.3e}, stance "
          f"{stance} swing {swing} leg-ticks")
    assert stance > 0 and swing > 0


@pytest.mark.parametrize("B,substeps", sorted(PARITY_SEEDS))
def test_parity_inputs_exclude_nothing(B, substeps):
    """The inputs of the device's teacher-forced parity test: on the restatement alone no robot-tick has a decision
    margin under 1e-9, the cap under which the device test would leave a robot-tick out."""
    init, tau, wr, terrain = parity_inputs(B, substeps)
    plant = tr.TerrainPlant(pr.default_params(substeps=substeps), B)
    worst, stance, swing, clipped = np.inf, 0, 0, 0
    for t in range(PARITY_TICKS):
        o, wrote, margin = plant.step(DT, tau[t], init, wrench=wr[t], terrain=terrain)
        worst = min(worst, float(margin.min()))
        stance += int(o["contacts"].sum())
        swing += int((~o["contacts"]).sum())
        clipped += sum(int(fr[2].sum()) for fr in plant.friction)
    print(f"[note] B={B} substeps={substeps}: smallest margin {worst:.3e}, stance {stance} swing {swing}, clipped "
          f"{clipped} leg-substeps")
    assert worst >= 1e-9
    if B > 1:
        assert stance > 0 and swing > 0
    # the shuffled pool hands every robot the same row
    es, table = shuffled_pool(B, terrain)
    assert np.array_equal(table[es[:, tr.ES_POOL].astype(int)], terrain)


def closed_loop(oracle, mu, ticks):
    """The slope fleet under the oracle's MPC fed the plant's true state (tests/test_plant.py's closed loop):
    substeps 1 on the even robots, 4 on the odd ones.  Returns the per-tick records."""
    terrain, init, euler_d = slope_fleet(mu)
    B = init.shape[0]
    op = oracle.default_params(10)
    idx = [np.arange(0, B, 2), np.arange(1, B, 2)]
    plants = [tr.TerrainPlant(pr.default_params(substeps=n), len(i)) for n, i in zip((1, 4), idx)]
    solvers = [oracle.WarmSolver(op) for _ in range(B)]
    pos_d = init[:, pr.PI_POS:pr.PI_POS + 3].copy()
    tau = np.zeros((B, 12))
    rec = dict(terrain=terrain, pos_d=pos_d, status=[], contacts=[], solve=[], grf=[], pos=[], foot=[], friction=[])
    for t in range(ticks + 1):
        outs = [pl.step(DT, tau[i], init[i], terrain=terrain[i])[0] for pl, i in zip(plants, idx)]
        out = {}
        for k in outs[0]:
            out[k] = np.zeros((B,) + outs[0][k].shape[1:], dtype=outs[0][k].dtype)
            for o, i in zip(outs, idx):
                out[k][i] = o[k]
        for pl, i in zip(plants, idx):
            for ft, lim, clip in pl.friction:
                rec["friction"].append((i, ft, lim, clip))
        rec["status"].append(out["status"].copy())
        rec["contacts"].append(out["contacts"].copy())
        rec["grf"].append(out["grf"].copy())
        rec["pos"].append(out["root_pos"].copy())
        rec["foot"].append(out["foot_world"].copy())
        recs = mpcqp.assemble_compute_grf(truth_states(out, pos_d, euler_d), 10)
        res = np.array([sv.step(recs[b])[0] for b, sv in enumerate(solvers)])
        rec["solve"].append(res["status"].copy())
        fb = res["f_body"].reshape(B, 4, 3)
        tau = np.einsum("blji,blj->bli", out["j_foot"], -fb).reshape(B, 12)
    for sv in solvers:
        sv.close()
    return {k: np.array(v) if k not in ("friction",) else v for k, v in rec.items()}


_LOOPS = {}


def loop(oracle, mu):
    if mu not in _LOOPS:
        _LOOPS[mu] = closed_loop(oracle, mu, 400 if mu == 0.6 else 150)
    return _LOOPS[mu]


def slope_conditions(terrain, pos_d, status, contacts, solve, grf_end, pos_end, foot, mass, gravity):
    """The conditions of the closed loop on slopes, shared with the device twin.  status / contacts per tick, solve
    the solve statuses from tick 1 on, grf_end / pos_end the last tick's, foot every tick's held feet [T,B,4,3]."""
    assert np.all(status == 0.0), status.max(0)
    assert np.all(contacts)
    assert np.all(solve == _lib.STATUS_SOLVED)
    ratio = grf_end.sum(1) / (mass * gravity) - np.array([0.0, 0.0, 1.0])
    dh = mpcqp.terrain_height(terrain, pos_end) - mpcqp.terrain_height(terrain, pos_d)
    hf = np.abs(mpcqp.terrain_height(terrain, np.swapaxes(foot, 0, 1))).max()
    print(f"[note] slopes: |sum F / m g - e_z| {np.abs(ratio).max():.3e}, |hgt(pos) - hgt(pos_d)| {np.abs(dh).max():.3e}, "
          f"held feet |hgt| {hf:.3e}")
    assert np.all(np.abs(ratio) <= 0.01), ratio
    assert np.all(np.abs(dh) <= 0.01), dh
    assert hf <= 1e-15


def test_closed_loop_on_slopes_with_the_oracle_mpc(oracle):
    """Eight robots standing slope-parallel on the eight slopes at mu 0.6 for 400 ticks."""
    r = loop(oracle, 0.6)
    p = pr.default_params()
    slope_conditions(r["terrain"], r["pos_d"], r["status"], r["contacts"], r["solve"][1:], r["grf"][-1], r["pos"][-1],
                     r["foot"], p.mass, p.gravity)


def test_friction_decides(oracle):
    """The same fleet at mu 0.1: every stance leg-substep stays inside the cone and some are clipped; by tick 150
    each robot on a slope of 0.15 rad or more has left its reach or slid 3 cm, while its mu 0.6 twin stays within
    1e-3."""
    low, high = loop(oracle, 0.1), loop(oracle, 0.6)
    ft = np.concatenate([f[1].ravel() for f in low["friction"]])
    lim = np.concatenate([f[2].ravel() for f in low["friction"]])
    clipped = sum(int(f[3].sum()) for f in low["friction"])
    on = np.isfinite(ft)
    assert on.any() and np.all(ft[on] <= lim[on] * (1.0 + 1e-12))
    assert clipped > 0
    steep = np.arccos(low["terrain"][:, tr.TR_NORMAL + 2]) >= 0.15
    assert steep.sum() == 4
    slid = np.linalg.norm(low["pos"][:151] - low["pos_d"], axis=2).max(0)
    reach = (low["status"][:151] == 1.0).any(0)
    twin = np.linalg.norm(high["pos"][:151] - high["pos_d"], axis=2).max(0)
    print(f"[note] mu 0.1: clipped {clipped} of {int(on.sum())} stance leg-substeps; by tick 150 slid {np.round(slid, 4)}, "
          f"out of reach {reach}; the mu 0.6 twins moved {np.round(twin, 6)}")
    assert np.all(reach[steep] | (slid[steep] > 0.03))
    assert np.all(twin[steep] <= 1e-3)
