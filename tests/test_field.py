"""Bilinear height-field ground on the CPU: the header's defines and the new entry's argument checks,
pack_height_field / field_lookup / place_on_field, tests/field_reference.py on a planar tile against
tests/terrain_reference.py, the inputs of the device's parity test, and the model in closed loop under the oracle's
MPC on rolling, step and stairs tiles.  No device."""
import ctypes
import re

import numpy as np
import pytest

import mpcqp
from mpcqp import _lib

import estimator_reference as er
import field_reference as fr
import plant_reference as pr
import terrain_reference as tr
import test_terrain as tt
from test_disturb import DT, mixed_init, wrench_rows
from test_plant import truth_states
from test_terrain import feet_of

PARITY_TICKS = 30
# the seeds of tests/test_gpu_plant_field.py::test_teacher_forced_parity, per (B, substeps): (init, inputs);
# test_parity_inputs_exclude_nothing holds them to the margin the device test relies on
PARITY_SEEDS = {(B, n): (400 + B, 17 * B + n) for B in (1, 5, 67) for n in (1, 4)}

# The closed loop's largest tilt, measured on the CPU restatement (profiles/field/measured.jsonl has the run), and the
# gate of both twins: four times that, and at least 1e-6 rad so a value near zero leaves a gate that means something.
TILT_MEASURED = 2.6411293607060864e-06
TILT_GATE = max(4.0 * TILT_MEASURED, 1e-6)


def parity_tiles(rng):
    """Four tiles of unequal, non-square sizes and asymmetric heights: 5x7 and 3x5 rough ones (+-3 cm on cells of 15
    and 20 cm), one 2x2 cell, and a level 4x3 one.  (tiles, cell per tile)."""
    tiles = [rng.uniform(-0.03, 0.03, (5, 7)), rng.uniform(-0.03, 0.03, (3, 5)), rng.uniform(-0.02, 0.02, (2, 2)),
             np.full((4, 3), 0.01)]
    return tiles, np.array([0.15, 0.2, 0.3, 0.5])


def parity_inputs(B, substeps):
    """(init rows, torques [T,B,12], wrench rows per tick (None: a NULL pointer), header rows [B, HF_SIZE], heights).
    Robot b stands on tile b % 4, centred under it up to +-5 cm, so the feet of the robots on the small tiles reach
    beyond the border; the starts are tests/test_disturb.py's mixed ones, lifted so that the lowest foot keeps the
    height over the ground it had over z = 0."""
    s_init, s_in = PARITY_SEEDS[(B, substeps)]
    rng = np.random.Generator(np.random.PCG64(s_in))
    tau = rng.uniform(-8.0, 8.0, (PARITY_TICKS, B, 12))
    wr = [None if t % 5 == 2 else wrench_rows(rng, B) for t in range(PARITY_TICKS)]
    tiles, cells = parity_tiles(rng)
    init = mixed_init(B, s_init)
    which = np.arange(B) % 4
    cell = cells[which]
    nx = np.array([tiles[k].shape[1] for k in which])
    ny = np.array([tiles[k].shape[0] for k in which])
    x0 = init[:, pr.PI_POS] - cell * (nx - 1) / 2 + rng.uniform(-0.05, 0.05, B)
    y0 = init[:, pr.PI_POS + 1] - cell * (ny - 1) / 2 + rng.uniform(-0.05, 0.05, B)
    rows, heights = mpcqp.pack_height_field(tiles, x0, y0, cell, rng.uniform(0.1, 0.9, B), share=which)
    feet = feet_of(init)
    h, n = mpcqp.field_lookup(rows, heights, np.arange(B), feet)
    init[:, pr.PI_POS + 2] += feet[..., 2].min(1) - (h / n[..., 2]).min(1)
    return init, tau, wr, rows, heights


def shuffled_pool(B, rows, seed=3):
    """A hand-made episode slot whose MPCQP_ES_POOL is a permutation, and the header table that gives robot b the row
    rows[b] through it (two spare rows in front, so no robot's index is its own)."""
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(B) + 2
    table = np.zeros((B + 2, fr.HF_SIZE))
    table[:2] = rows[0]
    table[perm] = rows
    es = np.full((B, tr.ES_SIZE), 3.5)
    es[:, tr.ES_POOL] = perm
    return es, table


def planar_tiles(terrain, centre, nx=9, ny=7, cell=0.25):
    """One tile per terrain row, sampled from the row's plane on a grid of nx x ny nodes centred at centre [B,2]."""
    t = np.asarray(terrain).reshape(-1, tr.TR_SIZE)
    B = t.shape[0]
    x0 = centre[:, 0] - cell * (nx - 1) / 2
    y0 = centre[:, 1] - cell * (ny - 1) / 2
    x = x0[:, None, None] + cell * np.arange(nx)[None, None, :]
    y = y0[:, None, None] + cell * np.arange(ny)[None, :, None]
    n, d = t[:, tr.TR_NORMAL:tr.TR_NORMAL + 3], t[:, tr.TR_OFFSET]
    z = (d[:, None, None] - n[:, 0, None, None] * x - n[:, 1, None, None] * y) / n[:, 2, None, None]
    return mpcqp.pack_height_field(list(z), x0, y0, cell, t[:, tr.TR_MU])


def test_defines_agree_with_the_header():
    hdr = open(_lib.PKG_ROOT + "/../include/mpcqp.h").read()
    for name in ("HF_X0", "HF_Y0", "HF_CELL", "HF_MU", "HF_NX", "HF_NY", "HF_OFFSET", "HF_SIZE"):
        assert re.search(rf"^#define MPCQP_{name} {getattr(fr, name)}\s", hdr, flags=re.M), name
        assert getattr(_lib, name) == getattr(fr, name), name


def test_invalid_arguments_need_no_device():
    L = _lib.load()
    p = ctypes.byref(mpcqp.default_plant_params())
    call = L.mpcqp_plant_step_field_device
    rest = (None,) * 7
    bad = _lib.ERR_INVALID_ARG
    # what the wrench entry rejects
    assert call(None, DT, 8, None, 8, 1, 8, 4, None, 1, 8, *rest) == bad
    assert call(p, 0.0, 8, None, 8, 1, 8, 4, None, 1, 8, *rest) == bad
    assert call(p, float("nan"), 8, None, 8, 1, 8, 4, None, 1, 8, *rest) == bad
    assert call(p, DT, None, None, 8, 1, 8, 4, None, 1, 8, *rest) == bad
    assert call(p, DT, 8, None, 8, 1, 8, 4, None, 1, None, *rest) == bad
    assert call(p, DT, 8, None, 8, 1, 8, 4, None, -1, 8, *rest) == bad
    for n in (0, 17):
        q = ctypes.byref(mpcqp.default_plant_params(substeps=n))
        assert call(q, DT, 8, None, 8, 1, 8, 4, None, 1, 8, *rest) == bad
    # the table and the heights
    assert call(p, DT, 8, None, 8, 0, 8, 4, None, 1, 8, *rest) == bad
    assert call(p, DT, 8, None, 8, 0, 8, 4, 8, 1, 8, *rest) == bad
    assert call(p, DT, 8, None, 8, 4, 8, 4, None, 5, 8, *rest) == bad
    assert call(p, DT, 8, None, 8, 1, None, 4, None, 1, 8, *rest) == bad
    assert call(p, DT, 8, None, 8, 1, 8, 3, None, 1, 8, *rest) == bad
    assert call(p, DT, None, None, 8, 4, 8, 4, None, 0, None, *rest) == _lib.ERR_OK
    assert call(p, DT, None, None, None, 0, None, 0, None, 0, None, *rest) == _lib.ERR_OK


def test_pack_height_field():
    a, b = np.arange(15.0).reshape(3, 5) * 0.01, np.array([[0.0, 0.1], [0.2, 0.4]])
    rows, heights = mpcqp.pack_height_field([a, b], [0.5, -1.0], 0.25, [0.1, 0.2], 0.6)
    assert rows.shape == (2, fr.HF_SIZE) and heights.shape == (19,) and not rows[:, 7:].any()
    assert np.array_equal(rows[0, :7], [0.5, 0.25, 0.1, 0.6, 5.0, 3.0, 0.0])
    assert np.array_equal(rows[1, :7], [-1.0, 0.25, 0.2, 0.6, 2.0, 2.0, 15.0])
    assert np.array_equal(heights[:15], a.ravel()) and np.array_equal(heights[15:], b.ravel())
    # several header rows on one tile
    rows, heights = mpcqp.pack_height_field([a, b], [0.0, 1.0, 2.0], 0.0, 0.1, [0.3, 0.4, 0.5], share=[1, 0, 1])
    assert heights.shape == (19,) and np.array_equal(rows[:, fr.HF_OFFSET], [15.0, 0.0, 15.0])
    assert np.array_equal(rows[:, fr.HF_NX], [2.0, 5.0, 2.0]) and np.array_equal(rows[:, fr.HF_MU], [0.3, 0.4, 0.5])
    nan = a.copy()
    nan[1, 2] = np.nan
    for tiles, cell, mu, share in (([nan], 0.1, 0.6, None), ([np.zeros((1, 5))], 0.1, 0.6, None),
                                   ([np.zeros((3, 1))], 0.1, 0.6, None), ([np.zeros(4)], 0.1, 0.6, None),
                                   ([a], 0.0, 0.6, None), ([a], -0.1, 0.6, None), ([a], 0.1, -0.1, None),
                                   ([a], np.inf, 0.6, None), ([a], 0.1, np.nan, None), ([a], 0.1, 0.6, [1])):
        with pytest.raises(ValueError):
            mpcqp.pack_height_field(tiles, 0.0, 0.0, cell, mu, share=share)
    with pytest.raises(ValueError):
        mpcqp.pack_height_field([a], np.nan, 0.0, 0.1, 0.6)


def _rough():
    rng = np.random.Generator(np.random.PCG64(12))
    a, b = rng.uniform(-0.05, 0.05, (4, 6)), rng.uniform(-0.05, 0.05, (2, 2))
    return mpcqp.pack_height_field([a, b], [-0.3, 0.2], [0.1, -0.4], [0.2, 0.35], 0.6) + (a, b)


def test_field_lookup_agrees_with_the_restatement_and_a_central_difference():
    rows, heights, a, b = _rough()
    rng = np.random.Generator(np.random.PCG64(13))
    N = 2000
    idx = rng.integers(0, 2, N)
    p = np.stack([rng.uniform(-0.6, 1.0, N), rng.uniform(-0.7, 1.0, N), rng.uniform(-0.1, 0.3, N)], 1)
    hg, n = mpcqp.field_lookup(rows, heights, idx, p)
    hr, nr, edge = fr.lookup(rows[idx], heights, p)
    assert np.array_equal(hg, hr) and np.array_equal(n, nr)
    np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, rtol=1e-15)
    # inside cells, the gradient the normal encodes is the central difference of h = p_z - hgt / n_z
    r = rows[idx]
    u = (p[:, 0] - r[:, fr.HF_X0]) / r[:, fr.HF_CELL]
    v = (p[:, 1] - r[:, fr.HF_Y0]) / r[:, fr.HF_CELL]
    eps = 1e-6
    inside = (u > 0) & (u < r[:, fr.HF_NX] - 1) & (v > 0) & (v < r[:, fr.HF_NY] - 1) & \
        (edge * r[:, fr.HF_CELL] > 2 * eps)
    assert inside.sum() > 50
    height = lambda q: q[:, 2] - (lambda h, m: h / m[:, 2])(*mpcqp.field_lookup(rows, heights, idx, q))  # noqa: E731
    for k in range(2):
        d = np.zeros(3)
        d[k] = eps
        slope = (height(p + d) - height(p - d)) / (2 * eps)
        np.testing.assert_allclose((-n[:, k] / n[:, 2])[inside], slope[inside], atol=1e-9)
    # the nodes themselves
    i, j = 3, 2
    node = np.array([-0.3 + i * 0.2, 0.1 + j * 0.2, 0.0])
    assert abs(-mpcqp.field_lookup(rows, heights, 0, node[None])[0][0]
               / mpcqp.field_lookup(rows, heights, 0, node[None])[1][0, 2] - a[j, i]) <= 1e-16


def test_field_lookup_is_continuous_across_cell_lines():
    rows, heights, a, b = _rough()
    rng = np.random.Generator(np.random.PCG64(14))
    height = lambda q: q[:, 2] - (lambda h, m: h / m[:, 2])(*mpcqp.field_lookup(rows, heights, 0, q))  # noqa: E731
    for axis, count in ((0, 6), (1, 4)):
        for line in range(1, count - 1):
            q = np.stack([rng.uniform(-0.3, 0.7, 50), rng.uniform(0.1, 0.7, 50), np.zeros(50)], 1)
            at = (-0.3, 0.1)[axis] + line * 0.2
            lo, hi = q.copy(), q.copy()
            lo[:, axis], hi[:, axis] = at - 1e-12, at + 1e-12
            assert np.abs(height(hi) - height(lo)).max() <= 1e-11, (axis, line)


def test_field_lookup_is_flat_beyond_the_border_and_indexes_nothing_outside():
    rows, heights, a, b = _rough()
    z = 0.2
    # beyond each border the height is the border's, with no gradient across it
    for p, want in (([-0.9, 0.3, z], None), ([1.5, 0.3, z], None), ([0.1, -0.5, z], None), ([0.1, 2.0, z], None)):
        p = np.array(p)
        inner = np.array([min(max(p[0], -0.3), 0.7), min(max(p[1], 0.1), 0.7), z])
        (h0, n0), (h1, n1) = mpcqp.field_lookup(rows, heights, 0, p[None]), mpcqp.field_lookup(rows, heights, 0, inner[None])
        assert abs(h0[0] / n0[0, 2] - h1[0] / n1[0, 2]) <= 1e-16
        across = 0 if p[0] != inner[0] else 1
        assert n0[0, across] == 0.0
    h, n = mpcqp.field_lookup(rows, heights, 0, np.array([[-5.0, -5.0, z]]))
    assert np.array_equal(n[0], [0.0, 0.0, 1.0]) and h[0] == z - a[0, 0]
    # far points and non-finite ones: the cell index is clamped on the double, so nothing outside the tile is indexed
    for fn in (mpcqp.plant._field_cell, fr._cell):
        with np.errstate(all="ignore"):
            c, _ = fn(np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 4e9, -4e9, 1e6, -1e6, 2.5]), 6.0)
        assert np.array_equal(c, [0, 4, 0, 4, 0, 4, 0, 4, 0, 2])
    guard = np.full(heights.size + 16, np.nan)
    guard[8:-8] = heights
    shifted = rows.copy()
    shifted[:, fr.HF_OFFSET] += 8
    far = np.array([[1e6, 1e6, z], [-1e6, 1e6, z], [1e6, -1e6, z], [-1e6, -1e6, z]])
    for k, tile in ((0, a), (1, b)):
        h, n = mpcqp.field_lookup(shifted, guard, k, far)
        assert np.array_equal(h, z - np.array([tile[-1, -1], tile[-1, 0], tile[0, -1], tile[0, 0]]))
        assert np.all(n == [0.0, 0.0, 1.0])
    with np.errstate(all="ignore"):
        h, n = mpcqp.field_lookup(shifted, guard, 1, np.array([[np.nan, 0.0, z], [0.0, np.nan, z], [np.inf, -np.inf, z]]))
        fr.lookup(shifted[[1, 1, 1]], guard, np.array([[np.nan, 0.0, z], [0.0, np.nan, z], [np.inf, -np.inf, z]]))
    assert h.shape == (3,)


# ---- the closed-loop fleet: eight robots on four tiles of one heights array -------------------------------------------
CELL, NX, NY, X0, Y0 = 0.05, 33, 25, -0.8, -0.6


def loop_tiles():
    """Rolling ground of 3 cm amplitude, a 5 cm step with a one-cell riser, the same step as a ramp of slope 0.25, and
    stairs of 8 cm with 30 cm treads; each on 33 x 25 nodes of 5 cm."""
    x = (X0 + CELL * np.arange(NX))[None, :] + np.zeros((NY, 1))
    y = (Y0 + CELL * np.arange(NY))[:, None] + np.zeros((1, NX))
    ramp = lambda at, width: np.clip((x - at) / width, 0.0, 1.0)  # noqa: E731
    rolling = 0.03 * np.sin(2 * np.pi * x / 0.9 + 0.4) * np.cos(2 * np.pi * y / 1.3 - 0.2)
    step = 0.05 * ramp(0.0, CELL)
    gentle = 0.05 * ramp(0.0, 4 * CELL)
    stairs = 0.08 * (ramp(-0.35, CELL) + ramp(-0.05, CELL) + ramp(0.25, CELL) + ramp(0.55, CELL))
    return [rolling, step, gentle, stairs]


# (tile, x, y, yaw) of the eight robots
FLEET = [(0, 0.0, 0.0, 0.3), (0, 0.1, -0.05, -2.0), (1, 0.02, 0.0, 0.0), (1, 0.03, 0.02, np.pi / 2),
         (2, -0.08, 0.0, 0.0), (3, 0.04, 0.0, 0.0), (3, 0.22, 0.05, np.pi), (3, 0.04, 0.0, np.pi / 2)]


def field_fleet(mu=0.6):
    """(header rows, heights, init rows, euler_d) of the closed-loop fleet, shared with the device twin."""
    which = [f[0] for f in FLEET]
    rows, heights = mpcqp.pack_height_field(loop_tiles(), X0, Y0, CELL, mu, share=which)
    B = len(FLEET)
    p = pr.default_params()
    ro, rf = pr._geom(p)
    q = np.tile(np.array(p.default_joint_pos), (B, 1))
    z0 = -er.fk(q.reshape(B, 4, 3), ro, rf)[:, 0, 2]
    yaw = np.array([f[3] for f in FLEET])
    quat = np.stack([np.cos(yaw / 2), np.zeros(B), np.zeros(B), np.sin(yaw / 2)], 1)
    flat = mpcqp.pack_plant_init(np.stack([[f[1] for f in FLEET], [f[2] for f in FLEET], z0], 1), quat, q)
    init, euler = mpcqp.place_on_field(flat, rows, heights, np.arange(B))
    return rows, heights, init, euler


def tilt_of(quat):
    """The angle between the trunk's z axis and the world's, from the quaternion [..., 4] (w, x, y, z)."""
    w, x, y, z = (quat[..., k] for k in range(4))
    return np.arctan2(np.hypot(2 * (x * z + w * y), 2 * (y * z - w * x)), 1 - 2 * (x * x + y * y))


def test_pack_and_place_on_field():
    rows, heights, init, euler = field_fleet()
    B = init.shape[0]
    feet = feet_of(init)
    h, n = mpcqp.field_lookup(rows, heights, np.arange(B), feet)
    slope = np.sqrt(1.0 / n[..., 2] ** 2 - 1.0)
    print(f"[note] placed feet: hgt {h.min():.3e} .. {h.max():.3e}; facet slopes up to {slope.max():.3f}; foot heights "
          f"{np.round((feet[..., 2]).min(), 3)} .. {np.round((feet[..., 2]).max(), 3)}")
    assert np.all(h <= 0.0) and np.all(h >= -1e-15)
    assert slope.max() <= 0.3 and slope.max() > 0.2  # under the friction angle of mu 0.6, and not flat
    assert np.ptp(feet[..., 2], axis=1).max() >= 0.079  # a robot stands across a stair
    # level at the start row's yaw and x, y
    np.testing.assert_allclose(er.quat_to_euler(init[:, 3:7]), euler, atol=1e-15)
    assert np.all(euler[:, :2] == 0.0) and np.allclose(euler[:, 2], [f[3] for f in FLEET], atol=1e-15)
    assert np.array_equal(init[:, :2], np.array([[f[1], f[2]] for f in FLEET]))
    # the height over the mean ground under the nominal feet: the start row's own, or the one given
    p = pr.default_params()
    z0 = -er.fk(np.array(p.default_joint_pos).reshape(1, 4, 3), *pr._geom(p))[0, 0, 2]
    ground = (feet[..., 2] - h / n[..., 2]).mean(1)
    np.testing.assert_allclose(init[:, 2] - ground, z0, atol=1e-12)
    low, _ = mpcqp.place_on_field(init, rows, heights, np.arange(B), height=0.25)
    np.testing.assert_allclose(low[:, 2] - ground, 0.25, atol=1e-12)
    # every foot starts held
    plant = fr.FieldPlant(p, B)
    o = plant.step(DT, np.zeros((B, 12)), init, field=(rows, heights))[0]
    assert o["contacts"].all() and np.all(o["status"] == 0.0)
    with pytest.raises(ValueError, match="reach"):
        mpcqp.place_on_field(init, rows, heights, np.arange(B), height=0.6)


@pytest.mark.parametrize("substeps", [1, 4])
def test_planar_tile_is_the_plane_model(substeps):
    """A tile sampled from each robot's plane against terrain_reference.TerrainPlant, teacher-forced on the inputs of
    the terrain parity test: equal statuses and contacts, values within 1e-12 (the level-row test's tolerance)."""
    B = 67
    init, tau, wr, terrain = tt.parity_inputs(B, substeps)
    rows, heights = planar_tiles(terrain, init[:, :2])
    p = pr.default_params(substeps=substeps)
    slot = np.zeros((B, pr.PN_SIZE))
    worst, stance, swing = 0.0, 0, 0
    for t in range(tt.PARITY_TICKS):
        a, b = tr.TerrainPlant(p, B, slot=slot), fr.FieldPlant(p, B, slot=slot)
        oa, wa, ma = a.step(DT, tau[t], init, wrench=wr[t], terrain=terrain)
        ob, wb, mb = b.step(DT, tau[t], init, wrench=wr[t], field=(rows, heights))
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
        slot = a.slot
    print(f"[note] planar tile against terrain_reference, substeps {substeps}: worst difference {worst:.3e}, stance "
          f"{stance} swing {swing} leg-ticks")
    assert stance > 0 and swing > 0


@pytest.mark.parametrize("B,substeps", sorted(PARITY_SEEDS))
def test_parity_inputs_exclude_nothing(B, substeps):
    """The inputs of the device's teacher-forced parity test: on the restatement alone no robot-tick has a decision
    margin under 1e-9, the cap under which the device test would leave a robot-tick out."""
    init, tau, wr, rows, heights = parity_inputs(B, substeps)
    plant = fr.FieldPlant(pr.default_params(substeps=substeps), B)
    worst, stance, swing, clipped = np.inf, 0, 0, 0
    for t in range(PARITY_TICKS):
        o, wrote, margin = plant.step(DT, tau[t], init, wrench=wr[t], field=(rows, heights))
        worst = min(worst, float(margin.min()))
        stance += int(o["contacts"].sum())
        swing += int((~o["contacts"]).sum())
        clipped += sum(int(f[2].sum()) for f in plant.friction)
    print(f"[note] B={B} substeps={substeps}: smallest margin {worst:.3e}, stance {stance} swing {swing}, clipped "
          f"{clipped} leg-substeps")
    assert worst >= 1e-9
    if B > 1:
        assert stance > 0 and swing > 0 and clipped > 0
    es, table = shuffled_pool(B, rows)
    assert np.array_equal(table[es[:, tr.ES_POOL].astype(int)], rows)


def closed_loop(oracle, ticks):
    """tests/test_terrain.py's closed loop on the field fleet: the oracle's MPC fed the plant's true state, substeps 1
    on the even robots, 4 on the odd ones.  Returns the per-tick records."""
    rows, heights, init, euler_d = field_fleet()
    B = init.shape[0]
    op = oracle.default_params(10)
    idx = [np.arange(0, B, 2), np.arange(1, B, 2)]
    plants = [fr.FieldPlant(pr.default_params(substeps=n), len(i)) for n, i in zip((1, 4), idx)]
    solvers = [oracle.WarmSolver(op) for _ in range(B)]
    pos_d = init[:, pr.PI_POS:pr.PI_POS + 3].copy()
    tau = np.zeros((B, 12))
    rec = dict(status=[], contacts=[], solve=[], grf=[], pos=[], foot=[], quat=[])
    for t in range(ticks + 1):
        outs = [pl.step(DT, tau[i], init[i], field=(rows[i], heights))[0] for pl, i in zip(plants, idx)]
        out = {}
        for k in outs[0]:
            out[k] = np.zeros((B,) + outs[0][k].shape[1:], dtype=outs[0][k].dtype)
            for o, i in zip(outs, idx):
                out[k][i] = o[k]
        rec["status"].append(out["status"].copy())
        rec["contacts"].append(out["contacts"].copy())
        rec["grf"].append(out["grf"].copy())
        rec["pos"].append(out["root_pos"].copy())
        rec["foot"].append(out["foot_world"].copy())
        rec["quat"].append(out["quat"].copy())
        recs = mpcqp.assemble_compute_grf(truth_states(out, pos_d, euler_d), 10)
        res = np.array([sv.step(recs[b])[0] for b, sv in enumerate(solvers)])
        rec["solve"].append(res["status"].copy())
        fb = res["f_body"].reshape(B, 4, 3)
        tau = np.einsum("blji,blj->bli", out["j_foot"], -fb).reshape(B, 12)
    for sv in solvers:
        sv.close()
    rec = {k: np.array(v) for k, v in rec.items()}
    rec.update(rows=rows, heights=heights, pos_d=pos_d)
    return rec


def field_conditions(rows, heights, pos_d, status, contacts, solve, grf_end, pos_end, foot, quat, mass, gravity):
    """tests/test_terrain.py's slope_conditions with the hgt of the field, shared with the device twin: status /
    contacts / quat per tick, solve the solve statuses from tick 1 on, grf_end / pos_end the last tick's, foot every
    tick's held feet [T,B,4,3].  Returns the largest tilt."""
    B = rows.shape[0]
    idx = np.arange(B)
    assert np.all(status == 0.0), status.max(0)
    assert np.all(contacts)
    assert np.all(solve == _lib.STATUS_SOLVED)
    ratio = grf_end.sum(1) / (mass * gravity) - np.array([0.0, 0.0, 1.0])
    dh = mpcqp.field_lookup(rows, heights, idx, pos_end)[0] - mpcqp.field_lookup(rows, heights, idx, pos_d)[0]
    hf = np.abs(mpcqp.field_lookup(rows, heights, idx, np.swapaxes(foot, 0, 1))[0]).max()
    tilt = float(tilt_of(quat).max())
    print(f"[note] field: |sum F / m g - e_z| {np.abs(ratio).max():.3e}, |hgt(pos) - hgt(pos_d)| {np.abs(dh).max():.3e}, "
          f"held feet |hgt| {hf:.3e}, largest tilt {tilt:.3e} rad (gate {TILT_GATE:.3e})")
    assert np.all(np.abs(ratio) <= 0.01), ratio
    assert np.all(np.abs(dh) <= 0.01), dh
    assert hf <= 1e-12
    assert tilt <= TILT_GATE
    return tilt


def test_closed_loop_on_the_field_with_the_oracle_mpc(oracle):
    """Eight robots standing level on rolling, step, ramp and stairs tiles at mu 0.6 for 400 ticks."""
    r = closed_loop(oracle, 400)
    p = pr.default_params()
    field_conditions(r["rows"], r["heights"], r["pos_d"], r["status"], r["contacts"], r["solve"][1:], r["grf"][-1],
                     r["pos"][-1], r["foot"], r["quat"], p.mass, p.gravity)
