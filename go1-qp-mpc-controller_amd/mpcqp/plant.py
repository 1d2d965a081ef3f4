"""Plant stage of the control tick (host side of mpcqp_plant_step_device).

Per robot and per tick the device stage advances a rigid-body model of the robot by one control period
under the tick's joint torques and writes the next tick's sensor-level rows: a single rigid trunk on
massless stance legs (a held foot turns the joint torques into the ground reaction f = -R J^-T tau),
joint-space swing legs, flat ground, (plant_step_terrain_device) a per-robot inclined plane with its own friction
coefficient or (plant_step_field_device) a bilinear height field of steps, stairs or rough ground, semi-implicit
Euler in ``substeps`` substeps.  Left out: leg mass, the swing legs' reaction on the trunk, foot slip, overhangs, a
riser's vertical face as anything but one steep cell, trunk-ground contact, joint limits, and impact dynamics
beyond zeroing the landing foot's velocity.  The state lives in a per-robot device slot of ``plant_state_size()`` doubles;
zero-filled = fresh, and zeroing a robot's slots is how a fleet resets a fallen robot (a robot whose status
is not 0 is frozen until then).  The episode stage (episode.py) does that on the device: it ends a fallen
robot's episode, zeroes its slots over two ticks and restarts it from a drawn start row.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import (HF_CELL, HF_MU, HF_NX, HF_NY, HF_OFFSET, HF_SIZE, HF_X0, HF_Y0, PI_JOINT_POS, PI_POS, PI_QUAT,
                   PI_SIZE, TR_MU, TR_NORMAL, TR_OFFSET, TR_SIZE, PlantParams, check, load, override)

# the slot (include/mpcqp.h MPCQP_PN_*) and the output row (MPCQP_PT_*)
PLANT_STATE_DTYPE = np.dtype([
    ("init", "f8"), ("pos", "f8", 3), ("quat", "f8", 4), ("lin_vel", "f8", 3), ("ang_vel", "f8", 3),
    ("joint_pos", "f8", 12), ("joint_vel", "f8", 12), ("foot", "f8", (4, 3)), ("contact", "f8", 4),
    ("acc", "f8", 3), ("status", "f8"), ("pad", "f8", 6),
])
assert PLANT_STATE_DTYPE.itemsize == 8 * _lib.PN_SIZE
PLANT_OUT_DTYPE = np.dtype([
    ("pos", "f8", 3), ("quat", "f8", 4), ("euler", "f8", 3), ("lin_vel", "f8", 3), ("ang_vel", "f8", 3),
    ("contacts", "f8", 4), ("grf", "f8", (4, 3)), ("foot", "f8", (4, 3)), ("acc", "f8", 3), ("status", "f8"),
])
assert PLANT_OUT_DTYPE.itemsize == 8 * _lib.PT_SIZE

PLANT_OK, PLANT_OUT_OF_REACH, PLANT_FALLEN, PLANT_BAD_TORQUE = 0, 1, 2, 3

def default_plant_params(**over):
    """mpcqp_plant_default_params + keyword overrides; the array fields accept anything that flattens to
    their size (rho_fix [4][5], rho_opt [4][3], inertia [3][3], ...)."""
    p = PlantParams()
    load().mpcqp_plant_default_params(ctypes.byref(p))
    return override(p, over)


def plant_state_size():
    """Doubles per robot of the plant slot (mpcqp_plant_state_size)."""
    return int(load().mpcqp_plant_state_size())


def pack_plant_init(pos, quat, joint_pos):
    """Init rows [B, PI_SIZE] (include/mpcqp.h MPCQP_PI_*): pos [B,3], quat [B,4] as w, x, y, z, joint_pos
    [B,12] (FL FR RL RR x hip, thigh, calf)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    B = pos.shape[0]
    row = np.zeros((B, PI_SIZE))
    row[:, PI_POS:PI_POS + 3] = pos
    row[:, PI_QUAT:PI_QUAT + 4] = np.asarray(quat, dtype=np.float64).reshape(B, 4)
    row[:, PI_JOINT_POS:PI_JOINT_POS + 12] = np.asarray(joint_pos, dtype=np.float64).reshape(B, 12)
    return row


def pack_terrain(normal, offset, mu):
    """Terrain rows [P, TR_SIZE] (include/mpcqp.h MPCQP_TR_*) of the planes {p : n.p = offset} with friction
    ``mu``: ``normal`` [P,3] is normalised here; ``offset`` and ``mu`` broadcast over the rows.  Raises on a
    normal whose z is not positive, a non-finite entry or a negative mu."""
    n = np.asarray(normal, dtype=np.float64).reshape(-1, 3)
    P = n.shape[0]
    d = np.broadcast_to(np.asarray(offset, dtype=np.float64), (P,))
    m = np.broadcast_to(np.asarray(mu, dtype=np.float64), (P,))
    if not (np.all(np.isfinite(n)) and np.all(np.isfinite(d)) and np.all(np.isfinite(m))):
        raise ValueError("pack_terrain: non-finite entry")
    if np.any(n[:, 2] <= 0.0):
        raise ValueError("pack_terrain: the normal's z must be positive")
    if np.any(m < 0.0):
        raise ValueError("pack_terrain: mu must not be negative")
    row = np.zeros((P, TR_SIZE))
    row[:, TR_NORMAL:TR_NORMAL + 3] = n / np.linalg.norm(n, axis=1, keepdims=True)
    row[:, TR_OFFSET] = d
    row[:, TR_MU] = m
    return row


def terrain_from_slope(pitch, roll, mu, point=(0.0, 0.0, 0.0)):
    """Terrain rows of the planes through ``point`` with the normal n = R_y(pitch) R_x(roll) e_z (a robot that
    heads along +x on a ground of positive pitch looks downhill, as a positive body pitch is nose down); the
    arguments broadcast over the rows."""
    pitch, roll, mu = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64).reshape(-1) for a in (pitch, roll, mu)))
    n = np.stack([np.sin(pitch) * np.cos(roll), -np.sin(roll), np.cos(pitch) * np.cos(roll)], 1)
    pt = np.broadcast_to(np.asarray(point, dtype=np.float64), n.shape)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    return pack_terrain(n, np.sum(n * pt, 1), mu)


def terrain_height(terrain_rows, p):
    """hgt(p) = ((n0 p0 + n1 p1) + n2 p2) - d of points p [P, ..., 3] over the planes of the rows [P, TR_SIZE]."""
    t = np.asarray(terrain_rows, dtype=np.float64).reshape(-1, TR_SIZE)
    p = np.asarray(p, dtype=np.float64)
    n = t[:, TR_NORMAL:TR_NORMAL + 3].reshape((t.shape[0],) + (1,) * (p.ndim - 2) + (3,))
    d = t[:, TR_OFFSET].reshape((t.shape[0],) + (1,) * (p.ndim - 2))
    return ((n[..., 0] * p[..., 0] + n[..., 1] * p[..., 1]) + n[..., 2] * p[..., 2]) - d


def _quat_mul(a, b):
    aw, ax, ay, az = (a[:, k] for k in range(4))
    bw, bx, by, bz = (b[:, k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], 1)


def _quat_rot(q):
    w, x, y, z = (q[:, k] for k in range(4))
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def place_on_terrain(init_rows, terrain_rows, pp=None, point=None, lower=True):
    """Flat-ground init rows [B, PI_SIZE] (feet on z = 0) placed on the planes of ``terrain_rows`` [B, TR_SIZE]:
    position and attitude are rotated about the origin by the ground rotation G = R_y(pitch) R_x(roll) with
    G e_z = n and shifted by ``point`` [B,3] on the plane (default: d n, the plane's point nearest the origin);
    the trunk is then lowered along n by the highest foot's height over the plane plus 5e-16, so every foot starts
    held (a foot a few 1e-17 above the ground would start in swing) and none deeper than 1e-15: the feet of a stance
    differ by a few 1e-17 after the rotation and the lowered position rounds to its last place, which 1e-15 itself
    would leave no room for.  ``lower=False`` leaves that out, and every foot keeps the height it had over z = 0.
    ``pp``: the PlantParams whose leg geometry places the feet (default: the library's).  Returns the init rows and
    the slope-parallel (roll, pitch, yaw) [B,3] of the placed attitude, for root_euler_d."""
    init = np.array(init_rows, dtype=np.float64).reshape(-1, PI_SIZE)
    B = init.shape[0]
    t = np.asarray(terrain_rows, dtype=np.float64).reshape(B, TR_SIZE)
    n, d = t[:, TR_NORMAL:TR_NORMAL + 3], t[:, TR_OFFSET]
    pitch, roll = np.arctan2(n[:, 0], n[:, 2]), -np.arcsin(np.clip(n[:, 1], -1.0, 1.0))
    zero = np.zeros(B)
    qg = _quat_mul(np.stack([np.cos(pitch / 2), zero, np.sin(pitch / 2), zero], 1),
                   np.stack([np.cos(roll / 2), np.sin(roll / 2), zero, zero], 1))
    G = _quat_rot(qg)
    shift = n * d[:, None] if point is None else np.broadcast_to(np.asarray(point, dtype=np.float64), (B, 3))
    quat = _quat_mul(qg, init[:, PI_QUAT:PI_QUAT + 4])
    quat = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    pos = np.einsum("bij,bj->bi", G, init[:, PI_POS:PI_POS + 3]) + shift
    pp = default_plant_params() if pp is None else pp
    feet = _feet_body(pp, init[:, PI_JOINT_POS:PI_JOINT_POS + 12].reshape(B, 4, 3))
    R = _quat_rot(quat)
    for again in range(4 if lower else 0):  # (again only for a robot whose highest foot rounded to above the plane)
        top = terrain_height(t, pos[:, None] + np.einsum("bij,blj->bli", R, feet)).max(1)
        if again and np.all(top <= 0.0):
            break
        pos = pos - np.where((top > 0.0) | (again == 0), top + 5e-16, 0.0)[:, None] * n
    out = init.copy()
    out[:, PI_POS:PI_POS + 3] = pos
    out[:, PI_QUAT:PI_QUAT + 4] = quat
    euler = np.stack([np.arctan2(R[:, 2, 1], R[:, 2, 2]), np.arcsin(np.clip(-R[:, 2, 0], -1.0, 1.0)),
                      np.arctan2(R[:, 1, 0], R[:, 0, 0])], 1)
    return out, euler


def _feet_body(pp, q):
    """Foot positions in the body frame [B,4,3] from joint angles [B,4,3]: the forward kinematics of the plant
    (csrc/mpcqp_plant.hip fk_jac) on the geometry of ``pp``."""
    fix = np.array(list(pp.rho_fix), dtype=np.float64).reshape(1, 4, 5)
    opt = np.array(list(pp.rho_opt), dtype=np.float64).reshape(1, 4, 3)
    ox, oy, dd, lt, le, a0 = fix[..., 0], fix[..., 1], fix[..., 2] + opt[..., 1], fix[..., 3], fix[..., 4] - opt[..., 2], opt[..., 0]
    s0, c0, s1, c1 = np.sin(q[..., 0]), np.cos(q[..., 0]), np.sin(q[..., 1]), np.cos(q[..., 1])
    s12, c12 = np.sin(q[..., 1] + q[..., 2]), np.cos(q[..., 1] + q[..., 2])
    hh = lt * c1 + (le * c12 + a0 * s12)
    xx = (a0 * c12 - le * s12) - lt * s1
    return np.stack([ox + xx, oy + (dd * c0 + hh * s0), dd * s0 - hh * c0], -1)


def pack_height_field(tiles, x0, y0, cell, mu, share=None):
    """Header rows [P, HF_SIZE] (include/mpcqp.h MPCQP_HF_*) and the heights array of the bilinear height-field
    ground.  ``tiles``: a list of 2-D arrays H[ny][nx] of possibly different shapes, node (i, j) of a row's tile at
    (x0 + i cell, y0 + j cell).  ``share`` [P]: the tile of each header row, so several rows (start poses) share a
    tile; None: one row per tile, in order.  ``x0``, ``y0``, ``cell`` and ``mu`` broadcast over the rows.  Raises on a
    non-finite entry, a tile under 2x2, cell <= 0 and mu < 0 (the device checks the header, not the heights)."""
    tiles = [np.asarray(t, dtype=np.float64) for t in tiles]
    for t in tiles:
        if t.ndim != 2 or t.shape[0] < 2 or t.shape[1] < 2:
            raise ValueError(f"pack_height_field: a tile needs at least 2x2 nodes, not {t.shape}")
        if not np.all(np.isfinite(t)):
            raise ValueError("pack_height_field: non-finite height")
    which = np.arange(len(tiles)) if share is None else np.asarray(share, dtype=np.int64).reshape(-1)
    if which.size == 0 or which.min() < 0 or which.max() >= len(tiles):
        raise ValueError("pack_height_field: share names a tile that is not there")
    P = which.shape[0]
    x0, y0, cell, mu = (np.broadcast_to(np.asarray(a, dtype=np.float64), (P,)) for a in (x0, y0, cell, mu))
    if not all(np.all(np.isfinite(a)) for a in (x0, y0, cell, mu)):
        raise ValueError("pack_height_field: non-finite entry")
    if np.any(cell <= 0.0):
        raise ValueError("pack_height_field: cell must be positive")
    if np.any(mu < 0.0):
        raise ValueError("pack_height_field: mu must not be negative")
    offset = np.concatenate([[0], np.cumsum([t.size for t in tiles])])
    rows = np.zeros((P, HF_SIZE))
    rows[:, HF_X0], rows[:, HF_Y0], rows[:, HF_CELL], rows[:, HF_MU] = x0, y0, cell, mu
    rows[:, HF_NX] = [tiles[k].shape[1] for k in which]
    rows[:, HF_NY] = [tiles[k].shape[0] for k in which]
    rows[:, HF_OFFSET] = offset[which]
    return rows, np.concatenate([t.ravel() for t in tiles])


def _field_cell(u, n):
    """The cell index along one axis, clamped on the double to [0, n - 2], and u - index."""
    with np.errstate(invalid="ignore"):
        c = np.floor(u)
        c = np.where(c > 0.0, c, 0.0)  # (a NaN ends as 0)
        c = np.where(c < n - 2.0, c, n - 2.0)
        return c.astype(np.int64), u - c


def field_lookup(rows, heights, row_index, p):
    """(hgt, n) of the world points p [..., 3] over the tiles of the header rows ``row_index`` (an int or an int array
    that broadcasts against p's leading axes from the left), with the arithmetic of the statement in
    include/mpcqp.h: hgt [...] = (p_z - h) n_z, the first-order normal distance, and the unit normal n [..., 3]."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, HF_SIZE)
    H = np.asarray(heights, dtype=np.float64).reshape(-1)
    p = np.asarray(p, dtype=np.float64)
    idx = np.asarray(row_index, dtype=np.int64)
    r = rows[idx.reshape(idx.shape + (1,) * (p.ndim - 1 - idx.ndim))]
    x0, y0, cell = r[..., HF_X0], r[..., HF_Y0], r[..., HF_CELL]
    nx, ny, off = r[..., HF_NX], r[..., HF_NY], r[..., HF_OFFSET].astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        i, fu_raw = _field_cell((p[..., 0] - x0) / cell, nx)
        j, fv_raw = _field_cell((p[..., 1] - y0) / cell, ny)
        at = off + j * nx.astype(np.int64) + i
        h00, h10, h01, h11 = H[at], H[at + 1], H[at + nx.astype(np.int64)], H[at + nx.astype(np.int64) + 1]
        fu, fv = np.minimum(np.maximum(fu_raw, 0.0), 1.0), np.minimum(np.maximum(fv_raw, 0.0), 1.0)
        d0, d1 = h10 - h00, h11 - h01
        a = h00 + fu * d0
        b = h01 + fu * d1
        ba = b - a
        h = a + fv * ba
        gx = np.where((fu_raw < 0.0) | (fu_raw > 1.0), 0.0, (d0 + fv * (d1 - d0)) / cell)
        gy = np.where((fv_raw < 0.0) | (fv_raw > 1.0), 0.0, ba / cell)
        s = np.sqrt((gx * gx + gy * gy) + 1.0)
        n = np.stack([(-gx) / s, (-gy) / s, 1.0 / s], -1)
        return (p[..., 2] - h) * n[..., 2], n


def _ik_body(pp, p):
    """Joint angles [B,4,3] of body-frame foot positions [B,4,3] and the in-reach flag [B,4]: the inverse kinematics
    of the plant (csrc/mpcqp_plant.hip ik) on the geometry of ``pp``."""
    fix = np.array(list(pp.rho_fix), dtype=np.float64).reshape(1, 4, 5)
    opt = np.array(list(pp.rho_opt), dtype=np.float64).reshape(1, 4, 3)
    ox, oy, dd, lt, le, a0 = fix[..., 0], fix[..., 1], fix[..., 2] + opt[..., 1], fix[..., 3], fix[..., 4] - opt[..., 2], opt[..., 0]
    lce, phi = np.sqrt(le * le + a0 * a0), np.arctan2(a0, le)
    x, y, z = p[..., 0] - ox, p[..., 1] - oy, p[..., 2]
    with np.errstate(invalid="ignore"):
        arg = (y * y + z * z) - dd * dd
        hh = np.sqrt(arg)
        c = (((x * x + hh * hh) - lt * lt) - lce * lce) / ((2.0 * lt) * lce)
        qk = -np.arccos(c)
        q = np.stack([np.arctan2(z, y) - np.arctan2(-hh, dd),
                      np.arctan2(-x, hh) - np.arctan2(lce * np.sin(qk), lt + lce * np.cos(qk)), qk + phi], -1)
        return q, (arg >= 0.0) & (np.abs(c) <= 1.0)


def place_on_field(init_rows, rows, heights, row_index, pp=None, height=None):
    """Init rows [B, PI_SIZE] placed as a stance on the height field of the header rows ``row_index`` [B]: the trunk
    is level at the start row's yaw and x, y, at ``height`` (default: the start row's own z) over the mean ground
    under the four nominal feet (those of the start row's joint angles); every leg's joint angles come from the
    plant's inverse kinematics with its foot on the surface under the nominal foot, 5e-16 under it in hgt so that
    rounding leaves every foot held and none deeper than 1e-15.  Raises if a foot is out of reach.  ``pp``: the
    PlantParams whose leg geometry places the feet (default: the library's).  Returns the init rows and the
    (roll, pitch, yaw) [B,3] of the placed attitude, for root_euler_d."""
    init = np.array(init_rows, dtype=np.float64).reshape(-1, PI_SIZE)
    B = init.shape[0]
    idx = np.broadcast_to(np.asarray(row_index, dtype=np.int64), (B,))
    pp = default_plant_params() if pp is None else pp
    q0 = init[:, PI_QUAT:PI_QUAT + 4]
    yaw = np.arctan2(2.0 * (q0[:, 0] * q0[:, 3] + q0[:, 1] * q0[:, 2]), 1.0 - 2.0 * (q0[:, 2] ** 2 + q0[:, 3] ** 2))
    zero = np.zeros(B)
    quat = np.stack([np.cos(yaw / 2), zero, zero, np.sin(yaw / 2)], 1)
    R = _quat_rot(quat)
    nominal = np.einsum("bij,blj->bli", R, _feet_body(pp, init[:, PI_JOINT_POS:PI_JOINT_POS + 12].reshape(B, 4, 3)))
    xy = init[:, None, PI_POS:PI_POS + 2] + nominal[..., :2]
    hf, n = field_lookup(rows, heights, idx, np.concatenate([xy, np.zeros((B, 4, 1))], -1))
    ground = -hf / n[..., 2]  # h under each nominal foot
    pos = init[:, PI_POS:PI_POS + 3].copy()
    pos[:, 2] = ground.mean(1) + (init[:, PI_POS + 2] if height is None else np.broadcast_to(height, (B,)))
    target = np.concatenate([xy, ground[..., None]], -1)
    for _ in range(8):
        q, ok = _ik_body(pp, np.einsum("bji,blj->bli", R, target - pos[:, None]))
        if not np.all(ok):
            raise ValueError(f"place_on_field: a foot of robot(s) {np.nonzero(~ok.all(1))[0].tolist()} is out of reach")
        foot = pos[:, None] + np.einsum("bij,blj->bli", R, _feet_body(pp, q))
        hf, n = field_lookup(rows, heights, idx, foot)
        if np.all((hf <= -2e-16) & (hf >= -8e-16)):
            break
        target[..., 2] -= (hf + 5e-16) / n[..., 2]
    else:
        raise ValueError("place_on_field: the feet did not settle on the surface")
    out = init.copy()
    out[:, PI_POS:PI_POS + 3] = pos
    out[:, PI_QUAT:PI_QUAT + 4] = quat
    out[:, PI_JOINT_POS:PI_JOINT_POS + 12] = q.reshape(B, 12)
    return out, np.stack([zero, zero, yaw], 1)


def plant_step_field_device(pp, dt, d_torques, d_wrench, d_field, field_rows, d_heights, heights_len, d_episode_state,
                            batch, d_plant_state, d_init=0, d_sensors=0, d_plan_in=0, d_states=0, d_tq_records=0,
                            d_plant_out=0, stream=0):
    """mpcqp_plant_step_field_device on device pointers (ints; 0 for the optional ones, d_wrench, d_field and
    d_episode_state among them).  Robot b stands on the tile of header row (int) episode_state[b][ES_POOL], or of row
    b without an episode slot."""
    check(load().mpcqp_plant_step_field_device(
        ctypes.byref(pp), float(dt), d_torques or None, d_wrench or None, d_field or None, int(field_rows),
        d_heights or None, int(heights_len), d_episode_state or None, int(batch), d_plant_state or None,
        d_init or None, d_sensors or None, d_plan_in or None, d_states or None, d_tq_records or None,
        d_plant_out or None, stream or None), None, "mpcqp_plant_step_field_device")


def plant_step_terrain_device(pp, dt, d_torques, d_wrench, d_terrain, terrain_rows, d_episode_state, batch,
                              d_plant_state, d_init=0, d_sensors=0, d_plan_in=0, d_states=0, d_tq_records=0,
                              d_plant_out=0, stream=0):
    """mpcqp_plant_step_terrain_device on device pointers (ints; 0 for the optional ones, d_wrench, d_terrain and
    d_episode_state among them).  Robot b stands on row (int) episode_state[b][ES_POOL] of the terrain table, or on
    row b without an episode slot."""
    check(load().mpcqp_plant_step_terrain_device(
        ctypes.byref(pp), float(dt), d_torques or None, d_wrench or None, d_terrain or None, int(terrain_rows),
        d_episode_state or None, int(batch), d_plant_state or None, d_init or None, d_sensors or None,
        d_plan_in or None, d_states or None, d_tq_records or None, d_plant_out or None, stream or None),
          None, "mpcqp_plant_step_terrain_device")


def plant_step_device(pp, dt, d_torques, batch, d_plant_state, d_init=0, d_sensors=0, d_plan_in=0, d_states=0,
                      d_tq_records=0, d_plant_out=0, stream=0):
    """mpcqp_plant_step_device on device pointers (ints; 0 for the optional ones)."""
    check(load().mpcqp_plant_step_device(ctypes.byref(pp), float(dt), d_torques or None, int(batch),
                                         d_plant_state or None, d_init or None, d_sensors or None, d_plan_in or None,
                                         d_states or None, d_tq_records or None, d_plant_out or None, stream or None),
          None, "mpcqp_plant_step_device")
