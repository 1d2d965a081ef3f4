"""Shared by the episode tests: start rows for a pool, and the teacher-forced cases of the episode stage: one
arena of doubles holding every buffer the stage may touch with guard gaps in between, filled with a canary
pattern, and per-tick hand-written plant_out / torque / sensor / cmd / result rows.  No device here."""
import numpy as np

import estimator_reference as er
import episode_reference as ep
import plant_reference as pr

GUARD = 16  # doubles between two buffers
OPTIONAL = ("plant_init", "joint_torques", "sensors", "cmd", "results", "pool", "scripts", "states", "counter", "log",
            "totals", "est_state", "plan_state", "cmd_state", "policy_state", "warm")
SLOTS = ("est_state", "plan_state", "cmd_state", "policy_state", "warm")
SIZES = dict(est_state=332, plan_state=940, cmd_state=8, policy_state=28, warm=1234)


def quat_rpy(roll, pitch, yaw):
    """w, x, y, z of Rz(yaw) Ry(pitch) Rx(roll)."""
    cr, sr, cp, sp, cy, sy = (f(0.5 * a) for a in (roll, pitch, yaw) for f in (np.cos, np.sin))
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy])


def start_row(q_leg, rpy=(0.0, 0.0, 0.0)):
    """A plant init row: every leg at q_leg, the trunk at rpy, lowered so the deepest foot is 1 um under the
    ground (held from the start).  Returns (row [PI_SIZE], trunk height)."""
    p = pr.default_params()
    ro, rf = pr._geom(p)
    q = np.broadcast_to(np.asarray(q_leg, dtype=np.float64), (1, 4, 3))
    quat = quat_rpy(*rpy)
    rel = er.mat_vec(er.quat_to_rot(quat[None])[:, None], er.fk(q, ro, rf))
    z = -rel[..., 2].min() - 1e-6
    row = np.zeros(pr.PI_SIZE)
    row[pr.PI_POS + 2] = z
    row[pr.PI_QUAT:pr.PI_QUAT + 4] = quat
    row[pr.PI_JOINT_POS:pr.PI_JOINT_POS + 12] = q.reshape(12)
    return row, float(z)


def pool_rows(rows, heights, yaws=None):
    """Pool rows [P, POOL_SIZE] from init rows: root_euler_d = (0, 0, yaw), root_pos_d = (0, 0, height)."""
    P = len(rows)
    out = np.zeros((P, ep.POOL_SIZE))
    out[:, :pr.PI_SIZE] = rows
    out[:, ep.POOL_EULER_D + 2] = 0.0 if yaws is None else yaws
    out[:, ep.POOL_POS_D + 2] = heights
    return out


class Arena:
    """Every buffer of the stage in one array of doubles, GUARD doubles apart, each at an even offset."""

    def __init__(self, B, p, sizes=SIZES, missing=()):
        self.B, self.p, self.sizes, self.missing = B, p, dict(sizes), set(missing)
        shapes = dict(
            episode_state=(B, ep.ES_SIZE), plant_out=(B, ep.PT_SIZE), plant_state=(B, ep.PN_SIZE),
            plant_init=(B, ep.PI_SIZE), joint_torques=(B, 12), sensors=(B, ep.SN_SIZE), cmd=(B, ep.CM_SIZE),
            results=(B, ep.RESULT_DOUBLES), pool=(max(p.pool_count, 1), ep.POOL_SIZE),
            scripts=(max(p.script_count, 1), max(p.script_segments, 1), ep.SEG_SIZE), states=(B, ep.ST_SIZE),
            counter=((B + 1) // 2,), log=(B, p.log_len, ep.EL_SIZE), totals=(B, ep.ET_SIZE),
            **{k: (B, v) for k, v in self.sizes.items()})
        self.at, off = {}, GUARD
        for name, shape in shapes.items():
            n = int(np.prod(shape))
            self.at[name] = (off, n, shape)
            off += n + GUARD + ((n + GUARD) & 1)
        self.n = off

    def fill(self, pool, scripts):
        """The start: canaries everywhere, zero episode slots and totals, the pool and the scripts."""
        h = 1000.0 + np.arange(self.n, dtype=np.float64) * 0.5
        v = self.views(h)
        v["episode_state"][:] = 0.0
        v["totals"][:] = 0.0
        v["pool"][:] = pool if pool is not None else 0.0
        v["scripts"][:] = scripts if scripts is not None else -1.0
        v["counter"][:] = 7 + np.arange(v["counter"].size, dtype=np.int32)
        return h

    def views(self, h):
        """name -> array view into the arena h (counter as int32 [2 * ceil(B / 2)])."""
        out = {}
        for name, (off, n, shape) in self.at.items():
            a = h[off:off + n]
            out[name] = a.view(np.int32) if name == "counter" else a.reshape(shape)
        return out

    def guards(self, h):
        keep = np.ones(self.n, bool)
        for off, n, _ in self.at.values():
            keep[off:off + n] = False
        return h[keep]

    def stage_arrays(self, h):
        """The dict tests/episode_reference.step takes: the optional buffers that are `missing` left out."""
        v = self.views(h)
        a = {k: v[k] for k in v if k not in self.missing}
        if "counter" in a:
            a["counter"] = a["counter"][:self.B]
        return a


def hand_rows(B, t, seed, events):
    """The rows the host writes before tick t: healthy random robots, and per `events` {(t, b): kind} what goes
    wrong.  Non-finite values: NaN in any pose entry, inf in the position and the Euler angles."""
    rng = np.random.default_rng(1000 * seed + t)
    po = np.zeros((B, ep.PT_SIZE))
    po[:, ep.PT_POS:ep.PT_POS + 3] = rng.uniform(-1, 1, (B, 3)) * [2.0, 2.0, 0.02] + [0.0, 0.0, 0.3]
    q = rng.normal(size=(B, 4)) * [0.02, 0.05, 0.05, 0.3] + [1.0, 0.0, 0.0, 0.0]
    po[:, ep.PT_QUAT:ep.PT_QUAT + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
    po[:, ep.PT_EULER:ep.PT_EULER + 3] = rng.uniform(-1, 1, (B, 3)) * [0.1, 0.1, 3.0]
    po[:, ep.PT_LIN_VEL:ep.PT_LIN_VEL + 3] = rng.normal(size=(B, 3)) * 0.3
    po[:, ep.PT_ANG_VEL:ep.PT_ANG_VEL + 3] = rng.normal(size=(B, 3)) * 0.5
    po[:, ep.PT_CONTACTS:ep.PT_CONTACTS + 4] = rng.integers(0, 4, (B, 4)) > 0
    po[:, 20:ep.PT_STATUS] = rng.normal(size=(B, ep.PT_STATUS - 20))
    tq = rng.normal(size=(B, 12)) * 8.0
    sn = rng.normal(size=(B, ep.SN_SIZE))
    res = rng.normal(size=(B, ep.RESULT_DOUBLES))
    ri = res.view(np.int32).reshape(B, -1)
    ri[:, ep.RESULT_STATUS_I32] = rng.choice([1, 1, 1, 2, -2, -100], B)
    ri[:, ep.RESULT_ITERS_I32] = rng.integers(0, 200, B)
    for (te, b), kind in events.items():
        if te != t or b >= B:
            continue
        if kind.startswith("status"):
            po[b, ep.PT_STATUS] = float(kind[-1])
        elif kind == "tilt":
            po[b, ep.PT_EULER] = 0.6
        elif kind == "low":
            po[b, ep.PT_POS + 2] = 0.05
        elif kind == "high":
            po[b, ep.PT_POS + 2] = 0.9
        elif kind == "all":  # every reason at once: the first in the order wins
            po[b, ep.PT_STATUS], po[b, ep.PT_EULER], po[b, ep.PT_POS + 2] = 1.0, 0.6, 0.05
        else:
            what, at = kind.split(":")  # nan:<offset in the plant_out row>, inf:<offset>
            po[b, int(at)] = np.nan if what == "nan" else (np.inf if what == "inf" else -np.inf)
    return dict(plant_out=po, joint_torques=tq, sensors=sn, results=res)


def cmd_rows(B, seed):
    rng = np.random.default_rng(77 + seed)
    cm = np.zeros((B, ep.CM_SIZE))
    cm[:, :6] = rng.normal(size=(B, 6)) * 0.4
    return cm


def default_pool(P=3):
    rows, hs = zip(*(start_row([0.0, 0.8 + 0.05 * i, -1.6 - 0.1 * i], (0.01 * i, -0.02 * i, 0.3 * i)) for i in range(P)))
    return pool_rows(np.array(rows), np.array(hs), 0.3 * np.arange(P))


def default_scripts():
    """Two scripts of three segments: one that starts at tick 0 and toggles walking at tick 2, one whose first
    segment is at tick 1 and that has two segments only."""
    sc = np.full((2, 3, ep.SEG_SIZE), -1.0)
    sc[0, 0] = [0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    sc[0, 1] = [2, 0.3, 0.0, 0.0, 0.0, 0.0, 0.1, 1.0]
    sc[0, 2] = [4, 0.5, -0.1, 0.0, 0.0, 0.0, -0.2, 0.0]
    sc[1, 0] = [1, 0.2, 0.1, 0.0, 0.0, 0.0, 0.0, 1.0]
    sc[1, 1] = [3, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    return sc


def case_params(name, B):
    """(Params, events, ticks) of a named teacher-forced case."""
    kw = dict(seed=0x1234ABCD5678EF01, pool_count=3, script_count=2, script_segments=3, log_len=4, max_ticks=1000)
    ev, T = {}, 9
    if name == "none_end":
        pass
    elif name == "all_end":
        ev = {(5, b): "status2" for b in range(B)}
    elif name == "two_of_a_wave":
        ev = {(5, 1): "status1", (5, 3): "tilt"} if B > 3 else {(5, 0): "tilt"}
    elif name == "each_reason":
        kinds = ("status1", "status2", "status3", "tilt", "low", "high", "all", None)
        ev = {(4, b): kinds[b % 8] for b in range(B) if kinds[b % 8]}
        kw["max_ticks"] = 4  # the robots nothing happens to time out at the tick the others end at, or after
        T = 12
    elif name == "non_finite":
        # pos x y z, quat w x y z, roll pitch yaw as NaN and as +-inf
        kinds = [f"nan:{i}" for i in range(10)] + [f"inf:{i}" for i in range(10)] + ["ninf:2", "ninf:4", "ninf:9"]
        ev = {(3 + (b // len(kinds)) % 2, b): kinds[b % len(kinds)] for b in range(B)}
        if B < len(kinds):
            ev.update({(5 + i // B, i % B): kinds[i] for i in range(B, len(kinds))})
            T = 6 + len(kinds) // B + 3
    elif name == "ring":
        kw.update(log_len=2, max_ticks=3)
        T = 1 + 3 * 4  # the fresh tick, then three times priming and three episode ticks
    else:
        raise ValueError(name)
    return ep.Params(**kw), ev, T


CASES = ("none_end", "all_end", "two_of_a_wave", "each_reason", "non_finite", "ring")
