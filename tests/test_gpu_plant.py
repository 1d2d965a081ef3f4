"""The plant stage on the device (mpcqp_plant_step_device) against tests/plant_reference.py: teacher-forced
parity over mixed stance and swing, the two closed forms, and the isolation rules of frozen and non-finite
robots."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib

import estimator_reference as er
import plant_reference as pr
from test_plant import DT, stance_torques

pytestmark = pytest.mark.gpu

ROWS = ("sensors", "plan_in", "states", "tq", "out")
WIDTH = dict(sensors=_lib.SN_SIZE, plan_in=_lib.PL_SIZE, states=_lib.ST_SIZE, tq=_lib.TQ_SIZE, out=_lib.PT_SIZE)


class DevicePlant:
    """The stage's buffers for B robots; the rows start from a recognisable fill so an unwritten double shows."""

    def __init__(self, p, B, init=None, rows=ROWS):
        f64 = dict(dtype=torch.float64, device="cuda")
        self.p, self.B = p, B
        self.slot = torch.zeros((B, mpcqp.plant_state_size()), **f64)
        self.torques = torch.zeros((B, 12), **f64)
        self.init = None if init is None else torch.from_numpy(np.ascontiguousarray(init)).cuda()
        for name in ROWS:
            setattr(self, name, torch.full((B, WIDTH[name]), -7.25, **f64) if name in rows else None)

    def step(self, tau):
        self.torques.copy_(torch.from_numpy(np.ascontiguousarray(tau, dtype=np.float64).reshape(self.B, 12)))
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        mpcqp.plant_step_device(self.p, DT, self.torques.data_ptr(), self.B, self.slot.data_ptr(), ptr(self.init),
                                ptr(self.sensors), ptr(self.plan_in), ptr(self.states), ptr(self.tq), ptr(self.out),
                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return self.get()

    def get(self):
        d = {name: getattr(self, name).cpu().numpy() for name in ROWS if getattr(self, name) is not None}
        d["slot"] = self.slot.cpu().numpy()
        return d


def expected_rows(o):
    """{row: [(offset, values [B, n])]} of the doubles a tick writes, from the restatement's outputs."""
    B = o["quat"].shape[0]
    f = lambda a: np.asarray(a, dtype=np.float64).reshape(B, -1)  # noqa: E731
    return dict(
        sensors=[(_lib.SN_QUAT, f(o["quat"])), (_lib.SN_JOINT_POS, f(o["joint_pos"])),
                 (_lib.SN_JOINT_VEL, f(o["joint_vel"])), (_lib.SN_IMU_ACC, f(o["imu_acc"])),
                 (_lib.SN_IMU_ANG_VEL, f(o["imu_ang_vel"]))],
        plan_in=[(_lib.PL_ROT_Z, f(o["rot_z"])), (_lib.PL_FOOT_FORCE, f(o["foot_force"]))],
        states=[(_lib.ST_EULER, f(o["root_euler"])), (_lib.ST_POS, f(o["root_pos"])),
                (_lib.ST_ANG_VEL, f(o["root_ang_vel"])), (_lib.ST_LIN_VEL, f(o["root_lin_vel"])),
                (_lib.ST_ROT, f(o["root_rot_mat"])), (_lib.ST_FEET, f(o["foot_pos_abs"]))],
        tq=[(_lib.TQ_JFOOT, f(o["j_foot"]))],
        out=[(_lib.PT_POS, f(o["root_pos"])), (_lib.PT_QUAT, f(o["quat"])), (_lib.PT_EULER, f(o["root_euler"])),
             (_lib.PT_LIN_VEL, f(o["root_lin_vel"])), (_lib.PT_ANG_VEL, f(o["imu_ang_vel"])),
             (_lib.PT_CONTACTS, f(o["contacts"])), (_lib.PT_GRF, f(o["grf"])), (_lib.PT_FOOT, f(o["foot_world"])),
             (_lib.PT_ACC, f(o["acc"])), (_lib.PT_STATUS, f(o["status"]))])


def mixed_init(B, seed):
    """Init rows from the IK test's joint domain at a small tilt, the lowest foot 0 to 3 cm above the ground."""
    p = pr.default_params()
    ro, rf = pr._geom(p)
    rng = np.random.Generator(np.random.PCG64(seed))
    q = np.stack([rng.uniform(-0.6, 0.6, (B, 4)), rng.uniform(0.2, 1.4, (B, 4)), rng.uniform(-2.4, -1.0, (B, 4))], -1)
    quat = np.concatenate([np.ones((B, 1)), rng.uniform(-0.05, 0.05, (B, 3))], 1)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    rel = er.mat_vec(er.quat_to_rot(quat)[:, None], er.fk(q, ro, rf))
    z = -rel[..., 2].min(1) + rng.uniform(0.0, 0.03, B)
    z[::3] = -rel[::3, :, 2].min(1) - 1e-6  # every third robot touches: its lowest foot starts held (1 um in)
    pos = np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), z], 1)
    return mpcqp.pack_plant_init(pos, quat, q.reshape(B, 12))


PARITY = {}


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_teacher_forced_parity(B, substeps):
    """5. 30 ticks; each tick the restatement steps from the device's own slot before that tick."""
    T = 30
    init = mixed_init(B, 100 + B)
    rng = np.random.Generator(np.random.PCG64(7 * B + substeps))
    dev = DevicePlant(mpcqp.default_plant_params(substeps=substeps), B, init)
    rp = pr.default_params(substeps=substeps)
    before = dev.get()
    worst, left_out, stance, swing, statuses = 0.0, 0, 0, 0, set()
    for t in range(T):
        tau = rng.uniform(-8.0, 8.0, (B, 12))
        ref = pr.Plant(rp, B, slot=before["slot"])
        o, wrote, margin = ref.step(DT, tau, init)
        got = dev.step(tau)
        sure = margin >= 1e-9
        left_out += int((~sure).sum())
        # discrete decisions
        assert np.array_equal(got["slot"][sure, _lib.PN_STATUS], ref.slot[sure, pr.PN_STATUS]), f"tick {t}: status"
        assert np.array_equal(got["slot"][sure, _lib.PN_CONTACT:_lib.PN_CONTACT + 4],
                              ref.slot[sure, pr.PN_CONTACT:pr.PN_CONTACT + 4]), f"tick {t}: contacts"
        # values: the robots the tick wrote, within 1e-10 max(1, |ref|); the others keep every bit
        w = wrote & sure
        pairs = [("slot", 0, ref.slot)] + [(name, off, val) for name, lst in expected_rows(o).items()
                                           for off, val in lst]
        for name, off, val in pairs:
            g = got[name][:, off:off + val.shape[1]]
            with np.errstate(invalid="ignore"):
                ratio = np.abs(g[w] - val[w]) / np.maximum(1.0, np.abs(val[w]))
            assert np.all(np.isfinite(val[w])) and np.all(np.isfinite(g[w])), f"tick {t}: {name}+{off} not finite"
            if ratio.size:
                worst = max(worst, float(ratio.max()))
            assert np.all(ratio <= 1e-10), f"tick {t}: {name}+{off} off by {ratio.max():.3e}"
        keep = ~wrote & sure
        for name in ROWS + ("slot",):
            a, b = got[name][keep].copy(), before[name][keep].copy()
            if name == "slot":
                a[:, _lib.PN_STATUS] = b[:, _lib.PN_STATUS] = 0.0  # the status alone may be written
            if name == "out":
                a[:, _lib.PT_STATUS] = b[:, _lib.PT_STATUS] = 0.0
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), f"tick {t}: {name} of an unwritten robot"
        st = got["slot"][:, _lib.PN_CONTACT:_lib.PN_CONTACT + 4] != 0.0
        stance += int(st.sum())
        swing += int((~st).sum())
        statuses |= set(got["slot"][:, _lib.PN_STATUS].tolist())
        before = got
    PARITY[(B, substeps)] = worst
    print(f"[note] plant parity B={B} substeps={substeps}: worst |dev - ref| / max(1, |ref|) = {worst:.3e}, "
          f"left out {left_out} of {B * T} robot-ticks, stance {stance} swing {swing} leg-ticks, statuses {statuses}")
    assert left_out <= 0.01 * B * T
    if B > 1:
        assert stance > 0 and swing > 0


def test_free_fall_on_the_device():
    """6a. test_plant's free fall: z = z0 - g h^2 n (n + 1) / 2 within 1e-12."""
    p = mpcqp.default_plant_params()
    init = mpcqp.pack_plant_init([[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0, 0.0]], [list(p.default_joint_pos)])
    dev = DevicePlant(p, 1, init)
    dev.step(np.zeros((1, 12)))
    h = DT / p.substeps
    worst = 0.0
    for t in range(1, 41):
        got = dev.step(np.zeros((1, 12)))
        n = t * p.substeps
        worst = max(worst, abs(got["out"][0, _lib.PT_POS + 2] - (1.0 - p.gravity * h * h * n * (n + 1) / 2.0)))
        assert not got["out"][0, _lib.PT_CONTACTS:_lib.PT_CONTACTS + 4].any() and got["out"][0, _lib.PT_STATUS] == 0.0
    print(f"[note] device free fall: max |z - closed form| {worst:.3e}")
    assert worst <= 1e-12


def test_static_equilibrium_on_the_device():
    """6b. test_plant's static equilibrium with the torques recomputed every tick from the device's rows."""
    p = mpcqp.default_plant_params()
    dev = DevicePlant(p, 1)
    got = dev.step(np.zeros((1, 12)))
    pos0 = got["out"][:, _lib.PT_POS:_lib.PT_POS + 3].copy()
    dp = dv = dw = 0.0
    for _ in range(200):
        rows = dict(root_rot_mat=got["states"][:, _lib.ST_ROT:_lib.ST_ROT + 9].reshape(1, 3, 3),
                    j_foot=got["tq"][:, _lib.TQ_JFOOT:_lib.TQ_JFOOT + 36].reshape(1, 4, 3, 3))
        got = dev.step(stance_torques(p, rows))
        o = got["out"][0]
        assert o[_lib.PT_CONTACTS:_lib.PT_CONTACTS + 4].all() and o[_lib.PT_STATUS] == 0.0
        dp = max(dp, np.abs(o[_lib.PT_POS:_lib.PT_POS + 3] - pos0).max())
        dv = max(dv, np.abs(o[_lib.PT_LIN_VEL:_lib.PT_LIN_VEL + 3]).max())
        dw = max(dw, np.abs(o[_lib.PT_ANG_VEL:_lib.PT_ANG_VEL + 3]).max())
    print(f"[note] device static equilibrium: |dpos| {dp:.3e} |v| {dv:.3e} |w| {dw:.3e}")
    assert dp <= 1e-10 and dv <= 1e-10 and dw <= 1e-9
    assert np.all(got["out"][0, _lib.PT_FOOT + 2:_lib.PT_FOOT + 12:3] == 0.0)
    np.testing.assert_allclose(got["plan_in"][0, _lib.PL_FOOT_FORCE:_lib.PL_FOOT_FORCE + 4],
                               p.mass * p.gravity / 4.0, rtol=1e-12)
    np.testing.assert_allclose(got["sensors"][0, _lib.SN_IMU_ACC:_lib.SN_IMU_ACC + 3], [0.0, 0.0, p.gravity],
                               atol=1e-9)


def _bits(d):
    return {k: v.view(np.int64).copy() for k, v in d.items()}


def test_isolation_of_bad_frozen_and_reset_robots():
    """7. B = 5: a NaN torque row, a robot out of reach, a zeroed slot, NULL outputs."""
    B, bad, far = 5, 2, 3
    p = mpcqp.default_plant_params()
    rng = np.random.Generator(np.random.PCG64(3))
    # weight-bearing torques of the default stance plus a little noise: every foot stays held
    o0 = pr.Plant(pr.default_params(), B).step(DT, np.zeros((B, 12)))[0]
    taus = stance_torques(p, o0)[None] + rng.uniform(-0.2, 0.2, (6, B, 12))
    a, c = DevicePlant(p, B), DevicePlant(p, B)
    for t in range(3):
        ga, gc = a.step(taus[t]), c.step(taus[t])
    # a NaN in robot 2's torque row: status 3 in the output row, every other double of the robot as it was
    t3 = taus[3].copy()
    t3[bad, 7] = np.nan
    ga2, gc2 = a.step(t3), c.step(taus[3])
    for name in ga:
        x, y = ga2[name][bad].copy(), ga[name][bad].copy()
        if name == "out":
            assert x[_lib.PT_STATUS] == 3.0
            x[_lib.PT_STATUS] = y[_lib.PT_STATUS]
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), name
        others = np.arange(B) != bad
        assert np.array_equal(ga2[name][others].view(np.int64), gc2[name][others].view(np.int64)), name
    assert ga2["slot"][bad, _lib.PN_STATUS] == 0.0
    ga3 = a.step(taus[4])  # the next finite row: the robot carries on
    assert ga3["out"][bad, _lib.PT_STATUS] == 0.0
    assert not np.array_equal(ga3["slot"][bad], ga2["slot"][bad])
    # a robot driven out of reach: its held feet stay while the slot's trunk is moved 1 m up
    moved = a.slot.clone()
    moved[far, _lib.PN_POS + 2] += 1.0
    a.slot.copy_(moved)
    g0 = a.get()
    g1 = a.step(taus[5])
    assert g1["slot"][far, _lib.PN_STATUS] == 1.0 and g1["out"][far, _lib.PT_STATUS] == 1.0
    status_at = dict(slot=_lib.PN_STATUS, out=_lib.PT_STATUS)
    for name in g1:  # the tick is undone: but for the two status doubles, every double as it was
        x, y = g1[name][far].copy(), g0[name][far].copy()
        if name in status_at:
            x[status_at[name]] = y[status_at[name]]
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), name
    g2 = a.step(taus[0])
    g3 = a.step(taus[1])
    for name in g1:  # frozen: not one double on later ticks
        assert np.array_equal(g2[name][far].view(np.int64), g1[name][far].view(np.int64)), name
        assert np.array_equal(g3[name][far].view(np.int64), g1[name][far].view(np.int64)), name
    assert not np.array_equal(g3["slot"][0], g1["slot"][0])  # the others moved on
    # zeroing the slot re-initialises the robot
    z = a.slot.clone()
    z[far] = 0.0
    a.slot.copy_(z)
    g4 = a.step(taus[2])
    fresh = DevicePlant(p, 1).step(np.zeros((1, 12)))
    assert g4["slot"][far, _lib.PN_STATUS] == 0.0 and g4["slot"][far, _lib.PN_INIT] == 1.0
    assert np.array_equal(g4["slot"][far].view(np.int64), fresh["slot"][0].view(np.int64))
    assert np.array_equal(g4["out"][far].view(np.int64), fresh["out"][0].view(np.int64))
    # NULL output pointers write nothing and change nothing of the slot
    n = DevicePlant(p, B, rows=())
    for t in range(3):
        gn = n.step(taus[t])
    assert set(gn) == {"slot"}
    assert np.array_equal(gn["slot"].view(np.int64), ga["slot"].view(np.int64))
