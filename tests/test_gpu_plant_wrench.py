"""The plant stage with external forces (mpcqp_plant_step_wrench_device) against the wrench restatement of
tests/disturb_reference.py: teacher-forced parity as tests/test_gpu_plant.py::test_teacher_forced_parity, the NULL
and the all-zero wrench against mpcqp_plant_step_device, two closed forms, and a non-finite wrench row."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib

import disturb_reference as dr
import plant_reference as pr
from test_disturb import DT, PARITY_TICKS, mixed_init, parity_inputs, wrench_rows
from test_gpu_plant import ROWS, DevicePlant, expected_rows

pytestmark = pytest.mark.gpu


class DeviceWrenchPlant(DevicePlant):
    """DevicePlant through the wrench entry point; ``wrench=None`` passes a NULL row."""

    def step(self, tau, wrench=None):
        self.torques.copy_(torch.from_numpy(np.ascontiguousarray(tau, dtype=np.float64).reshape(self.B, 12)))
        w = None if wrench is None else torch.from_numpy(np.ascontiguousarray(wrench, dtype=np.float64)).cuda()
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        mpcqp.plant_step_wrench_device(self.p, DT, self.torques.data_ptr(), ptr(w), self.B, self.slot.data_ptr(),
                                       ptr(self.init), ptr(self.sensors), ptr(self.plan_in), ptr(self.states),
                                       ptr(self.tq), ptr(self.out), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return self.get()


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_teacher_forced_parity(B, substeps):
    """30 ticks of random torques and random wrench rows (zero rows among them); each tick the restatement steps
    from the device's own slot before that tick.  |device - ref| / max(1, |ref|) <= 1e-10; a robot-tick with a
    decision margin under 1e-9 would be left out, and on these inputs (tests/test_disturb.py checks them on the
    CPU) none is."""
    init, taus, wrs = parity_inputs(B, substeps)
    dev = DeviceWrenchPlant(mpcqp.default_plant_params(substeps=substeps), B, init)
    rp = pr.default_params(substeps=substeps)
    before = dev.get()
    worst, left_out, stance, swing, least = 0.0, 0, 0, 0, np.inf
    for t in range(PARITY_TICKS):
        ref = dr.WrenchPlant(rp, B, slot=before["slot"])
        o, wrote, margin = ref.step(DT, taus[t], init, wrench=wrs[t])
        got = dev.step(taus[t], wrs[t])
        sure = margin >= 1e-9
        left_out += int((~sure).sum())
        least = min(least, float(margin.min()))
        assert np.array_equal(got["slot"][sure, _lib.PN_STATUS], ref.slot[sure, pr.PN_STATUS]), f"tick {t}: status"
        assert np.array_equal(got["slot"][sure, _lib.PN_CONTACT:_lib.PN_CONTACT + 4],
                              ref.slot[sure, pr.PN_CONTACT:pr.PN_CONTACT + 4]), f"tick {t}: contacts"
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
                a[:, _lib.PN_STATUS] = b[:, _lib.PN_STATUS] = 0.0
            if name == "out":
                a[:, _lib.PT_STATUS] = b[:, _lib.PT_STATUS] = 0.0
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), f"tick {t}: {name} of an unwritten robot"
        st = got["slot"][:, _lib.PN_CONTACT:_lib.PN_CONTACT + 4] != 0.0
        stance += int(st.sum())
        swing += int((~st).sum())
        before = got
    print(f"[note] wrench plant parity B={B} substeps={substeps}: worst |dev - ref| / max(1, |ref|) = {worst:.3e}, "
          f"left out {left_out} of {B * PARITY_TICKS} robot-ticks (smallest margin {least:.3e}), stance {stance} "
          f"swing {swing} leg-ticks")
    assert left_out == 0
    if B > 1:
        assert stance > 0 and swing > 0


@pytest.mark.parametrize("B", [1, 5, 67])
def test_null_and_zero_wrench_are_the_old_entry_point(B):
    init = mixed_init(B, 40 + B)
    rng = np.random.Generator(np.random.PCG64(B))
    p = mpcqp.default_plant_params()
    old, null, zero = DevicePlant(p, B, init), DeviceWrenchPlant(p, B, init), DeviceWrenchPlant(p, B, init)
    for t in range(12):
        tau = rng.uniform(-8.0, 8.0, (B, 12))
        a, b, c = old.step(tau), null.step(tau, None), zero.step(tau, np.zeros((B, dr.PW_SIZE)))
        for name in a:
            assert np.array_equal(a[name].view(np.int64), b[name].view(np.int64)), f"tick {t}: {name}, NULL wrench"
            assert np.array_equal(a[name].view(np.int64), c[name].view(np.int64)), f"tick {t}: {name}, zero wrench"
    # robots standing under zero torques: their legs' forces sum to exactly -0.0 sideways, which a zero row keeps
    old, zero = DevicePlant(p, B), DeviceWrenchPlant(p, B)
    for t in range(4):
        a, c = old.step(np.zeros((B, 12))), zero.step(np.zeros((B, 12)), np.zeros((B, dr.PW_SIZE)))
        for name in a:
            assert np.array_equal(a[name].view(np.int64), c[name].view(np.int64)), f"standing, tick {t}: {name}"


def _falling(p):
    init = mpcqp.pack_plant_init([[0.0, 0.0, 5.0]], [[1.0, 0.0, 0.0, 0.0]], [list(p.default_joint_pos)])
    dev = DeviceWrenchPlant(p, 1, init)
    ref = dr.WrenchPlant(pr.default_params(substeps=p.substeps), 1)
    dev.step(np.zeros((1, 12)), np.zeros((1, dr.PW_SIZE)))
    ref.step(DT, np.zeros((1, 12)), init, wrench=np.zeros((1, dr.PW_SIZE)))
    return dev, ref, init


def test_free_fall_under_a_constant_force():
    """A force at the centre of mass of a falling trunk: the velocity is exactly the restatement's, and within
    1e-12 relative of (F / m - g) T."""
    p = mpcqp.default_plant_params()
    dev, ref, init = _falling(p)
    F = np.array([13.0, -6.5, 26.0])
    w = np.zeros((1, dr.PW_SIZE))
    w[0, dr.PW_FORCE0:dr.PW_FORCE0 + 3] = F
    T = 40
    for _ in range(T):
        got = dev.step(np.zeros((1, 12)), w)
        o = ref.step(DT, np.zeros((1, 12)), init, wrench=w)[0]
    v = got["out"][0, _lib.PT_LIN_VEL:_lib.PT_LIN_VEL + 3]
    assert np.array_equal(v.view(np.int64), o["root_lin_vel"][0].view(np.int64))
    want = (F / p.mass - np.array([0.0, 0.0, p.gravity])) * (T * DT)
    rel = np.abs(v - want) / np.abs(want)
    print(f"[note] free fall under a force: |v - (F/m - g) T| / |.| = {rel.tolist()}")
    assert np.all(rel <= 1e-12)
    assert not got["out"][0, _lib.PT_ANG_VEL:_lib.PT_ANG_VEL + 3].any()
    assert not got["out"][0, _lib.PT_CONTACTS:_lib.PT_CONTACTS + 4].any()


def test_offset_force_turns_a_free_trunk():
    """A force at an offset point on a free trunk at rest: w = h I^-1 (p x R'F) after the first substep."""
    p = mpcqp.default_plant_params(substeps=1)
    dev, ref, init = _falling(p)
    F, pt = np.array([13.0, -6.5, 26.0]), np.array([0.2, -0.1, 0.05])
    w = np.zeros((1, dr.PW_SIZE))
    w[0, dr.PW_FORCE1:dr.PW_FORCE1 + 3], w[0, dr.PW_POINT1:dr.PW_POINT1 + 3] = F, pt
    got = dev.step(np.zeros((1, 12)), w)
    o = ref.step(DT, np.zeros((1, 12)), init, wrench=w)[0]
    wd = np.cross(pt, F) / np.array(list(p.inertia)).reshape(3, 3).diagonal()
    av = got["out"][0, _lib.PT_ANG_VEL:_lib.PT_ANG_VEL + 3]
    assert np.array_equal(av.view(np.int64), o["imu_ang_vel"][0].view(np.int64))
    np.testing.assert_allclose(av, wd * DT, rtol=1e-12)


def test_a_non_finite_wrench_row_is_a_bad_torque_row():
    B, bad = 5, 2
    init = mixed_init(B, 9)
    rng = np.random.Generator(np.random.PCG64(4))
    p = mpcqp.default_plant_params()
    a, c = DeviceWrenchPlant(p, B, init), DeviceWrenchPlant(p, B, init)
    for t in range(3):
        tau, w = rng.uniform(-8.0, 8.0, (B, 12)), wrench_rows(rng, B)
        ga, gc = a.step(tau, w), c.step(tau, w)
    for at, value in ((dr.PW_POINT1 + 1, np.nan), (dr.PW_FORCE0, np.inf)):
        tau, w = rng.uniform(-8.0, 8.0, (B, 12)), wrench_rows(rng, B)
        wb = w.copy()
        wb[bad, at] = value
        ga2, gc2 = a.step(tau, wb), c.step(tau, w)
        for name in ga:
            x, y = ga2[name][bad].copy(), ga[name][bad].copy()
            if name == "out":
                assert x[_lib.PT_STATUS] == 3.0
                x[_lib.PT_STATUS] = y[_lib.PT_STATUS]
            assert np.array_equal(x.view(np.int64), y.view(np.int64)), name
            others = np.arange(B) != bad
            assert np.array_equal(ga2[name][others].view(np.int64), gc2[name][others].view(np.int64)), name
        assert ga2["slot"][bad, _lib.PN_STATUS] == 0.0
        # the next finite row: the robot carries on from where it stood
        c.slot.copy_(a.slot)
        for name in ROWS:
            getattr(c, name).copy_(getattr(a, name))
        tau, w = rng.uniform(-8.0, 8.0, (B, 12)), wrench_rows(rng, B)
        ga, gc = a.step(tau, w), c.step(tau, w)
        assert ga["out"][bad, _lib.PT_STATUS] == 0.0 and not np.array_equal(ga["slot"][bad], ga2["slot"][bad])
