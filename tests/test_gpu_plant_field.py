"""The plant stage on a bilinear height field (mpcqp_plant_step_field_device) against tests/field_reference.py:
teacher-forced parity as tests/test_gpu_plant_terrain.py::test_teacher_forced_parity, the NULL field against the wrench
and the plain entry, a planar tile against the device's own plane entry, and each kind of bad header row.  The heights
always stand in the middle of a larger NaN-filled buffer, so a read outside them would show."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib

import field_reference as fr
import plant_reference as pr
import terrain_reference as tr
import test_terrain as tt
from test_disturb import DT, mixed_init, wrench_rows
from test_field import PARITY_TICKS, parity_inputs, planar_tiles, shuffled_pool
from test_gpu_plant import ROWS, DevicePlant, expected_rows
from test_gpu_plant_terrain import DeviceTerrainPlant
from test_gpu_plant_wrench import DeviceWrenchPlant

pytestmark = pytest.mark.gpu

GUARD = 32


class DeviceFieldPlant(DevicePlant):
    """DevicePlant through the field entry point; ``wrench=None`` / ``field=None`` / ``es=None`` pass NULL.  The
    heights are a slice of a NaN-filled buffer with GUARD doubles on either side."""

    def __init__(self, p, B, init=None, field=None, es=None):
        super().__init__(p, B, init)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()  # noqa: E731
        self.field, self.heights, self.es = None, None, up(es)
        if field is not None:
            self.field = up(field[0])
            n = len(field[1])
            self.guard = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
            self.heights = self.guard[GUARD:GUARD + n]
            self.heights.copy_(up(field[1]))

    def step(self, tau, wrench=None):
        self.torques.copy_(torch.from_numpy(np.ascontiguousarray(tau, dtype=np.float64).reshape(self.B, 12)))
        w = None if wrench is None else torch.from_numpy(np.ascontiguousarray(wrench, dtype=np.float64)).cuda()
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        mpcqp.plant_step_field_device(
            self.p, DT, self.torques.data_ptr(), ptr(w), ptr(self.field),
            0 if self.field is None else self.field.shape[0], ptr(self.heights),
            0 if self.heights is None else self.heights.numel(), ptr(self.es), self.B, self.slot.data_ptr(),
            ptr(self.init), ptr(self.sensors), ptr(self.plan_in), ptr(self.states), ptr(self.tq), ptr(self.out),
            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return self.get()


@pytest.mark.parametrize("B,substeps,pool", [(B, n, False) for B in (1, 5, 67) for n in (1, 4)] + [(67, 4, True)])
def test_teacher_forced_parity(B, substeps, pool):
    """30 ticks of random torques, random wrench rows (zero rows and NULL pointers among them) on four tiles of unequal
    sizes in one array; each tick the restatement steps from the device's own slot before that tick.
    |device - ref| / max(1, |ref|) <= 1e-10; a robot-tick with a decision margin under 1e-9 would be left out, and on
    these inputs (tests/test_field.py checks them on the CPU) none is.  ``pool``: the rows are chosen through a
    hand-made episode slot with a shuffled MPCQP_ES_POOL."""
    init, taus, wrs, rows, heights = parity_inputs(B, substeps)
    es, table = shuffled_pool(B, rows) if pool else (None, rows)
    dev = DeviceFieldPlant(mpcqp.default_plant_params(substeps=substeps), B, init, (table, heights), es)
    rp = pr.default_params(substeps=substeps)
    before = dev.get()
    worst, left_out, stance, swing, least = 0.0, 0, 0, 0, np.inf
    for t in range(PARITY_TICKS):
        ref = fr.FieldPlant(rp, B, slot=before["slot"])
        o, wrote, margin = ref.step(DT, taus[t], init, wrench=wrs[t], field=(table, heights), episode_state=es)
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
    print(f"[note] field plant parity B={B} substeps={substeps} pool={pool}: worst |dev - ref| / max(1, |ref|) = "
          f"{worst:.3e}, left out {left_out} of {B * PARITY_TICKS} robot-ticks (smallest margin {least:.3e}), stance "
          f"{stance} swing {swing} leg-ticks")
    assert left_out == 0
    if B > 1:
        assert stance > 0 and swing > 0


@pytest.mark.parametrize("B", [1, 5, 67])
def test_null_field_is_the_wrench_and_the_plain_entry(B):
    init = mixed_init(B, 40 + B)
    rng = np.random.Generator(np.random.PCG64(B))
    p = mpcqp.default_plant_params()
    old, wr, a, b = DevicePlant(p, B, init), DeviceWrenchPlant(p, B, init), DeviceFieldPlant(p, B, init), \
        DeviceFieldPlant(p, B, init)
    for t in range(12):
        tau, w = rng.uniform(-8.0, 8.0, (B, 12)), wrench_rows(rng, B)
        plain, null = old.step(tau), a.step(tau, None)
        pushed, same = wr.step(tau, w), b.step(tau, w)
        for name in plain:
            assert np.array_equal(plain[name].view(np.int64), null[name].view(np.int64)), f"tick {t}: {name}, plain"
            assert np.array_equal(pushed[name].view(np.int64), same[name].view(np.int64)), f"tick {t}: {name}, wrench"


@pytest.mark.parametrize("substeps", [1, 4])
def test_planar_tile_is_the_plane_entry(substeps):
    """A tile sampled from each robot's plane against mpcqp_plant_step_terrain_device on that plane, teacher-forced on
    the terrain parity test's inputs (each tick both start from the plane entry's slot): equal statuses and contacts,
    every written double within 1e-12."""
    B = 67
    init, taus, wrs, terrain = tt.parity_inputs(B, substeps)
    rows, heights = planar_tiles(terrain, init[:, :2])
    p = mpcqp.default_plant_params(substeps=substeps)
    a, b = DeviceTerrainPlant(p, B, init, terrain), DeviceFieldPlant(p, B, init, (rows, heights))
    worst = 0.0
    for t in range(tt.PARITY_TICKS):
        for name in ROWS + ("slot",):
            getattr(b, name).copy_(getattr(a, name))
        ga, gb = a.step(taus[t], wrs[t]), b.step(taus[t], wrs[t])
        assert np.array_equal(ga["slot"][:, _lib.PN_STATUS], gb["slot"][:, _lib.PN_STATUS]), f"tick {t}: status"
        assert np.array_equal(ga["out"][:, _lib.PT_STATUS], gb["out"][:, _lib.PT_STATUS]), f"tick {t}: status row"
        assert np.array_equal(ga["slot"][:, _lib.PN_CONTACT:_lib.PN_CONTACT + 4],
                              gb["slot"][:, _lib.PN_CONTACT:_lib.PN_CONTACT + 4]), f"tick {t}: contacts"
        for name in ga:
            ratio = np.abs(gb[name] - ga[name]) / np.maximum(1.0, np.abs(ga[name]))
            worst = max(worst, float(ratio.max()))
            assert np.all(ratio <= 1e-12), f"tick {t}: {name} off by {ratio.max():.3e}"
    print(f"[note] planar tile against the plane entry, substeps {substeps}: worst difference {worst:.3e}")


@pytest.mark.parametrize("how", ["nan", "nx1", "overrun", "index_below", "index_at_rows"])
def test_a_bad_header_row_is_a_bad_torque_row(how):
    """A NaN header entry, nx = 1, OFFSET + nx ny = heights_len + 1, or a pool index of -1 or field_rows: 3.0 in
    MPCQP_PT_STATUS, every other double of the robot bitwise what it was, and its neighbours in the quad and the wave
    bitwise those of a fleet whose rows are all fine.  Then the robot carries on at the next good row.  The header
    table, too, stands in the middle of a larger NaN-filled buffer."""
    B, bad = 5, 2
    init, taus, wrs, rows, heights = parity_inputs(B, 4)
    rng = np.random.Generator(np.random.PCG64(4))
    p = mpcqp.default_plant_params()
    guard = torch.full((B + 4, fr.HF_SIZE), float("nan"), dtype=torch.float64, device="cuda")
    es = np.full((B, tr.ES_SIZE), 3.5)
    es[:, tr.ES_POOL] = np.arange(B)
    a, c = DeviceFieldPlant(p, B, init, (rows, heights), es), DeviceFieldPlant(p, B, init, (rows, heights), es)
    guard[2:2 + B].copy_(a.field)
    a.field = guard[2:2 + B]
    for t in range(3):
        tau, w = rng.uniform(-8.0, 8.0, (B, 12)), wrench_rows(rng, B)
        ga, gc = a.step(tau, w), c.step(tau, w)
    for name in ga:
        assert np.array_equal(ga[name].view(np.int64), gc[name].view(np.int64)), name
    if how == "nan":
        a.field[bad, fr.HF_Y0] = float("nan")
    elif how == "nx1":
        a.field[bad, fr.HF_NX] = 1.0
    elif how == "overrun":
        a.field[bad, fr.HF_OFFSET] = float(len(heights) + 1 - int(rows[bad, fr.HF_NX] * rows[bad, fr.HF_NY]))
    else:
        a.es[bad, tr.ES_POOL] = -1.0 if how == "index_below" else float(B)
    tau, w = rng.uniform(-8.0, 8.0, (B, 12)), wrench_rows(rng, B)
    ga2, gc2 = a.step(tau, w), c.step(tau, w)
    others = np.arange(B) != bad
    for name in ga:
        x, y = ga2[name][bad].copy(), ga[name][bad].copy()
        if name == "out":
            assert x[_lib.PT_STATUS] == 3.0
            x[_lib.PT_STATUS] = y[_lib.PT_STATUS]
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), name
        assert np.array_equal(ga2[name][others].view(np.int64), gc2[name][others].view(np.int64)), name
    assert ga2["slot"][bad, _lib.PN_STATUS] == 0.0
    # the next good row: the robot carries on from where it stood
    a.field.copy_(c.field)
    a.es.copy_(c.es)
    tau, w = rng.uniform(-8.0, 8.0, (B, 12)), wrench_rows(rng, B)
    ga3 = a.step(tau, w)
    assert ga3["out"][bad, _lib.PT_STATUS] == 0.0 and not np.array_equal(ga3["slot"][bad], ga2["slot"][bad])
