"""The plant stage on inclined ground (mpcqp_plant_step_terrain_device) against tests/terrain_reference.py:
teacher-forced parity as tests/test_gpu_plant_wrench.py::test_teacher_forced_parity, the NULL table against the wrench
and the plain entry, and a non-finite row or a pool index outside the table."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib

import plant_reference as pr
import terrain_reference as tr
from test_disturb import DT, mixed_init, wrench_rows
from test_gpu_plant import ROWS, DevicePlant, expected_rows
from test_gpu_plant_wrench import DeviceWrenchPlant
from test_terrain import PARITY_TICKS, parity_inputs, shuffled_pool, terrain_rows

pytestmark = pytest.mark.gpu


class DeviceTerrainPlant(DevicePlant):
    """DevicePlant through the terrain entry point; ``wrench=None`` / ``terrain=None`` / ``es=None`` pass NULL."""

    def __init__(self, p, B, init=None, terrain=None, es=None):
        super().__init__(p, B, init)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()  # noqa: E731
        self.terrain, self.es = up(terrain), up(es)

    def step(self, tau, wrench=None):
        self.torques.copy_(torch.from_numpy(np.ascontiguousarray(tau, dtype=np.float64).reshape(self.B, 12)))
        w = None if wrench is None else torch.from_numpy(np.ascontiguousarray(wrench, dtype=np.float64)).cuda()
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        mpcqp.plant_step_terrain_device(
            self.p, DT, self.torques.data_ptr(), ptr(w), ptr(self.terrain),
            0 if self.terrain is None else self.terrain.shape[0], ptr(self.es), self.B, self.slot.data_ptr(),
            ptr(self.init), ptr(self.sensors), ptr(self.plan_in), ptr(self.states), ptr(self.tq), ptr(self.out),
            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return self.get()


@pytest.mark.parametrize("B,substeps,pool", [(B, n, False) for B in (1, 5, 67) for n in (1, 4)] + [(67, 4, True)])
def test_teacher_forced_parity(B, substeps, pool):
    """30 ticks of random torques, random wrench rows (zero rows and NULL pointers among them) and random terrain
    rows (level ones among them); each tick the restatement steps from the device's own slot before that tick.
    |device - ref| / max(1, |ref|) <= 1e-10; a robot-tick with a decision margin under 1e-9 would be left out, and on
    these inputs (tests/test_terrain.py checks them on the CPU) none is.  ``pool``: the rows are chosen through a
    hand-made episode slot with a shuffled MPCQP_ES_POOL."""
    init, taus, wrs, terrain = parity_inputs(B, substeps)
    es, table = shuffled_pool(B, terrain) if pool else (None, terrain)
    dev = DeviceTerrainPlant(mpcqp.default_plant_params(substeps=substeps), B, init, table, es)
    rp = pr.default_params(substeps=substeps)
    before = dev.get()
    worst, left_out, stance, swing, least = 0.0, 0, 0, 0, np.inf
    for t in range(PARITY_TICKS):
        ref = tr.TerrainPlant(rp, B, slot=before["slot"])
        o, wrote, margin = ref.step(DT, taus[t], init, wrench=wrs[t], terrain=table, episode_state=es)
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
    print(f"[note] terrain plant parity B={B} substeps={substeps} pool={pool}: worst |dev - ref| / max(1, |ref|) = "
          f"{worst:.3e}, left out {left_out} of {B * PARITY_TICKS} robot-ticks (smallest margin {least:.3e}), stance "
          f"{stance} swing {swing} leg-ticks")
    assert left_out == 0
    if B > 1:
        assert stance > 0 and swing > 0


@pytest.mark.parametrize("B", [1, 5, 67])
def test_null_terrain_is_the_wrench_and_the_plain_entry(B):
    init = mixed_init(B, 40 + B)
    rng = np.random.Generator(np.random.PCG64(B))
    p = mpcqp.default_plant_params()
    old, wr, a, b = DevicePlant(p, B, init), DeviceWrenchPlant(p, B, init), DeviceTerrainPlant(p, B, init), \
        DeviceTerrainPlant(p, B, init)
    for t in range(12):
        tau, w = rng.uniform(-8.0, 8.0, (B, 12)), wrench_rows(rng, B)
        plain, null = old.step(tau), a.step(tau, None)
        pushed, same = wr.step(tau, w), b.step(tau, w)
        for name in plain:
            assert np.array_equal(plain[name].view(np.int64), null[name].view(np.int64)), f"tick {t}: {name}, plain"
            assert np.array_equal(pushed[name].view(np.int64), same[name].view(np.int64)), f"tick {t}: {name}, wrench"


@pytest.mark.parametrize("how", ["nan", "inf_mu", "index_below", "index_at_rows"])
def test_a_bad_terrain_row_is_a_bad_torque_row(how):
    """A non-finite terrain row, or a pool index of -1 or terrain_rows: 3.0 in MPCQP_PT_STATUS, every other double of
    the robot bitwise what it was, and its neighbours in the quad and the wave bitwise those of a fleet whose rows are
    all fine.  The table stands in the middle of a larger NaN-filled buffer, so a read outside it would show."""
    B, bad = 5, 2
    init = mixed_init(B, 9)
    rng = np.random.Generator(np.random.PCG64(4))
    p = mpcqp.default_plant_params()
    terrain = terrain_rows(rng, B)
    init, _ = mpcqp.place_on_terrain(init, terrain, lower=False)
    guard = torch.full((B + 4, tr.TR_SIZE), float("nan"), dtype=torch.float64, device="cuda")
    es = np.full((B, tr.ES_SIZE), 3.5)
    es[:, tr.ES_POOL] = np.arange(B)
    a, c = DeviceTerrainPlant(p, B, init, terrain, es), DeviceTerrainPlant(p, B, init, terrain, es)
    guard[2:2 + B].copy_(a.terrain)
    a.terrain = guard[2:2 + B]
    for t in range(3):
        tau, w = rng.uniform(-8.0, 8.0, (B, 12)), wrench_rows(rng, B)
        ga, gc = a.step(tau, w), c.step(tau, w)
    for name in ga:
        assert np.array_equal(ga[name].view(np.int64), gc[name].view(np.int64)), name
    if how == "nan":
        a.terrain[bad, tr.TR_NORMAL + 1] = float("nan")
    elif how == "inf_mu":
        a.terrain[bad, tr.TR_MU] = float("inf")
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
    a.terrain.copy_(c.terrain)
    a.es.copy_(c.es)
    tau, w = rng.uniform(-8.0, 8.0, (B, 12)), wrench_rows(rng, B)
    ga3 = a.step(tau, w)
    assert ga3["out"][bad, _lib.PT_STATUS] == 0.0 and not np.array_equal(ga3["slot"][bad], ga2["slot"][bad])
