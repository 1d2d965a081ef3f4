"""The disturbance stage on the CPU: tests/disturb_reference.py (the Philox with a four-word counter, the push
windows, the noise, the phases) against known answers and its own rules, the library's defaults and
mpcqp.disturbance_of against it, and the wrench restatement against tests/plant_reference.py.  No device."""
import ctypes

import numpy as np
import pytest

import mpcqp

import disturb_reference as dr
import plant_reference as pr

DT = 0.0025


def ref_params(dp):
    """The restatement's Params of a DisturbParams."""
    return dr.Params(load_mass_max=dp.load_mass_max, gravity=dp.gravity, load_point=list(dp.load_point),
                     bias_acc=dp.bias_acc, bias_gyro=dp.bias_gyro, push_force=list(dp.push_force),
                     push_point=list(dp.push_point), sigma=list(dp.sigma), seed=dp.seed[0] | (dp.seed[1] << 32),
                     push_start=dp.push_start, push_interval=dp.push_interval, push_duration=dp.push_duration,
                     dir_count=dp.dir_count)


def everything_on(**over):
    kw = dict(load_mass_max=4.0, load_point=[0.15, 0.05, 0.03], bias_acc=0.2, bias_gyro=0.02, push_force=[20.0, 90.0],
              push_point=[0.2, 0.1, 0.05], sigma=[0.01, 0.2, 0.3, 0.05], seed=0x123456789ABCDEF, push_start=3,
              push_interval=7, push_duration=3, dir_count=8)
    kw.update(over)
    return mpcqp.default_disturb_params(**kw)


def slot_rows(phase, tick, episode):
    """Hand-made episode slot rows [B, ES_SIZE]; the unused doubles carry a fill the stage must not care about."""
    phase, tick, episode = np.broadcast_arrays(np.asarray(phase, float), np.asarray(tick, float), np.asarray(episode, float))
    es = np.full((phase.size, dr.ES_SIZE), 3.5)
    es[:, dr.ES_PHASE], es[:, dr.ES_TICK], es[:, dr.ES_EPISODE] = phase.ravel(), tick.ravel(), episode.ravel()
    return es


def wrench_rows(rng, B):
    """Random wrench rows: forces up to 30 N per axis at points up to 0.2 m off the centre; every fourth robot a
    zero row, every fourth one force only."""
    w = np.concatenate([rng.uniform(-30, 30, (B, 3)), rng.uniform(-0.2, 0.2, (B, 3)), rng.uniform(-30, 30, (B, 3)),
                        rng.uniform(-0.2, 0.2, (B, 3))], 1)
    w[1::4] = 0.0
    w[2::4, dr.PW_FORCE1:] = 0.0
    return w


def mixed_init(B, seed):
    from test_gpu_plant import mixed_init as mi
    return mi(B, seed)


# the seeds of tests/test_gpu_plant_wrench.py::test_teacher_forced_parity, per (B, substeps): (init, torques)
# (the B = 67 torque seeds were searched for: test_parity_seeds_exclude_nothing holds them to their margin)
PARITY_SEEDS = {(B, n): (100 + B, 11 * B + n) for B in (1, 5) for n in (1, 4)}
PARITY_SEEDS.update({(67, 1): (167, 253), (67, 4): (167, 236)})
PARITY_TICKS = 30


def parity_inputs(B, substeps):
    s_init, s_tau = PARITY_SEEDS[(B, substeps)]
    rng = np.random.Generator(np.random.PCG64(s_tau))
    tau = rng.uniform(-8.0, 8.0, (PARITY_TICKS, B, 12))
    wr = np.stack([wrench_rows(rng, B) for _ in range(PARITY_TICKS)])
    return mixed_init(B, s_init), tau, wr


def test_philox_known_answers_with_a_four_word_counter():
    """Philox4x32-10, the published vectors (Random123 kat_vectors), every counter word in use."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{int(w):08x}" for w in dr.philox4x32(*ctr, key)) == want
        assert " ".join(f"{w:08x}" for w in mpcqp.disturb._philox4(ctr, key)) == want
    # vectorised over a counter word = one call per element
    w = dr.philox4x32(np.arange(5), 7, 2, 9, 0xDEADBEEF12345678)
    for b in range(5):
        assert [int(x[b]) for x in w] == [int(x) for x in dr.philox4x32(b, 7, 2, 9, 0xDEADBEEF12345678)]
    # u and s stay inside their open intervals at both ends
    assert 0.0 < dr.unit(0) < dr.unit(0xFFFFFFFF) < 1.0 and -1.0 < dr.sym(0) < dr.sym(0xFFFFFFFF) < 1.0


def test_library_defaults_are_everything_off():
    d, r = mpcqp.default_disturb_params(), dr.Params()
    got = ref_params(d)
    assert got == r
    assert ctypes.sizeof(mpcqp.DisturbParams) == mpcqp.load().mpcqp_disturb_params_size()
    es = slot_rows(1.0, np.arange(6), 2)
    sn = np.random.Generator(np.random.PCG64(1)).uniform(-1, 1, (6, dr.SN_SIZE))
    sn[0, dr.SN_JOINT_POS] = -0.0
    wrench, noisy, out = dr.step(r, es, sn)
    assert not wrench.any() and not out.any() and np.array_equal(noisy.view(np.int64), sn.view(np.int64))


@pytest.mark.parametrize("interval,duration,start", [(7, 3, 3), (5, 5, 0), (4, 1, 9), (1, 1, 2)])
def test_pushes_never_overlap_and_lie_inside_their_windows(interval, duration, start):
    p = ref_params(everything_on(push_interval=interval, push_duration=duration, push_start=start))
    T = start + 12 * interval
    windows = set()
    for robot in range(4):
        for episode in range(3):
            got = dr.pushes_of(p, robot, episode, T)
            assert len(got) == 12  # one push per window, whole
            last = start
            for k, a, b in got:
                lo = start + k * interval
                assert lo <= a and b <= lo + interval and b - a == duration and a >= last
                last = b
                windows.add(a - lo)
    if duration < interval:
        assert len(windows) > 1  # the jitter moves
    else:
        assert windows == {0}


def test_noise_moments():
    """About 10^5 samples through `step`: the mean within 5 standard errors of 0 and the standard deviation within
    5 sigma / sqrt(2 n) of sigma, per group; the biases shift the IMU groups' means by what the output row says."""
    B = 3400
    p = ref_params(everything_on(bias_acc=0.0, bias_gyro=0.0))
    rng = np.random.Generator(np.random.PCG64(5))
    es = slot_rows(1.0, rng.integers(0, 2000, B), rng.integers(0, 50, B))
    wrench, noisy, out = dr.step(p, es, np.zeros((B, dr.SN_SIZE)), mpcqp.pack_push_dirs(8))
    x = noisy[:, dr.SN_JOINT_POS:dr.SN_JOINT_POS + 30]
    for (lo, hi), sigma in zip(((0, 12), (12, 24), (24, 27), (27, 30)), p.sigma):
        v = x[:, lo:hi].ravel()
        n = v.size
        print(f"[note] noise group {lo}:{hi}: n {n} mean {v.mean():.3e} std {v.std():.6e} sigma {sigma}")
        assert abs(v.mean()) <= 5.0 * sigma / np.sqrt(n)
        assert abs(v.std() - sigma) <= 5.0 * sigma / np.sqrt(2.0 * n)
    allv = (x / np.repeat(p.sigma, [12, 12, 3, 3])).ravel()
    assert allv.size >= 100000
    assert abs(allv.mean()) <= 5.0 / np.sqrt(allv.size) and abs(allv.std() - 1.0) <= 5.0 / np.sqrt(2.0 * allv.size)
    assert np.abs(allv).max() <= 2.0 * dr.SQRT3  # the Irwin-Hall sum of four is bounded
    assert not noisy[:, :dr.SN_JOINT_POS].any() and not noisy[:, dr.SN_JOINT_POS + 30:].any()
    # the 30 streams of a robot are different streams (z is a multiple of 2^-32 in (-2, 2): two of 10^5 samples may
    # coincide by chance, 30 of one robot practically never)
    assert all(len(np.unique(row / np.repeat(p.sigma, [12, 12, 3, 3]))) == 30 for row in x[:200])


def test_other_phases_get_zeros_and_a_plain_copy():
    p = ref_params(everything_on())
    B = 9
    es = slot_rows([0, 1, 2, 1, 0, 2, 1, 1, 2], 4, 1)  # tick 4: inside window 0 of every robot
    sn = np.random.Generator(np.random.PCG64(2)).uniform(-1, 1, (B, dr.SN_SIZE))
    wrench, noisy, out = dr.step(p, es, sn, mpcqp.pack_push_dirs(8))
    off = es[:, dr.ES_PHASE] != 1.0
    assert not wrench[off].any() and not out[off].any()
    assert np.array_equal(noisy[off].view(np.int64), sn[off].view(np.int64))
    on = ~off
    assert np.all(out[on, dr.DO_LOAD_FORCE] > 0) and np.all(wrench[on, dr.PW_FORCE1 + 2] < 0)
    assert np.all(noisy[on, dr.SN_JOINT_POS:dr.SN_JOINT_POS + 30] != sn[on, dr.SN_JOINT_POS:dr.SN_JOINT_POS + 30])
    # the quaternion and the pad are copied for everybody
    for sl in (slice(0, dr.SN_JOINT_POS), slice(dr.SN_JOINT_POS + 30, dr.SN_SIZE)):
        assert np.array_equal(noisy[:, sl].view(np.int64), sn[:, sl].view(np.int64))


def test_disturbance_of_is_the_per_tick_restatement():
    dp = everything_on()
    dirs = mpcqp.pack_push_dirs(dp.dir_count)
    p = ref_params(dp)
    T = 40
    for robot, episode in ((0, 0), (3, 2), (66, 5)):
        d = mpcqp.disturbance_of(dp, dirs, robot, episode, T)
        rows = [dr.step_one(p, slot_rows(1.0, t, episode), robot, dirs) for t in range(T)]
        wr = []
        for t in range(T):
            es = np.zeros((robot + 1, dr.ES_SIZE))
            es[robot] = slot_rows(1.0, t, episode)
            wr.append(dr.step(p, es, None, dirs)[0][robot])
        assert d["load_force"] == rows[0][dr.DO_LOAD_FORCE]
        assert np.array_equal(d["load_point"], rows[0][dr.DO_LOAD_POINT:dr.DO_LOAD_POINT + 3])
        assert np.array_equal(d["bias_acc"], rows[0][dr.DO_BIAS_ACC:dr.DO_BIAS_ACC + 3])
        assert np.array_equal(d["bias_gyro"], rows[0][dr.DO_BIAS_GYRO:dr.DO_BIAS_GYRO + 3])
        active = np.zeros(T, dtype=bool)
        for push in d["pushes"]:
            assert not active[push["start"]:push["stop"]].any()
            active[push["start"]:push["stop"]] = True
            for t in range(push["start"], push["stop"]):
                assert rows[t][dr.DO_PUSH_WINDOW] == push["window"] and rows[t][dr.DO_PUSH_FORCE] == push["force"]
                assert rows[t][dr.DO_PUSH_DIR] == push["dir"]
                assert np.array_equal(rows[t][dr.DO_PUSH_POINT:dr.DO_PUSH_POINT + 3], push["point"])
                assert np.array_equal(wr[t][dr.PW_FORCE0:dr.PW_FORCE0 + 3], push["vector"])
                assert np.array_equal(wr[t][dr.PW_POINT0:dr.PW_POINT0 + 3], push["point"])
        assert np.array_equal(active, np.array([r[dr.DO_PUSH_ACTIVE] for r in rows]) != 0.0)
        assert active.any() and not active.all()
    assert mpcqp.disturbance_of(mpcqp.default_disturb_params(), None, 1, 1, 10)["pushes"] == []


def test_push_dirs_are_horizontal_unit_vectors():
    for n in (1, 4, 7):
        d = mpcqp.pack_push_dirs(n)
        assert d.shape == (n, 4) and not d[:, 2:].any()
        np.testing.assert_allclose(np.hypot(d[:, 0], d[:, 1]), 1.0, rtol=1e-15)
    assert np.array_equal(mpcqp.pack_push_dirs(1)[0], [1.0, 0.0, 0.0, 0.0])
    np.testing.assert_allclose(mpcqp.pack_push_dirs(4)[:, :2], [[1, 0], [0, 1], [-1, 0], [0, -1]], atol=1e-15)


@pytest.mark.parametrize("substeps", [1, 4])
def test_wrench_restatement_with_a_zero_row_is_plant_reference(substeps):
    B, T = 12, 12
    init = mixed_init(B, 31)
    rng = np.random.Generator(np.random.PCG64(8))
    p = pr.default_params(substeps=substeps)
    a, b, c = pr.Plant(p, B), dr.WrenchPlant(p, B), dr.WrenchPlant(p, B)
    moved = False
    for t in range(T):
        tau = rng.uniform(-8.0, 8.0, (B, 12))
        oa, wa, ma = a.step(DT, tau, init)
        ob, wb, mb = b.step(DT, tau, init, wrench=np.zeros((B, dr.PW_SIZE)))
        oc, wc, mc = c.step(DT, tau, init, wrench=wrench_rows(rng, B))
        assert np.array_equal(a.slot.view(np.int64), b.slot.view(np.int64)), f"tick {t}"
        assert np.array_equal(wa, wb) and np.array_equal(ma, mb)
        for k in oa:
            x, y = np.asarray(oa[k], dtype=np.float64), np.asarray(ob[k], dtype=np.float64)
            assert np.array_equal(x.view(np.int64), y.view(np.int64)), f"tick {t}: {k}"
        moved = moved or not np.array_equal(a.slot[::4], c.slot[::4])
        assert np.array_equal(a.slot[1::4].view(np.int64), c.slot[1::4].view(np.int64))  # their rows are zero
    assert moved


def test_zero_wrench_keeps_a_negative_zero():
    """A robot standing under zero torques: its legs' forces sum to exactly -0.0 sideways.  A zero wrench row
    leaves that bit (the terms are skipped, not added)."""
    p = pr.default_params()
    a, b = pr.Plant(p, 2), dr.WrenchPlant(p, 2)
    seen = False
    for t in range(4):
        oa = a.step(DT, np.zeros((2, 12)))[0]
        ob = b.step(DT, np.zeros((2, 12)), wrench=np.zeros((2, dr.PW_SIZE)))[0]
        assert np.array_equal(a.slot.view(np.int64), b.slot.view(np.int64)), f"tick {t}"
        assert np.array_equal(oa["acc"].view(np.int64), ob["acc"].view(np.int64))
        seen = seen or bool(np.any(np.signbit(oa["acc"]) & (oa["acc"] == 0.0)))
    assert seen  # the case is there


def test_wrench_restatement_closed_forms():
    """Free fall under a constant force at the centre of mass: v = (F / m - g) T; a force at an offset point on a
    free trunk at rest: wd = I^-1 (p x R'F) on the first substep."""
    p = pr.default_params()
    init = mpcqp.pack_plant_init([[0.0, 0.0, 5.0]], [[1.0, 0.0, 0.0, 0.0]], [p.default_joint_pos])
    plant = dr.WrenchPlant(p, 1)
    plant.step(DT, np.zeros((1, 12)), init, wrench=np.zeros((1, dr.PW_SIZE)))
    F = np.array([13.0, -6.5, 26.0])
    w = np.zeros((1, dr.PW_SIZE))
    w[0, dr.PW_FORCE0:dr.PW_FORCE0 + 3] = F
    T = 40
    for _ in range(T):
        o = plant.step(DT, np.zeros((1, 12)), init, wrench=w)[0]
    want = (F / p.mass - np.array([0.0, 0.0, p.gravity])) * (T * DT)
    np.testing.assert_allclose(o["root_lin_vel"][0], want, rtol=1e-12)
    assert not o["imu_ang_vel"].any()
    q = dr.WrenchPlant(pr.default_params(substeps=1), 1)
    q.step(DT, np.zeros((1, 12)), init, wrench=np.zeros((1, dr.PW_SIZE)))
    w[0, dr.PW_POINT0:dr.PW_POINT0 + 3] = [0.2, -0.1, 0.05]
    o = q.step(DT, np.zeros((1, 12)), init, wrench=w)[0]
    wd = np.cross([0.2, -0.1, 0.05], F) / np.array(p.inertia).reshape(3, 3).diagonal()
    np.testing.assert_allclose(o["imu_ang_vel"][0], wd * DT, rtol=1e-12)


@pytest.mark.parametrize("B,substeps", sorted(PARITY_SEEDS))
def test_parity_seeds_exclude_nothing(B, substeps):
    """The inputs of the device's teacher-forced parity test: the restatement alone meets no decision margin under
    1e-7 on them, a hundred times the 1e-9 under which a robot-tick would be left out, so none is."""
    init, tau, wr = parity_inputs(B, substeps)
    plant = dr.WrenchPlant(pr.default_params(substeps=substeps), B)
    worst, stance, swing = np.inf, 0, 0
    for t in range(PARITY_TICKS):
        o, wrote, margin = plant.step(DT, tau[t], init, wrench=wr[t])
        worst = min(worst, float(margin.min()))
        stance += int(o["contacts"].sum())
        swing += int((~o["contacts"]).sum())
    print(f"[note] B={B} substeps={substeps}: smallest margin {worst:.3e}, stance {stance} swing {swing}")
    assert worst >= 1e-7
    if B > 1:
        assert stance > 0 and swing > 0
