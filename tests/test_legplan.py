"""Leg plan without a GPU: the C ABI's defaults and slot size, the Python packers, and self-checks of
the numpy restatement (tests/legplan_reference.py) that the GPU tests compare the kernel with."""
import ctypes

import numpy as np

import mpcqp
from mpcqp import _lib, legplan

import legplan_reference as ref

EPS = np.finfo(np.float64).eps


def _walk_inputs(B, rng=None, mode=1):
    """A level robot walking forward: the arguments of LegPlan.step after dt."""
    eye = np.broadcast_to(np.eye(3), (B, 3, 3)).copy()
    feet = np.broadcast_to(mpcqp.records.GO1_DEFAULT_FOOT_POS, (B, 4, 3)).copy()
    if rng is not None:
        feet += rng.uniform(-0.02, 0.02, feet.shape)
    return dict(root_lin_vel=np.tile([0.3, 0.0, 0.0], (B, 1)), root_lin_vel_d=np.tile([0.4, 0.1, 0.0], (B, 1)),
                root_rot_mat=eye, root_pos=np.tile([0.0, 0.0, 0.3], (B, 1)), foot_pos_abs=feet,
                root_euler_d=np.zeros((B, 3)), rot_z=eye, foot_force=np.zeros((B, 4)),
                movement_mode=np.full(B, mode))


def test_default_params_are_the_reference_constants():
    p = mpcqp.default_plan_params()
    # A1CtrlStates.h:45-47 (matlab-style 3x4, stored leg-major here)
    assert np.array_equal(np.array(p.default_foot_pos).reshape(4, 3),
                          [[0.17, 0.15, -0.35], [0.17, -0.15, -0.35], [-0.17, 0.15, -0.35], [-0.17, -0.15, -0.35]])
    assert list(p.kp_foot) == [300.0, 400.0, 400.0] * 4 and list(p.kd_foot) == [8.0] * 12  # :105-120
    assert list(p.gait_counter_speed) == [2.0] * 4                                             # :103
    assert list(p.gait_counter_init) == [0.0, 120.0, 120.0, 0.0]                               # :325
    assert (p.counter_per_gait, p.counter_per_swing) == (240.0, 120.0)                         # :24-25
    assert p.control_dt == 0.5 / 1000.0                                                        # :333
    assert (p.foot_force_low, p.foot_delta_x_limit, p.foot_delta_y_limit) == (30.0, 0.1, 0.1)  # A1Params.h:38-45
    assert p.swing_clearance1 == 0.0 and p.swing_clearance2 == float(np.float32(0.4)) == 0.4000000059604645
    assert (p.terrain, p.use_terrain_adapt) == (1, 1)                                          # :21-22
    assert ctypes.sizeof(_lib.PlanParams) == 8 * 52 + 8
    q = mpcqp.default_plan_params(gait_counter_speed=[2, 1.5, 2, 1.5], kp_foot=np.full((4, 3), 7.0), terrain=0)
    assert list(q.gait_counter_speed) == [2.0, 1.5, 2.0, 1.5] and list(q.kp_foot) == [7.0] * 12 and q.terrain == 0


def test_slot_and_row_sizes():
    n = mpcqp.plan_state_size()
    # gait counters, start / last points and 13 filters with their rings
    assert n >= 12 * _lib.PLAN_CONTACT_WINDOW + _lib.PLAN_TERRAIN_WINDOW + 4 * 13 and n % 4 == 0
    assert _lib.PL_SIZE % 4 == 0 and _lib.PO_SIZE % 4 == 0
    assert legplan.PLAN_OUT_DTYPE.itemsize == 8 * _lib.PO_SIZE
    offs = {k: legplan.PLAN_OUT_DTYPE.fields[k][1] // 8 for k in legplan.PLAN_OUT_DTYPE.names}
    assert (offs["foot_pos_target_rel"], offs["foot_forces_kin"], offs["gait_counter"], offs["contacts"],
            offs["plane"], offs["angle_cos"], offs["terrain_pitch_angle"]) == (0, 60, 84, 96, 100, 103, 104)
    hdr = open(_lib.PKG_ROOT + "/../include/mpcqp.h").read()
    for name, val in (("PL_ROT_Z", _lib.PL_ROT_Z), ("PL_FOOT_FORCE", _lib.PL_FOOT_FORCE),
                      ("PL_MOVEMENT_MODE", _lib.PL_MOVEMENT_MODE), ("PL_SIZE", _lib.PL_SIZE),
                      ("PO_SIZE", _lib.PO_SIZE), ("PO_ANGLE", 104), ("PLAN_CONTACT_WINDOW", 60),
                      ("PLAN_TERRAIN_WINDOW", 100)):
        assert f"#define MPCQP_{name} {val} " in hdr, name


def test_invalid_arguments_need_no_device():
    L, p = _lib.load(), mpcqp.default_plan_params()
    one = ctypes.c_void_p(64)  # never dereferenced: every call below returns before a launch
    call = lambda pp, dt, st, pin, B, slot: L.mpcqp_leg_plan_device(pp, dt, st, pin, B, slot, None, None, None)
    assert call(ctypes.byref(p), 0.0005, None, None, 0, None) == _lib.ERR_OK
    assert call(None, 0.0005, one, one, 1, one) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), 0.0005, one, one, -1, one) == _lib.ERR_INVALID_ARG
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        assert call(ctypes.byref(p), dt, one, one, 1, one) == _lib.ERR_INVALID_ARG
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert call(ctypes.byref(p), 0.0005, args[0], args[1], 1, args[2]) == _lib.ERR_INVALID_ARG


def test_packers_round_trip():
    rng = np.random.default_rng(1)
    B = 5
    rz, ff, mode = rng.normal(size=(B, 3, 3)), rng.uniform(0, 80, (B, 4)), np.array([0, 1, 1, 0, 3])
    rows = mpcqp.pack_plan_inputs(rz, ff, mode)
    assert rows.shape == (B, _lib.PL_SIZE)
    rz2, ff2, mode2 = legplan.unpack_plan_inputs(rows)
    np.testing.assert_array_equal(rz2, rz)
    np.testing.assert_array_equal(ff2, ff)
    np.testing.assert_array_equal(mode2, [0, 1, 1, 0, 1])
    assert np.array_equal(rows[:, _lib.PL_MOVEMENT_MODE], [0.0, 1.0, 1.0, 0.0, 1.0]) and not rows[:, 14:].any()
    np.testing.assert_array_equal(mpcqp.pack_plan_inputs(rz, ff, 1)[:, _lib.PL_MOVEMENT_MODE], np.ones(B))


def test_restatement_trot_period_and_pairs():
    plan = ref.LegPlan(mpcqp.default_plan_params(), 1)
    pc = np.array([plan.step(0.0005, **_walk_inputs(1))["plan_contacts"][0] for _ in range(480)], dtype=bool)
    assert np.array_equal(pc[:, 0], pc[:, 3]) and np.array_equal(pc[:, 1], pc[:, 2])  # FL+RR, FR+RL
    # speed 2 over counter_per_gait 240: a 120-tick period; pair A is down while gc <= 120 (61 ticks)
    assert np.array_equal(pc[:120], pc[120:240]) and np.array_equal(pc[:240], pc[240:])
    assert 0 < pc[:120, 0].sum() < 120 and all(not np.array_equal(pc[:120], pc[k:120 + k]) for k in range(1, 120))
    both = pc[:, 0] & pc[:, 1]
    assert np.all(pc[:, 0] | pc[:, 1]) and both.sum() == 2 * 4  # the pairs overlap only at gc == 0 / 120
    assert np.array_equal(pc[:120, 0], np.arange(1, 121) * 2 % 240 <= 120)


def test_restatement_standstill_resets():
    plan = ref.LegPlan(mpcqp.default_plan_params(), 2)
    for _ in range(17):
        plan.step(0.0005, **_walk_inputs(2))
    assert not np.array_equal(plan.gait_counter[0], [0.0, 120.0, 120.0, 0.0])
    out = plan.step(0.0005, **_walk_inputs(2, mode=np.array([0, 1])))
    np.testing.assert_array_equal(out["gait_counter"][0], [0.0, 120.0, 120.0, 0.0])  # gait_counter_reset()
    np.testing.assert_array_equal(out["plan_contacts"][0], np.ones(4))
    np.testing.assert_array_equal(out["contacts"][0], np.ones(4))
    np.testing.assert_array_equal(out["gait_counter"][1], np.fmod(np.array([0.0, 120, 120, 0]) + 36, 240))
    assert out["counter"].tolist() == [18, 18]


def test_restatement_filter_is_the_window_mean():
    rng = np.random.default_rng(5)
    x = rng.normal(0.0, 3.0, (200, 4))
    f = ref.MovingWindowFilter((4,), 60)
    for t in range(200):
        avg = f.calculate_average(x[t])
        if t == 0:
            np.testing.assert_array_equal(avg, x[0] / 60.0)  # divides by the window while filling
        elif t < 59:
            np.testing.assert_allclose(avg, x[:t + 1].sum(0) / 60.0, rtol=0, atol=8 * EPS * 60 * np.abs(x).max())
        else:
            np.testing.assert_allclose(avg, np.mean(x[t - 59:t + 1], 0), rtol=0, atol=8 * EPS * 60 * np.abs(x).max())
    # a masked filter does not advance
    g = ref.MovingWindowFilter((2,), 60)
    g.calculate_average(np.array([1.0, 2.0]), np.array([True, False]))
    assert g.count.tolist() == [1, 0] and g.sum.tolist() == [1.0, 0.0]


def test_multiplied_bezier_is_within_rounding_of_pow():
    """Every reachable spline_time: float(gc - cps) / float(cps) for the gait counters of both test gaits
    (speeds 2 and 1.5 over 240).  sum(c) = 16 and the two forms differ by at most 4 roundings per
    term, hence 64 eps max|P|."""
    gcs = np.unique(np.concatenate([np.fmod(np.arange(1, 2000) * s + o, 240.0)
                                    for s in (2.0, 1.5) for o in (0.0, 120.0)]))
    gcs = gcs[gcs > 120.0]
    t = ((gcs - 120.0).astype(np.float32) / np.float32(120.0)).astype(np.float64)
    t = np.concatenate([[0.0], t])
    assert t.min() == 0.0 and 0.98 < t.max() < 1.0 and t.size > 100
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(20):
        s, f = rng.uniform(-0.4, 0.4, 2)
        P = [np.full_like(t, v) for v in (s, s + 0.0, f + 0.4000000059604645, f, f)]
        gap = np.abs(ref.bezier_mul(t, P) - ref.bezier_pow(t, P)).max()
        bound = 64 * EPS * max(abs(v[0]) for v in P)
        worst = max(worst, gap / bound)
        assert gap <= bound
    print(f"[note] bezier mul vs pow: worst gap / bound {worst:.3f}")
