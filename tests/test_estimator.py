"""State front end without a GPU: the C ABI's defaults and sizes, the Python packers, and self-checks of
the numpy restatement (tests/estimator_reference.py) that the GPU tests compare the kernel with."""
import ctypes

import numpy as np

import mpcqp
from mpcqp import _lib, estimator

import estimator_reference as ref

EPS = np.finfo(np.float64).eps
STAND = np.tile([0.0, 0.8, -1.6], 4)


def test_default_params_are_the_reference_constants():
    p = mpcqp.default_estimator_params()
    fix = np.array(p.rho_fix).reshape(4, 5)
    assert np.array_equal(fix[:, 0], [0.1881, 0.1881, -0.1881, -0.1881])       # GazeboA1ROS.cpp:76-79
    assert np.array_equal(fix[:, 1], [0.04675, -0.04675, 0.04675, -0.04675])   # :80-83
    assert np.array_equal(fix[:, 2], [0.08, -0.08, 0.08, -0.08])               # :84-87
    assert np.all(fix[:, 3:] == 0.213) and list(p.rho_opt) == [0.0] * 12       # :88-95
    assert (p.process_noise_pimu, p.process_noise_vimu, p.process_noise_pfoot) == (0.01, 0.01, 0.01)
    assert (p.sensor_noise_pimu_rel_foot, p.sensor_noise_vimu_rel_foot, p.sensor_noise_zfoot) == (0.001, 0.1, 0.001)
    assert (p.assume_flat_ground, p.height_noise_no_flat) == (1, 1e5)          # A1BasicEKF.cpp:40, :51
    assert (p.init_height, p.init_cov, p.gravity, p.contact_force_scale) == (0.09, 3.0, 9.81, 100.0)
    assert (p.drift_threshold, p.drift_divisor) == (1e-6, 10.0)                # :143-146
    q = mpcqp.default_estimator_params(process_noise_pimu=1.0, rho_opt=np.full((4, 3), 0.01), assume_flat_ground=0)
    assert q.process_noise_pimu == 1.0 and list(q.rho_opt) == [0.01] * 12 and q.assume_flat_ground == 0


def test_sizes_agree_with_the_header():
    hdr = open(_lib.PKG_ROOT + "/../include/mpcqp.h").read()
    for name, val in (("SN_QUAT", _lib.SN_QUAT), ("SN_JOINT_POS", _lib.SN_JOINT_POS),
                      ("SN_JOINT_VEL", _lib.SN_JOINT_VEL), ("SN_IMU_ACC", _lib.SN_IMU_ACC),
                      ("SN_IMU_ANG_VEL", _lib.SN_IMU_ANG_VEL), ("SN_SIZE", _lib.SN_SIZE),
                      ("EO_FOOT_POS_REL", _lib.EO_FOOT_POS_REL), ("EO_FOOT_VEL_REL", _lib.EO_FOOT_VEL_REL),
                      ("EO_FOOT_VEL_ABS", _lib.EO_FOOT_VEL_ABS), ("EO_CONTACT_W", _lib.EO_CONTACT_W),
                      ("EO_X", _lib.EO_X), ("EO_DIAG_P", _lib.EO_DIAG_P), ("EO_DET", _lib.EO_DET),
                      ("EO_SIZE", _lib.EO_SIZE)):
        assert f"#define MPCQP_{name} {val} " in hdr, name
    assert (_lib.SN_SIZE, _lib.EO_SIZE) == (36, 80) and _lib.SN_SIZE % 4 == 0 and _lib.EO_SIZE % 4 == 0
    assert estimator.EST_OUT_DTYPE.itemsize == 8 * _lib.EO_SIZE
    offs = {k: estimator.EST_OUT_DTYPE.fields[k][1] // 8 for k in estimator.EST_OUT_DTYPE.names}
    assert (offs["foot_pos_rel"], offs["foot_vel_rel"], offs["foot_vel_abs"], offs["contact_weights"], offs["x"],
            offs["diag_P"], offs["det"]) == (0, 12, 24, 36, 40, 58, 76)
    # the struct: 20 + 12 + 13 doubles and two int32
    assert _lib.load().mpcqp_est_params_size() == ctypes.sizeof(_lib.EstimatorParams) == 8 * 45 + 8
    n = mpcqp.estimator_state_size()
    assert n >= 1 + 18 + 18 * 18 and n % 4 == 0


def test_invalid_arguments_need_no_device():
    L, p = _lib.load(), mpcqp.default_estimator_params()
    call = lambda pp, dt, n: L.mpcqp_state_estimate_device(pp, dt, None, None, None, n, None, None, None, None)
    assert call(None, 0.0005, 0) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), 0.0005, -1) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), 0.0005, 3) == _lib.ERR_INVALID_ARG  # NULL required pointers
    for dt in (0.0, -0.0005, float("nan"), float("inf")):
        assert call(ctypes.byref(p), dt, 0) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), 0.0005, 0) == _lib.ERR_OK  # batch 0: nothing to launch


def test_packers_round_trip():
    rng = np.random.default_rng(0)
    B = 5
    parts = (rng.normal(size=(B, 4)), rng.normal(size=(B, 12)), rng.normal(size=(B, 12)), rng.normal(size=(B, 3)),
             rng.normal(size=(B, 3)))
    rows = mpcqp.pack_sensors(*parts)
    assert rows.shape == (B, _lib.SN_SIZE) and np.all(rows[:, 34:] == 0.0)
    for a, b in zip(parts, estimator.unpack_sensors(rows)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(rows[:, _lib.SN_QUAT], parts[0][:, 0])  # w first
    x, P = rng.normal(size=(B, 18)), rng.normal(size=(B, 18, 18))
    slot = mpcqp.pack_estimator_slot(x, P)
    assert slot.shape == (B, mpcqp.estimator_state_size())
    inited, x2, P2 = mpcqp.unpack_estimator_slot(slot)
    assert inited.all()
    np.testing.assert_array_equal(x2, x)
    np.testing.assert_array_equal(P2, P)
    assert not mpcqp.unpack_estimator_slot(np.zeros_like(slot))[0].any()  # a zero slot is not initialized


def test_jacobian_is_the_finite_difference_of_fk():
    """Central difference with step h: truncation h^2/6 |f'''| and rounding (evaluation error of f) / h.
    Every component of fk is a sum of at most three link terms, each a length <= 0.25 times a product of
    sines and cosines in which each joint angle appears once, so any third partial derivative is bounded
    by 3 * 0.25 = 0.75; |f| <= 1 and the restatement evaluates it within 8 eps.  With h = 1e-5:
    1e-10 / 6 * 0.75 + 8 eps / 1e-5 = 1.3e-11 + 1.8e-10 < 2e-10."""
    rng = np.random.default_rng(1)
    p = mpcqp.default_estimator_params(rho_opt=rng.uniform(-0.02, 0.02, (4, 3)))
    fix, opt = np.array(p.rho_fix).reshape(4, 5), np.array(p.rho_opt).reshape(4, 3)
    assert np.abs(fix[:, 2:]).max() <= 0.25 and np.abs(opt).max() <= 0.25
    h, tol = 1e-5, 2e-10
    q = STAND.reshape(1, 4, 3) + rng.uniform(-0.6, 0.6, (200, 4, 3))
    J = ref.jac(q, opt[None], fix[None])
    for j in range(3):
        dq = np.zeros(3)
        dq[j] = h
        fd = (ref.fk(q + dq, opt[None], fix[None]) - ref.fk(q - dq, opt[None], fix[None])) / (2 * h)
        assert np.abs(fd - J[..., j]).max() <= tol, (j, np.abs(fd - J[..., j]).max())
    assert np.abs(J[..., 1:, :]).max() > 0.1 and np.all(J[..., 0, 0] == 0.0)
    # the standing pose of the default geometry: feet under the hips, about 0.3 below
    p0 = mpcqp.default_estimator_params()
    f0 = ref.fk(STAND.reshape(4, 3), np.zeros((4, 3)), np.array(p0.rho_fix).reshape(4, 5))
    assert np.all(np.sign(f0[:, 0]) == [1, 1, -1, -1]) and np.all(np.sign(f0[:, 1]) == [1, -1, 1, -1])
    assert np.all(np.abs(f0[:, 2] + 0.2968) < 1e-3)


def _random_step(rng, B, p, dt):
    quat = rng.normal(size=(B, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    fe = ref.front_end(p, quat, STAND + rng.uniform(-0.6, 0.6, (B, 12)), rng.normal(size=(B, 12)), rng.normal(size=(B, 3)))
    x = rng.normal(0.0, 0.3, (B, 18))
    G = rng.normal(size=(B, 18, 18))
    P = G @ G.transpose(0, 2, 1) / 18 + 0.1 * np.eye(18)
    c = ref.contact_weights(p, rng.uniform(-20.0, 140.0, (B, 4)), np.arange(B) % 5 != 0)
    return ref.predict_and_measure(p, dt, x, P, fe, rng.normal(size=(B, 3)) + [0, 0, 9.81], rng.normal(size=(B, 3)), c)


def test_filter_step_is_the_textbook_gain_form():
    """x = xbar + K e, P = (I - K C) Pbar with K = Pbar C' S^-1 against the restatement's two pivoted-QR
    solves: both are backward-stable solves with S, so they agree to 64 kappa_2(S) eps max(1, |ref|_inf)."""
    rng = np.random.default_rng(2)
    B, dt = 40, 0.0005
    for p in (mpcqp.default_estimator_params(), mpcqp.default_estimator_params(assume_flat_ground=0)):
        xbar, Pbar, err, S = _random_step(rng, B, p, dt)
        x, P = ref.correct(xbar, Pbar, err, S)
        C = ref.make_C()
        K = np.linalg.solve(S, C @ Pbar).transpose(0, 2, 1)  # S symmetric: (S^-1 C Pbar)' = Pbar C' S^-1
        x_t = xbar + np.einsum("bij,bj->bi", K, err)
        P_t = (np.eye(18) - K @ C) @ Pbar
        kappa = np.linalg.cond(S)
        assert kappa.max() < 1e8 and kappa.min() > 10
        bx = 64 * kappa * EPS * np.maximum(1.0, np.abs(x).max(1))
        bP = 64 * kappa * EPS * np.maximum(1.0, np.abs(P).max((1, 2)))
        assert np.all(np.abs(x_t - x).max(1) <= bx), (np.abs(x_t - x).max(1) / bx).max()
        assert np.all(np.abs(P_t - P).max((1, 2)) <= bP), (np.abs(P_t - P).max((1, 2)) / bP).max()
        np.testing.assert_array_equal(P, P.transpose(0, 2, 1))
        # the pivoted QR itself: residual of a plain solve
        sol = ref.qr_solve(S, err[:, :, None])[:, :, 0]
        res = np.abs(np.einsum("bij,bj->bi", S, sol) - err).max(1)
        assert np.all(res <= 64 * EPS * np.abs(S).sum(2).max(1) * np.abs(sol).max(1))


def test_first_tick_is_init_state_and_resets_follow():
    p = mpcqp.default_estimator_params()
    B = 4
    rng = np.random.default_rng(3)
    quat = np.tile([1.0, 0.0, 0.0, 0.0], (B, 1))
    est = ref.Estimator(p, B)
    pos0, vel0 = rng.normal(size=(B, 3)), rng.normal(size=(B, 3))
    args = (quat, np.tile(STAND, (B, 1)), np.zeros((B, 12)), np.tile([0.0, 0.0, 9.81], (B, 1)), np.zeros((B, 3)),
            np.full((B, 4), 80.0), np.ones(B, dtype=np.int64))
    o = est.step(0.0005, *args, pos0, vel0)
    np.testing.assert_array_equal(o["root_pos"], pos0)  # init_state leaves root_pos / root_lin_vel alone
    np.testing.assert_array_equal(o["root_lin_vel"], vel0)
    np.testing.assert_array_equal(o["P"], np.broadcast_to(3.0 * np.eye(18), (B, 18, 18)))
    np.testing.assert_array_equal(o["x"][:, :6], np.tile([0, 0, 0.09, 0, 0, 0], (B, 1)))
    np.testing.assert_array_equal(o["x"][:, 6:].reshape(B, 4, 3), o["foot_pos_abs"] + [0.0, 0.0, 0.09])
    np.testing.assert_array_equal(o["root_rot_mat"], np.broadcast_to(np.eye(3), (B, 3, 3)))
    o = est.step(0.0005, *args, pos0, vel0)
    # P = 3 I: the first update's determinant is far above 1e-6, the reset fires and decouples x, y
    assert o["reset"].all() and np.all(o["P"][:, 0:2, 2:] == 0.0) and np.all(o["P"][:, 2:, 0:2] == 0.0)
    assert np.all(o["contact_weights"] == 0.8) and o["contacts"].all()
    np.testing.assert_array_equal(o["root_pos"], o["x"][:, 0:3])
    # a level robot standing still at the height its legs give: the estimate moves towards it
    assert np.all(np.abs(o["x"][:, 2] - 0.2968) < np.abs(0.09 - 0.2968))
