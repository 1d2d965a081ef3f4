"""Warm start across control ticks on the device vs the oracle's persistent
solver (oracle/mpc_oracle.c orc_solver_step: OsqpEigen 0.6.3 initSolver on the first tick, then
updateHessianMatrix / updateGradient / updateLowerBound / updateUpperBound and a warm-started
solve; A1RobotControl.cpp:522-540).  Gates per tick: SURVEY §8(c) P1 (u0 within 1e-4 relative,
status identical, iterations within one check interval and identical for >= 99 % of the robots of
every tick; the measured fraction is printed)."""
import numpy as np
import pytest
import torch

import mpcqp
from gpu_helpers import rel_err_u0, solve_gpu

pytestmark = pytest.mark.gpu


def _oracle_sequence(oracle, params, recs_t):
    op = oracle.default_params(params.horizon, q=list(params.q_weights), r=list(params.r_weights))
    T, B = recs_t.shape[:2]
    return oracle.solve_sequence(op, recs_t, nthreads=8)


def _gpu_sequence(params, recs_t):
    T, B = recs_t.shape[:2]
    out = np.zeros((T, B), dtype=mpcqp.RESULT_DTYPE)
    with mpcqp.MpcQpSolver(params) as s:
        d_state = torch.zeros((B, s.warm_state_size), dtype=torch.float64, device="cuda")
        d_res = torch.zeros((B, mpcqp._lib.RESULT_DOUBLES), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for t in range(T):
            d_rec = torch.from_numpy(np.ascontiguousarray(recs_t[t])).cuda()
            s.solve_warm_device(d_rec.data_ptr(), B, d_state.data_ptr(), d_res.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            out[t] = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE)
    return out


def _check(got, ref, label, min_iter_equal=0.99):
    for t in range(got.shape[0]):
        np.testing.assert_array_equal(got[t]["status"], ref[t]["status"], err_msg=f"{label} tick {t}")
        ok = ref[t]["status"] != mpcqp._lib.STATUS_NAN_INPUT  # those carry NaN forces on both sides
        err = rel_err_u0(got[t]["u0"][ok], ref[t]["u0"][ok])
        assert np.all(err <= 1e-4), f"{label} tick {t}: worst {err.max():.3g}"
        di = np.abs(got[t]["iters"].astype(int) - ref[t]["iters"].astype(int))
        assert di.max() <= 25, f"{label} tick {t}: iteration drift {di.max()}"
        print(f"{label} tick {t}: iteration-equal fraction {np.mean(di == 0):.4f}")
        assert np.mean(di == 0) >= min_iter_equal, f"{label} tick {t}: {np.mean(di == 0):.2f} equal"


@pytest.mark.parametrize("gait", ["trot", "stance"])
def test_warm_sequence_matches_oracle(oracle, gait):
    T, B, N = 12, 96, 10
    ticks = mpcqp.records.synthetic_go1_ticks(B, T, seed=31, gait=gait, swing_ticks=5)
    recs_t = np.stack([mpcqp.assemble_compute_grf(s, N) for s in ticks])
    p = mpcqp.default_params(N)
    got = _gpu_sequence(p, recs_t)
    ref = _oracle_sequence(oracle, p, recs_t)
    _check(got, ref, f"warm {gait}")
    # the first tick is a cold solve, bit for bit the cold kernel's
    with mpcqp.MpcQpSolver(p) as s:
        cold, _, _ = solve_gpu(s, recs_t[0])
    np.testing.assert_array_equal(got[0]["u0"], cold["u0"])
    np.testing.assert_array_equal(got[0]["iters"], cold["iters"])
    # warm starting pays: fewer iterations than cold solves of the same ticks
    cold_iters = np.stack([oracle.solve_batch(oracle.default_params(N), recs_t[t], nthreads=8)["iters"]
                           for t in range(1, T)])
    assert got[1:]["iters"].mean() < cold_iters.mean()


def test_warm_pattern_change_reinit(oracle):
    """test_mpc's stance has exact zeros in H (upper triangle).  A yaw rotation (feet rotated along) keeps that zero
    pattern: level -> yaw -> yaw -> level is setup and then osqp_update_P on every tick, branches [0, 1, 1, 1] on the
    oracle.  A pitched or rolled copy is dense: level -> pitch -> roll -> level takes OsqpEigen's re-init, update_P
    and the re-init again, branches [0, 2, 1, 2].  (tests/test_gpu_warm_slot.py looks at the branch and the slot of
    every such tick on the device; here the results.)"""
    rec, q, r = mpcqp.assemble_test_mpc(10)
    p = mpcqp.default_params(10, q_weights=q, r_weights=r)
    op = oracle.default_params(10, q=list(q), r=list(r))
    P0, *_ = oracle.build_qp(op, rec)
    assert np.sum(np.triu(P0) == 0) > 120 * 119 // 2  # exact zeros above the diagonal

    def modes(seq):
        w = oracle.WarmSolver(op)
        out = [w.step_image(x[0])[1]["mode"] for x in seq]
        w.close()
        return out

    def posed(roll, pitch):
        x = rec.copy()
        x[mpcqp._lib.REC_EULER:mpcqp._lib.REC_EULER + 2] = (roll, pitch)
        x[mpcqp._lib.REC_X0:mpcqp._lib.REC_X0 + 2] = (roll, pitch)
        x[mpcqp._lib.REC_ROT:mpcqp._lib.REC_ROT + 9] = mpcqp.records.rot_zyx(
            np.array([roll]), np.array([pitch]), np.array([0.0]))[0].reshape(9)
        return x
    tilt = np.stack([rec, posed(0.0, 0.2), posed(0.2, 0.0), rec])[:, None, :]
    assert modes(tilt) == [0, 2, 1, 2]
    _check(_gpu_sequence(p, tilt), _oracle_sequence(oracle, p, tilt), "pattern change (pitch, roll)", min_iter_equal=1.0)

    def rotated(yaw):
        x = rec.copy()
        c, s_ = np.cos(yaw), np.sin(yaw)
        Rz = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1.0]])
        x[mpcqp._lib.REC_EULER + 2] = yaw
        x[mpcqp._lib.REC_X0 + 2] = yaw
        x[mpcqp._lib.REC_ROT:mpcqp._lib.REC_ROT + 9] = Rz.reshape(9)
        f = mpcqp._lib.rec_feet(10)
        feet = x[f:f + 120].reshape(10, 4, 3)
        x[f:f + 120] = np.einsum("ij,klj->kli", Rz, feet).reshape(120)
        return x
    seq = np.stack([rec, rotated(0.3), rotated(0.31), rec])[:, None, :]
    assert modes(seq) == [0, 1, 1, 1]
    got = _gpu_sequence(p, seq)
    ref = _oracle_sequence(oracle, p, seq)
    _check(got, ref, "pattern change", min_iter_equal=1.0)


def test_warm_nan_tick_leaves_state(oracle):
    T, B = 4, 8
    ticks = mpcqp.records.synthetic_go1_ticks(B, T, seed=5, gait="stance")
    recs_t = np.stack([mpcqp.assemble_compute_grf(s, 10) for s in ticks])
    bad = recs_t.copy()
    bad[2, 3, 7] = np.nan
    p = mpcqp.default_params(10)
    got = _gpu_sequence(p, bad)
    assert got[2]["status"][3] == mpcqp._lib.STATUS_NAN_INPUT
    ref = _oracle_sequence(oracle, p, bad)
    _check(got, ref, "nan tick")


def test_warm_mu_change_reinit(oracle):
    """A robot whose friction coefficient changes between ticks is re-initialized with the new
    friction cone (the update_P branch keeps the constraint matrix of the last init)."""
    T, B, N = 6, 32, 10
    ticks = mpcqp.records.synthetic_go1_ticks(B, T, seed=17, gait="stance")
    recs_t = np.stack([mpcqp.assemble_compute_grf(s, N) for s in ticks])
    mu = np.full((T, B), 0.6)
    mu[3:, ::2] = 0.3  # every other robot loses friction from tick 3 on
    recs_t[:, :, mpcqp._lib.REC_MU] = mu
    p = mpcqp.default_params(N)
    got = _gpu_sequence(p, recs_t)
    ref = _oracle_sequence(oracle, p, recs_t)
    _check(got, ref, "mu change", min_iter_equal=1.0)
    # the solution of a tick after the change respects the new (tighter) cone
    u = got[4]["u0"][::2].reshape(-1, 4, 3)
    fz = u[:, :, 2]
    tol = 0.25  # OSQP primal tolerance (test_oracle.test_solution_respects_friction_pyramid)
    assert np.all(np.abs(u[:, :, :2]).max(-1) <= 0.3 * fz + tol)


def test_python_robot_control_is_warm_and_mutates_state(oracle):
    """mpcqp.RobotControl.compute_grf over consecutive ticks == the oracle's persistent solver, and
    it writes mpc_states / mpc_states_d / root_lin_vel_d_world like A1RobotControl.cpp:452-488."""
    T, B, N = 8, 32, 10
    ticks = mpcqp.records.synthetic_go1_ticks(B, T, seed=77, gait="trot", swing_ticks=3)
    recs_t = np.stack([mpcqp.assemble_compute_grf(s, N) for s in ticks])
    ref = _oracle_sequence(oracle, mpcqp.default_params(N), recs_t)
    ctrl = mpcqp.RobotControl()
    try:
        for t, st in enumerate(ticks):
            f = ctrl.compute_grf(st, dt=0.002)
            got = ctrl.last_results
            np.testing.assert_array_equal(got["status"], ref[t]["status"])
            assert np.mean(got["iters"] == ref[t]["iters"]) >= 0.99
            assert np.all(rel_err_u0(got["u0"], ref[t]["u0"]) <= 1e-4)
            np.testing.assert_allclose(f, ref[t]["f_body"].reshape(B, 4, 3).transpose(0, 2, 1), atol=1e-4 * 200)
            np.testing.assert_array_equal(st.mpc_states, recs_t[t][:, :13])
            np.testing.assert_array_equal(st.mpc_states_d, recs_t[t][:, 44:44 + 13 * N])
            np.testing.assert_allclose(st.root_lin_vel_d_world,
                                       np.einsum("bij,bj->bi", st.root_rot_mat, st.root_lin_vel_d))
    finally:
        ctrl.close()
