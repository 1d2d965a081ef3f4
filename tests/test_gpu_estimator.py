"""mpcqp_state_estimate_device on the GPU against the numpy restatement (tests/estimator_reference.py):
frames and leg kinematics within rounding-derived bounds, the Kalman filter over 300 free-running ticks
within the forward-error bound of its 28x28 solve, re-entered drift resets, a start from a chosen slot,
that nothing but the documented fields moves, and the five-stage ControlTick eager against its graph."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib, estimator, legplan
from mpcqp.records import RobotStates, synthetic_go1_ticks
from mpcqp.tick import ControlTick

import estimator_reference as ref
import legplan_reference as plan_ref
from test_torques import torque_inputs

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DT = 0.0005
T_SEQ = 300
STAND = np.tile([0.0, 0.8, -1.6], 4)
# "pimu" lets the position covariance grow back past the drift threshold between resets; "no_flat" is the
# same without the flat-ground height rows (R = 1e5 there)
PARAM_SETS = {"default": {}, "pimu": dict(process_noise_pimu=1.0),
              "no_flat": dict(process_noise_pimu=1.0, assume_flat_ground=0)}


def _quat(roll, pitch, yaw):
    """w, x, y, z of Rz(yaw) Ry(pitch) Rx(roll)."""
    cr, sr, cp, sp, cy, sy = (f(a / 2) for a in (roll, pitch, yaw) for f in (np.cos, np.sin))
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy], -1)


def _sequence(B, T, seed):
    """[T][B] sensor-level inputs: random attitudes with |roll|, |pitch| <= 0.5, joint angles within
    +-0.6 of the standing pose, joint rates N(0, 1), foot forces alternating per leg pair between 0-30 and
    60-140 every 60 ticks, one robot in five standing."""
    rng = np.random.default_rng(seed)
    roll, pitch = rng.uniform(-0.5, 0.5, (T, B)), rng.uniform(-0.5, 0.5, (T, B))
    yaw = rng.uniform(-np.pi, np.pi, (T, B))
    quat = _quat(roll, pitch, yaw)
    joint_pos = STAND + rng.uniform(-0.6, 0.6, (T, B, 12))
    joint_vel = rng.normal(0.0, 1.0, (T, B, 12))
    imu_acc = rng.normal(0.0, 0.5, (T, B, 3)) + np.array([0.0, 0.0, 9.81])
    imu_ang_vel = rng.normal(0.0, 0.3, (T, B, 3))
    low, high = rng.uniform(0.0, 30.0, (T, B, 4)), rng.uniform(60.0, 140.0, (T, B, 4))
    pair_a = np.array([True, False, False, True])
    a_high = ((np.arange(T) // 60) % 2 == 0)[:, None, None]
    force = np.where(pair_a[None, None, :] == a_high, high, low)
    mode = (np.arange(B) % 5 != 4).astype(np.int64)
    return dict(quat=quat, joint_pos=joint_pos, joint_vel=joint_vel, imu_acc=imu_acc, imu_ang_vel=imu_ang_vel,
                force=force, mode=mode, pos0=rng.normal(0.0, 1.0, (B, 3)), vel0=rng.normal(0.0, 1.0, (B, 3)))


def _ref_steps(p, seq, B, T, x=None, P=None):
    est = ref.Estimator(p, B, x, P)
    return [est.step(DT, seq["quat"][t], seq["joint_pos"][t], seq["joint_vel"][t], seq["imu_acc"][t],
                     seq["imu_ang_vel"][t], seq["force"][t], seq["mode"], seq["pos0"], seq["vel0"]) for t in range(T)]


def _state_rows(seq, T, B, pad, rng):
    """Caller's MPCQP_ST_* rows: arbitrary finite values everywhere (the stage must leave the fields it
    does not own), ST_POS / ST_LIN_VEL as the caller's initial guess; NaN sentinel rows beyond B."""
    st = np.full((T, B + pad, _lib.ST_SIZE), np.nan)
    st[:, :B] = rng.normal(size=(T, B, _lib.ST_SIZE))
    st[:, :B, _lib.ST_POS:_lib.ST_POS + 3] = seq["pos0"]
    st[:, :B, _lib.ST_LIN_VEL:_lib.ST_LIN_VEL + 3] = seq["vel0"]
    return st


def _run(p, seq, B, T, pad=0, with_out=True, with_tq=True, slot0=None, sensors_edit=None):
    """One launch per tick on inputs uploaded once as [T][B][..]; everything is downloaded after the last
    tick (the slot after each tick through a device-side copy)."""
    rng = np.random.default_rng(99)
    nan = float("nan")
    sn = np.full((T, B + pad, _lib.SN_SIZE), nan)
    pin = np.full((T, B + pad, _lib.PL_SIZE), nan)
    for t in range(T):
        sn[t, :B] = mpcqp.pack_sensors(seq["quat"][t], seq["joint_pos"][t], seq["joint_vel"][t], seq["imu_acc"][t],
                                       seq["imu_ang_vel"][t])
        pin[t, :B] = mpcqp.pack_plan_inputs(np.full((B, 3, 3), 7.0), seq["force"][t], seq["mode"])
    if sensors_edit is not None:
        sensors_edit(sn)
    st = _state_rows(seq, T, B, pad, rng)
    tq = np.full((T, B + pad, _lib.TQ_SIZE), nan)
    tq[:, :B] = rng.normal(size=(T, B, _lib.TQ_SIZE))
    n = mpcqp.estimator_state_size()
    slot = np.full((B + pad, n), nan)
    slot[:B] = 0.0 if slot0 is None else slot0
    d_sn, d_pin, d_st = (torch.from_numpy(a).cuda() for a in (sn, pin, st))
    d_tq = torch.from_numpy(tq).cuda() if with_tq else None
    d_out = torch.full((T, B + pad, _lib.EO_SIZE), nan, dtype=torch.float64, device="cuda") if with_out else None
    d_slot = torch.from_numpy(slot).cuda()
    d_hist = torch.empty((T, B + pad, n), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for t in range(T):
        mpcqp.state_estimate_device(p, DT, d_sn[t].data_ptr(), d_pin[t].data_ptr(), d_st[t].data_ptr(), B,
                                    d_slot.data_ptr(), d_tq[t].data_ptr() if with_tq else 0,
                                    d_out[t].data_ptr() if with_out else 0, s)
        d_hist[t].copy_(d_slot)
    torch.cuda.synchronize()
    out_raw = d_out.cpu().numpy() if with_out else None
    return dict(sensors=sn, plan_in0=pin, plan_in=d_pin.cpu().numpy(), states0=st, states=d_st.cpu().numpy(),
                tq0=tq, tq=d_tq.cpu().numpy() if with_tq else None, out_raw=out_raw,
                out=out_raw.view(estimator.EST_OUT_DTYPE)[..., 0] if with_out else None,
                slots=d_hist.cpu().numpy(), slot0=slot)


@functools.lru_cache(maxsize=None)
def _case(B, pset):
    """The 300-tick sequence, its reference and its GPU run, shared by the tests that read them."""
    seq = _sequence(B, T_SEQ, 5 + B)
    p = mpcqp.default_estimator_params(**PARAM_SETS[pset])
    return seq, p, _ref_steps(p, seq, B, T_SEQ), _run(p, seq, B, T_SEQ)


def _stack(want, key):
    return np.stack([w[key] for w in want])


@pytest.mark.parametrize("B", [1, 67])
def test_frames_and_legs(B):
    seq, p, want, got = _case(B, "default")
    T = T_SEQ
    st, out = got["states"], got["out"]
    R = _stack(want, "root_rot_mat")
    np.testing.assert_array_equal(st[:, :, _lib.ST_ROT:_lib.ST_ROT + 9].reshape(T, B, 3, 3), R)  # pure arithmetic
    for name, g, w in (("euler", st[:, :, _lib.ST_EULER:_lib.ST_EULER + 3], _stack(want, "root_euler")),
                       ("rot_z", got["plan_in"][:, :, _lib.PL_ROT_Z:_lib.PL_ROT_Z + 9].reshape(T, B, 3, 3),
                        _stack(want, "rot_z"))):
        ratio = np.abs(g - w) / (8 * EPS * np.maximum(1.0, np.abs(w)))
        print(f"[note] B={B} {name}: worst error / bound {ratio.max():.3f}")
        assert ratio.max() <= 1.0, name
    # L = sum |rho_fix| + sum |rho_opt| of the leg; at most ten terms, each a link length times at most
    # three trig values of <= 2 ulp, plus the sum's own rounding: 32 eps L
    L = (np.abs(np.array(p.rho_fix).reshape(4, 5)).sum(1) + np.abs(np.array(p.rho_opt).reshape(4, 3)).sum(1))
    qd1 = np.abs(seq["joint_vel"].reshape(T, B, 4, 3)).sum(-1)
    b_pos = 32 * EPS * L[None, None, :, None]
    b_vel = 40 * EPS * L[None, None, :, None] * qd1[..., None]
    w_pos, w_vel = _stack(want, "foot_pos_rel"), _stack(want, "foot_vel_rel")
    w_abs, w_vabs, w_ang = _stack(want, "foot_pos_abs"), _stack(want, "foot_vel_abs"), _stack(want, "root_ang_vel")
    checks = (
        ("foot_pos_rel", out["foot_pos_rel"], w_pos, b_pos),
        ("TQ_JFOOT", got["tq"][:, :, _lib.TQ_JFOOT:_lib.TQ_JFOOT + 36].reshape(T, B, 4, 3, 3), _stack(want, "j_foot"),
         b_pos[..., None]),
        ("foot_vel_rel", out["foot_vel_rel"], w_vel, b_vel),
        # rotated: the same bounds times |R|_1 <= 3, plus the product's own rounding 4 eps |ref|
        ("ST_FEET", st[:, :, _lib.ST_FEET:_lib.ST_FEET + 12].reshape(T, B, 4, 3), w_abs, 3 * b_pos + 4 * EPS * np.abs(w_abs)),
        ("foot_vel_abs", out["foot_vel_abs"], w_vabs, 3 * b_vel + 4 * EPS * np.abs(w_vabs)),
        ("ST_ANG_VEL", st[:, :, _lib.ST_ANG_VEL:_lib.ST_ANG_VEL + 3], w_ang, 4 * EPS * np.abs(w_ang)),
    )
    for name, g, w, bound in checks:
        bound = np.broadcast_to(bound, w.shape)
        err = np.abs(g - w)
        nz = bound > 0
        print(f"[note] B={B} {name}: worst error / bound {(err[nz] / bound[nz]).max():.3f}")
        assert np.all(err <= bound), name
    # the Jacobian went in row-major: J[1][0] = d p_y / d q_hip is not J[0][1] = d p_x / d q_thigh
    J = got["tq"][0, :, _lib.TQ_JFOOT:_lib.TQ_JFOOT + 36].reshape(B, 4, 3, 3)
    assert np.all(J[..., 0, 0] == 0.0) and np.all(J[..., 0, 1] != J[..., 1, 0])


def _check_filter(B, want, got, label, first_update=1, kappa_max=1e6):
    """|got - ref| <= 64 kappa_2(S) eps max(1, |ref|_inf) for ST_POS, ST_LIN_VEL, x, diag P and the
    slot's P on every robot-tick (the forward error of a backward-stable solve of order 28); equal contact
    flags and drift-reset decisions.  kappa comes from the restatement and is itself bounded by kappa_max."""
    T = len(want)
    st, out = got["states"], got["out"]
    _, xs, Ps = mpcqp.unpack_estimator_slot(got["slots"].reshape(T * B, -1))
    xs, Ps = xs.reshape(T, B, 18), Ps.reshape(T, B, 18, 18)
    worst = 0.0
    for t in range(first_update, T):
        w = want[t]
        kappa = w["cond"]
        assert np.all(kappa <= kappa_max), (t, kappa.max())
        unit = 64 * kappa * EPS
        bx = unit * np.maximum(1.0, np.abs(w["x"]).max(1))
        bP = unit * np.maximum(1.0, np.abs(w["P"]).max((1, 2)))
        errs = (
            (np.abs(st[t, :, _lib.ST_POS:_lib.ST_POS + 3] - w["root_pos"]).max(1), unit * np.maximum(1.0, np.abs(w["root_pos"]).max(1))),
            (np.abs(st[t, :, _lib.ST_LIN_VEL:_lib.ST_LIN_VEL + 3] - w["root_lin_vel"]).max(1),
             unit * np.maximum(1.0, np.abs(w["root_lin_vel"]).max(1))),
            (np.abs(out["x"][t] - w["x"]).max(1), bx),
            (np.abs(xs[t] - w["x"]).max(1), bx),
            (np.abs(out["diag_P"][t] - w["diag_P"]).max(1), unit * np.maximum(1.0, np.abs(w["diag_P"]).max(1))),
            (np.abs(Ps[t] - w["P"]).max((1, 2)), bP),
        )
        for k, (e, b) in enumerate(errs):
            worst = max(worst, (e / b).max())
            assert np.all(e <= b), (label, t, k, (e / b).max())
        np.testing.assert_array_equal(~(out["contact_weights"][t] < 0.5), w["contacts"])
        np.testing.assert_array_equal(out["det"][t] > 1e-6, w["reset"], err_msg=f"{label} tick {t}")
        np.testing.assert_array_equal(np.all(Ps[t][:, 0:2, 2:] == 0.0, axis=(1, 2)) | ~w["reset"], np.ones(B, bool))
        np.testing.assert_array_equal(Ps[t], Ps[t].transpose(0, 2, 1))
    print(f"[note] {label}: worst filter error / bound {worst:.4f}")
    return worst


@pytest.mark.parametrize("B", [1, 67])
def test_filter_free_running(B):
    seq, p, want, got = _case(B, "default")
    # tick 0 is init_state: P = 3 I and x[0:6] exactly, the feet from the stage's own foot_pos_abs, and
    # root_pos / root_lin_vel as the caller wrote them
    inited, x0, P0 = mpcqp.unpack_estimator_slot(got["slots"][0])
    assert inited.all()
    np.testing.assert_array_equal(P0, np.broadcast_to(3.0 * np.eye(18), (B, 18, 18)))
    np.testing.assert_array_equal(x0[:, :6], np.tile([0, 0, 0.09, 0, 0, 0], (B, 1)))
    np.testing.assert_array_equal(x0[:, 6:], got["states"][0, :, _lib.ST_FEET:_lib.ST_FEET + 12] + np.tile([0, 0, 0.09], 4))
    np.testing.assert_array_equal(got["states"][0, :, _lib.ST_POS:_lib.ST_POS + 3], seq["pos0"])
    np.testing.assert_array_equal(got["states"][0, :, _lib.ST_LIN_VEL:_lib.ST_LIN_VEL + 3], seq["vel0"])
    np.testing.assert_array_equal(got["out"]["x"][0], x0)
    assert np.all(got["out"]["diag_P"][0] == 3.0) and np.all(got["out"]["det"][0] == 0.0)
    resets = _stack(want, "reset")
    assert resets[1:4].all() and not resets[6:].any()  # the first updates reset (P = 3 I), then P has contracted
    weights = _stack(want, "contact_weights")[1:]
    assert (weights == 1.0).any() and ((weights > 0) & (weights < 0.5)).any() and ((weights > 0.5) & (weights < 1)).any()
    _check_filter(B, want, got, f"free running B={B}")


@pytest.mark.parametrize("pset", ["pimu", "no_flat"])
@pytest.mark.parametrize("B", [1, 67])
def test_drift_reset_is_reentered(B, pset):
    """The resets are asserted for the walking robots.  A standing robot has all four contact weights at 1,
    so its position covariance settles with det P[0:2,0:2] below 9e-7 and never reaches the threshold again
    (restatement, 300 ticks); that it is not reset either is part of the equal-decisions check.
    Without the flat-ground rows R holds 1e5 beside 1e-3, so kappa_2(S) is about 1e8 by construction; the
    bound scales with it and the kappa <= 1e6 condition applies to the flat-ground sets."""
    seq, p, want, got = _case(B, pset)
    resets, det = _stack(want, "reset"), _stack(want, "det")
    walking = seq["mode"] != 0
    assert walking[0] and (B == 1 or (~walking).any())
    assert np.all(resets[6:, walking].sum(0) > 3), resets[6:, walking].sum(0).min()  # more than three after tick 5
    assert not resets[6:, ~walking].any()
    margin = np.abs(det[1:] - 1e-6).min()
    print(f"[note] {pset} B={B}: resets per robot {resets[6:].sum(0).min()}..{resets[6:].sum(0).max()}, "
          f"nearest |det - 1e-6| = {margin:.3e}")
    assert margin >= 1e-6 * 1e-6
    _check_filter(B, want, got, f"{pset} B={B}", kappa_max=1e6 if p.assume_flat_ground else 1e9)


def test_start_from_a_chosen_slot():
    B = 67
    rng = np.random.default_rng(17)
    seq = _sequence(B, 1, 31)
    p = mpcqp.default_estimator_params()
    x = rng.normal(0.0, 0.3, (B, 18))
    G = rng.normal(size=(B, 18, 18))
    P = G @ G.transpose(0, 2, 1) / 18 + 0.05 * np.eye(18)
    P = 0.5 * (P + P.transpose(0, 2, 1))
    want = _ref_steps(p, seq, B, 1, x, P)
    got = _run(p, seq, B, 1, slot0=mpcqp.pack_estimator_slot(x, P))
    assert np.all(got["out"]["contact_weights"][0] == want[0]["contact_weights"])
    _check_filter(B, want, got, "chosen slot", first_update=0)
    # a zero slot: exactly init_state, ST_POS / ST_LIN_VEL untouched
    zero = _run(p, seq, B, 1)
    inited, x0, P0 = mpcqp.unpack_estimator_slot(zero["slots"][0])
    assert inited.all()
    np.testing.assert_array_equal(P0, np.broadcast_to(p.init_cov * np.eye(18), (B, 18, 18)))
    np.testing.assert_array_equal(x0[:, :6], np.tile([0, 0, p.init_height, 0, 0, 0], (B, 1)))
    np.testing.assert_array_equal(x0[:, 6:], zero["states"][0, :, _lib.ST_FEET:_lib.ST_FEET + 12]
                                  + np.tile([0, 0, p.init_height], 4))
    np.testing.assert_array_equal(zero["states"][0, :, _lib.ST_POS:_lib.ST_POS + 3], seq["pos0"])
    np.testing.assert_array_equal(zero["states"][0, :, _lib.ST_LIN_VEL:_lib.ST_LIN_VEL + 3], seq["vel0"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _moves():
    st = np.zeros(_lib.ST_SIZE, bool)
    for off, n in ((_lib.ST_EULER, 3), (_lib.ST_POS, 3), (_lib.ST_ANG_VEL, 3), (_lib.ST_LIN_VEL, 3), (_lib.ST_ROT, 9),
                   (_lib.ST_FEET, 12)):
        st[off:off + n] = True
    pl = np.zeros(_lib.PL_SIZE, bool)
    pl[_lib.PL_ROT_Z:_lib.PL_ROT_Z + 9] = True
    tq = np.zeros(_lib.TQ_SIZE, bool)
    tq[_lib.TQ_JFOOT:_lib.TQ_JFOOT + 36] = True
    return st, pl, tq


def test_nothing_else_moves():
    B, T, pad = 5, 4, 3
    seq = _sequence(B, T, 41)
    p = mpcqp.default_estimator_params()
    got = _run(p, seq, B, T, pad=pad)
    st_m, pl_m, tq_m = _moves()
    np.testing.assert_array_equal(_bits(got["states"])[:, :B, ~st_m], _bits(got["states0"])[:, :B, ~st_m])
    np.testing.assert_array_equal(_bits(got["plan_in"])[:, :B, ~pl_m], _bits(got["plan_in0"])[:, :B, ~pl_m])
    np.testing.assert_array_equal(_bits(got["tq"])[:, :B, ~tq_m], _bits(got["tq0"])[:, :B, ~tq_m])
    assert not np.isnan(got["states"][:, :B, st_m]).any() and not np.isnan(got["tq"][:, :B, tq_m]).any()
    assert np.all(got["plan_in"][:, :B, :9] != 7.0)  # root_rot_mat_z was written
    assert not np.isnan(got["out_raw"][:, :B]).any() and np.all(got["out_raw"][:, :B, 77:] == 0.0)
    # NaN sentinel rows beyond batch are untouched, in every buffer
    for key in ("states", "plan_in", "tq", "out_raw", "slots"):
        assert np.isnan(got[key][:, B:]).all(), key
    # optional outputs left out: every other buffer comes out the same
    bare = _run(p, seq, B, T, pad=pad, with_out=False, with_tq=False)
    for key in ("states", "plan_in", "slots"):
        np.testing.assert_array_equal(_bits(bare[key]), _bits(got[key]), err_msg=key)

    # a robot with a NaN in its sensor row from tick 2 on: its slot stays bitwise, ST_POS / ST_LIN_VEL are
    # NaN, and its neighbours are unaffected
    def poison(sn):
        sn[2:, 1, _lib.SN_JOINT_VEL + 4] = np.nan

    bad = _run(p, seq, B, T, pad=pad, sensors_edit=poison)
    others = [0, 2, 3, 4]
    for key in ("states", "plan_in", "tq", "out_raw", "slots"):
        np.testing.assert_array_equal(_bits(bad[key])[:, others], _bits(got[key])[:, others], err_msg=key)
        np.testing.assert_array_equal(_bits(bad[key])[:2, 1], _bits(got[key])[:2, 1], err_msg=key)
    for t in (2, 3):
        np.testing.assert_array_equal(_bits(bad["slots"])[t, 1], _bits(got["slots"])[1, 1])
        assert np.isnan(bad["states"][t, 1, _lib.ST_POS:_lib.ST_POS + 3]).all()
        assert np.isnan(bad["states"][t, 1, _lib.ST_LIN_VEL:_lib.ST_LIN_VEL + 3]).all()
        assert np.isnan(bad["out"]["x"][t, 1]).all()
    # a non-finite sensor row on the very first tick: the slot stays zero (not initialized)
    first = _run(p, seq, B, 1, sensors_edit=lambda sn: sn.__setitem__((0, 3, _lib.SN_QUAT), np.inf))
    assert not first["slots"][0, 3].any() and np.isnan(first["states"][0, 3, _lib.ST_POS:_lib.ST_POS + 3]).all()
    assert first["slots"][0, [0, 1, 2, 4], 0].all()


def test_argument_checks_on_the_device():
    L, p = _lib.load(), mpcqp.default_estimator_params()
    B = 3
    f64 = dict(dtype=torch.float64, device="cuda")
    sn = torch.from_numpy(mpcqp.pack_sensors(np.tile([1.0, 0, 0, 0], (B, 1)), np.tile(STAND, (B, 1)), np.zeros((B, 12)),
                                             np.tile([0, 0, 9.81], (B, 1)), np.zeros((B, 3)))).cuda()
    pin, st = torch.zeros((B, _lib.PL_SIZE), **f64), torch.zeros((B, _lib.ST_SIZE), **f64)
    slot = torch.zeros((B, mpcqp.estimator_state_size()), **f64)
    vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    call = lambda pp, dt, a, b, c, n, d: L.mpcqp_state_estimate_device(pp, dt, vp(a), vp(b), vp(c), n, vp(d), None,
                                                                       None, None)
    ok = ctypes.byref(p)
    assert call(ok, DT, sn, pin, st, 0, slot) == _lib.ERR_OK
    assert call(ok, DT, None, None, None, 0, None) == _lib.ERR_OK
    torch.cuda.synchronize()
    assert not slot.any() and not st.any() and not pin.any()  # batch == 0 launched nothing
    assert call(None, DT, sn, pin, st, B, slot) == _lib.ERR_INVALID_ARG
    assert call(ok, DT, sn, pin, st, -1, slot) == _lib.ERR_INVALID_ARG
    for dt in (0.0, -DT, float("nan"), float("inf")):
        assert call(ok, dt, sn, pin, st, B, slot) == _lib.ERR_INVALID_ARG
    for a, b, c, d in ((None, pin, st, slot), (sn, None, st, slot), (sn, pin, None, slot), (sn, pin, st, None)):
        assert call(ok, DT, a, b, c, B, d) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not slot.any()
    assert call(ok, DT, sn, pin, st, B, slot) == _lib.ERR_OK
    torch.cuda.synchronize()
    assert (slot[:, 0] == 1.0).all()  # every robot's filter left the uninitialized state


# ---- the five-stage tick ------------------------------------------------------------------------------
def _tick_inputs(B, T):
    """Near-level robots near the standing pose with small joint rates, three in four walking."""
    rng = np.random.default_rng(23)
    states_t = synthetic_go1_ticks(B, T, seed=8, gait="stance")
    quat = np.stack([_quat(st.root_euler[:, 0], st.root_euler[:, 1], st.root_euler[:, 2]) for st in states_t])
    seq = dict(quat=quat, joint_pos=STAND + rng.uniform(-0.1, 0.1, (T, B, 12)), joint_vel=rng.normal(0.0, 0.05, (T, B, 12)),
               imu_acc=rng.normal(0.0, 0.1, (T, B, 3)) + np.array([0.0, 0.0, 9.81]),
               imu_ang_vel=rng.normal(0.0, 0.1, (T, B, 3)), force=rng.uniform(0.0, 60.0, (T, B, 4)),
               mode=(np.arange(B) % 4 != 0).astype(np.int64))
    sensors = [mpcqp.pack_sensors(seq["quat"][t], seq["joint_pos"][t], seq["joint_vel"][t], seq["imu_acc"][t],
                                  seq["imu_ang_vel"][t]) for t in range(T)]
    plan_in = [mpcqp.pack_plan_inputs(np.zeros((B, 3, 3)), seq["force"][t], seq["mode"]) for t in range(T)]
    return states_t, seq, sensors, plan_in


def _drive(tick, states_t, sensors, plan_in, tq, use_graph, zero_warm_before=None):
    outs = []
    tick.tq_records.copy_(torch.from_numpy(tq))
    tick.states.copy_(torch.from_numpy(mpcqp.pack_states(states_t[0])))  # the caller's fields, written once
    for t, (sn, pin) in enumerate(zip(sensors, plan_in)):
        tick.sensors.copy_(torch.from_numpy(sn))
        tick.plan_in[:, _lib.PL_FOOT_FORCE:].copy_(torch.from_numpy(pin[:, _lib.PL_FOOT_FORCE:]))
        if zero_warm_before == t:
            tick.warm.zero_()
        if use_graph:
            if tick.graph is None:
                tick.capture()
            tick.replay()
        else:
            tick.step()
        torch.cuda.synchronize()
        res = np.frombuffer(tick.results.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE).copy()
        outs.append(dict(res=res, torques=tick.torques.cpu().numpy().copy(), counter=tick.counter.cpu().numpy().copy(),
                         plan_out=tick.plan_out.cpu().numpy().copy(), plan_in=tick.plan_in.cpu().numpy().copy(),
                         states=tick.states.cpu().numpy().copy(), est_out=tick.est_out.cpu().numpy().copy(),
                         est_state=tick.est_state.cpu().numpy().copy()))
    return outs


def test_five_stage_tick_graph_matches_eager_and_oracle(oracle):
    B, T = 512, 14
    states_t, seq, sensors, plan_in = _tick_inputs(B, T)
    J, fkin, _, _ = torque_inputs(B, 3)
    tq = mpcqp.assemble_torque_records(J, fkin, states_t[0].contacts)
    pp, pe = mpcqp.default_plan_params(), mpcqp.default_estimator_params()
    a, b = ControlTick(B, plan=pp, estimator=pe), ControlTick(B, plan=pp, estimator=pe)
    c = ControlTick(B, plan=pp, estimator=pe)
    try:
        assert a.dt == pp.control_dt
        eager = _drive(a, states_t, sensors, plan_in, tq, use_graph=False)
        graph = _drive(b, states_t, sensors, plan_in, tq, use_graph=True)
        # tick 2 solved cold: the warm slots zeroed before it (zero-filled = not initialized yet)
        cold = _drive(c, states_t, sensors[:2], plan_in[:2], tq, use_graph=False, zero_warm_before=1)
    finally:
        a.close()
        b.close()
        c.close()
    for ea, gr in zip(eager, graph):
        np.testing.assert_array_equal(ea["res"]["u0"], gr["res"]["u0"])
        np.testing.assert_array_equal(ea["res"]["iters"], gr["res"]["iters"])
        np.testing.assert_array_equal(ea["res"]["status"], gr["res"]["status"])
        for key in ("torques", "counter"):
            np.testing.assert_array_equal(ea[key], gr[key])
        for key in ("plan_out", "plan_in", "states", "est_out", "est_state"):
            np.testing.assert_array_equal(_bits(ea[key]), _bits(gr[key]), err_msg=key)
    assert eager[-1]["counter"].min() == T and np.abs(eager[-1]["torques"]).max() > 0  # past the 10-tick start-up
    assert not np.isnan(eager[-1]["states"]).any()
    # tick 2 against the oracle's cold solve of records assembled on the host from the restatements' states
    st0 = states_t[0]
    est, plan = ref.Estimator(pe, B), plan_ref.LegPlan(pp, B)
    euler_d = st0.root_euler_d
    for t in range(2):
        w = est.step(pp.control_dt, seq["quat"][t], seq["joint_pos"][t], seq["joint_vel"][t], seq["imu_acc"][t],
                     seq["imu_ang_vel"][t], seq["force"][t], seq["mode"], st0.root_pos, st0.root_lin_vel)
        pw = plan.step(pp.control_dt, w["root_lin_vel"], st0.root_lin_vel_d, w["root_rot_mat"], w["root_pos"],
                       w["foot_pos_abs"], euler_d, w["rot_z"], seq["force"][t], seq["mode"])
        euler_d = pw["root_euler_d"]  # the stage writes root_euler_d[1] in place
    np.testing.assert_array_equal(cold[1]["states"][:, _lib.ST_CONTACTS:_lib.ST_CONTACTS + 4], pw["contacts"])
    st = RobotStates(root_euler=w["root_euler"], root_pos=w["root_pos"], root_ang_vel=w["root_ang_vel"],
                     root_lin_vel=w["root_lin_vel"], root_rot_mat=w["root_rot_mat"], root_euler_d=pw["root_euler_d"],
                     root_pos_d=st0.root_pos_d, root_ang_vel_d=st0.root_ang_vel_d, root_lin_vel_d=st0.root_lin_vel_d,
                     foot_pos_abs=w["foot_pos_abs"], contacts=pw["contacts"].astype(bool), mu=st0.mu)
    ref_res = oracle.solve_batch(oracle.default_params(10), mpcqp.assemble_compute_grf(st, 10), nthreads=8)
    r = cold[1]["res"]
    np.testing.assert_array_equal(r["status"], ref_res["status"])
    err = np.abs(r["u0"] - ref_res["u0"]).max(1) / np.maximum(np.abs(ref_res["u0"]).max(1), 1.0)
    print(f"[note] five-stage tick 2: max u0 rel err {err.max():.3e}")
    assert err.max() <= 1e-4
