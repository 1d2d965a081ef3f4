"""The rigid-body plant model on the CPU: tests/plant_reference.py against closed forms and, in closed loop,
against the oracle's MPC.  No device."""
import ctypes
import re

import numpy as np
import pytest

import mpcqp
from mpcqp import _lib

import estimator_reference as er
import plant_reference as pr

DT = 0.0025


def test_default_params_and_sizes_agree_with_the_library():
    p = mpcqp.default_plant_params()
    r = pr.default_params()
    assert _lib.load().mpcqp_plant_params_size() == ctypes.sizeof(mpcqp.PlantParams)
    for k in ("rho_fix", "rho_opt", "inertia", "joint_inertia", "joint_damping", "default_joint_pos"):
        assert list(getattr(p, k)) == list(getattr(r, k)), k
    for k in ("mass", "mu", "gravity", "min_height", "substeps"):
        assert getattr(p, k) == getattr(r, k), k
    e = mpcqp.default_estimator_params()
    assert list(p.rho_fix) == list(e.rho_fix) and list(p.rho_opt) == list(e.rho_opt)
    assert p.mass == mpcqp.records.GO1_MASS and list(p.inertia) == list(mpcqp.records.GO1_INERTIA.reshape(9))
    assert mpcqp.plant_state_size() == pr.PN_SIZE == 64
    hdr = open(_lib.PKG_ROOT + "/../include/mpcqp.h").read()
    for name in ("PN_INIT", "PN_POS", "PN_QUAT", "PN_LIN_VEL", "PN_ANG_VEL", "PN_JOINT_POS", "PN_JOINT_VEL", "PN_FOOT",
                 "PN_CONTACT", "PN_ACC", "PN_STATUS", "PN_SIZE", "PI_POS", "PI_QUAT", "PI_JOINT_POS", "PI_SIZE",
                 "PT_POS", "PT_QUAT", "PT_EULER", "PT_LIN_VEL", "PT_ANG_VEL", "PT_CONTACTS", "PT_GRF", "PT_FOOT",
                 "PT_ACC", "PT_STATUS", "PT_SIZE"):
        assert re.search(rf"^#define MPCQP_{name} {getattr(pr, name)}\s", hdr, flags=re.M), name
        assert getattr(_lib, name) == getattr(pr, name), name


def test_invalid_arguments_need_no_device():
    L = _lib.load()
    p = mpcqp.default_plant_params()
    call = L.mpcqp_plant_step_device
    assert call(None, DT, 8, 1, 8, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), 0.0, 8, 1, 8, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), DT, None, 1, 8, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), DT, 8, 1, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), DT, 8, -1, 8, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    for n in (0, 17):
        bad = mpcqp.default_plant_params(substeps=n)
        assert call(ctypes.byref(bad), DT, 8, 1, 8, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), DT, None, 0, None, None, None, None, None, None, None, None) == _lib.ERR_OK


@pytest.mark.parametrize("rho_opt", [(0.0, 0.0, 0.0), (0.004, -0.003, 0.005)])
def test_ik_inverts_fk(rho_opt):
    """1. 2e5 poses per leg over the working domain: |IK(fk(q)) - q| <= 1e-12."""
    p = pr.default_params(rho_opt=list(rho_opt) * 4)
    ro, rf = pr._geom(p)
    rng = np.random.Generator(np.random.PCG64(11))
    n = 200000
    q = np.stack([rng.uniform(-0.6, 0.6, (n, 4)), rng.uniform(0.2, 1.4, (n, 4)), rng.uniform(-2.4, -1.0, (n, 4))], -1)
    back, ok, margin = pr.ik(er.fk(q, ro, rf), ro, rf)
    err = np.max(np.abs(back - q))
    print(f"IK o FK: max |dq| {err:.3e}, smallest reach margin {margin.min():.3e}")
    assert np.all(ok)
    assert err <= 1e-12


def test_free_fall_is_the_closed_form():
    """2. all feet in swing, zero torques, 40 ticks of 2.5 ms at 4 substeps: z = z0 - g h^2 n (n + 1) / 2."""
    p = pr.default_params()
    init = np.zeros((1, pr.PI_SIZE))
    init[0, pr.PI_POS + 2] = 1.0
    init[0, pr.PI_QUAT] = 1.0
    init[0, pr.PI_JOINT_POS:pr.PI_JOINT_POS + 12] = p.default_joint_pos
    pl = pr.Plant(p, 1)
    pl.step(DT, np.zeros((1, 12)), init)
    h = DT / p.substeps
    worst = 0.0
    for t in range(1, 41):
        out, wrote, _ = pl.step(DT, np.zeros((1, 12)), init)
        n = t * p.substeps
        worst = max(worst, abs(out["root_pos"][0, 2] - (1.0 - p.gravity * h * h * n * (n + 1) / 2.0)))
        assert wrote[0] and not out["contacts"].any() and out["status"][0] == 0.0
    print(f"free fall: max |z - closed form| {worst:.3e}")
    assert worst <= 1e-12


def stance_torques(p, out):
    """tau = J^T (-R^T (0, 0, m g / 4)) per leg from a tick's rows."""
    R = out["root_rot_mat"]
    fb = pr.mat_t_vec(R, np.broadcast_to(np.array([0.0, 0.0, p.mass * p.gravity / 4.0]), (R.shape[0], 3)))
    return np.einsum("blji,bj->bli", out["j_foot"], -fb).reshape(-1, 12)


def test_static_equilibrium_holds():
    """3. default stance with the weight-bearing torques recomputed every tick, 200 ticks."""
    p = pr.default_params()
    pl = pr.Plant(p, 1)
    out, _, _ = pl.step(DT, np.zeros((1, 12)))
    pos0 = out["root_pos"].copy()
    assert out["contacts"].all() and np.all(out["foot_world"][..., 2] == 0.0)
    np.testing.assert_allclose(out["imu_acc"][0], [0.0, 0.0, p.gravity], atol=1e-15)
    dp = dv = dw = 0.0
    for _ in range(200):
        out, wrote, _ = pl.step(DT, stance_torques(p, out))
        assert wrote[0] and out["contacts"].all() and out["status"][0] == 0.0
        dp = max(dp, np.abs(out["root_pos"] - pos0).max())
        dv = max(dv, np.abs(out["root_lin_vel"]).max())
        dw = max(dw, np.abs(out["imu_ang_vel"]).max())
    print(f"static equilibrium: |dpos| {dp:.3e} |v| {dv:.3e} |w| {dw:.3e}")
    assert dp <= 1e-10 and dv <= 1e-10 and dw <= 1e-9
    np.testing.assert_allclose(out["foot_force"][0], p.mass * p.gravity / 4.0, rtol=1e-12)


def tilted_fleet(seed=5, B=8):
    """Test 4's start: level stance at a random yaw, the trunk then tilted by roll, pitch in +-0.08 about its
    own origin with the feet held: init rows [B, PI_SIZE] and the (roll, pitch, yaw) they encode."""
    p = pr.default_params()
    ro, rf = pr._geom(p)
    rng = np.random.Generator(np.random.PCG64(seed))
    yaw = rng.uniform(-np.pi, np.pi, B)
    roll = rng.uniform(-0.08, 0.08, B)
    pitch = rng.uniform(-0.08, 0.08, B)
    q0 = np.broadcast_to(np.array(p.default_joint_pos).reshape(1, 4, 3), (B, 4, 3))
    pb = er.fk(q0, ro, rf)
    z0 = -pb[:, 0, 2]
    pos = np.stack([np.zeros(B), np.zeros(B), z0], 1)
    Rz = mpcqp.records.rot_zyx(np.zeros(B), np.zeros(B), yaw)
    feet_w = pos[:, None] + np.einsum("bij,blj->bli", Rz, pb)
    feet_w[..., 2] = 0.0
    R = mpcqp.records.rot_zyx(roll, pitch, yaw)
    q, ok, _ = pr.ik(np.einsum("bji,blj->bli", R, feet_w - pos[:, None]), ro, rf)
    assert np.all(ok)
    cr, sr, cp, sp, cy, sy = (f(a / 2) for a in (roll, pitch, yaw) for f in (np.cos, np.sin))
    quat = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy], 1)
    init = np.zeros((B, pr.PI_SIZE))
    init[:, pr.PI_POS:pr.PI_POS + 3] = pos
    init[:, pr.PI_QUAT:pr.PI_QUAT + 4] = quat
    init[:, pr.PI_JOINT_POS:pr.PI_JOINT_POS + 12] = q.reshape(B, 12)
    # the IK puts a held foot back to z = 0 only to rounding: lift the trunk by the deepest foot's error so
    # every foot starts at z <= 0 exactly once clamped (a foot a few 1e-17 above the ground would start in swing)
    foot = pos[:, None] + np.einsum("bij,blj->bli", er.quat_to_rot(quat), er.fk(q, ro, rf))
    init[:, pr.PI_POS + 2] -= np.maximum(foot[..., 2].max(1), 0.0) + 1e-15
    return init, np.stack([roll, pitch, yaw], 1)


def truth_states(out, pos_d, euler_d):
    B = out["root_pos"].shape[0]
    z = np.zeros((B, 3))
    return mpcqp.RobotStates(
        root_euler=out["root_euler"], root_pos=out["root_pos"], root_ang_vel=out["root_ang_vel"],
        root_lin_vel=out["root_lin_vel"], root_rot_mat=out["root_rot_mat"], root_euler_d=euler_d, root_pos_d=pos_d,
        root_ang_vel_d=z, root_lin_vel_d=z, foot_pos_abs=out["foot_pos_abs"], contacts=np.ones((B, 4), dtype=bool),
        mu=np.full(B, 0.3))


def closed_loop_conditions(tilt0, tilt1, fz_ratio, dz, statuses, contacts):
    """The five conditions of the closed-loop test, shared with its device twin."""
    assert np.all(statuses == _lib.STATUS_SOLVED)
    assert np.all(contacts)
    assert np.all(tilt1 <= 0.5 * tilt0), (tilt1 / tilt0)
    assert np.all(np.abs(fz_ratio - 1.0) <= 0.01), fz_ratio
    assert np.all(np.abs(dz) <= 0.01), dz


def test_closed_loop_with_the_oracle_mpc(oracle):
    """4. eight tilted robots under the oracle's MPC fed the plant's true state, 400 ticks, substeps 1 / 4."""
    init, rpy = tilted_fleet()
    B = init.shape[0]
    op = oracle.default_params(10)
    idx = [np.arange(0, B, 2), np.arange(1, B, 2)]  # substeps 1 on the even robots, 4 on the odd ones
    plants = [pr.Plant(pr.default_params(substeps=n), len(i)) for n, i in zip((1, 4), idx)]
    solvers = [oracle.WarmSolver(op) for _ in range(B)]
    pos_d = init[:, pr.PI_POS:pr.PI_POS + 3].copy()
    euler_d = np.stack([np.zeros(B), np.zeros(B), rpy[:, 2]], 1)
    tau = np.zeros((B, 12))
    tilt0 = np.hypot(rpy[:, 0], rpy[:, 1])
    statuses, contacts, fz, z = [], [], [], []
    mg = plants[0].p.mass * plants[0].p.gravity
    for t in range(401):
        outs = [pl.step(DT, tau[i], init[i])[0] for pl, i in zip(plants, idx)]
        out = {}
        for k in outs[0]:
            out[k] = np.zeros((B,) + outs[0][k].shape[1:], dtype=outs[0][k].dtype)
            for o, i in zip(outs, idx):
                out[k][i] = o[k]
        assert np.all(out["status"] == 0.0), (t, out["status"])
        contacts.append(out["contacts"].copy())
        if t > 0:
            fz.append(out["grf"][..., 2].sum(1) / mg)
            z.append(out["root_pos"][:, 2].copy())
        recs = mpcqp.assemble_compute_grf(truth_states(out, pos_d, euler_d), 10)
        res = np.array([sv.step(recs[b])[0] for b, sv in enumerate(solvers)])
        statuses.append(res["status"].copy())
        fb = res["f_body"].reshape(B, 4, 3)
        tau = np.einsum("blji,blj->bli", out["j_foot"], -fb).reshape(B, 12)
    for sv in solvers:
        sv.close()
    tilt1 = np.hypot(out["root_euler"][:, 0], out["root_euler"][:, 1])
    fz, z = np.array(fz), np.array(z)
    print(f"closed loop: tilt ratio {np.round(tilt1 / tilt0, 4)} Fz/mg {fz.min():.5f}..{fz.max():.5f} "
          f"max |dz| {np.abs(z - pos_d[:, 2]).max():.3e}")
    closed_loop_conditions(tilt0, tilt1, fz[-1], z[-1] - pos_d[:, 2], np.array(statuses), np.array(contacts))
