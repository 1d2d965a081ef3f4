"""mpcqp_leg_plan_device on the GPU against the numpy restatement (tests/legplan_reference.py):
a bitwise 260-tick sequence, the terrain fit within conditioning-based bounds, that nothing but the
documented fields moves, and the four-stage ControlTick eager against its captured graph."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib, legplan
from mpcqp.records import GO1_DEFAULT_FOOT_POS, RobotStates, rot_zyx, synthetic_go1_ticks
from mpcqp.tick import ControlTick

import legplan_reference as ref
from test_torques import torque_inputs

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DT = 0.0005
PARAM_SETS = {
    "default": {},
    "mixed_speed": dict(gait_counter_speed=[2, 1.5, 2, 1.5], kp_foot=np.tile([250.0, 380.0, 420.0, 310.0], 3),
                        kd_foot=np.tile([6.0, 9.5, 7.25], 4), foot_delta_x_limit=0.08),
}
BITWISE = ("gait_counter", "plan_contacts", "early_contacts", "contacts", "foot_pos_target_rel",
           "foot_pos_target_abs", "foot_pos_target_world", "foot_pos_cur", "foot_pos_target", "foot_forces_kin",
           "foot_pos_recent_contact")


def _sequence(B, T, seed):
    """[T] per-tick inputs: (RobotStates, rot_z, foot_force, movement_mode).  Three standstill ticks,
    then walking; every third robot stands again from tick 150; foot forces mostly under the
    FOOT_FORCE_LOW threshold with spikes above it, some of which fall late in a swing."""
    rng = np.random.default_rng(seed)
    euler = np.stack([rng.uniform(-0.15, 0.15, B), rng.uniform(-0.15, 0.15, B), rng.uniform(-np.pi, np.pi, B)], 1)
    pos = np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(0.25, 0.35, B)], 1)
    v = rng.normal(0.0, 0.4, (B, 3))
    vd = np.stack([rng.uniform(-0.8, 0.8, B), rng.uniform(-0.5, 0.5, B), np.zeros(B)], 1)  # some footholds clamp
    ticks = []
    for t in range(T):
        R = rot_zyx(euler[:, 0], euler[:, 1], euler[:, 2])
        Rz = rot_zyx(np.zeros(B), np.zeros(B), euler[:, 2])
        feet = np.einsum("bij,blj->bli", R, GO1_DEFAULT_FOOT_POS[None] + rng.uniform(-0.03, 0.03, (B, 4, 3)))
        st = RobotStates(root_euler=euler.copy(), root_pos=pos.copy(), root_ang_vel=rng.normal(0.0, 0.2, (B, 3)),
                         root_lin_vel=v.copy(), root_rot_mat=R, root_euler_d=np.tile([0.01, 0.02, 0.03], (B, 1)),
                         root_pos_d=np.tile([0.0, 0.0, 0.3], (B, 1)), root_ang_vel_d=np.zeros((B, 3)),
                         root_lin_vel_d=vd, foot_pos_abs=feet, contacts=np.zeros((B, 4), bool))
        force = rng.uniform(0.0, 28.0, (B, 4)) + 40.0 * (rng.random((B, 4)) < 0.04)
        mode = np.ones(B, dtype=np.int64) if t >= 3 else np.zeros(B, dtype=np.int64)
        if t >= 150:
            mode[::3] = 0
        ticks.append((st, Rz, force, mode))
        pos = pos + v * DT
        euler = euler + rng.normal(0.0, 0.002, (B, 3))
        euler[:, :2] = np.clip(euler[:, :2], -0.2, 0.2)
        v = v + rng.normal(0.0, 0.02, (B, 3))
    return ticks


def _ref_step(plan, dt, st, rz, force, mode):
    return plan.step(dt, st.root_lin_vel, st.root_lin_vel_d, st.root_rot_mat, st.root_pos, st.foot_pos_abs,
                     st.root_euler_d, rz, force, mode)


@functools.lru_cache(maxsize=None)
def _sequence_and_reference(B, T, seed, pset):
    ticks = _sequence(B, T, seed)
    p = mpcqp.default_plan_params(**PARAM_SETS[pset])
    plan = ref.LegPlan(p, B)
    return ticks, p, [_ref_step(plan, DT, *tk) for tk in ticks]


def _run(p, ticks, tq0=None, dt=DT, with_out=True, pad=0):
    """One launch per tick on inputs uploaded once as [T][B][..]; returns the downloaded per-tick
    state rows, torque records and output rows (rows beyond B are NaN sentinels when pad > 0)."""
    T, B = len(ticks), ticks[0][0].batch
    nan = float("nan")
    states = np.full((T, B + pad, _lib.ST_SIZE), nan)
    pin = np.full((T, B + pad, _lib.PL_SIZE), nan)
    for t, (st, rz, force, mode) in enumerate(ticks):
        states[t, :B] = mpcqp.pack_states(st)
        pin[t, :B] = mpcqp.pack_plan_inputs(rz, force, mode)
    d_states, d_in = torch.from_numpy(states).cuda(), torch.from_numpy(pin).cuda()
    d_slot = torch.zeros((B + pad, mpcqp.plan_state_size()), dtype=torch.float64, device="cuda")
    if pad:
        d_slot[B:] = nan
    d_tq = d_out = None
    if tq0 is not None:
        d_tq = torch.from_numpy(np.broadcast_to(tq0, (T,) + tq0.shape).copy()).cuda()
    if with_out:
        d_out = torch.full((T, B + pad, _lib.PO_SIZE), nan, dtype=torch.float64, device="cuda")
    outs = []
    s = torch.cuda.current_stream().cuda_stream
    for t in range(T):
        mpcqp.leg_plan_device(p, dt, d_states[t].data_ptr(), d_in[t].data_ptr(), B, d_slot.data_ptr(),
                              d_tq[t].data_ptr() if d_tq is not None else 0,
                              d_out[t].data_ptr() if d_out is not None else 0, s)
        if d_out is not None:
            torch.cuda.synchronize()
            outs.append(d_out[t].cpu().numpy())  # downloaded per tick
    torch.cuda.synchronize()
    out = np.stack(outs).view(legplan.PLAN_OUT_DTYPE)[..., 0] if outs else None
    return dict(states_in=states, states=d_states.cpu().numpy(), tq=None if d_tq is None else d_tq.cpu().numpy(),
                out=out, out_raw=np.stack(outs) if outs else None, slot=d_slot.cpu().numpy())


@pytest.mark.parametrize("pset", list(PARAM_SETS))
@pytest.mark.parametrize("B", [1, 67])
def test_sequence_is_bitwise_the_restatement(B, pset):
    T = 260
    ticks, p, want = _sequence_and_reference(B, T, 11 + B, pset)
    J, fkin, contacts, _ = torque_inputs(B, 4)
    tq0 = mpcqp.assemble_torque_records(J, fkin, contacts)
    got = _run(p, ticks, tq0)
    seen_early = sum(w["early_contacts"].sum() for w in want)
    clamped = sum((np.abs(w["foot_pos_target_rel"][:, :, 0] - np.array(p.default_foot_pos).reshape(4, 3)[:, 0])
                   == p.foot_delta_x_limit).sum() for w in want)
    if B > 1:
        assert seen_early > 0 and clamped > 0  # the inputs reach the early-contact and clamp branches
    for t in range(T):
        for name in BITWISE:
            np.testing.assert_array_equal(got["out"][name][t], want[t][name], err_msg=f"tick {t} {name}")
        np.testing.assert_array_equal(got["states"][t, :, _lib.ST_CONTACTS:_lib.ST_CONTACTS + 4], want[t]["contacts"])
        np.testing.assert_array_equal(got["tq"][t, :, _lib.TQ_CONTACTS:_lib.TQ_CONTACTS + 4], want[t]["contacts"])
        np.testing.assert_array_equal(got["tq"][t, :, _lib.TQ_FKIN:_lib.TQ_FKIN + 12].reshape(B, 4, 3),
                                      want[t]["foot_forces_kin"], err_msg=f"tick {t} TQ_FKIN")


def _terrain_sequence(T, seed):
    """Standing / walking robots whose feet lie on planes z = a0 + a1 x + a2 y (body-origin frame):
    slopes with a dihedral angle in [0.05, 0.45] uphill and downhill, a flat fleet, robots that are
    low (root_pos_z <= 0.1) always or for the first 30 ticks, and one robot with all-zero feet."""
    rng = np.random.default_rng(seed)
    theta = np.concatenate([np.linspace(0.05, 0.45, 9), np.linspace(0.45, 0.05, 9), np.zeros(4)])
    B = theta.size + 1
    heading = rng.uniform(-0.5, 0.5, B - 1) + np.where(np.arange(B - 1) % 2 == 0, 0.0, np.pi)  # up / down along x
    slope = np.tan(theta)
    a1, a2 = slope * np.cos(heading), slope * np.sin(heading)
    low_always = np.zeros(B, bool)
    low_always[[3, 20]] = True
    low_start = np.zeros(B, bool)
    low_start[[5, 12, 19]] = True
    zero_feet = B - 1
    ticks = []
    for t in range(T):
        xy = GO1_DEFAULT_FOOT_POS[None, :, :2] + rng.uniform(-0.03, 0.03, (B, 4, 2))
        feet = np.zeros((B, 4, 3))
        feet[:, :, :2] = xy
        feet[:-1, :, 2] = -0.3 + a1[:, None] * xy[:-1, :, 0] + a2[:, None] * xy[:-1, :, 1]
        feet[zero_feet] = 0.0
        pz = np.where(low_always | (low_start & (t < 30)), 0.08, 0.3)
        eye = np.broadcast_to(np.eye(3), (B, 3, 3)).copy()
        st = RobotStates(root_euler=np.zeros((B, 3)), root_pos=np.stack([np.zeros(B), np.zeros(B), pz], 1),
                         root_ang_vel=np.zeros((B, 3)), root_lin_vel=np.tile([0.2, 0.0, 0.0], (B, 1)), root_rot_mat=eye,
                         root_euler_d=np.tile([0.0, 0.125, 0.0], (B, 1)), root_pos_d=np.tile([0.0, 0.0, 0.3], (B, 1)),
                         root_ang_vel_d=np.zeros((B, 3)), root_lin_vel_d=np.tile([0.2, 0.0, 0.0], (B, 1)),
                         foot_pos_abs=feet, contacts=np.zeros((B, 4), bool))
        mode = np.full(B, 1 if t >= 2 else 0)
        mode[zero_feet] = 0  # standing: all four (zero) feet are recorded every tick
        ticks.append((st, eye, rng.uniform(0.0, 25.0, (B, 4)), mode))
    return ticks, theta, low_always, low_start, zero_feet


def test_terrain_fit_within_conditioning_bounds():
    """Tolerances, all from reference quantities.  kappa = cond_2(W'W) from numpy per robot-tick.

    plane:  |a - a_ref|_inf <= da := 16 kappa eps max(|a_ref|_inf, 1)  (normal equations solved by a
            backward-stable symmetric eigen-solver against numpy's SVD pinv).
    cos:    c(a) = (1 + a1^2 + a2^2)^(-1/2), |grad c|_2 = |a|_2 c^3 <= |a|_2, so with |d|_2 <= sqrt2 da
            |c - c_ref| <= dc := (|a_ref|_2 + sqrt2 da) sqrt2 da + 4 eps.
    angle:  acos is concave and decreasing on [0, 1], so for a gap h the largest change is at the end
            point 1: |acos x - acos y| <= acos(1 - h) = 2 asin(sqrt(h / 2)) =: H(h), the Hoelder-1/2
            bound used near zero.  Away from zero both angles lie in [theta_ref - H, pi/2], where
            |acos'| = 1 / sin(theta) <= 1 / sin(theta_ref - H): dtheta := min(H, dc / sin(theta_ref - H))
            + 4 eps for acos' own rounding.
    filter: terrain_pitch_angle is the sum of the window's raw angles over 100, clamped (1-Lipschitz):
            the sum of the window's dtheta over 100, + 16 eps for the Neumaier sums' own rounding.
            ST_EULER_D[1] is +-that; its sign comes from foot_pos_recent_contact, which is bitwise."""
    T = 130  # wraps the 100-tick terrain window (and the 60-tick contact windows)
    ticks, theta, low_always, low_start, zero_feet = _terrain_sequence(T, 3)
    B = theta.size + 1
    p = mpcqp.default_plan_params()
    plan = ref.LegPlan(p, B)
    want = [_ref_step(plan, DT, *tk) for tk in ticks]
    got = _run(p, ticks)
    fit = np.ones(B, bool)
    fit[zero_feet] = False
    window = [[] for _ in range(B)]
    flips = set()
    worst = dict(plane=0.0, cos=0.0, angle=0.0)
    for t in range(T):
        w, g = want[t], got["out"][t]
        np.testing.assert_array_equal(g["foot_pos_recent_contact"], w["foot_pos_recent_contact"])
        kappa = w["cond"][fit]
        assert np.all(kappa <= 1e6), (t, kappa.max())
        a_ref = w["plane"][fit]
        da = 16 * kappa * EPS * np.maximum(np.abs(a_ref).max(1), 1.0)
        err_a = np.abs(g["plane"][fit] - a_ref).max(1)
        dc = (np.hypot(a_ref[:, 1], a_ref[:, 2]) + np.sqrt(2) * da) * np.sqrt(2) * da + 4 * EPS
        err_c = np.abs(g["angle_cos"][fit] - w["angle_cos"][fit])
        hoelder = 2 * np.arcsin(np.sqrt(np.minimum(dc, 1.0) / 2))
        away = w["raw_angle"][fit] > hoelder
        with np.errstate(divide="ignore", invalid="ignore"):
            lipschitz = np.where(away, dc / np.sin(np.where(away, w["raw_angle"][fit] - hoelder, 1.0)), np.inf)
        dtheta = np.minimum(hoelder, lipschitz) + 4 * EPS
        high = ticks[t][0].root_pos[:, 2] > 0.1
        tol = np.zeros(B)
        for i, b in enumerate(np.flatnonzero(fit)):
            if high[b]:
                window[b] = (window[b] + [dtheta[i]])[-100:]
            tol[b] = sum(window[b]) / 100 + 16 * EPS
        err_t = np.abs(g["terrain_pitch_angle"] - w["terrain_pitch_angle"])
        err_e = np.abs(got["states"][t, :, _lib.ST_EULER_D + 1] - w["root_euler_d"][:, 1])
        worst["plane"] = max(worst["plane"], (err_a / da).max())
        worst["cos"] = max(worst["cos"], (err_c / dc).max())
        worst["angle"] = max(worst["angle"], (np.maximum(err_t, err_e)[fit] / tol[fit]).max())
        assert np.all(err_a <= da), (t, err_a / da)
        assert np.all(err_c <= dc), (t, err_c / dc)
        assert np.all(err_t[fit] <= tol[fit]) and np.all(err_e[fit] <= tol[fit]), (t, err_t[fit] / tol[fit])
        # low robots report exactly 0 and write +-0 (here +0: |F_R_diff| of a low-window robot varies)
        low = ~high
        assert np.all(g["terrain_pitch_angle"][low] == 0.0)
        assert np.all(got["states"][t, low, _lib.ST_EULER_D + 1] == 0.0)
        # all-zero recent contacts: W'W = diag(4, 0, 0), a = 0, cos = 1, angle exactly 0
        assert np.all(w["foot_pos_recent_contact"][zero_feet] == 0.0)
        assert np.all(g["plane"][zero_feet] == 0.0) and g["angle_cos"][zero_feet] == 1.0
        assert g["terrain_pitch_angle"][zero_feet] == 0.0 and got["states"][t, zero_feet, _lib.ST_EULER_D + 1] == 0.0
        for b in np.flatnonzero(fit & high & (w["terrain_pitch_angle"] > 1e-3)):
            flips.add(bool(w["f_r_diff"][b] > 0.05))
        # the other components of root_euler_d stay
        np.testing.assert_array_equal(got["states"][t, :, [_lib.ST_EULER_D, _lib.ST_EULER_D + 2]],
                                      got["states_in"][t, :, [_lib.ST_EULER_D, _lib.ST_EULER_D + 2]])
    print(f"[note] terrain error / bound: {worst}")
    assert flips == {True, False}  # root_euler_d[1] = -angle and +angle both exercised
    # a robot that was low for its first 30 ticks started its window then: its later ticks show it
    b = np.flatnonzero(low_start)[0]
    first = want[30]["raw_angle"][b] / 100
    assert abs(got["out"][30]["terrain_pitch_angle"][b] - first) <= window[b][0] / 100 + 16 * EPS and first > 1e-4
    assert np.all(got["out"]["terrain_pitch_angle"][:, low_always] == 0.0)

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("flags", [dict(), dict(terrain=0), dict(use_terrain_adapt=0)])
def test_nothing_else_moves(flags):
    B, T, pad = 5, 4, 2
    ticks = _sequence(B, T, 21)
    p = mpcqp.default_plan_params(**flags)
    J, fkin, contacts, _ = torque_inputs(B, 6)
    tq0 = np.full((B + pad, _lib.TQ_SIZE), float("nan"))
    tq0[:B] = mpcqp.assemble_torque_records(J, fkin, contacts)
    got = _run(p, ticks, tq0, pad=pad)
    st_moves = np.zeros(_lib.ST_SIZE, bool)
    st_moves[_lib.ST_CONTACTS:_lib.ST_CONTACTS + 4] = True
    if not flags:
        st_moves[_lib.ST_EULER_D + 1] = True
    tq_moves = np.zeros(_lib.TQ_SIZE, bool)
    tq_moves[_lib.TQ_FKIN:_lib.TQ_FKIN + 12] = True
    tq_moves[_lib.TQ_CONTACTS:_lib.TQ_CONTACTS + 4] = True
    np.testing.assert_array_equal(_bits(got["states"])[:, :B, ~st_moves], _bits(got["states_in"])[:, :B, ~st_moves])
    np.testing.assert_array_equal(_bits(got["tq"])[:, :B, ~tq_moves],
                                  _bits(np.broadcast_to(tq0, got["tq"].shape))[:, :B, ~tq_moves])
    assert not np.isnan(got["states"][:, :B, st_moves]).any() and not np.isnan(got["tq"][:, :B, tq_moves]).any()
    if not flags:
        assert np.any(got["states"][:, :B, _lib.ST_EULER_D + 1] != 0.02)  # the adapted pitch was written
    else:
        assert np.all(got["states"][:, :B, _lib.ST_EULER_D + 1] == 0.02)
    if flags.get("terrain") == 0:
        assert np.all(got["out"]["plane"][:, :B] == 0.0) and np.all(got["out"]["terrain_pitch_angle"][:, :B] == 0.0)
    # NaN sentinel rows beyond batch are untouched, in every buffer
    assert np.isnan(got["states"][:, B:]).all() and np.isnan(got["tq"][:, B:]).all()
    assert np.isnan(got["out_raw"][:, B:]).all() and np.isnan(got["slot"][B:]).all()
    # optional outputs left out: the state rows and the slot come out the same
    bare = _run(p, ticks, None, with_out=False, pad=pad)
    np.testing.assert_array_equal(_bits(bare["states"]), _bits(got["states"]))
    np.testing.assert_array_equal(_bits(bare["slot"]), _bits(got["slot"]))


def test_argument_checks_on_the_device():
    L, p = _lib.load(), mpcqp.default_plan_params()
    B = 3
    st = torch.zeros((B, _lib.ST_SIZE), dtype=torch.float64, device="cuda")
    pin = torch.zeros((B, _lib.PL_SIZE), dtype=torch.float64, device="cuda")
    slot = torch.zeros((B, mpcqp.plan_state_size()), dtype=torch.float64, device="cuda")
    vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    call = lambda pp, dt, a, b, n, c: L.mpcqp_leg_plan_device(pp, dt, vp(a), vp(b), n, vp(c), None, None, None)
    assert call(ctypes.byref(p), DT, st, pin, 0, slot) == _lib.ERR_OK
    assert call(ctypes.byref(p), DT, None, None, 0, None) == _lib.ERR_OK
    torch.cuda.synchronize()
    assert not slot.any() and not st.any()  # batch == 0 launched nothing
    assert call(None, DT, st, pin, B, slot) == _lib.ERR_INVALID_ARG
    assert call(ctypes.byref(p), DT, st, pin, -1, slot) == _lib.ERR_INVALID_ARG
    for dt in (0.0, -DT, float("nan"), float("inf")):
        assert call(ctypes.byref(p), dt, st, pin, B, slot) == _lib.ERR_INVALID_ARG
    for a, b, c in ((None, pin, slot), (st, None, slot), (st, pin, None)):
        assert call(ctypes.byref(p), DT, a, b, B, c) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not slot.any()
    assert call(ctypes.byref(p), DT, st, pin, B, slot) == _lib.ERR_OK
    torch.cuda.synchronize()
    assert slot.any(dim=1).all()  # every robot's slot left the reset state


def _drive(tick, states_t, plan_in_t, tq, use_graph):
    outs = []
    tick.tq_records.copy_(torch.from_numpy(tq))
    for st, pin in zip(states_t, plan_in_t):
        tick.states.copy_(torch.from_numpy(mpcqp.pack_states(st)))
        tick.plan_in.copy_(torch.from_numpy(pin))
        if use_graph:
            if tick.graph is None:
                tick.capture()
            tick.replay()
        else:
            tick.step()
        torch.cuda.synchronize()
        res = np.frombuffer(tick.results.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE).copy()
        outs.append((res, tick.torques.cpu().numpy().copy(), tick.counter.cpu().numpy().copy(),
                     tick.plan_out.cpu().numpy().copy(), tick.states.cpu().numpy().copy()))
    return outs


def test_four_stage_tick_graph_matches_eager_and_oracle(oracle):
    B, T = 512, 14
    states_t = synthetic_go1_ticks(B, T, seed=8, gait="stance")
    rng = np.random.default_rng(9)
    rot_z = [rot_zyx(np.zeros(B), np.zeros(B), st.root_euler[:, 2]) for st in states_t]
    force = rng.uniform(0.0, 60.0, (T, B, 4))
    mode = (np.arange(B) % 4 != 0).astype(np.int64)  # three in four walk from the first tick
    plan_in_t = [mpcqp.pack_plan_inputs(rot_z[t], force[t], mode) for t in range(T)]
    J, fkin, _, _ = torque_inputs(B, 3)
    tq = mpcqp.assemble_torque_records(J, fkin, states_t[0].contacts)
    p = mpcqp.default_plan_params()
    a, b = ControlTick(B, plan=p), ControlTick(B, plan=p)
    try:
        assert a.dt == p.control_dt
        eager = _drive(a, states_t, plan_in_t, tq, use_graph=False)
        graph = _drive(b, states_t, plan_in_t, tq, use_graph=True)
    finally:
        a.close()
        b.close()
    for (ra, ta, ca, pa, sa), (rb, tb, cb, pb, sb) in zip(eager, graph):
        np.testing.assert_array_equal(ra["u0"], rb["u0"])
        np.testing.assert_array_equal(ra["iters"], rb["iters"])
        np.testing.assert_array_equal(ta, tb)
        np.testing.assert_array_equal(ca, cb)
        np.testing.assert_array_equal(_bits(pa), _bits(pb))
        np.testing.assert_array_equal(_bits(sa), _bits(sb))
    assert eager[-1][2].min() == T and np.abs(eager[-1][1]).max() > 0  # past the 10-tick start-up
    # tick 1 against the restatement and the oracle's cold solve of host-assembled records
    st0 = states_t[0]
    w = _ref_step(ref.LegPlan(p, B), p.control_dt, st0, rot_z[0], force[0], mode)
    out0 = eager[0][3].view(legplan.PLAN_OUT_DTYPE)[:, 0]
    np.testing.assert_array_equal(out0["contacts"], w["contacts"])
    np.testing.assert_array_equal(eager[0][4][:, _lib.ST_CONTACTS:_lib.ST_CONTACTS + 4], w["contacts"])
    assert 0 < w["contacts"].sum() < 4 * B
    st0.contacts = w["contacts"].astype(bool)
    st0.root_euler_d = w["root_euler_d"]
    ref_res = oracle.solve_batch(oracle.default_params(10), mpcqp.assemble_compute_grf(st0, 10), nthreads=8)
    r0 = eager[0][0]
    np.testing.assert_array_equal(r0["status"], ref_res["status"])
    err = np.abs(r0["u0"] - ref_res["u0"]).max(1) / np.maximum(np.abs(ref_res["u0"]).max(1), 1.0)
    assert err.max() <= 1e-4
