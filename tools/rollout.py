"""Closed-loop rollouts of a fleet on the device: ControlTick(plant=) replayed T times with no host write in
between, for three ticks, each under standing commands:

  mpc     the MPC-only tick fed the plant's true state (no estimator; zero gravity-compensation torques, the
          setup of tests/test_plant.py's closed loop), robots started 0.03 to 0.09 rad off level
  full    command + estimator + plan + MPC on the plant's sensor rows, robots started 0.05 rad off level at
          most, at the command stage's body height
  servo   the policy stage in servo stand (control type 2; the network never runs), robots started in the
          plant's default stance
  servo_walk_gains   (not in the default list) the same with the walk mode's gains (20 / 50 / 50, 1 / 2 / 2) in
          place of the servo gains

and, with the episode stage as the tick's last stage (ControlTick(episode=): on-device resets from a pool of start
rows, a time-out, an envelope; not in the default list), four more:

  mpc_ep     the mpc setup; every robot that leaves the standing envelope or times out is restarted on the device
  full_ep    the full setup, likewise
  full_walk  the full setup under a script that toggles walk mode and commands 0.3 m/s forward at episode tick 100
  servo_ep   the servo setup: the fleet that sinks and falls, restarted and counted

and, with the disturbance stage as the tick's first stage (ControlTick(disturb=)), two more on the full_ep setup:

  full_push  one push per episode: PUSH_TICKS ticks long, starting at a drawn tick from episode tick PUSH_START on,
             of a magnitude uniform in PUSH_FORCE, in one of 16 horizontal directions, at the centre of mass.  Its
             line carries the push-recovery curve: per push-magnitude bin, the share of logged episodes ended by
             the envelope or a plant status, from the log rows and mpcqp.disturbance_of
  full_noise sensor noise NOISE_SIGMA (joint angles, joint rates, accelerometer, gyro) and IMU biases up to
             NOISE_BIAS per axis, redrawn every episode

and, with the plant's ground as a terrain table parallel to the pool (ControlTick(terrain=): a robot's ground and
friction restart with its start pose), three more:

  mpc_slope  the mpc_ep setup standing slope-parallel on a grid of SLOPE_GRID x SLOPE_GRID pitch / roll angles in
             +-SLOPE_MAX rad at mu 0.6, the envelope widened to hold the tilted stance
  full_slope the full_walk setup (standing, then WALK_VX m/s forward from episode tick WALK_AT) on the same pool, the
             height envelope widened by SLOPE_HEIGHT for the climb.  Its line carries, per pool row, the median
             MPCQP_PO_ANGLE (the plan stage's filtered terrain pitch) of the robots on that row after the last replay
             beside the ground's pitch along each robot's heading, and the root_euler_d[1] the plan stage wrote
  full_mu    the full_walk setup on level ground whose mu is MU_SET[row % 4]; its line carries the end reasons per mu

and, with the plant's ground as a height-field table parallel to the pool (ControlTick(field=)), two more:

  mpc_field  the mpc_ep setup standing level on a pool of start poses at random places and headings on three tiles:
             rolling ground of 3 cm amplitude, a 5 cm step and stairs of 8 cm (one-cell risers of 5 cm), the height
             envelope widened to the pool's trunk heights.  Its line carries the end reasons per tile
  full_steps the full_walk setup heading for a step of STEP_SET[row % 5] m whose riser lies STEP_AHEAD m in front of
             the front feet; its line carries, per step height, the end reasons and the distance walked

These report episodes completed, the end-reason histogram, ticks/s and medians of the logged episodes' metrics
from the device's totals and log, read once after the last replay; they never rerun with a read per tick.

Per form of the first kind: ticks/s over the timed replays (HIP events around chunks of replays; the host only reads between
chunks), how many robots ended with a plant status != 0, and how many are out of a standing envelope (tilt >
0.3 rad, or the trunk more than 5 cm from where standing should hold it).  If any robot went wrong the form is
run once more with a read after every tick to find the first tick at which it did.
usage: python tools/rollout.py [--batch 4096] [--ticks 2000] [--forms mpc full servo]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "go1-qp-mpc-controller_amd"), os.path.join(REPO, "tests"),
                os.path.join(REPO, "tools")]
import mpcqp  # noqa: E402
from mpcqp import _lib  # noqa: E402
from mpcqp.tick import ControlTick  # noqa: E402
import estimator_reference as er  # noqa: E402  (fk, to place the start poses)
from policy_bench import seeded_weights  # noqa: E402
from time_estimator import quat_zyx  # noqa: E402

DT = 0.0025
CHUNK = 50


def start_rows(B, q_leg, tilt, seed):
    """Init rows: every leg at q_leg, the trunk tilted by roll, pitch in +-tilt at a random yaw, lowered so
    the deepest foot is 1 um under the ground (held from the start)."""
    pp = mpcqp.default_plant_params()
    rho_opt = np.array(pp.rho_opt).reshape(1, 4, 3)
    rho_fix = np.array(pp.rho_fix).reshape(1, 4, 5)
    rng = np.random.default_rng(seed)
    e = np.stack([rng.uniform(-tilt, tilt, B), rng.uniform(-tilt, tilt, B), rng.uniform(-np.pi, np.pi, B)], 1)
    quat = quat_zyx(e)
    q = np.broadcast_to(np.asarray(q_leg, dtype=np.float64), (B, 4, 3))
    rel = er.mat_vec(er.quat_to_rot(quat)[:, None], er.fk(q, rho_opt, rho_fix))
    pos = np.stack([np.zeros(B), np.zeros(B), -rel[..., 2].min(1) - 1e-6], 1)
    return mpcqp.pack_plant_init(pos, quat, q.reshape(B, 12)), e


def caller_rows(k, B, pos_d, yaw, gravity_comp):
    z = np.zeros((B, 3))
    st = mpcqp.RobotStates(
        root_euler=z, root_pos=z, root_ang_vel=z, root_lin_vel=z, root_rot_mat=np.zeros((B, 3, 3)),
        root_euler_d=np.stack([z[:, 0], z[:, 0], yaw], 1), root_pos_d=pos_d, root_ang_vel_d=z, root_lin_vel_d=z,
        foot_pos_abs=np.zeros((B, 4, 3)), contacts=np.ones((B, 4), bool), mu=np.full(B, 0.3))
    k.states.copy_(torch.from_numpy(mpcqp.pack_states(st)))
    kw = {} if gravity_comp else dict(torques_gravity=np.zeros(12))
    k.tq_records.copy_(torch.from_numpy(mpcqp.assemble_torque_records(np.zeros((B, 4, 3, 3)), np.zeros((B, 4, 3)),
                                                                      np.ones((B, 4), bool), **kw)))


def make(form, B, seed):
    """(tick, the height standing should hold, anything to close afterwards)."""
    pp = mpcqp.default_plant_params()
    if form == "mpc":
        init, e = start_rows(B, [0.0, 0.8, -1.6], 0.09, seed)
        k = ControlTick(B, dt=DT, plant=pp, plant_init=init)
        caller_rows(k, B, init[:, :3], e[:, 2], False)
        return k, init[:, 2].copy(), None
    if form == "full":
        h = mpcqp.default_command_params().body_height_init
        q1 = float(np.arccos(h / (2.0 * pp.rho_fix[3])))  # both links at the same angle to the vertical
        init, e = start_rows(B, [0.0, q1, -2.0 * q1], 0.05, seed)
        k = ControlTick(B, plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                        command=mpcqp.default_command_params(), dt=DT, plant=pp, plant_init=init)
        # (the command stage integrates root_euler_d from the row, so the row starts at the robot's yaw)
        caller_rows(k, B, init[:, :3], e[:, 2], True)
        return k, np.full(B, h), None
    if form in ("servo", "servo_walk_gains"):
        ws, bs = seeded_weights(0)
        pq = mpcqp.default_policy_params()
        if form == "servo_walk_gains":  # the servo stand with the walk mode's softer gains
            for i in range(12):
                pq.kp_servo[i], pq.kd_servo[i] = pq.kp_walk[i], pq.kd_walk[i]
        pol = mpcqp.Policy(ws, bs, pq)
        init, e = start_rows(B, [0.0, 0.8, -1.6], 0.0, seed)
        k = ControlTick(B, dt=DT, control_type=2, policy=pol, plant=pp, plant_init=init)
        caller_rows(k, B, init[:, :3], e[:, 2], True)
        stand = np.array(mpcqp.default_policy_params().stand_pos).reshape(1, 4, 3)
        rel = er.fk(stand, np.array(pp.rho_opt).reshape(1, 4, 3), np.array(pp.rho_fix).reshape(1, 4, 5))
        return k, np.full(B, -rel[0, :, 2].mean()), pol
    raise ValueError(form)


def full_stance():
    """(leg angles, trunk height) of the stance at the command stage's body height: both links at the same
    angle to the vertical."""
    pp = mpcqp.default_plant_params()
    h = mpcqp.default_command_params().body_height_init
    q1 = float(np.arccos(h / (2.0 * pp.rho_fix[3])))
    return [0.0, q1, -2.0 * q1], h


def episode_pool(P, q_leg, tilt, seed, height=None):
    """P pool rows for the episode stage: start_rows, with root_pos_d = (0, 0, start height or `height`) and
    root_euler_d = (0, 0, start yaw)."""
    init, e = start_rows(P, q_leg, tilt, seed)
    z = init[:, 2] if height is None else np.full(P, float(height))
    zero = np.zeros(P)
    return mpcqp.pack_episode_pool(init, np.stack([zero, zero, e[:, 2]], 1), np.stack([zero, zero, z], 1))


EPISODE_FORMS = ("mpc_ep", "full_ep", "full_walk", "servo_ep", "full_push", "full_noise", "mpc_slope", "full_slope",
                 "full_mu", "mpc_field", "full_steps")
FIELD_CELL, FIELD_NX, FIELD_NY, FIELD_X0, FIELD_Y0, FIELD_MU = 0.05, 49, 25, -0.8, -0.6, 0.6
FIELD_TILES, STEP_SET, STEP_AHEAD = ("rolling", "step", "stairs"), (0.0, 0.02, 0.04, 0.06, 0.08), 0.1
SLOPE_GRID, SLOPE_MAX, SLOPE_MU, SLOPE_HEIGHT, MU_SET = 5, 0.2, 0.6, 0.25, (0.2, 0.4, 0.6, 0.8)
PUSH_START, PUSH_TICKS, PUSH_FORCE, PUSH_DIRS, PUSH_BIN = 100, 40, (0.0, 300.0), 16, 25.0
NOISE_SIGMA, NOISE_BIAS = (0.005, 0.1, 0.2, 0.02), (0.1, 0.01)
POOL, MAX_TICKS, WALK_AT, WALK_VX = 64, 500, 100, 0.3


def slope_pool(q_leg, seed):
    """(pool rows, terrain rows) of the slope forms: the stance q_leg at a random yaw, slope-parallel on each plane of
    the pitch / roll grid through the origin; root_euler_d the slope-parallel angles, root_pos_d the start."""
    a = np.linspace(-SLOPE_MAX, SLOPE_MAX, SLOPE_GRID)
    pitch, roll = (g.ravel() for g in np.meshgrid(a, a, indexing="ij"))
    terrain = mpcqp.terrain_from_slope(pitch, roll, SLOPE_MU)
    flat, _ = start_rows(pitch.size, q_leg, 0.0, seed)
    init, euler = mpcqp.place_on_terrain(flat, terrain)
    return mpcqp.pack_episode_pool(init, euler, init[:, :3]), terrain


def field_grid():
    x = (FIELD_X0 + FIELD_CELL * np.arange(FIELD_NX))[None, :] + np.zeros((FIELD_NY, 1))
    y = (FIELD_Y0 + FIELD_CELL * np.arange(FIELD_NY))[:, None] + np.zeros((1, FIELD_NX))
    return x, y, lambda at: np.clip((x - at) / FIELD_CELL, 0.0, 1.0)  # a riser: one cell wide


def field_pool(q_leg, seed):
    """(pool rows, (header rows, heights), a label per pool row) of mpc_field: the stance q_leg placed level by
    place_on_field at a random place within +-0.3 m and a random heading on tile row % 3."""
    x, y, riser = field_grid()
    tiles = [0.03 * np.sin(2 * np.pi * x / 0.9 + 0.4) * np.cos(2 * np.pi * y / 1.3 - 0.2), 0.05 * riser(0.0),
             0.08 * (riser(-0.35) + riser(-0.05) + riser(0.25) + riser(0.55))]
    which = np.arange(POOL) % 3
    rows, heights = mpcqp.pack_height_field(tiles, FIELD_X0, FIELD_Y0, FIELD_CELL, FIELD_MU, share=which)
    flat, e = start_rows(POOL, q_leg, 0.0, seed)
    flat[:, :2] = np.random.default_rng(seed + 1).uniform(-0.3, 0.3, (POOL, 2))
    init, euler = mpcqp.place_on_field(flat, rows, heights, np.arange(POOL))
    return mpcqp.pack_episode_pool(init, euler, init[:, :3]), (rows, heights), [FIELD_TILES[k] for k in which]


def steep_starts(pool, field):
    """Per pool row: whether a foot of the start stance stands on a facet steeper than the friction angle."""
    from mpcqp.plant import _feet_body, _quat_rot
    init = pool[:, :_lib.PI_SIZE]
    P = init.shape[0]
    feet = init[:, None, :3] + np.einsum("bij,blj->bli", _quat_rot(init[:, 3:7]),
                                         _feet_body(mpcqp.default_plant_params(), init[:, 7:19].reshape(P, 4, 3)))
    n = mpcqp.field_lookup(field[0], field[1], np.arange(P), feet)[1]
    return (np.sqrt(1.0 / n[..., 2] ** 2 - 1.0) > FIELD_MU).any(1)


def steps_pool(q_leg, seed):
    """(pool rows, (header rows, heights), a label per pool row) of full_steps: the stance q_leg heading along +x
    (within 0.05 rad) towards a step up of STEP_SET[row % 5] whose riser begins STEP_AHEAD in front of the front
    feet, at a y within +-0.2 m."""
    x, y, riser = field_grid()
    which = np.arange(POOL) % len(STEP_SET)
    rows, heights = mpcqp.pack_height_field([h * riser(0.0) for h in STEP_SET], FIELD_X0, FIELD_Y0, FIELD_CELL, FIELD_MU,
                                            share=which)
    flat, _ = start_rows(POOL, q_leg, 0.0, seed)
    rng = np.random.default_rng(seed + 1)
    yaw = rng.uniform(-0.05, 0.05, POOL)
    zero = np.zeros(POOL)
    flat[:, 3:7] = np.stack([np.cos(yaw / 2), zero, zero, np.sin(yaw / 2)], 1)
    pp = mpcqp.default_plant_params()
    front = er.fk(np.asarray(q_leg, dtype=np.float64).reshape(1, 1, 3), np.array(pp.rho_opt).reshape(1, 4, 3)[:, :1],
                  np.array(pp.rho_fix).reshape(1, 4, 5)[:, :1])[0, 0, 0]
    flat[:, 0] = -STEP_AHEAD - front
    flat[:, 1] = rng.uniform(-0.2, 0.2, POOL)
    init, euler = mpcqp.place_on_field(flat, rows, heights, np.arange(POOL))
    return mpcqp.pack_episode_pool(init, euler, init[:, :3]), (rows, heights), [f"{h:.2f}" for h in np.array(STEP_SET)[which]]


def make_episode(form, B, seed):
    """The mpc / full setups with the episode stage: a pool of POOL start rows, a time-out of MAX_TICKS ticks and
    the standing envelope of `look` (tilt 0.3 rad, 5 cm about the standing height).  full_walk: every episode's
    script toggles walk mode and commands WALK_VX m/s forward at episode tick WALK_AT; its envelope keeps the
    tilt bound and takes the height bounds of the stage's defaults."""
    pp = mpcqp.default_plant_params()
    extra = None
    if form == "mpc_ep":
        q, tilt = [0.0, 0.8, -1.6], 0.09
        pool = episode_pool(POOL, q, tilt, seed)
        stand = float(np.median(pool[:, 2]))
        kw, comp = {}, False
    elif form == "servo_ep":
        ws, bs = seeded_weights(0)
        extra = mpcqp.Policy(ws, bs, mpcqp.default_policy_params())
        pool = episode_pool(POOL, [0.0, 0.8, -1.6], 0.0, seed)
        stand_pos = np.array(mpcqp.default_policy_params().stand_pos).reshape(1, 4, 3)
        rel = er.fk(stand_pos, np.array(pp.rho_opt).reshape(1, 4, 3), np.array(pp.rho_fix).reshape(1, 4, 5))
        stand = float(-rel[0, :, 2].mean())
        kw, comp = dict(control_type=2, policy=extra), True
    else:
        q, stand = full_stance()
        pool = episode_pool(POOL, q, 0.05, seed, stand)
        kw, comp = dict(plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                        command=mpcqp.default_command_params()), True
    over = dict(height_min=stand - 0.05, height_max=stand + 0.05)
    scripts = None
    tilt_max = 0.3
    if form in ("mpc_slope", "full_slope"):
        # the envelope is the world's: the tilt of the steepest ground is added to the bound, and the trunk stands
        # lower by the ground's cosine (and climbs or descends while it walks)
        pool, terrain = slope_pool([0.0, 0.8, -1.6] if form == "mpc_slope" else full_stance()[0], seed)
        if form == "mpc_slope":
            stand = float(np.median(pool[:, 2]))
            kw, comp = {}, False
        tilt_max = 0.3 + float(np.arccos(terrain[:, 2].min()))
        grow = SLOPE_HEIGHT if form == "full_slope" else 0.0
        over = dict(height_min=stand * float(terrain[:, 2].min()) - 0.05 - grow, height_max=stand + 0.05 + grow)
        kw["terrain"] = terrain
    labels = None
    if form == "mpc_field":
        kw, comp = {}, False
        pool, kw["field"], labels = field_pool([0.0, 0.8, -1.6], seed)
        over = dict(height_min=float(pool[:, 2].min()) - 0.05, height_max=float(pool[:, 2].max()) + 0.05)
    if form == "full_steps":
        pool, kw["field"], labels = steps_pool(full_stance()[0], seed)
    if form == "full_mu":
        kw["terrain"] = mpcqp.pack_terrain(np.tile([0.0, 0.0, 1.0], (POOL, 1)), 0.0, np.array(MU_SET)[np.arange(POOL) % 4])
    if form in ("full_walk", "full_slope", "full_mu", "full_steps"):
        over = {} if form != "full_slope" else over
        scripts = mpcqp.pack_episode_scripts([[(0, (0, 0, 0), (0, 0, 0), False),
                                               (WALK_AT, (WALK_VX, 0, 0), (0, 0, 0), True)]])
    if form == "full_push":
        # one window per episode: it starts at PUSH_START and is as long as what is left of the episode
        kw.update(disturb=mpcqp.default_disturb_params(seed=seed, push_force=PUSH_FORCE, push_start=PUSH_START,
                                                       push_interval=max(MAX_TICKS - PUSH_START, PUSH_TICKS),
                                                       push_duration=PUSH_TICKS),
                  disturb_dirs=mpcqp.pack_push_dirs(PUSH_DIRS))
    elif form == "full_noise":
        kw.update(disturb=mpcqp.default_disturb_params(seed=seed, sigma=NOISE_SIGMA, bias_acc=NOISE_BIAS[0],
                                                       bias_gyro=NOISE_BIAS[1]))
    ep = mpcqp.default_episode_params(max_ticks=MAX_TICKS, tilt_max=tilt_max, seed=seed, **over)
    k = ControlTick(B, dt=DT, plant=pp, episode=ep, episode_pool=pool, episode_scripts=scripts, episode_log_len=8,
                    **kw)
    caller_rows(k, B, np.zeros((B, 3)), np.zeros(B), comp)  # the constants; the stage writes the desired values
    k.field_labels = labels
    k.field_steep = steep_starts(pool, kw["field"]) if form == "mpc_field" else None
    return k, extra


def run_episode(form, B, T, seed):
    """T replays of the tick that ends with the episode stage; everything reported comes from the totals and the
    log rows, read once after the last replay."""
    from mpcqp import episode as me
    k, extra = make_episode(form, B, seed)
    try:
        k.capture()
        torch.cuda.synchronize()
        ms = 0.0
        for t0 in range(0, T, CHUNK):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(min(CHUNK, T - t0)):
                k.replay()
            ev[1].record()
            torch.cuda.synchronize()
            ms += ev[0].elapsed_time(ev[1])
        tot = np.frombuffer(k.episode_totals.cpu().numpy().tobytes(), dtype=mpcqp.EPISODE_TOTALS_DTYPE)
        log = np.frombuffer(k.episode_log.cpu().numpy().tobytes(), dtype=mpcqp.EPISODE_LOG_DTYPE)
        es = np.frombuffer(k.episode_state.cpu().numpy().tobytes(), dtype=mpcqp.EPISODE_STATE_DTYPE)
        robot = np.repeat(np.arange(B), k.episode_log.shape[1])[log["length"] > 0]
        log = log[log["length"] > 0]
        r = {"form": form, "batch": B, "ticks": T, "dt": DT, "ticks_per_s": T / (ms * 1e-3),
             "robot_ticks_per_s": B * T / (ms * 1e-3), "ms_per_tick": ms / T, "max_ticks": MAX_TICKS, "pool": int(k.episode_pool.shape[0]),
             "episodes": int(tot["episodes"].sum()), "episode_ticks": int(tot["ticks"].sum()),
             "end_reasons": {n: int(c) for n, c in zip(me.END_NAMES, tot["reason"].sum(0))},
             "robots_running_at_the_end": int((es["phase"] == 1.0).sum()),
             "logged_episodes": int(log.size)}
        if log.size:
            with np.errstate(invalid="ignore"):
                r.update({"length_mean": float(log["length"].mean()), "length_median": float(np.median(log["length"])),
                          "tilt_max_median": float(np.sqrt(np.nanmedian(log["tilt2_max"]))),
                          "z_min_median": float(np.nanmedian(log["z_min"])),
                          "energy_per_tick_median": float(np.nanmedian(log["energy"] / log["length"])),
                          "err_vx_rms_median": float(np.sqrt(np.nanmedian(log["err_v"][:, 0] / log["length"]))),
                          "not_solved_share": float(log["not_solved"].sum() / log["length"].sum()),
                          "low_contact_share": float(log["low_contact"].sum() / log["length"].sum())})
                if form == "full_push":
                    r.update(push_curve(k, robot, log))
                if form == "full_noise":
                    r.update({"noise_sigma": list(NOISE_SIGMA), "noise_bias": list(NOISE_BIAS)})
                if form in ("mpc_slope", "full_slope", "full_mu"):
                    r.update(terrain_report(form, k, es, log))
                if form in ("mpc_field", "full_steps"):
                    r.update(field_report(form, k, log))
                if form in ("full_walk", "full_slope", "full_mu", "full_steps"):
                    d = log["end"][:, :2] - log["start"][:, :2]
                    yaw = log["start"][:, 2]
                    fwd = d[:, 0] * np.cos(yaw) + d[:, 1] * np.sin(yaw)
                    walked = log["length"] > WALK_AT
                    r.update({"walk_at": WALK_AT, "walk_vx": WALK_VX, "episodes_that_reached_the_toggle": int(walked.sum()),
                              "ticks_after_the_toggle_median": float(np.median(log["length"][walked] - WALK_AT))
                              if walked.any() else None,
                              "forward_m_median": float(np.nanmedian(fwd[walked])) if walked.any() else None,
                              "forward_m_max": float(np.nanmax(fwd[walked])) if walked.any() else None,
                              "end_reasons_after_the_toggle": {
                                  n: int((log["reason"][walked] == i).sum()) for i, n in enumerate(me.END_NAMES)}})
    finally:
        k.close()
        if extra is not None:
            extra.close()
    return r


def terrain_report(form, k, es, log):
    """Per terrain row (full_mu: per mu): the logged episodes and their end reasons; for full_slope also the median
    MPCQP_PO_ANGLE of the robots that run on the row after the last replay beside the ground's pitch along their
    heading, atan((n_x cos yaw + n_y sin yaw) / n_z) (positive: nose down, as root_euler[1])."""
    from mpcqp import episode as me
    terrain = k.terrain.cpu().numpy()
    n = terrain[:, :3]
    key = terrain[:, _lib.TR_MU] if form == "full_mu" else np.arange(terrain.shape[0])
    lrow, rrow = log["pool"].astype(int), es["pool"].astype(int)
    running = es["phase"] == 1.0
    if form == "full_slope":
        angle = np.frombuffer(k.plan_out.cpu().numpy().tobytes(), dtype=mpcqp.PLAN_OUT_DTYPE)["terrain_pitch_angle"]
        yaw = k.plant_out.cpu().numpy()[:, _lib.PT_EULER + 2]
        along = np.arctan((n[rrow, 0] * np.cos(yaw) + n[rrow, 1] * np.sin(yaw)) / n[rrow, 2])
        walking = running & (es["tick"] > WALK_AT + 100)
        pitch_d = k.states.cpu().numpy()[:, _lib.ST_EULER_D + 1]  # what the plan stage made of the angle
    rows = []
    for v in np.unique(key):
        m = np.isin(lrow, np.nonzero(key == v)[0])
        row = {"episodes": int(m.sum()), "length_median": float(np.median(log["length"][m])) if m.any() else None,
               "end_reasons": {nm: int((log["reason"][m] == i).sum()) for i, nm in enumerate(me.END_NAMES)}}
        if form == "full_mu":
            row["mu"] = float(v)
        else:
            row.update(row=int(v), normal=[float(x) for x in n[int(v)]])
        if form == "full_slope":
            w = walking & (rrow == v)
            row.update(robots_walking=int(w.sum()),
                       po_angle_median=float(np.median(angle[w])) if w.any() else None,
                       ground_pitch_along_heading_median=float(np.median(along[w])) if w.any() else None,
                       euler_d_pitch_median=float(np.median(pitch_d[w])) if w.any() else None,
                       euler_d_sign_agrees_share=float(np.mean(np.sign(pitch_d[w]) == np.sign(along[w])))
                       if w.any() else None)
        rows.append(row)
    return {"terrain_rows": rows}


def field_report(form, k, log):
    """Per label of the pool rows (mpc_field: the tile; full_steps: the step height): the logged episodes, their end
    reasons, and for full_steps the distance walked along the start heading and the height climbed by the episodes that
    reached the toggle."""
    from mpcqp import episode as me
    labels = np.array(k.field_labels)
    lrow = log["pool"].astype(int)
    rows = []
    for v in sorted(set(labels)):
        m = labels[lrow] == v
        row = {"ground": v, "episodes": int(m.sum()),
               "length_median": float(np.median(log["length"][m])) if m.any() else None,
               "end_reasons": {nm: int((log["reason"][m] == i).sum()) for i, nm in enumerate(me.END_NAMES)},
               "lost_share": float(np.mean(log["reason"][m] != me.END_NAMES.index("timeout"))) if m.any() else None}
        if form == "mpc_field":  # the starts with a foot on a facet steeper than the friction angle (a riser), apart
            steep = k.field_steep[lrow]
            lost = log["reason"] != me.END_NAMES.index("timeout")
            row.update(pool_rows=int((labels == v).sum()), pool_rows_with_a_foot_on_a_riser=int(k.field_steep[labels == v].sum()),
                       episodes_from_those=int((m & steep).sum()), lost_from_those=int((m & steep & lost).sum()),
                       lost_from_the_others=int((m & ~steep & lost).sum()))
        if form == "full_steps":
            w = m & (log["length"] > WALK_AT)
            d = log["end"][:, :2] - log["start"][:, :2]
            fwd = d[:, 0] * np.cos(log["start"][:, 2]) + d[:, 1] * np.sin(log["start"][:, 2])
            row.update(reached_the_toggle=int(w.sum()),
                       forward_m_median=float(np.nanmedian(fwd[w])) if w.any() else None,
                       forward_m_max=float(np.nanmax(fwd[w])) if w.any() else None)
        rows.append(row)
    return {"field_rows": rows, "field_mu": FIELD_MU, "step_ahead": STEP_AHEAD if form == "full_steps" else None}


def push_curve(k, robot, log):
    """The push-recovery curve of the logged episodes: each episode's push recomputed on the host from the seed, the
    robot and the episode index; per magnitude bin the episodes and how many ended by the envelope or a plant
    status.  An episode that ended before its push began is counted apart."""
    from mpcqp import episode as me
    dirs = k.disturb_dirs.cpu().numpy()
    force, failed, before = [], [], 0
    for b, row in zip(robot, log):
        pushes = mpcqp.disturbance_of(k.disturb, dirs, int(b), int(row["episode"]), int(row["length"]))["pushes"]
        if not pushes:
            before += 1
            continue
        force.append(pushes[0]["force"])
        failed.append(int(row["reason"]) in (me.END_OUT_OF_REACH, me.END_FALLEN, me.END_BAD_TORQUE, me.END_ENVELOPE))
    force, failed = np.array(force), np.array(failed, dtype=bool)
    edges = np.arange(PUSH_FORCE[0], PUSH_FORCE[1] + PUSH_BIN, PUSH_BIN)
    curve = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        m = (force >= lo) & (force < hi)
        curve.append({"force_lo": float(lo), "force_hi": float(hi), "episodes": int(m.sum()),
                      "failed": int(failed[m].sum()), "failed_share": float(failed[m].mean()) if m.any() else None})
    return {"push_start": PUSH_START, "push_ticks": PUSH_TICKS, "push_force": list(PUSH_FORCE), "push_dirs": PUSH_DIRS,
            "episodes_ended_before_their_push": before, "push_recovery_curve": curve}


def look(k, stand_z):
    po = k.plant_out.cpu().numpy()
    tilt = np.hypot(po[:, _lib.PT_EULER], po[:, _lib.PT_EULER + 1])
    bad = po[:, _lib.PT_STATUS] != 0.0
    with np.errstate(invalid="ignore"):
        out = ~(tilt <= 0.3) | ~(np.abs(po[:, _lib.PT_POS + 2] - stand_z) <= 0.05)
    return po, tilt, bad, out


def run(form, B, T, seed):
    k, stand_z, extra = make(form, B, seed)
    try:
        k.prime_plant()
        k.capture()
        torch.cuda.synchronize()
        ms = 0.0
        for t0 in range(0, T, CHUNK):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(min(CHUNK, T - t0)):
                k.replay()
            ev[1].record()
            torch.cuda.synchronize()
            ms += ev[0].elapsed_time(ev[1])
        po, tilt, bad, out = look(k, stand_z)
        res = np.frombuffer(k.results.cpu().numpy().tobytes(), dtype=mpcqp.RESULT_DTYPE)
        r = {"form": form, "batch": B, "ticks": T, "dt": DT, "ticks_per_s": T / (ms * 1e-3),
             "robot_ticks_per_s": B * T / (ms * 1e-3), "ms_per_tick": ms / T,
             "status_nonzero": int(bad.sum()), "status_counts": {str(int(s)): int((po[:, _lib.PT_STATUS] == s).sum())
                                                                 for s in np.unique(po[:, _lib.PT_STATUS])},
             "out_of_envelope": int((out & ~bad).sum()),
             "tilt_max": float(np.nanmax(tilt)), "tilt_median": float(np.nanmedian(tilt)),
             "height_median": float(np.nanmedian(po[:, _lib.PT_POS + 2])), "height_stand": float(np.median(stand_z)),
             "contacts_mean": float(po[:, _lib.PT_CONTACTS:_lib.PT_CONTACTS + 4].sum(1).mean()),
             "fz_over_mg_median": float(np.nanmedian(po[:, _lib.PT_GRF + 2:_lib.PT_GRF + 12:3].sum(1)) /
                                        (k.plant.mass * k.plant.gravity))}
        if not form.startswith("servo"):
            r["solved_share_last_tick"] = float((res["status"] == _lib.STATUS_SOLVED).mean())
    finally:
        k.close()
        if extra is not None:
            extra.close()
    if r["status_nonzero"] or r["out_of_envelope"]:
        # once more, reading after every tick: the first tick at which a robot goes wrong
        k, stand_z, extra = make(form, B, seed)
        try:
            k.prime_plant()
            k.capture()
            first_status = first_env = None
            for t in range(1, T + 1):
                k.replay()
                torch.cuda.synchronize()
                _, _, bad, out = look(k, stand_z)
                if first_status is None and bad.any():
                    first_status = t
                if first_env is None and (out & ~bad).any():
                    first_env = t
                if first_status is not None and first_env is not None:
                    break
            r["first_tick_status_nonzero"] = first_status
            r["first_tick_out_of_envelope"] = first_env
        finally:
            k.close()
            if extra is not None:
                extra.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--forms", nargs="+", default=["mpc", "full", "servo"])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-ticks", type=int, default=MAX_TICKS, help="time-out of the episode forms")
    a = ap.parse_args()
    globals()["MAX_TICKS"] = a.max_ticks
    for form in a.forms:
        go = run_episode if form in EPISODE_FORMS else run
        print(json.dumps(go(form, a.batch, a.ticks, a.seed)), flush=True)


if __name__ == "__main__":
    main()
