"""ControlTick(disturb=): the tick that disturbs its fleet.  The fused step is bitwise the staged C calls and the
captured graph's replays; a tick with the default (all-off) params is bitwise the tick without the stage; an
episode is bitwise the same when a fresh tick replays it from the seed; a push moves the trunk in the tick the
host-side recomputation predicts, and not before; and the per-robot tick's policy stage reads the noisy row."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib
from mpcqp.tick import ControlTick

import disturb_reference as dr
import episode_reference as ep
import test_gpu_tick_episode as te
from test_disturb import ref_params
from test_gpu_tick_plant import DT, _bits

pytestmark = pytest.mark.gpu

B = 5
DISTURB = ("wrench", "disturb_out")
NAMES = {"mpc": te.NAMES["mpc"] + DISTURB, "full": te.NAMES["full"] + DISTURB + ("sensors_noisy",)}


def _params(**over):
    kw = dict(load_mass_max=3.0, load_point=[0.1, 0.05, 0.02], bias_acc=0.05, bias_gyro=0.01, push_force=[10.0, 40.0],
              push_point=[0.1, 0.05, 0.03], sigma=[0.002, 0.05, 0.05, 0.01], seed=11, push_start=2, push_interval=5,
              push_duration=2)
    kw.update(over)
    return mpcqp.default_disturb_params(**kw)


def _caller_rows(n):
    st = mpcqp.synthetic_go1(n, seed=9, gait="stance")
    st.root_euler_d[:] = 0.0
    st.root_ang_vel_d[:] = 0.0
    st.root_lin_vel_d[:] = 0.0
    st.root_pos_d[:] = [0.0, 0.0, 0.29]
    tq = mpcqp.assemble_torque_records(np.zeros((n, 4, 3, 3)), np.zeros((n, 4, 3)), np.ones((n, 4), bool))
    return mpcqp.pack_states(st), tq


def _make(kind, epar, disturb=None, dirs=None, n=B, pool=None, scripts=None):
    pool = pool if pool is not None else te._stance_pool(kind, ((0.0, 0.0, 0.0), (0.02, -0.03, 0.4)))
    kw = dict(dt=DT, plant=mpcqp.default_plant_params(), episode=epar, episode_pool=pool, episode_scripts=scripts,
              disturb=disturb, disturb_dirs=dirs)
    if kind == "full":
        k = ControlTick(n, plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                        command=mpcqp.default_command_params(), **kw)
    else:
        k = ControlTick(n, **kw)
    rows, tq = _caller_rows(n)
    k.states.copy_(torch.from_numpy(rows))
    k.tq_records.copy_(torch.from_numpy(tq))
    return k


def _staged(k, kind):
    """ControlTick.step's stages with the disturbance stage, one entry point at a time on the object's buffers,
    the disturbance and the episode stage on buffers structs of their own."""
    s = torch.cuda.current_stream().cuda_stream
    full = kind == "full"
    p = lambda n: getattr(k, n).data_ptr() if getattr(k, n, None) is not None else 0  # noqa: E731
    n = lambda name: getattr(k, name).shape[1] if hasattr(k, name) else 0  # noqa: E731
    mpcqp.disturb_device(k.disturb, mpcqp.disturb_buffers(p("episode_state"), p("wrench"), p("sensors"),
                                                         p("sensors_noisy"), p("disturb_dirs"), p("disturb_out")),
                         k.B, s)
    if full:
        mpcqp.command_device(k.command, k.dt, k.cmd.data_ptr(), k.states.data_ptr(), k.plan_in.data_ptr(), k.B,
                             k.cmd_state.data_ptr(), s)
        mpcqp.state_estimate_device(k.estimator, k.dt, k.sensors_noisy.data_ptr(), k.plan_in.data_ptr(),
                                    k.states.data_ptr(), k.B, k.est_state.data_ptr(), k.tq_records.data_ptr(),
                                    k.est_out.data_ptr(), s)
        mpcqp.leg_plan_device(k.plan, k.dt, k.states.data_ptr(), k.plan_in.data_ptr(), k.B, k.plan_state.data_ptr(),
                              k.tq_records.data_ptr(), k.plan_out.data_ptr(), s)
    mpcqp.assemble_records_device(10, k.states.data_ptr(), k.B, k.records.data_ptr(), s)
    k.solver.solve_warm_device(k.records.data_ptr(), k.B, k.warm.data_ptr(), k.results.data_ptr(), 0, s)
    mpcqp.joint_torques_device(k.tq_records.data_ptr(), k.results.data_ptr(), k.B, k.counter.data_ptr(),
                               k.torques.data_ptr(), s)
    mpcqp.plant_step_wrench_device(k.plant, k.dt, k.torques.data_ptr(), k.wrench.data_ptr(), k.B,
                                   k.plant_state.data_ptr(), k.plant_init.data_ptr(),
                                   k.sensors.data_ptr() if full else 0, k.plan_in.data_ptr(),
                                   0 if full else k.states.data_ptr(), 0 if full else k.tq_records.data_ptr(),
                                   k.plant_out.data_ptr(), s)
    bf = mpcqp.episode_buffers(
        d_plant_out=p("plant_out"), d_plant_state=p("plant_state"), d_plant_init=p("plant_init"),
        d_joint_torques=p("torques"), d_sensors=p("sensors"), d_cmd=p("cmd"), d_results=p("results"),
        d_pool=p("episode_pool"), d_scripts=p("episode_scripts"), d_states=p("states"), d_counter=p("counter"),
        d_log=p("episode_log"), d_totals=p("episode_totals"), d_est_state=p("est_state"),
        est_state_size=n("est_state"), d_plan_state=p("plan_state"), plan_state_size=n("plan_state"),
        d_cmd_state=p("cmd_state"), cmd_state_size=n("cmd_state"), d_warm=p("warm"), warm_size=n("warm"))
    mpcqp.episode_device(k.episode, bf, k.B, k.episode_state.data_ptr(), s)


def _snap(k, names):
    return {n: _bits(getattr(k, n)) for n in names}


# ---- 1. fused = staged = graph replays ----
T1 = 30
_RUNS = {}


def _runs(kind):
    if kind not in _RUNS:
        out = {}
        for how in ("eager", "staged", "graph"):
            k = _make(kind, mpcqp.default_episode_params(max_ticks=12, seed=7), _params(), mpcqp.pack_push_dirs(8),
                      scripts=mpcqp.pack_episode_scripts(te.SCRIPT) if kind == "full" else None)
            try:
                rows = [_snap(k, NAMES[kind])]
                for _ in range(T1):
                    if how == "graph":
                        if k.graph is None:
                            k.capture()
                        k.replay()
                    elif how == "eager":
                        k.step()
                    else:
                        _staged(k, kind)
                    torch.cuda.synchronize()
                    rows.append(_snap(k, NAMES[kind]))
                out[how] = rows
            finally:
                k.close()
        _RUNS[kind] = out
    return _RUNS[kind]


@pytest.mark.parametrize("other", ["staged", "graph"])
@pytest.mark.parametrize("kind", ["mpc", "full"])
def test_fused_tick_is_bitwise_the_stages_and_its_graph(kind, other):
    out = _runs(kind)
    for t, (a, b) in enumerate(zip(out["eager"], out[other])):
        for name in NAMES[kind]:
            assert np.array_equal(a[name], b[name]), f"{kind} tick {t}: {name} of the eager tick and the {other} one differ"
    rows = np.stack([o["disturb_out"].view(np.float64) for o in out["eager"]])
    wrench = np.stack([o["wrench"].view(np.float64) for o in out["eager"]])
    tot = out["eager"][-1]["episode_totals"].view(np.float64)
    print(f"[note] {kind} tick, {T1} ticks: {int(rows[:, :, dr.DO_PUSH_ACTIVE].sum())} pushed robot-ticks, episodes "
          f"per robot {tot[:, ep.ET_EPISODES].tolist()}")
    # the stage did something: pushes, a load, and (full) a noisy row that is not the clean one
    assert rows[:, :, dr.DO_PUSH_ACTIVE].sum() > 0 and np.abs(wrench[:, :, dr.PW_FORCE0:dr.PW_FORCE0 + 3]).max() >= 10.0
    assert wrench[:, :, dr.PW_FORCE1 + 2].min() < 0.0 and np.all(tot[:, ep.ET_EPISODES] >= 1.0)
    if kind == "full":
        assert any(not np.array_equal(o["sensors"], o["sensors_noisy"]) for o in out["eager"])
    # the rows of the last tick are the restatement's of the slot before it
    k_dp = _params()
    k_dp.dir_count = 8
    es = out["eager"][-2]["episode_state"].view(np.float64)
    sn = out["eager"][-2]["sensors"].view(np.float64) if kind == "full" else None
    w, noisy, o = dr.step(ref_params(k_dp), es, sn, mpcqp.pack_push_dirs(8))
    assert np.array_equal(w.view(np.int64), out["eager"][-1]["wrench"])
    assert np.array_equal(o.view(np.int64), out["eager"][-1]["disturb_out"])
    if kind == "full":
        assert np.array_equal(noisy.view(np.int64), out["eager"][-1]["sensors_noisy"])


# ---- 2. all off = no stage ----
@pytest.mark.parametrize("kind", ["mpc", "full"])
def test_default_params_are_the_tick_without_the_stage(kind):
    """20 ticks at max_ticks 8, so they span a restart: every buffer the two ticks share is bitwise the same."""
    rows = {}
    for how in ("without", "off"):
        k = _make(kind, mpcqp.default_episode_params(max_ticks=8, seed=7),
                  mpcqp.default_disturb_params() if how == "off" else None,
                  scripts=mpcqp.pack_episode_scripts(te.SCRIPT) if kind == "full" else None)
        try:
            if how == "without":
                assert k.disturb is None and not hasattr(k, "wrench") and not hasattr(k, "sensors_noisy")
            rows[how] = []
            for _ in range(20):
                k.step()
                torch.cuda.synchronize()
                rows[how].append(_snap(k, te.NAMES[kind]))
            if how == "off":
                assert not k.wrench.any() and not k.disturb_out.any()
        finally:
            k.close()
    for t, (a, b) in enumerate(zip(rows["without"], rows["off"])):
        for name in te.NAMES[kind]:
            assert np.array_equal(a[name], b[name]), f"{kind} tick {t}: {name}"
    assert np.all(rows["off"][-1]["episode_totals"].view(np.float64)[:, ep.ET_EPISODES] >= 1.0)


def test_disturb_needs_plant_and_episode():
    with pytest.raises(ValueError, match="needs plant= and episode="):
        ControlTick(B, dt=DT, plant=mpcqp.default_plant_params(), disturb=mpcqp.default_disturb_params())


# ---- 3. an episode replayed from the seed ----
@pytest.mark.parametrize("kind", ["mpc", "full"])
def test_an_episode_is_replayed_by_a_fresh_tick(kind):
    """The stage keeps no state, and a restart is complete: episode 1 of a run is bitwise what a freshly built
    tick with the same seeds computes when its (fresh) episode slots start at episode index 1."""
    M = 12
    names = ("plant_out", "torques", "wrench", "disturb_out") + (("sensors_noisy",) if kind == "full" else ())
    pool = te._stance_pool(kind, ((0.01, -0.02, 0.3),))
    scripts = mpcqp.pack_episode_scripts(te.SCRIPT) if kind == "full" else None
    seen = {}
    for how in ("run", "replay"):
        k = _make(kind, mpcqp.default_episode_params(max_ticks=M, seed=3), _params(), mpcqp.pack_push_dirs(8),
                  pool=pool, scripts=scripts)
        try:
            if how == "replay":
                k.episode_state[:, ep.ES_EPISODE] = 1.0
            rows = []
            for _ in range(2 + M + (M + 1 if how == "run" else 0)):
                k.step()
                torch.cuda.synchronize()
                rows.append(_snap(k, names + ("episode_state",)))
            seen[how] = rows[-M:]  # the M ticks of the last episode: episode 1 in both
        finally:
            k.close()
    for i, (a, b) in enumerate(zip(seen["run"], seen["replay"])):
        es = a["episode_state"].view(np.float64)
        if i < M - 1:
            assert np.all(es[:, ep.ES_EPISODE] == 1.0) and np.all(es[:, ep.ES_TICK] == i + 1.0)
        for name in names:
            assert np.array_equal(a[name], b[name]), f"{kind}: {name} at tick {i} of episode 1"
    assert any(o["disturb_out"].view(np.float64)[:, dr.DO_PUSH_ACTIVE].any() for o in seen["run"])


# ---- 4. a push arrives when the host says ----
def test_a_push_moves_the_trunk_in_the_predicted_tick():
    """8 robots under the truth-fed MPC tick, one 300 N push of 2 ticks per episode: MPCQP_PT_LIN_VEL is bitwise
    the unpushed run's until the tick mpcqp.disturbance_of gives, and departs from it in that tick."""
    n, M = 8, 40
    dirs = mpcqp.pack_push_dirs(6)
    vel = {}
    for how, force in (("pushed", 300.0), ("unpushed", 0.0)):
        dp = mpcqp.default_disturb_params(seed=5, push_force=[force, force], push_start=12, push_interval=M - 12,
                                          push_duration=2)
        k = _make("mpc", mpcqp.default_episode_params(max_ticks=M, seed=5), dp, dirs, n=n,
                  pool=te._stance_pool("mpc"))
        try:
            vel[how] = []
            for _ in range(2 + M):
                k.step()
                torch.cuda.synchronize()
                vel[how].append(k.plant_out[:, _lib.PT_LIN_VEL:_lib.PT_LIN_VEL + 3].cpu().numpy().copy())
            if how == "pushed":
                dp.dir_count = dirs.shape[0]
                want = [mpcqp.disturbance_of(dp, dirs, b, 0, M)["pushes"] for b in range(n)]
        finally:
            k.close()
    starts = set()
    for b in range(n):
        assert len(want[b]) == 1 and 12 <= want[b][0]["start"] < M - 1
        at = 2 + want[b][0]["start"]  # step 1 draws, step 2 primes, step 3 is episode tick 0
        starts.add(at)
        for t in range(2 + M):
            same = np.array_equal(vel["pushed"][t][b].view(np.int64), vel["unpushed"][t][b].view(np.int64))
            assert same == (t < at), f"robot {b}: step {t}, push predicted at step {at}"
        dv = vel["pushed"][at][b] - vel["unpushed"][at][b]
        # the first pushed tick adds F dt / m along the push, less what the held feet take up
        assert np.dot(dv[:2], want[b][0]["vector"][:2]) > 0.0
    print(f"[note] pushes predicted at steps {sorted(starts)}")
    assert len(starts) > 1


# ---- 5. the per-robot tick with the policy stage ----
def test_typed_tick_with_the_policy_reads_the_noisy_row():
    """The tick with a control type per robot (balance QP, MPC and the policy stage) has the longest stage list: its
    eager steps and its graph's replays agree bitwise, and the noise reaches the policy stage: the policy's output
    row is that of the same tick without noise until the first running tick, and differs from it there."""
    import policy_reference as ref
    names = NAMES["full"] + ("bal_records", "policy_state", "policy_out")
    ws, bs = ref.seeded_weights(31)
    types = torch.tensor([1, 0, 2, 1, 2], dtype=torch.int32)
    rows = {}
    with mpcqp.Policy(ws, bs) as pol:
        for how in ("eager", "graph", "quiet"):
            dp = _params(sigma=[0.0] * 4, bias_acc=0.0, bias_gyro=0.0) if how == "quiet" else _params()
            k = ControlTick(B, plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                            command=mpcqp.default_command_params(), control_type="per_robot", policy=pol, dt=DT,
                            plant=mpcqp.default_plant_params(), episode=mpcqp.default_episode_params(max_ticks=12, seed=7),
                            episode_pool=te._stance_pool("full"), episode_scripts=mpcqp.pack_episode_scripts(te.SCRIPT),
                            disturb=dp, disturb_dirs=mpcqp.pack_push_dirs(8))
            try:
                st, tq = _caller_rows(B)
                k.states.copy_(torch.from_numpy(st))
                k.tq_records.copy_(torch.from_numpy(tq))
                k.control_type.copy_(types)
                if how == "graph":
                    k.capture()
                rows[how] = []
                for _ in range(T1):
                    k.replay() if how == "graph" else k.step()
                    torch.cuda.synchronize()
                    rows[how].append(_snap(k, names))
            finally:
                k.close()
    for t, (a, b) in enumerate(zip(rows["eager"], rows["graph"])):
        for name in names:
            assert np.array_equal(a[name], b[name]), f"typed tick {t}: {name}"
    pol_rows = types.numpy() == 2
    for t in range(2):  # the fresh and the priming tick: a plain copy of the sensor row
        assert np.array_equal(rows["eager"][t]["policy_out"], rows["quiet"][t]["policy_out"]), f"tick {t}"
        assert np.array_equal(rows["eager"][t]["sensors_noisy"], rows["quiet"][t]["sensors_noisy"]), f"tick {t}"
    a, q = rows["eager"][2], rows["quiet"][2]  # episode tick 0
    assert not np.array_equal(a["sensors_noisy"][pol_rows], q["sensors_noisy"][pol_rows])
    assert not np.array_equal(a["policy_out"][pol_rows], q["policy_out"][pol_rows])
    tot = rows["eager"][-1]["episode_totals"].view(np.float64)
    assert np.all(tot[:, ep.ET_EPISODES] >= 1.0)
