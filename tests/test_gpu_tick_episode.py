"""ControlTick(episode=): the tick that evaluates its fleet.  The fused step is bitwise the staged C calls and the
captured graph's replays; the real freeze-and-restart path (a crouch under the plant's min_height, a time-out, a
tilted start outside the envelope) gives the log and totals of tests/episode_reference.py fed the device's own
rows; a restart is complete: every episode of a robot is bitwise the one before and a freshly built tick; and a
tick without episode= enqueues what it did before."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib
from mpcqp.tick import ControlTick

import episode_cases as ec
import episode_reference as ep
import test_gpu_tick_plant as tp
from test_gpu_tick_plant import B, DT, _bits, _caller_rows

pytestmark = pytest.mark.gpu

EPISODE = ("episode_state", "episode_log", "episode_totals", "plant_init")
NAMES = {"mpc": tp.MPC + EPISODE,
         "full": ("results", "torques", "counter", "states", "plan_in", "cmd", "records", "plan_out", "est_out",
                  "sensors", "tq_records", "plant_out", "warm", "plan_state", "est_state", "cmd_state",
                  "plant_state") + EPISODE}
# the names of the tick's buffers in tests/episode_reference.step
REF = dict(plant_out="plant_out", plant_state="plant_state", plant_init="plant_init", torques="joint_torques",
           sensors="sensors", cmd="cmd", results="results", episode_pool="pool", episode_scripts="scripts",
           states="states", counter="counter", est_state="est_state", plan_state="plan_state", cmd_state="cmd_state",
           policy_state="policy_state", warm="warm")


def _stance_pool(kind, tilts=((0.0, 0.0, 0.0),)):
    """Pool rows at the stance the tick's controller holds: the default stance for the MPC-only tick, the command
    stage's body height for the full one."""
    if kind == "full":
        pp = mpcqp.default_plant_params()
        q1 = float(np.arccos(mpcqp.default_command_params().body_height_init / (2.0 * pp.rho_fix[3])))
        q = [0.0, q1, -2.0 * q1]
    else:
        q = [0.0, 0.8, -1.6]
    rows, hs = zip(*(ec.start_row(q, t) for t in tilts))
    return ec.pool_rows(np.array(rows), np.array(hs), [t[2] for t in tilts])


SCRIPT = [[(0, (0, 0, 0), (0, 0, 0), False), (4, (0, 0, 0), (0, 0, 0.2), False), (8, (0.2, 0, 0), (0, 0, 0), True)]]


def _make(kind, pool, epar, scripts=None, plant=None, log_len=4):
    pp = plant if plant is not None else mpcqp.default_plant_params()
    kw = dict(dt=DT, plant=pp, episode=epar, episode_pool=pool, episode_scripts=scripts, episode_log_len=log_len)
    if kind in ("full", "typed"):
        if kind == "typed":
            kw["control_type"] = "per_robot"
        k = ControlTick(B, plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                        command=mpcqp.default_command_params(), **kw)
    else:
        k = ControlTick(B, **kw)
    rows, tq = _caller_rows()
    k.states.copy_(torch.from_numpy(rows))
    k.tq_records.copy_(torch.from_numpy(tq))
    return k


def _staged(k, kind):
    """ControlTick.step's stages, one entry point at a time on the object's buffers, the episode stage on a
    buffers struct of its own."""
    s = torch.cuda.current_stream().cuda_stream
    full = kind == "full"
    if full:
        mpcqp.command_device(k.command, k.dt, k.cmd.data_ptr(), k.states.data_ptr(), k.plan_in.data_ptr(), B,
                             k.cmd_state.data_ptr(), s)
        mpcqp.state_estimate_device(k.estimator, k.dt, k.sensors.data_ptr(), k.plan_in.data_ptr(), k.states.data_ptr(),
                                    B, k.est_state.data_ptr(), k.tq_records.data_ptr(), k.est_out.data_ptr(), s)
        mpcqp.leg_plan_device(k.plan, k.dt, k.states.data_ptr(), k.plan_in.data_ptr(), B, k.plan_state.data_ptr(),
                              k.tq_records.data_ptr(), k.plan_out.data_ptr(), s)
    mpcqp.assemble_records_device(10, k.states.data_ptr(), B, k.records.data_ptr(), s)
    k.solver.solve_warm_device(k.records.data_ptr(), B, k.warm.data_ptr(), k.results.data_ptr(), 0, s)
    mpcqp.joint_torques_device(k.tq_records.data_ptr(), k.results.data_ptr(), B, k.counter.data_ptr(),
                               k.torques.data_ptr(), s)
    mpcqp.plant_step_device(k.plant, k.dt, k.torques.data_ptr(), B, k.plant_state.data_ptr(), k.plant_init.data_ptr(),
                            k.sensors.data_ptr() if full else 0, k.plan_in.data_ptr(),
                            0 if full else k.states.data_ptr(), 0 if full else k.tq_records.data_ptr(),
                            k.plant_out.data_ptr(), s)
    p = lambda n: getattr(k, n).data_ptr() if getattr(k, n, None) is not None else 0
    n = lambda name: getattr(k, name).shape[1] if hasattr(k, name) else 0
    bf = mpcqp.episode_buffers(
        d_plant_out=p("plant_out"), d_plant_state=p("plant_state"), d_plant_init=p("plant_init"),
        d_joint_torques=p("torques"), d_sensors=p("sensors"), d_cmd=p("cmd"), d_results=p("results"),
        d_pool=p("episode_pool"), d_scripts=p("episode_scripts"), d_states=p("states"), d_counter=p("counter"),
        d_log=p("episode_log"), d_totals=p("episode_totals"), d_est_state=p("est_state"),
        est_state_size=n("est_state"), d_plan_state=p("plan_state"), plan_state_size=n("plan_state"),
        d_cmd_state=p("cmd_state"), cmd_state_size=n("cmd_state"), d_warm=p("warm"), warm_size=n("warm"))
    mpcqp.episode_device(k.episode, bf, B, k.episode_state.data_ptr(), s)


def _snap(k, names):
    return {n: _bits(getattr(k, n)) for n in names}


# ---- 1. fused = staged = graph replays ----
T1 = 30
_RUNS = {}


def _runs(kind):
    if kind not in _RUNS:
        out = {}
        for how in ("eager", "staged", "graph"):
            epar = mpcqp.default_episode_params(max_ticks=12, seed=7)
            pool = _stance_pool(kind, ((0.0, 0.0, 0.0), (0.02, -0.03, 0.4)))
            k = _make(kind, pool, epar, mpcqp.pack_episode_scripts(SCRIPT) if kind == "full" else None)
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
    tot = out["eager"][-1]["episode_totals"].view(np.float64)
    print(f"[note] {kind} tick, {T1} ticks: totals per robot {tot.tolist()}")
    assert np.all(tot[:, ep.ET_EPISODES] >= 2.0) and np.all(tot[:, ep.ET_REASON + ep.END_FRESH] == 1.0)
    # (the torque map holds zero torques for the first nine ticks of every episode)
    assert max(np.abs(o["torques"].view(np.float64)).max() for o in out["eager"]) > 0


def test_per_robot_typed_tick_ends_with_the_stage_too():
    """The tick with a control type per robot (balance QP for some, MPC for the others) takes the other step
    path: its eager steps and its graph's replays agree bitwise, and episodes complete."""
    names = NAMES["full"] + ("bal_records",)
    rows = {}
    for how in ("eager", "graph"):
        k = _make("typed", _stance_pool("full"), mpcqp.default_episode_params(max_ticks=12, seed=7),
                  mpcqp.pack_episode_scripts(SCRIPT))
        try:
            k.control_type.copy_(torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32))
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
    tot = rows["eager"][-1]["episode_totals"].view(np.float64)
    print(f"[note] typed tick: totals per robot {tot.tolist()}")
    assert np.all(tot[:, ep.ET_EPISODES] >= 2.0)


# ---- 2. the real freeze-and-restart path ----
def _mixed_seed(count, episodes=2):
    """A seed whose draws for the B robots' first episodes hit every pool row."""
    for seed in range(1, 100):
        if {ep.draw(seed, b, e, count, 0)[0] for b in range(B) for e in range(episodes)} == set(range(count)):
            return seed
    raise AssertionError("no seed")


def _ref_arrays(k, pre, own):
    a = {REF[n]: pre[n] for n in REF if n in pre}
    a.update(own)
    return a


def _follow(k, T, p):
    """T eager ticks with a read before and after the episode stage of every tick: the restatement, fed the
    device's rows of before the stage, gives every row of after it bitwise.  Returns the rows before each stage."""
    names = [n for n in REF if getattr(k, n, None) is not None]
    own = dict(episode_state=np.zeros((B, ep.ES_SIZE)), log=np.zeros((B, p.log_len, ep.EL_SIZE)),
               totals=np.zeros((B, ep.ET_SIZE)))
    seen = []
    for t in range(T):
        k.step(episode=False)
        torch.cuda.synchronize()
        pre = {n: getattr(k, n).cpu().numpy().copy() for n in names}
        seen.append({n: pre[n].copy() for n in ("plant_out", "torques", "results")})
        k.episode_stage()
        torch.cuda.synchronize()
        ep.step(p, _ref_arrays(k, pre, own), B)
        for n in names:
            got = getattr(k, n).cpu().numpy()
            assert np.array_equal(got.view(np.int64) if got.dtype == np.float64 else got,
                                  pre[n].view(np.int64) if got.dtype == np.float64 else pre[n]), f"tick {t}: {n}"
        for n, dn in (("episode_state", "episode_state"), ("log", "episode_log"), ("totals", "episode_totals")):
            got = getattr(k, dn).cpu().numpy().reshape(own[n].shape)
            assert np.array_equal(got.view(np.int64), own[n].view(np.int64)), f"tick {t}: {dn}"
    return seen, own


def _ref_params(k, seed):
    e = k.episode
    return ep.Params(dt=e.dt, tilt_max=e.tilt_max, height_min=e.height_min, height_max=e.height_max, seed=seed,
                     max_ticks=e.max_ticks, pool_count=e.pool_count, script_count=e.script_count,
                     script_segments=e.script_segments, log_len=e.log_len)


@pytest.mark.parametrize("case", ["crouch", "timeout", "tilted"])
def test_freeze_and_restart_is_the_restatement(case):
    """crouch: plant min_height 0.25, pool = the 0.29 m stance and a crouch under 0.25 m: the crouchers are frozen
    with plant status 2, end with reason 2 and are restarted with a fresh draw.  timeout: max_ticks 12.  tilted:
    a pool row 0.09 rad off level with tilt_max 0.05 ends with the envelope reason."""
    plant = None
    if case == "crouch":
        plant = mpcqp.default_plant_params(min_height=0.25)
        crouch, zc = ec.start_row([0.0, 1.2, -2.4])
        pool = np.concatenate([_stance_pool("mpc"), ec.pool_rows(crouch[None], [zc])])
        over = dict(max_ticks=15)
    elif case == "timeout":
        pool, over = _stance_pool("mpc"), dict(max_ticks=12)
    else:
        pool, over = _stance_pool("mpc", ((0.0, 0.0, 0.0), (0.09, 0.0, 0.0))), dict(max_ticks=12, tilt_max=0.05)
    seed = _mixed_seed(pool.shape[0])
    k = _make("mpc", pool, mpcqp.default_episode_params(seed=seed, **over), plant=plant, log_len=8)
    try:
        p = _ref_params(k, seed)
        _, own = _follow(k, 40, p)
    finally:
        k.close()
    log = own["log"].reshape(-1, ep.EL_SIZE)
    log = log[log[:, ep.EL_LENGTH] > 0]
    print(f"[note] {case}: totals {own['totals'].sum(0).tolist()}, (pool, length, reason) "
          f"{log[:, [ep.EL_POOL, ep.EL_LENGTH, ep.EL_REASON]].tolist()}")
    second = log[log[:, ep.EL_POOL] == 1.0]
    first = log[log[:, ep.EL_POOL] == 0.0]
    assert len(first) > 0 and np.all(own["totals"][:, ep.ET_EPISODES] >= 2.0)
    if case == "crouch":
        assert len(second) > 0 and np.all(second[:, ep.EL_REASON] == ep.END_FALLEN) and np.all(second[:, ep.EL_LENGTH] == 1.0)
    elif case == "timeout":
        assert np.all(log[:, ep.EL_REASON] == ep.END_TIMEOUT) and np.all(log[:, ep.EL_LENGTH] == 12.0)
    else:
        assert len(second) > 0 and np.all(second[:, ep.EL_REASON] == ep.END_ENVELOPE) and np.all(second[:, ep.EL_LENGTH] == 1.0)
        assert np.all(first[:, ep.EL_REASON] == ep.END_TIMEOUT)


# ---- 3. a reset is complete ----
@pytest.mark.parametrize("kind", ["mpc", "full"])
def test_every_episode_is_bitwise_the_one_before_and_a_fresh_tick(kind):
    """A pool of one row, one script, max_ticks 14 (past the torque map's nine zero-torque ticks): the rows of
    every tick of an episode are those of the episode before, and episode 0 is a freshly constructed tick without
    the stage, started by prime_plant() on the same init row and caller rows."""
    M, E = 14, 3
    pool = _stance_pool(kind, ((0.01, -0.02, 0.3),))
    scripts = mpcqp.pack_episode_scripts(SCRIPT) if kind == "full" else None
    k = _make(kind, pool, mpcqp.default_episode_params(max_ticks=M, seed=3), scripts)
    try:
        seen, own = _follow(k, 1 + E * (M + 1), _ref_params(k, 3))
    finally:
        k.close()
    log = own["log"]
    assert np.all(own["totals"][:, ep.ET_EPISODES] == E) and np.all(own["totals"][:, ep.ET_REASON + ep.END_TIMEOUT] == E)
    episodes = [[seen[2 + e * (M + 1) + i] for i in range(M)] for e in range(E)]
    for e in range(1, E):
        for i in range(M):
            for name in ("plant_out", "torques", "results"):
                assert np.array_equal(episodes[e][i][name].view(np.int64), episodes[e - 1][i][name].view(np.int64)), \
                    f"{kind}: {name} at tick {i} of episode {e} is not that of episode {e - 1}: a row leaks across a restart"
        assert np.array_equal(log[:, e, 1:].view(np.int64), log[:, e - 1, 1:].view(np.int64)), f"log row of episode {e}"
        assert np.all(log[:, e, ep.EL_EPISODE] == e)
    # a fresh tick without the stage
    pp = mpcqp.default_plant_params()
    init = np.repeat(pool[:, :_lib.PI_SIZE], B, 0)
    if kind == "full":
        f = ControlTick(B, plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                        command=mpcqp.default_command_params(), dt=DT, plant=pp, plant_init=init)
    else:
        f = ControlTick(B, dt=DT, plant=pp, plant_init=init)
    try:
        assert f.episode is None and not hasattr(f, "episode_state")
        rows, tq = _caller_rows()
        rows[:, _lib.ST_EULER_D:_lib.ST_EULER_D + 3] = pool[0, ep.POOL_EULER_D:ep.POOL_EULER_D + 3]
        rows[:, _lib.ST_POS_D:_lib.ST_POS_D + 3] = pool[0, ep.POOL_POS_D:ep.POOL_POS_D + 3]
        if kind == "full":  # the estimator's first tick leaves these as the caller wrote them; the stage: zero
            rows[:, _lib.ST_POS:_lib.ST_POS + 3] = 0.0
            rows[:, _lib.ST_LIN_VEL:_lib.ST_LIN_VEL + 3] = 0.0
        f.states.copy_(torch.from_numpy(rows))
        f.tq_records.copy_(torch.from_numpy(tq))
        f.prime_plant()
        for i in range(M):
            if kind == "full":
                for tick, vel, rate, request in SCRIPT[0]:
                    if tick == i:
                        f.cmd.copy_(torch.from_numpy(mpcqp.pack_commands(np.tile(vel, (B, 1)), np.tile(rate, (B, 1)),
                                                                         np.full(B, request))))
            f.step()
            torch.cuda.synchronize()
            for name in ("plant_out", "torques", "results"):
                assert np.array_equal(_bits(getattr(f, name)), episodes[0][i][name].view(np.int64)), \
                    f"{kind}: {name} at tick {i} of episode 0 is not that of a fresh tick"
    finally:
        f.close()


# ---- 4. a tick built without episode= ----
@pytest.mark.parametrize("kind", ["mpc", "full"])
def test_tick_without_episode_enqueues_what_it_did(kind):
    """The tick of tests/test_gpu_tick_plant.py, built without episode=: no episode buffer exists, and T ticks are
    bitwise the staged calls of the entry points as they were."""
    names = tp.FULL if kind == "full" else tp.MPC
    out = {}
    for how in ("eager", "staged"):
        k = tp._make(kind)
        try:
            assert k.episode is None and not hasattr(k, "episode_state") and not hasattr(k, "episode_buffers")
            out[how] = tp._drive(k, kind, how, names)
        finally:
            k.close()
    for t, (a, b) in enumerate(zip(out["eager"], out["staged"])):
        for name in names:
            assert np.array_equal(a[name], b[name]), f"{kind} tick {t}: {name}"
