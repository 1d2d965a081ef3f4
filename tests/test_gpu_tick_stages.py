"""ControlTick's stage list.  One table gives, per constructor configuration, the stages the tick enqueues, the
device tensors it owns (a buffer it does not own is an absent attribute) and what leaving each droppable stage out
gives: the shorter list, or the ValueError the constructor has for that combination.  A graph captured without a
stage is bitwise the graph of a tick built without it, on every buffer the two share; and the tick enqueued without
its episode stage and then the stage alone is bitwise the tick."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib
from mpcqp.episode import POOL_INIT
from mpcqp.tick import ControlTick

import policy_reference as ref
import test_gpu_tick_episode as te
from test_gpu_tick_disturb import _caller_rows, _params
from test_gpu_tick_plant import DT, _bits

pytestmark = pytest.mark.gpu

B = 4  # horizon 10: the default params

BASE = {"states", "tq_records", "records", "warm", "results", "counter", "torques"}
PLAN = {"plan_in", "plan_state", "plan_out"}
EST = {"plan_in", "sensors", "est_state", "est_out"}
CMD = {"plan_in", "cmd", "cmd_state"}
TYPED = {"plan_in", "control_type", "bal_records"}
POLICY = {"sensors", "cmd", "policy_state", "policy_out"}
PLANT = {"plan_in", "plant_state", "plant_out"}
EPISODE = {"episode_state", "episode_log", "episode_totals", "episode_pool", "plant_init"}
DISTURB = {"wrench", "disturb_out"}

MPC3 = ("assemble", "solve", "torques")
TYPED5 = ("assemble", "assemble_balance", "balance", "solve", "torques")
ALL = ("disturb", "command", "estimate", "plan") + TYPED5 + ("policy", "plant", "episode")

E_EST_DT = r"ControlTick\(estimator=\.\.\.\) without plan= needs dt"
E_TYPE = r"control_type must be None, 0, 1 or \"per_robot\""
E_POLICY = r"ControlTick\(policy=\.\.\.\) needs control_type="
E_EPISODE = r"ControlTick\(episode=\.\.\.\) needs plant= and episode_pool="
E_DISTURB = r"ControlTick\(disturb=\.\.\.\) needs plant= and episode="

# the stages `without=` takes, and what each takes out of the list: the two balance stages go together
DROPS = {"disturb": ("disturb",), "command": ("command",), "estimate": ("estimate",), "plan": ("plan",),
         "assemble_balance": ("assemble_balance", "balance"), "balance": ("assemble_balance", "balance"),
         "policy": ("policy",), "plant": ("plant",), "episode": ("episode",)}

# configuration: (the constructor's options, stages(), the tensor attributes, {dropped stage: its ValueError});
# a dropped stage that is not named leaves the list without it
CONFIGS = {
    "mpc": ((), MPC3, BASE, {}),
    "plan": (("plan",), ("plan",) + MPC3, BASE | PLAN, {}),
    "estimator_plan": (("estimator", "plan"), ("estimate", "plan") + MPC3, BASE | PLAN | EST, {"plan": E_EST_DT}),
    "command_estimator_plan": (("command", "estimator", "plan", "dt"), ("command", "estimate", "plan") + MPC3,
                               BASE | PLAN | EST | CMD, {}),
    "type0": (("type0",), TYPED5, BASE | TYPED, {}),
    "type1": (("type1",), TYPED5, BASE | TYPED, {}),
    "per_robot": (("per_robot",), TYPED5, BASE | TYPED, {}),
    "per_robot_policy": (("per_robot", "policy"), TYPED5 + ("policy",), BASE | TYPED | POLICY,
                         {"assemble_balance": E_POLICY, "balance": E_POLICY}),
    "type2_policy": (("type2", "policy"), TYPED5 + ("policy",), BASE | TYPED | POLICY,
                     {"assemble_balance": E_POLICY, "balance": E_POLICY, "policy": E_TYPE}),
    "plant": (("dt", "plant"), MPC3 + ("plant",), BASE | PLANT, {}),
    "plant_episode": (("dt", "plant", "episode"), MPC3 + ("plant", "episode"), BASE | PLANT | EPISODE,
                      {"plant": E_EPISODE}),
    "plant_episode_disturb": (("dt", "plant", "episode", "disturb"), ("disturb",) + MPC3 + ("plant", "episode"),
                              BASE | PLANT | EPISODE | DISTURB, {"plant": E_EPISODE, "episode": E_DISTURB}),
    "full": (("command", "estimator", "plan", "dt", "per_robot", "policy", "plant", "episode", "scripts", "disturb",
              "dirs"), ALL,
             BASE | PLAN | EST | CMD | TYPED | POLICY | PLANT | EPISODE | DISTURB |
             {"episode_scripts", "disturb_dirs", "sensors_noisy"},
             {"assemble_balance": E_POLICY, "balance": E_POLICY, "plant": E_EPISODE, "episode": E_DISTURB}),
}


@pytest.fixture(scope="module")
def policy():
    ws, bs = ref.seeded_weights(31)
    with mpcqp.Policy(ws, bs) as pol:
        yield pol


def _build(options, policy, disturb=None, plant_init=None):
    """The tick of `options` with the caller's rows written: "full"-style options stand at the command stage's
    body height, the others at the default stance."""
    o = set(options)
    kind = "full" if "command" in o else "mpc"
    kw = {}
    if "plan" in o:
        kw["plan"] = mpcqp.default_plan_params()
    if "estimator" in o:
        kw["estimator"] = mpcqp.default_estimator_params()
    if "command" in o:
        kw["command"] = mpcqp.default_command_params()
    if "dt" in o:
        kw["dt"] = DT
    for name, value in (("type0", 0), ("type1", 1), ("type2", 2), ("per_robot", "per_robot")):
        if name in o:
            kw["control_type"] = value
    if "policy" in o:
        kw["policy"] = policy
    if "plant" in o:
        kw.update(plant=mpcqp.default_plant_params(), plant_init=plant_init)
    if "episode" in o:
        kw.update(episode=mpcqp.default_episode_params(max_ticks=12, seed=7), episode_pool=_pool(kind))
    if "scripts" in o:
        kw["episode_scripts"] = mpcqp.pack_episode_scripts(te.SCRIPT)
    if "disturb" in o:
        kw["disturb"] = disturb if disturb is not None else mpcqp.default_disturb_params()
    if "dirs" in o:
        kw["disturb_dirs"] = mpcqp.pack_push_dirs(8)
    k = ControlTick(B, **kw)
    rows, tq = _caller_rows(B)
    k.states.copy_(torch.from_numpy(rows))
    k.tq_records.copy_(torch.from_numpy(tq))
    if "per_robot" in o:
        k.control_type.copy_(torch.tensor([1, 0, 2 if "policy" in o else 0, 1], dtype=torch.int32))
    return k


def _pool(kind):
    return te._stance_pool(kind, ((0.0, 0.0, 0.0), (0.02, -0.03, 0.4)))


def _tensors(k):
    return {n for n, v in vars(k).items() if isinstance(v, torch.Tensor)}


# ---- 1. the table ----
@pytest.mark.parametrize("config", list(CONFIGS))
def test_stages_and_buffers_follow_the_table(config, policy):
    options, stages, tensors, errors = CONFIGS[config]
    k = _build(options, policy)
    try:
        assert k.stages() == stages
        assert _tensors(k) == tensors
        for drop, gone in DROPS.items():
            if drop in errors:
                with pytest.raises(ValueError, match=errors[drop]):
                    k.stages(without=(drop,))
                with pytest.raises(ValueError, match=errors[drop]):
                    k.capture(without=(drop,))
            else:
                assert k.stages(without=(drop,)) == tuple(s for s in stages if s not in gone), drop
        for fixed in MPC3 + ("no_such_stage",):
            with pytest.raises(ValueError, match="not a stage that can be left out"):
                k.stages(without=(fixed,))
        assert k.stages() == stages and k.graph is None  # asking changed nothing
    finally:
        k.close()


# ---- 2. a graph captured without a stage is the graph of a tick built without it ----
KINDS = {"mpc": ("dt", "plant"),
         "full": ("command", "estimator", "plan", "dt", "per_robot", "policy", "plant")}
WITH = {"disturb": ("episode", "disturb"), "episode": ("episode",), "plant": ()}
CASES = [("disturb", "off"), ("disturb", "on"), ("episode", None), ("plant", None)]


@pytest.mark.parametrize("stage,params", CASES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_graph_without_a_stage_is_the_tick_built_without_it(kind, stage, params, policy):
    """A has the stage, B was built without it (and, for the episode stage, with the init rows A takes from its
    pool).  From the same rows, three replays of A's graph without the stage and of B's graph leave every buffer
    the two ticks share bitwise the same.  A's own buffers hold a fill first, which no kernel of the graph without
    the stage may read."""
    base = KINDS[kind] + (("scripts",) if kind == "full" and stage != "plant" else ())
    a_opt = base + WITH[stage] + (("dirs",) if params == "on" else ())
    b_opt = tuple(o for o in a_opt if o not in (stage, "dirs")) if stage != "plant" else \
        tuple(o for o in base if o != "plant")
    if stage == "episode":
        b_opt = tuple(o for o in b_opt if o != "scripts")
    dp = _params() if params == "on" else None
    init = None
    if stage == "episode":
        init = np.repeat(_pool(kind)[:1, POOL_INIT:POOL_INIT + _lib.PI_SIZE], B, 0)
    a, b = _build(a_opt, policy, disturb=dp), _build(b_opt, policy, plant_init=init)
    try:
        assert stage in a.stages() and stage not in b.stages()
        assert a.stages(without=(stage,)) == b.stages()
        common = sorted(_tensors(a) & _tensors(b))
        assert _tensors(b) <= _tensors(a) and set(common) >= BASE
        if stage == "plant":
            a.prime_plant()  # sensor-level rows of a standing robot, which B's caller has to write
            a.counter.fill_(100)  # past the torque map's zero-torque ticks
        for name in _tensors(a) - _tensors(b) - {"episode_pool", "episode_scripts", "disturb_dirs"}:
            getattr(a, name).fill_(7.0)
        for name in common:
            getattr(b, name).copy_(getattr(a, name))
        ga, gb = a.capture(without=(stage,)), b.capture()
        assert a.graph is None and b.graph is gb
        for t in range(3):
            ga.replay()
            gb.replay()
            torch.cuda.synchronize()
            for name in common:
                assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), f"tick {t}: {name}"
        assert a.results.any() and a.counter.min() >= 1  # the graphs ran the tick
        for name in _tensors(a) - _tensors(b) - {"episode_pool", "episode_scripts", "disturb_dirs"}:
            assert torch.all(getattr(a, name) == 7.0), f"{name} was written by the graph without {stage}"
    finally:
        a.close()
        b.close()


# ---- 3. the episode stage on its own ----
def test_step_without_episode_then_the_stage_is_the_step(policy):
    options = CONFIGS["full"][0]
    a, b = _build(options, policy, disturb=_params()), _build(options, policy, disturb=_params())
    try:
        names = sorted(_tensors(a))
        for t in range(3):
            a.step()
            b.step(episode=False)
            b.episode_stage()
            torch.cuda.synchronize()
            for name in names:
                assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), f"tick {t}: {name}"
        assert a.episode_state.any()
    finally:
        a.close()
        b.close()
