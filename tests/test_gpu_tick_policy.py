"""The tick with the policy stage: command -> estimate -> plan -> assemble -> balance solve (type 0) -> warm MPC
solve (type 1) -> torque map -> policy stage (type 2), with types 0 / 1 / 2 / 3 mixed and changing between ticks.
Type-2 robots' torques are bitwise a standalone mpcqp_policy_device call on the same rows; everything else is
bitwise the same tick built without policy=; a type-3 robot keeps its result row; the graph replay is bitwise
the eager tick."""
import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib
from mpcqp.tick import ControlTick

import policy_reference as ref
from test_gpu_tick_modes import ROWS, SLOTS, _bits, _inputs

pytestmark = pytest.mark.gpu

B, T = 67, 6
POLICY_ROWS = ("policy_state", "policy_out")


def _types():
    rng = np.random.default_rng(62)
    types = np.empty((T, B), np.int32)
    types[0:] = rng.integers(0, 4, B)
    types[2:] = rng.integers(0, 4, B)   # the types change on ticks 2 and 4
    types[4:] = rng.integers(0, 4, B)
    types[:, 7] = 3                     # never solved by any branch
    types[:, 8] = 2                     # always the policy
    return types


def _make(policy):
    return ControlTick(B, plan=mpcqp.default_plan_params(), estimator=mpcqp.default_estimator_params(),
                       command=mpcqp.default_command_params(), control_type="per_robot", policy=policy)


def _drive(k, inputs, types, how, standalone=None):
    states_t, sensors, plan_in, cmds, _, tq = inputs
    k.tq_records.copy_(torch.from_numpy(tq))
    k.states.copy_(torch.from_numpy(mpcqp.pack_states(states_t[0])))
    names = ROWS + SLOTS + (POLICY_ROWS if k.policy is not None else ())
    outs = []
    for t in range(T):
        k.sensors.copy_(torch.from_numpy(sensors[t]))
        k.plan_in[:, _lib.PL_FOOT_FORCE:_lib.PL_FOOT_FORCE + 4].copy_(
            torch.from_numpy(plan_in[t][:, _lib.PL_FOOT_FORCE:_lib.PL_FOOT_FORCE + 4]))
        k.cmd.copy_(torch.from_numpy(cmds[t]))
        k.control_type.copy_(torch.from_numpy(types[t]))
        if how == "graph":
            if k.graph is None:
                k.capture()
            k.replay()
        else:
            k.step()
        torch.cuda.synchronize()
        o = {name: _bits(getattr(k, name)) for name in names}
        if standalone is not None:
            # the same stage called by itself on the rows the tick left (the policy stage writes none of them)
            pol, slot, tau, out = standalone
            mpcqp.policy_device(pol, k.sensors.data_ptr(), k.states.data_ptr(), k.plan_in.data_ptr(), k.cmd.data_ptr(), B,
                                slot.data_ptr(), tau.data_ptr(), out.data_ptr(), k.control_type.data_ptr(), 2,
                                torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            o.update(alone_slot=_bits(slot), alone_tau=_bits(tau), alone_out=_bits(out))
        outs.append(o)
    return outs


@pytest.fixture(scope="module")
def runs():
    inputs, types = _inputs(), _types()
    ws, bs = ref.seeded_weights(31)
    out = {}
    with mpcqp.Policy(ws, bs) as pol:
        f64 = dict(dtype=torch.float64, device="cuda")
        alone = (pol, torch.zeros((B, mpcqp.policy_state_size()), **f64), torch.zeros((B, 12), **f64),
                 torch.zeros((B, _lib.PY_SIZE), **f64))
        for how, policy, standalone in (("eager", pol, alone), ("graph", pol, None), ("plain", None, None)):
            k = _make(policy)
            try:
                out[how] = _drive(k, inputs, types, how, standalone)
            finally:
                k.close()
    return types, out


def test_policy_robots_are_the_standalone_stage(runs):
    types, out = runs
    for t, o in enumerate(out["eager"]):
        p2 = types[t] == 2
        assert np.array_equal(o["torques"][p2], o["alone_tau"][p2]), f"tick {t}"
        assert np.array_equal(o["policy_state"], o["alone_slot"]) and np.array_equal(o["policy_out"], o["alone_out"])
        ticks = o["policy_state"].view(np.float64)[:, _lib.PS_TICK]
        assert np.array_equal(ticks, (types[:t + 1] == 2).sum(0).astype(np.float64))   # a slot advances only when selected
        out_rows = o["policy_out"].view(np.float64)
        assert np.array_equal(out_rows[p2][:, _lib.PY_TORQUE:_lib.PY_TORQUE + 12], o["torques"].view(np.float64)[p2])
        assert not out_rows[p2][:, _lib.PY_STATUS].any()
    assert np.abs(out["eager"][-1]["torques"].view(np.float64)[types[-1] == 2]).max() > 0


def test_other_robots_are_the_tick_without_policy(runs):
    types, out = runs
    for t, (a, b) in enumerate(zip(out["eager"], out["plain"])):
        for name in ROWS + SLOTS:
            if name == "torques":
                keep = types[t] != 2
                assert np.array_equal(a[name][keep], b[name][keep]), f"tick {t}: torques of the type 0 / 1 / 3 robots"
                assert not np.array_equal(a[name][~keep], b[name][~keep])
            else:
                assert np.array_equal(a[name], b[name]), f"tick {t}: {name} with and without policy="
        assert not a["results"][7].any() and not a["results"][8].any()   # type 3 and type 2: the row they started with
    for ty in range(4):
        assert (types == ty).sum() > 5


def test_graph_replay_is_the_eager_tick(runs):
    _, out = runs
    for t, (a, b) in enumerate(zip(out["eager"], out["graph"])):
        for name in ROWS + SLOTS + POLICY_ROWS:
            assert np.array_equal(a[name], b[name]), f"tick {t}: {name} of the eager tick and the graph replay differ"


def test_policy_needs_a_typed_tick():
    ws, bs = ref.seeded_weights(31, hidden=(32,))
    with mpcqp.Policy(ws, bs) as pol:
        with pytest.raises(ValueError):
            ControlTick(B, policy=pol)
        with pytest.raises(ValueError):
            ControlTick(B, control_type=1, policy=pol)
        with pytest.raises(ValueError):
            ControlTick(B, control_type=2)
        k = ControlTick(4, control_type=2, policy=pol)   # every robot takes the policy branch
        try:
            assert k.control_type.cpu().tolist() == [2] * 4
            assert k.sensors.shape == (4, _lib.SN_SIZE) and k.cmd.shape == (4, _lib.CM_SIZE)
            q = torch.from_numpy(np.tile(ref.DEFAULT_JOINT_POS + 0.1, (4, 1))).cuda()
            k.sensors[:, _lib.SN_JOINT_POS:_lib.SN_JOINT_POS + 12] = q
            k.step()
            torch.cuda.synchronize()
            # movement_mode 0: the servo stand's first tick on every robot
            p = ref.default_params()
            blk = ref.PolicyBlock(4, p)
            o = blk.step(np.zeros(4), q.cpu().numpy(), np.zeros((4, 12)), np.zeros((4, 12)))
            assert np.array_equal(_bits(k.torques), o["tau"].view(np.int64))
        finally:
            k.close()
