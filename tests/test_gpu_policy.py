"""mpcqp_policy_device on the GPU against the numpy restatement of src/go1_rl_ctrl_cpp's controller
(tests/policy_reference.py).

  1  an exact-integer network: the raw output bitwise, for the reference's widths and for hidden = [64, 32]
  2  observation, action, targets, slot and torques bitwise over 12 ticks, both observation clips, the action clip
     and both pose limits reached
  3  the float32 network within 4 x (torch CPU float32's own error) of the binary64 evaluation
  4  modes mixed in a tile and switched, decimation, selection by control type, a planted NaN
  5  arguments
B = 1, 33 (one robot past a 32-robot tile) and 67; rows past the batch are NaN-filled and must not change."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mpcqp
from mpcqp import _lib

import policy_reference as ref

pytestmark = pytest.mark.gpu

PAD = 3  # rows past the batch, NaN-filled: the stage must not touch them
SIZES = [1, 33, 67]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(name, got, exp):
    bad = np.argwhere(_bits(got) != _bits(exp))
    assert bad.size == 0, f"{name}: first differing (row, double) {bad[:5].tolist()}"


def make_inputs(B, T, seed, big=False, integer=False):
    """[T, B, ...] inputs of the stage.  big: magnitudes that reach both observation clips."""
    rng = np.random.default_rng(seed)
    if integer:
        draw = lambda *s: rng.integers(0, 2, s).astype(np.float64)
        rot = np.tile(np.array([1.0, 0, 0, 0, -1.0, 0, 0, 0, -1.0]), (T, B, 1))  # gravity entry (0, 0, 1)
        rot_z = np.tile(np.eye(3).reshape(9), (T, B, 1))
        return dict(rot_z=rot_z, lin_vel=draw(T, B, 3), imu=draw(T, B, 3), rot=rot, joy=draw(T, B, 3), q=draw(T, B, 12),
                    dq=draw(T, B, 12), mode=np.ones((T, B)))
    yaw = rng.uniform(-3.0, 3.0, (T, B))
    rot_z = np.zeros((T, B, 9))
    rot_z[..., 0], rot_z[..., 1], rot_z[..., 3], rot_z[..., 4], rot_z[..., 8] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    rot = rot_z + rng.normal(0.0, 0.1, (T, B, 9))
    s = 1.0
    lin_vel, imu, dq = rng.normal(0, 0.5, (T, B, 3)), rng.normal(0, 1.0, (T, B, 3)), rng.normal(0, 3.0, (T, B, 12))
    if big:
        lin_vel = lin_vel * np.where(rng.random((T, B, 1)) < 0.3, 200.0, s)   # x 2 -> beyond +-100
        dq = dq * np.where(rng.random((T, B, 1)) < 0.3, 1500.0, s)            # x 0.05 -> beyond +-100
    q = ref.DEFAULT_JOINT_POS + rng.normal(0, 0.3, (T, B, 12))
    return dict(rot_z=rot_z, lin_vel=lin_vel, imu=imu, rot=rot, joy=rng.uniform(-1, 1, (T, B, 3)), q=q, dq=dq,
                mode=np.ones((T, B)))


class Rig:
    """Device buffers of one batch: NaN past the batch, distinct finite sentinels where the stage must not write."""

    def __init__(self, B, seed=77):
        rng = np.random.default_rng(seed)
        self.B = B

        def sentinel(width):
            a = np.full((B + PAD, width), np.nan)
            a[:B] = 1000.0 + rng.permutation(B * width).reshape(B, width)
            return a

        self.sn0, self.st0, self.pl0, self.cm0 = (sentinel(w) for w in (_lib.SN_SIZE, _lib.ST_SIZE, _lib.PL_SIZE, _lib.CM_SIZE))
        self.tau0, self.out0 = sentinel(12), sentinel(_lib.PY_SIZE)
        self.slot0 = np.full((B + PAD, mpcqp.policy_state_size()), np.nan)
        self.slot0[:B] = 0.0
        self.d = {k: torch.from_numpy(getattr(self, k + "0").copy()).cuda() for k in ("sn", "st", "pl", "cm", "tau", "out", "slot")}
        self.d_type = None

    def write(self, inp, t):
        B, d = self.B, self.d
        put = lambda buf, off, a: buf[:B, off:off + a.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(a)))
        put(d["sn"], _lib.SN_JOINT_POS, inp["q"][t])
        put(d["sn"], _lib.SN_JOINT_VEL, inp["dq"][t])
        put(d["sn"], _lib.SN_IMU_ANG_VEL, inp["imu"][t])
        put(d["st"], _lib.ST_LIN_VEL, inp["lin_vel"][t])
        put(d["st"], _lib.ST_ROT, inp["rot"][t])
        put(d["pl"], _lib.PL_ROT_Z, inp["rot_z"][t])
        put(d["pl"], _lib.PL_MOVEMENT_MODE, inp["mode"][t][:, None])
        put(d["cm"], _lib.CM_VEL, inp["joy"][t][:, :2])
        put(d["cm"], _lib.CM_RATE + 2, inp["joy"][t][:, 2:3])

    def tick(self, policy, want=2):
        d = self.d
        mpcqp.policy_device(policy, d["sn"].data_ptr(), d["st"].data_ptr(), d["pl"].data_ptr(), d["cm"].data_ptr(), self.B,
                            d["slot"].data_ptr(), d["tau"].data_ptr(), d["out"].data_ptr(),
                            self.d_type.data_ptr() if self.d_type is not None else 0, want,
                            torch.cuda.current_stream().cuda_stream)

    def read(self):
        torch.cuda.synchronize()
        return {k: self.d[k].cpu().numpy() for k in ("slot", "tau", "out")}

    def inputs_now(self):
        return {k: self.d[k].cpu().numpy() for k in ("sn", "st", "pl", "cm")}


def run(policy, inp, B, types=None, want=2, nan_at=None):
    """The device sequence: per tick the slot, torques and output rows (whole buffers), plus the rig."""
    T = inp["q"].shape[0]
    rig = Rig(B)
    if types is not None:
        rig.d_type = torch.from_numpy(np.concatenate([types, np.full(PAD, want)]).astype(np.int32)).cuda()
    hist = []
    for t in range(T):
        rig.write(inp, t)
        if nan_at is not None and nan_at[0] == t:
            rig.d["sn"][nan_at[1], _lib.SN_JOINT_VEL + 5] = float("nan")
        before = rig.inputs_now() if t == T - 1 else None
        rig.tick(policy, want)
        hist.append(rig.read())
    after = rig.inputs_now()
    for k in before:
        _same("input " + k, after[k], before[k])   # the stage reads these and writes none of them
    return rig, hist


def check_sequence(p, inp, B, rig, hist, run_mask=None, bad_mask=None):
    """Every tick: observation bitwise; with the device's raw output read back, action, targets, torques, slot,
    status and update flag bitwise; nothing else moves.  run_mask [T, B]: robots selected; bad_mask [T, B]:
    selected robots with a non-finite input.  Returns the restatement's block."""
    T = inp["q"].shape[0]
    blk = ref.PolicyBlock(B, p)
    exp_slot, exp_tau, exp_out = rig.slot0.copy(), rig.tau0.copy(), rig.out0.copy()
    for t in range(T):
        sel = np.ones(B, bool) if run_mask is None else run_mask[t]
        bad = np.zeros(B, bool) if bad_mask is None else bad_mask[t]
        ok = sel & ~bad
        got = hist[t]
        with np.errstate(invalid="ignore"):
            obs = ref.observation(p, inp["rot_z"][t], inp["lin_vel"][t], inp["imu"][t], inp["rot"][t], inp["joy"][t],
                                  inp["q"][t], inp["dq"][t], blk.prev_action)
        raw_dev = got["out"][:B, _lib.PY_RAW:_lib.PY_RAW + 12]
        o = blk.step(inp["mode"][t], inp["q"][t], inp["dq"][t], raw_dev, run=ok)
        # raw is reported as 0 by robots that did not run the network this tick
        assert not raw_dev[ok & ~(o["updated"] & (inp["mode"][t] == 1.0))].any()
        exp_slot[:B][ok] = blk.slot_rows()[ok]
        exp_tau[:B][ok] = o["tau"][ok]
        row = exp_out[:B]
        row[ok, _lib.PY_OBS:_lib.PY_OBS + 48] = obs[ok].astype(np.float64)
        row[ok, _lib.PY_RAW:_lib.PY_RAW + 12] = o["raw"][ok]
        row[ok, _lib.PY_ACTION:_lib.PY_ACTION + 12] = o["action"][ok]
        row[ok, _lib.PY_TARGET:_lib.PY_TARGET + 12] = o["target"][ok]
        row[ok, _lib.PY_TORQUE:_lib.PY_TORQUE + 12] = o["tau"][ok]
        row[ok, _lib.PY_STATUS] = 0.0
        row[ok, _lib.PY_UPDATED] = o["updated"][ok].astype(np.float64)
        row[sel & bad, _lib.PY_STATUS] = 1.0
        row[sel & bad, _lib.PY_UPDATED] = 0.0
        _same(f"tick {t} out", got["out"], exp_out)
        _same(f"tick {t} slot", got["slot"], exp_slot)
        _same(f"tick {t} torques", got["tau"], exp_tau)
    return blk


def int_network(hidden, seed):
    """Non-negative integer weights and positive integer biases: every pre-activation is positive (ELU is the
    identity) and every partial sum is an integer no larger than the final one.  The first layer is dense in
    0..3; the later ones are sparse enough to keep the sums below 2^24 and dense enough for distinct columns."""
    rng = np.random.default_rng(seed)
    dims = [48] + list(hidden) + [12]
    ws, bs = [], []
    for l, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        if l == 0:
            w = rng.integers(0, 4, (o, i))
        elif l + 1 < len(dims) - 1:
            w = rng.integers(1, 4, (o, i)) * (rng.random((o, i)) < (1 / 16 if i >= 256 else 1 / 2))
        else:
            w = rng.integers(1, 3, (o, i)) * (rng.random((o, i)) < 1 / 2)
        ws.append(w.astype(np.float32))
        bs.append(rng.integers(1, 5, (o,)).astype(np.float32))
    return ws, bs


@pytest.mark.parametrize("hidden", [(512, 256, 128), (64, 32)])
@pytest.mark.parametrize("B", SIZES)
def test_exact_integer_network_bitwise(B, hidden):
    ws, bs = int_network(hidden, seed=len(hidden))
    for w in ws:
        m = min(w.shape)
        assert not np.array_equal(w[:m, :m], w[:m, :m].T), "asymmetric"
        assert len(np.unique(w, axis=0)) == w.shape[0] and np.unique(w, axis=1).shape[1] == w.shape[1], "distinct"
    p = ref.default_params(obs_scale=np.ones(36), default_joint_pos=np.zeros(12))
    pp = mpcqp.default_policy_params(hidden=hidden, obs_scale=np.ones(36), default_joint_pos=np.zeros(12))
    inp = make_inputs(B, 1, seed=B, integer=True)
    with mpcqp.Policy(ws, bs, pp) as pol:
        rig, hist = run(pol, inp, B)
    x = ref.observation(p, inp["rot_z"][0], inp["lin_vel"][0], inp["imu"][0], inp["rot"][0], inp["joy"][0], inp["q"][0],
                        inp["dq"][0], np.zeros((B, 12)))
    assert np.array_equal(x, np.round(x)) and (x >= 0).all() and x[:, 8].tolist() == [1.0] * B
    pre = ref.mlp_f64_layers(ws, bs, x)
    # the two conditions of exactness: ELU is the identity, and all terms are non-negative integers, so every
    # partial sum of every order is an integer bounded by the final sum, itself below 2^24
    assert all((h > 0).all() for h in pre[:-1]) and all((w >= 0).all() for w in ws) and all((b > 0).all() for b in bs)
    assert max(h.max() for h in pre) < 2.0 ** 24
    assert all(np.array_equal(h, np.round(h)) for h in pre)
    got = hist[0]["out"][:B]
    _same("observation", got[:, :48], x.astype(np.float64))
    _same("raw network output", got[:, _lib.PY_RAW:_lib.PY_RAW + 12], pre[-1])
    assert len(np.unique(pre[-1], axis=0)) == B   # the robots differ, so a row mix-up shows
    check_sequence(p, inp, B, rig, hist)


@functools.lru_cache(maxsize=None)
def seeded_run(B, last_gain):
    """12 ticks of seeded weights on inputs that reach both observation clips (shared, read-only)."""
    ws, bs = ref.seeded_weights(21)
    ws[-1], bs[-1] = ws[-1] * np.float32(last_gain), bs[-1] * np.float32(last_gain)
    inp = make_inputs(B, 12, seed=100 + B, big=True)
    with mpcqp.Policy(ws, bs) as pol:
        rig, hist = run(pol, inp, B)
    return ws, bs, inp, rig, hist


@pytest.mark.parametrize("last_gain", [1.0, 1e3])
@pytest.mark.parametrize("B", SIZES)
def test_observation_and_postprocessing_bitwise(B, last_gain):
    ws, bs, inp, rig, hist = seeded_run(B, last_gain)
    p = ref.default_params()
    check_sequence(p, inp, B, rig, hist)
    out = np.stack([h["out"][:B] for h in hist])
    obs = out[:, :, :36]
    if B > 1:
        assert (obs == 100.0).any() and (obs == -100.0).any()   # both observation clips
        assert (obs[:, :, 0:3] == 100.0).any() and (obs[:, :, 24:36] == -100.0).any()
    # the appended previous action is the device's own clipped action of the tick before
    _same("prev_action", out[1:, :, 36:48], out[:-1, :, _lib.PY_ACTION:_lib.PY_ACTION + 12].astype(np.float32).astype(np.float64))
    if last_gain > 1.0 and B > 1:
        act, tgt = out[:, :, _lib.PY_ACTION:_lib.PY_ACTION + 12], out[:, :, _lib.PY_TARGET:_lib.PY_TARGET + 12]
        assert (act == 100.0).any() and (act == -100.0).any()                        # the action clip
        assert (tgt == ref.POSE_UPPER).any() and (tgt == ref.POSE_LOWER).any()       # both pose limits


def test_network_accuracy():
    """max |device - binary64| <= 4 x max |torch CPU float32 - binary64| over 12 ticks of 67 robots."""
    B = 67
    ws, bs, inp, rig, hist = seeded_run(B, 1.0)
    x = np.concatenate([h["out"][:B, :48] for h in hist]).astype(np.float32)
    dev = np.concatenate([h["out"][:B, _lib.PY_RAW:_lib.PY_RAW + 12] for h in hist])
    y64 = ref.mlp_f64(ws, bs, x)
    e_ref = np.max(np.abs(ref.mlp_torch(ws, bs, x).astype(np.float64) - y64))
    e_dev = np.max(np.abs(dev - y64))
    print(f"policy network accuracy: e_dev {e_dev:.3e} e_ref {e_ref:.3e} ratio {e_dev / e_ref:.3f} max|y| {np.abs(y64).max():.3f}")
    assert e_ref > 0.0
    assert e_dev <= 4.0 * e_ref


def test_modes_and_decimation():
    B, T = 67, 10
    ws, bs = ref.seeded_weights(22)
    inp = make_inputs(B, T, seed=5)
    t, b = np.arange(T)[:, None], np.arange(B)[None, :]
    inp["mode"] = np.where(t < 5, (b % 3 != 0), (b % 2 == 0)).astype(np.float64)   # mixed in every tile, switched at tick 5
    pp = mpcqp.default_policy_params(decimation=4)
    p = ref.default_params(decimation=4)
    with mpcqp.Policy(ws, bs, pp) as pol:
        rig, hist = run(pol, inp, B)
    blk = check_sequence(p, inp, B, rig, hist)
    upd = np.stack([h["out"][:B, _lib.PY_UPDATED] for h in hist])
    assert upd[:, 0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0] and (upd == upd[:, :1]).all()
    tgt = np.stack([h["out"][:B, _lib.PY_TARGET:_lib.PY_TARGET + 12] for h in hist])
    tau = np.stack([h["tau"][:B] for h in hist])
    assert all(np.array_equal(tgt[k], tgt[4 * (k // 4)]) for k in range(T))          # held between updates
    assert all((tau[k] != tau[k - 1]).all() for k in range(1, T))                   # torques follow q, dq every tick
    modes = np.stack([h["slot"][:B, _lib.PS_MODE] for h in hist])
    assert np.array_equal(modes[4], inp["mode"][4]) and np.array_equal(modes[7], inp["mode"][4])
    assert np.array_equal(modes[8], inp["mode"][8]) and not np.array_equal(modes[8], modes[7])
    assert (blk.servo_motion_time > 0).any() and (blk.servo_motion_time == 0).any()
    # the servo stand, ticking every tick, with and without the clamp past servo_ticks
    for clamp in (0, 1):
        inp2 = make_inputs(33, 6, seed=6)
        inp2["mode"][:] = 0.0
        pp2 = mpcqp.default_policy_params(servo_ticks=4.0, servo_clamp=clamp)
        with mpcqp.Policy(ws, bs, pp2) as pol:
            rig2, hist2 = run(pol, inp2, 33)
        check_sequence(ref.default_params(servo_ticks=4.0, servo_clamp=clamp), inp2, 33, rig2, hist2)
        tg = hist2[5]["out"][:33, _lib.PY_TARGET:_lib.PY_TARGET + 12]
        assert np.array_equal(tg, np.tile(ref.STAND_POS, (33, 1))) == bool(clamp)


def test_selection_by_type():
    B, T = 67, 3
    ws, bs = ref.seeded_weights(23)
    inp = make_inputs(B, T, seed=7)
    types = (np.arange(B) % 4).astype(np.int32)
    types[32:40] = 1   # a tile's first robots not selected
    sel = types == 2
    with mpcqp.Policy(ws, bs) as pol:
        rig_a, all_ = run(pol, inp, B)
        rig_t, typed = run(pol, inp, B, types=types, want=2)
    p = ref.default_params()
    check_sequence(p, inp, B, rig_t, typed, run_mask=np.tile(sel, (T, 1)))
    for t in range(T):
        for k, init in (("slot", rig_t.slot0), ("tau", rig_t.tau0), ("out", rig_t.out0)):
            _same(f"tick {t} {k} of robots that are not selected", typed[t][k][:B][~sel], init[:B][~sel])
            _same(f"tick {t} {k} past the batch", typed[t][k][B:], init[B:])
            # (the pad doubles of the output row hold each rig's own sentinels, the same permutation)
            _same(f"tick {t} {k} of selected robots", typed[t][k][:B][sel], all_[t][k][:B][sel])
    assert sel.sum() > 10 and (~sel).sum() > 10


def test_nan_input_is_contained():
    B, T, NAN_TICK = 67, 4, 1
    nb = 40   # in the middle of the second tile
    ws, bs = ref.seeded_weights(24)
    inp = make_inputs(B, T, seed=8)
    with mpcqp.Policy(ws, bs) as pol:
        rig_c, clean = run(pol, inp, B)
        rig_n, dirty = run(pol, inp, B, nan_at=(NAN_TICK, nb))
    bad = np.zeros((T, B), bool)
    bad[NAN_TICK, nb] = True
    inp_n = {k: v.copy() for k, v in inp.items()}
    inp_n["dq"][NAN_TICK, nb, 5] = np.nan
    check_sequence(ref.default_params(), inp_n, B, rig_n, dirty, bad_mask=bad)
    others = np.arange(B) != nb
    for t in range(T):
        for k in ("slot", "tau", "out"):
            _same(f"tick {t} {k} of the other robots", dirty[t][k][:B][others], clean[t][k][:B][others])
    _same("slot kept", dirty[NAN_TICK]["slot"][nb], dirty[NAN_TICK - 1]["slot"][nb])
    _same("torques kept", dirty[NAN_TICK]["tau"][nb], dirty[NAN_TICK - 1]["tau"][nb])
    assert dirty[NAN_TICK]["out"][nb, _lib.PY_STATUS] == 1.0 and dirty[NAN_TICK + 1]["out"][nb, _lib.PY_STATUS] == 0.0
    assert dirty[T - 1]["slot"][nb, _lib.PS_TICK] == T - 1 and np.isfinite(dirty[T - 1]["tau"][nb]).all()


def test_policy_arguments():
    L = mpcqp.load()
    pp = mpcqp.default_policy_params()
    assert ctypes.sizeof(pp) == L.mpcqp_policy_params_size()
    assert (pp.n_hidden, list(pp.hidden), pp.servo_clamp, pp.decimation) == (3, [512, 256, 128], 0, 1)
    assert list(pp.obs_scale) == ref.OBS_SCALE.tolist() and list(pp.default_joint_pos) == ref.DEFAULT_JOINT_POS.tolist()
    assert list(pp.pose_lower) == ref.POSE_LOWER.tolist() and list(pp.pose_upper) == ref.POSE_UPPER.tolist()
    assert list(pp.kp_walk) == ref.KP_WALK.tolist() and list(pp.kd_walk) == ref.KD_WALK.tolist()
    assert list(pp.kp_servo) == ref.KP_SERVO.tolist() and list(pp.kd_servo) == ref.KD_SERVO.tolist()
    assert list(pp.stand_pos) == ref.STAND_POS.tolist()
    assert (pp.clip_obs, pp.clip_action, pp.action_scale, pp.servo_ticks) == (100.0, 100.0, 0.25, 1000.0)
    assert mpcqp.policy_state_size() == _lib.PS_SIZE
    ws, bs = ref.seeded_weights(1, hidden=(32,))
    with mpcqp.Policy(ws, bs) as pol:
        h = pol.handle
        assert pol.params.n_hidden == 1 and pol.params.hidden[0] == 32
        assert L.mpcqp_policy_device(h, None, None, None, None, 0, None, None, 2, None, None, None) == _lib.ERR_OK
        assert L.mpcqp_policy_device(h, None, None, None, None, 1, None, None, 2, None, None, None) == _lib.ERR_INVALID_ARG
        assert L.mpcqp_policy_device(h, None, None, None, None, -1, None, None, 2, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.mpcqp_policy_device(None, None, None, None, None, 0, None, None, 2, None, None, None) == _lib.ERR_INVALID_ARG
    for bad in (dict(hidden=[48]), dict(hidden=[544]), dict(decimation=0), dict(servo_ticks=0.0)):
        bp = mpcqp.default_policy_params(**{"hidden": [32], **bad})
        w2, b2 = ref.seeded_weights(1, hidden=(bp.hidden[0],))
        with pytest.raises(mpcqp.MpcQpError):
            mpcqp.Policy(w2, b2, bp)
    with pytest.raises(ValueError):
        mpcqp.Policy(ws[:1], bs[:1])
