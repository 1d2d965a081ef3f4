"""The disturbance stage on the device (mpcqp_disturb_device) against tests/disturb_reference.py: every double of
the wrench row, the noisy sensor row, the output row and the guard rows around them bitwise, over hand-made episode
slots that put robots on the edges of the push rule; and the invalid-argument cases, which launch nothing."""
import numpy as np
import pytest
import torch

import mpcqp

import disturb_reference as dr
from test_disturb import everything_on, ref_params, slot_rows

pytestmark = pytest.mark.gpu

FILL = -7.25
WIDTH = dict(wrench=dr.PW_SIZE, noisy=dr.SN_SIZE, out=dr.DO_SIZE)


class DeviceDisturb:
    """The stage's buffers for B robots, each output between two guard rows of a recognisable fill."""

    def __init__(self, B, es, sensors=None, dirs=None, out=True):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()  # noqa: E731
        self.B = B
        self.es = up(es)
        self.sensors = None if sensors is None else up(sensors)
        self.dirs = None if dirs is None else up(dirs)
        names = ["wrench"] + (["noisy"] if sensors is not None else []) + (["out"] if out else [])
        self.rows = {n: torch.full((B + 2, WIDTH[n]), FILL, dtype=torch.float64, device="cuda") for n in names}

    def buffers(self, **over):
        p = lambda n: self.rows[n][1:].data_ptr() if n in self.rows else 0  # noqa: E731
        kw = dict(d_episode_state=self.es.data_ptr(), d_wrench=p("wrench"),
                  d_sensors=0 if self.sensors is None else self.sensors.data_ptr(), d_sensors_noisy=p("noisy"),
                  d_dirs=0 if self.dirs is None else self.dirs.data_ptr(), d_disturb_out=p("out"))
        kw.update(over)
        return mpcqp.disturb_buffers(**kw)

    def run(self, dp, **over):
        mpcqp.disturb_device(dp, self.buffers(**over), self.B, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return {n: t.cpu().numpy() for n, t in self.rows.items()}


def edge_ticks(p, B, episode):
    """Per robot, an episode tick on an edge of the push rule, the kind cycling with the robot index: before
    push_start, the first and the last tick of a push, the tick before and after it, the last tick of a window and
    the first of the next."""
    ticks, kinds = [], []
    for b in range(B):
        k = 1 + b % 3
        jitter = int(dr.push_window(p, b, episode[b], k)[0])
        lo = p.push_start + k * p.push_interval
        kind = b % 8
        t = [p.push_start - 1, lo + jitter, lo + jitter + p.push_duration - 1, lo + jitter - 1,
             lo + jitter + p.push_duration, lo + p.push_interval - 1, lo, 0][kind]
        ticks.append(max(t, 0))
        kinds.append(kind)
    return np.array(ticks), np.array(kinds)


CASES = {
    "everything": dict(),
    "duration_is_interval": dict(push_interval=5, push_duration=5, push_start=2),
    "one_direction": dict(dir_count=1),
    "interval_one": dict(push_interval=1, push_duration=1, push_start=1),
    "noise_only": dict(push_interval=0, load_mass_max=0.0, load_point=[0, 0, 0]),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("B", [1, 5, 67])
def test_every_double_is_the_restatement(B, case):
    dp = everything_on(**CASES[case])
    p = ref_params(dp)
    rng = np.random.Generator(np.random.PCG64(10 * B + len(case)))
    episode = rng.integers(0, 40, B)
    if p.push_interval > 0:
        tick, kinds = edge_ticks(p, B, episode)
    else:
        tick, kinds = rng.integers(0, 3000, B), np.zeros(B, dtype=int)
    # phases 0 / 1 / 2 mixed among neighbours: robots 3, 11, 19, .. fresh and 6, 14, .. priming (B = 1: running)
    phase = np.ones(B)
    phase[3::8], phase[6::8] = 0.0, 2.0
    es = slot_rows(phase, tick, episode)
    sn = rng.uniform(-2.0, 2.0, (B, dr.SN_SIZE))
    sn[0, dr.SN_JOINT_VEL] = -0.0
    dirs = mpcqp.pack_push_dirs(dp.dir_count) if dp.dir_count else None
    dev = DeviceDisturb(B, es, sn, dirs)
    got = dev.run(dp)
    wrench, noisy, out = dr.step(p, es, sn, dirs)
    for name, want in (("wrench", wrench), ("noisy", noisy), ("out", out)):
        full = np.full((B + 2, WIDTH[name]), FILL)
        full[1:-1] = want
        bad = np.argwhere(got[name].view(np.int64) != full.view(np.int64))
        assert bad.size == 0, f"{name}: first differing (row + 1, double) {bad[0].tolist()}: {got[name][tuple(bad[0])]!r} " \
                              f"for {full[tuple(bad[0])]!r}"
    assert np.array_equal(dev.es.cpu().numpy().view(np.int64), es.view(np.int64))
    assert np.array_equal(dev.sensors.cpu().numpy().view(np.int64), sn.view(np.int64))
    run = phase == 1.0
    active = out[:, dr.DO_PUSH_ACTIVE] != 0.0
    if p.push_interval > 0 and B >= 5:  # the edges are on both sides
        assert active[run].any() and not active[run].all()
        if case == "everything":
            want_on = np.isin(kinds, (1, 2))
            want_off = np.isin(kinds, (0, 7))  # (the ticks next to a push may belong to a neighbouring window's)
            assert np.all(active[run & want_on]) and not np.any(active[run & want_off])
    print(f"[note] {case} B={B}: {int(active.sum())} of {int(run.sum())} running robots pushed, kinds {sorted(set(kinds))}")


@pytest.mark.parametrize("B", [1, 5, 67])
def test_every_optional_pointer_null(B):
    """The truth-fed tick's call: no sensor rows, no output row, and without pushes no direction table."""
    rng = np.random.Generator(np.random.PCG64(B))
    es = slot_rows(1.0, rng.integers(0, 50, B), rng.integers(0, 9, B))
    for over, dirs in ((dict(push_interval=0), None), (dict(), mpcqp.pack_push_dirs(8))):
        dp = everything_on(**over)
        dev = DeviceDisturb(B, es, None, dirs, out=False)
        got = dev.run(dp)
        assert set(got) == {"wrench"}
        full = np.full((B + 2, dr.PW_SIZE), FILL)
        full[1:-1] = dr.step(ref_params(dp), es, None, dirs)[0]
        assert np.array_equal(got["wrench"].view(np.int64), full.view(np.int64))
        assert np.all(full[1:-1, dr.PW_FORCE1 + 2] < 0.0)


def test_invalid_arguments_return_the_error_and_launch_nothing():
    B = 5
    es = slot_rows(1.0, 4, 0)
    es = np.repeat(es, B, 0)
    sn = np.ones((B, dr.SN_SIZE))
    dirs = mpcqp.pack_push_dirs(8)
    dev = DeviceDisturb(B, es, sn, dirs)
    bad = [(everything_on(push_duration=0), {}), (everything_on(push_duration=8), {}),
           (everything_on(push_duration=-1), {}), (everything_on(push_interval=-1), {}),
           (everything_on(), dict(d_dirs=0)), (everything_on(dir_count=0), {}),
           (everything_on(), dict(d_episode_state=0)), (everything_on(), dict(d_wrench=0)),
           (everything_on(), dict(d_sensors=0)), (everything_on(), dict(d_sensors_noisy=0)),
           (everything_on(), dict(d_sensors_noisy=dev.sensors.data_ptr()))]
    for dp, over in bad:
        with pytest.raises(mpcqp.MpcQpError, match="invalid argument|\\(1\\)"):
            dev.run(dp, **over)
    torch.cuda.synchronize()
    for name, t in dev.rows.items():
        assert torch.all(t == FILL), name
    # the same buffers, valid: the call goes through (so the rejections above were the arguments')
    got = dev.run(everything_on())
    assert np.all(got["wrench"][1:-1] != FILL)
    # duration == interval and a NULL direction table without pushes are valid
    dev.run(everything_on(push_duration=7))
    dev.run(everything_on(push_interval=0), d_dirs=0)
