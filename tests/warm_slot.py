"""The warm-start slot (WarmLayout<N>, csrc/mpcqp_wave_common.h) restated for the tests: offsets, decode / encode
between a slot and the oracle's persistent-solver state (pyoracle.WarmSolver.state()), the tick sequences that reach
every branch that consumes a slot (0 setup, 1 osqp_update_P, 2 OsqpEigen re-init by a changed mu and by a changed zero
pattern of H), and the oracle's run of a sequence with the state after every tick.  No GPU in here."""
import functools
from types import SimpleNamespace

import numpy as np

import mpcqp
import pyoracle
from mpcqp import _lib as L

SOLVED = L.STATUS_SOLVED
FIELDS = ("D", "E", "q", "ak0", "ak1", "x", "z", "y")  # the slot's vectors, named as WarmSolver.state() names them


def layout(N):
    """WarmLayout<N>: doubles per robot, in this order."""
    n, m = 12 * N, 20 * N
    w = SimpleNamespace(n=n, m=m, MW=(n + 63) // 64, FLAG=0, RHO=1, C=2, MU=3, D=4)
    w.E = w.D + n
    w.QT = w.E + m
    w.AK = w.QT + n
    w.X = w.AK + 2 * m
    w.Z = w.X + n
    w.Y = w.Z + m
    w.MASK = w.Y + m
    w.SIZE = w.MASK + w.MW * n
    return w


def decode(slot, N):
    """The slot's named fields (keys as WarmSolver.state()).  pzero [ri][j] is bit ri & 63 of word ri >> 6 of column
    j's MW mask words, for every ri < 12N (so a bit set below the diagonal shows); mask_extra counts the set bits at
    positions >= 12N of the columns' last words."""
    w = layout(N)
    slot = np.ascontiguousarray(slot, dtype=np.float64)
    assert slot.shape == (w.SIZE,)
    n, m = w.n, w.m
    words = slot[w.MASK:].view(np.uint64).reshape(n, w.MW)
    pos = np.arange(64 * w.MW)
    bits = ((words[:, pos >> 6] >> (pos & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)  # [j][position]
    return {"initialized": bool(slot[w.FLAG] != 0.0), "flag": slot[w.FLAG], "rho": slot[w.RHO], "c": slot[w.C],
            "mu": slot[w.MU], "D": slot[w.D:w.D + n].copy(), "E": slot[w.E:w.E + m].copy(),
            "q": slot[w.QT:w.QT + n].copy(), "ak0": slot[w.AK:w.AK + m].copy(),
            "ak1": slot[w.AK + m:w.AK + 2 * m].copy(), "x": slot[w.X:w.X + n].copy(), "z": slot[w.Z:w.Z + m].copy(),
            "y": slot[w.Y:w.Y + m].copy(), "pzero": bits[:, :n].T.copy(), "mask_extra": int(bits[:, n:].sum())}


def encode(state, N):
    """decode's inverse: the slot a kernel would have left for the oracle's solver state (all zero for an
    uninitialized solver)."""
    w = layout(N)
    slot = np.zeros(w.SIZE)
    if not state["initialized"]:
        return slot
    n, m = w.n, w.m
    slot[w.FLAG], slot[w.RHO], slot[w.C], slot[w.MU] = 1.0, state["rho"], state["c"], state["mu"]
    for off, key in ((w.D, "D"), (w.E, "E"), (w.QT, "q"), (w.AK, "ak0"), (w.AK + m, "ak1"), (w.X, "x"), (w.Z, "z"),
                     (w.Y, "y")):
        slot[off:off + len(state[key])] = state[key]
    pz = np.asarray(state["pzero"], dtype=bool)
    assert pz.shape == (n, n)
    words = np.zeros((n, w.MW), dtype=np.uint64)
    for ri, j in zip(*np.nonzero(pz)):
        words[j, ri >> 6] |= np.uint64(1) << np.uint64(ri & 63)
    slot[w.MASK:] = words.reshape(-1).view(np.float64)
    return slot


def unscaled(st):
    """The solver's iterates without its scaling: x = D x~, z = z~ / E, y = E y~ / c."""
    return {"x": st["D"] * st["x"], "z": st["z"] / st["E"], "y": st["E"] * st["y"] / st["c"], "rho": st["rho"]}


def upper_zeros(pzero):
    return int(np.count_nonzero(pzero))


# ---- the sequences ---------------------------------------------------------------------------------------------
TROT_B, TROT_T, TROT_MU = 24, 4, 0.45


@functools.lru_cache(maxsize=None)
def trot_sequence(N):
    """[4][24][rec]: a trot with contact changes, every fourth robot's friction coefficient changed from tick 2 on
    (a re-init by mu); Go1 weights."""
    ticks = mpcqp.records.synthetic_go1_ticks(TROT_B, TROT_T, seed=5300 + N, gait="trot", swing_ticks=2)
    recs = np.stack([mpcqp.assemble_compute_grf(s, N) for s in ticks])
    recs[2:, ::4, L.REC_MU] = TROT_MU
    recs.setflags(write=False)
    return recs


PATTERN_TICKS = ("level", "pitch", "roll", "yaw", "yaw90", "foot_y0", "foot_x0", "pitch+foot_y0", "level")
PATTERN_MODES = [0, 2, 1, 2, 1, 2, 2, 2, 2]
PATTERN_ZEROS_N10 = [608, 0, 0, 608, 608, 1332, 1332, 933, 608]


def _posed(rec, roll=0.0, pitch=0.0, yaw=0.0):
    x = rec.copy()
    x[L.REC_EULER:L.REC_EULER + 3] = (roll, pitch, yaw)
    x[L.REC_X0:L.REC_X0 + 3] = (roll, pitch, yaw)
    x[L.REC_ROT:L.REC_ROT + 9] = mpcqp.records.rot_zyx(np.array([roll]), np.array([pitch]), np.array([yaw]))[0].reshape(9)
    return x


@functools.lru_cache(maxsize=None)
def pattern_sequence(N):
    """([9][1][rec], q_weights, r_weights): test_mpc's stance, whose H has exact zeros, through poses and foot
    positions that change the zero pattern of H's upper triangle with mu unchanged: level (sparse), pitched and
    rolled (dense), yawed (the level pattern), one foot with y = 0 and another with x = 0 (more zeros), the pitched
    pose with the y = 0 foot (partly sparse: only some of a column's entries vanish), level again."""
    rec, q, r = mpcqp.assemble_test_mpc(N)
    f = L.rec_feet(N)
    foot_y0, foot_x0 = rec.copy(), rec.copy()
    foot_y0[f:f + 12 * N].reshape(N, 4, 3)[:, 1, 1] = 0.0
    foot_x0[f:f + 12 * N].reshape(N, 4, 3)[:, 2, 0] = 0.0
    seq = [rec, _posed(rec, pitch=0.2), _posed(rec, roll=0.2), _posed(rec, yaw=0.3), _posed(rec, yaw=np.pi / 2),
           foot_y0, foot_x0, _posed(foot_y0, pitch=0.2), rec]
    recs = np.stack(seq)[:, None, :]
    recs.setflags(write=False)
    return recs, tuple(q), tuple(r)


def oracle_params(N, q=None, r=None):
    return pyoracle.default_params(N, q=None if q is None else list(q), r=None if r is None else list(r))


def oracle_run(op, recs_t, robots=None):
    """The oracle's persistent solvers over recs_t [T][B][rec]: results [T][B], solutions [T][B][12N] and the solver
    state after every tick, states[t][b] (None for robots not in `robots`)."""
    T, B = recs_t.shape[:2]
    res = np.zeros((T, B), dtype=pyoracle.RESULT_DTYPE)
    sol = np.zeros((T, B, 12 * op.horizon))
    states = [[None] * B for _ in range(T)]
    for b in (range(B) if robots is None else robots):
        w = pyoracle.WarmSolver(op)
        for t in range(T):
            res[t, b], sol[t, b] = w.step(recs_t[t, b])
            states[t][b] = w.state()
        w.close()
    return SimpleNamespace(res=res, sol=sol, states=states)


@functools.lru_cache(maxsize=None)
def oracle_trot(N):
    return oracle_run(oracle_params(N), trot_sequence(N))


@functools.lru_cache(maxsize=None)
def oracle_pattern(N):
    recs, q, r = pattern_sequence(N)
    return oracle_run(oracle_params(N, q, r), recs)


def modes_of(run):
    return np.array([[s["last_mode"] for s in row] for row in run.states])
