"""Cases for the balance QP kernel (csrc/mpcqp_balance.hip): records that hold every contact pattern and a few
planted robots, the OSQP settings and balance parameters that take the kernel down each of its paths, and the
comparison of a result batch with the CPU oracle's that looks at every field of the result record.  No tests
here: tests/test_balance_cases.py checks the cases on the CPU oracle, tests/test_gpu_balance_cases.py runs them
on the device."""
import functools

import numpy as np

import mpcqp
from mpcqp import balance as bal
from mpcqp._lib import OSQP_INFTY, override

B_GPU = 130  # two full 64-thread blocks and a lane pair
SEED = 4
GAITS = ("trot", "stance", "mixed")
POOL = 192
WRAP = 3.1415926  # the literal of A1RobotControl.cpp:325-331; the yaw error wraps beyond 1.5 * WRAP

# planted robots (present when the batch is large enough to hold the index)
YAW_WRAP_DOWN = 17  # euler_d - euler = +6: above +1.5 WRAP, 2 WRAP is subtracted
YAW_WRAP_UP = 18    # -6: below -1.5 WRAP, 2 WRAP is added
NEAR_WRAP_POS = 19  # just under +1.5 WRAP: no wrap
NEAR_WRAP_NEG = 20  # just above -1.5 WRAP: no wrap
NAN_ROBOT, NAN_FIELD = 37, bal.BAL_FEET + 4
INF_ROBOT, INF_FIELD = 63, bal.BAL_SIZE - 2  # the last double the kernel checks, in the last lane of block 0
PAD_ROBOT = 41      # finite but for the padding double BAL_SIZE - 1, which nothing reads
NEAR_MARGIN = 1e-9
NONFINITE = (NAN_ROBOT, INF_ROBOT)


def contact_mask(b):
    """Contacts of robot b: bit `leg` of b % 16."""
    return np.array([(b % 16) >> leg & 1 for leg in range(4)], dtype=np.float64)


def records(B, seed=SEED):
    """[B][72] balance records: robot b from synthetic_go1 of gait GAITS[b % 3], contact mask b % 16 (so 16
    consecutive robots hold all 16 patterns), and the planted robots above.  Drawn from a pool of POOL robots,
    so a smaller batch is a prefix of a larger one."""
    sets = [bal.assemble_balance(mpcqp.synthetic_go1(max(B, POOL), seed=seed + 101 * k, gait=g))
            for k, g in enumerate(GAITS)]
    recs = np.stack([sets[b % 3][b] for b in range(B)])
    for b in range(B):
        recs[b, bal.BAL_CONTACTS:bal.BAL_CONTACTS + 4] = contact_mask(b)

    def yaw(b, euler, euler_d):
        if b < B:
            recs[b, bal.BAL_EULER + 2], recs[b, bal.BAL_EULER_D + 2] = euler, euler_d

    yaw(YAW_WRAP_DOWN, -3.0, 3.0)
    yaw(YAW_WRAP_UP, 3.0, -3.0)
    yaw(NEAR_WRAP_POS, -2.3, 1.5 * WRAP - 2.3 - NEAR_MARGIN)
    yaw(NEAR_WRAP_NEG, 2.3, -1.5 * WRAP + 2.3 + NEAR_MARGIN)
    if NAN_ROBOT < B:
        recs[NAN_ROBOT, NAN_FIELD] = np.nan
    if INF_ROBOT < B:
        recs[INF_ROBOT, INF_FIELD] = -np.inf
    if PAD_ROBOT < B:
        recs[PAD_ROBOT, bal.BAL_SIZE - 1] = np.nan
    return recs


def mask_records(seed=SEED):
    """16 robots, one per contact mask, identical in every other field (an all-stance synthetic robot)."""
    one = bal.assemble_balance(mpcqp.synthetic_go1(1, seed=seed, gait="stance"))
    recs = np.repeat(one, 16, axis=0)
    for b in range(16):
        recs[b, bal.BAL_CONTACTS:bal.BAL_CONTACTS + 4] = contact_mask(b)
    return recs


def yaw_error(recs):
    """(euler_d - euler)[2] before the wrap and after it, as compute_grf computes it."""
    raw = recs[:, bal.BAL_EULER_D + 2] - recs[:, bal.BAL_EULER + 2]
    out = raw.copy()
    hi, lo = raw > WRAP * 1.5, raw < -WRAP * 1.5
    out[hi] = recs[hi, bal.BAL_EULER_D + 2] - WRAP * 2 - recs[hi, bal.BAL_EULER + 2]
    out[lo] = recs[lo, bal.BAL_EULER_D + 2] + WRAP * 2 - recs[lo, bal.BAL_EULER + 2]
    return raw, out


# mpcqp_params overrides; every one passes mpcqp_create's validation
SETTINGS = [
    ("default", {}),
    ("scaling0", dict(scaling=0)),
    ("scaling3", dict(scaling=3)),
    ("check1", dict(check_termination=1)),
    ("check7", dict(check_termination=7)),
    ("check0", dict(check_termination=0)),
    ("check7_rho10", dict(check_termination=7, adaptive_rho_interval=10)),
    ("rho10", dict(adaptive_rho_interval=10)),
    ("no_adaptive_rho", dict(adaptive_rho=0)),
    ("rho_tol1.5", dict(adaptive_rho_tolerance=1.5)),
    ("alpha1.0", dict(alpha=1.0)),
    ("alpha1.9", dict(alpha=1.9)),
    ("rho1e-3", dict(rho=1e-3)),
    ("rho10.0", dict(rho=10.0)),
    ("sigma1e-3", dict(sigma=1e-3)),
    ("eps1e-6", dict(eps_abs=1e-6, eps_rel=1e-6)),
    ("eps1e-9_iter200", dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=200)),
    ("max_iter1", dict(max_iter=1)),
    ("max_iter24", dict(max_iter=24)),
    ("max_iter25", dict(max_iter=25)),
    ("max_iter26", dict(max_iter=26)),
    ("max_iter50", dict(max_iter=50)),
]

# mpcqp_balance_params overrides
BALANCE = [
    ("default", {}),
    ("f_min10", dict(f_min=10.0)),
    ("f_max5", dict(f_max=5.0)),
    ("mu0", dict(mu=0.0)),
    ("mu0.05", dict(mu=0.05)),
    ("q_zero", dict(q_diag=[0.0] * 6)),
    ("soft_weights", dict(q_diag=[2, 2, 5, 300, 300, 50], r=1e-4, mu=0.4)),
    ("r-1", dict(r=-1.0)),
    ("r-1e3", dict(r=-1e3)),
]

SETTINGS_BY_NAME, BALANCE_BY_NAME = dict(SETTINGS), dict(BALANCE)


def oracle_args(oracle, settings=None, balance=None):
    """The oracle's (params, balance params) under two override dictionaries."""
    return (override(oracle.default_params(1), settings or {}), override(oracle.default_balance_params(), balance or {}))


@functools.lru_cache(maxsize=None)
def _reference(sname, bname, B, seed):
    import pyoracle
    ref = pyoracle.balance_solve_batch(*oracle_args(pyoracle, SETTINGS_BY_NAME[sname], BALANCE_BY_NAME[bname]),
                                       records(B, seed), 8)
    ref.setflags(write=False)
    return ref


def reference(oracle, sname="default", bname="default", B=B_GPU, seed=SEED):
    """The oracle's results for records(B, seed) under a named setting and a named balance parameter set;
    computed once per process and read-only.  `oracle` is the fixture (it has built the library)."""
    return _reference(sname, bname, B, seed)


def assert_full_parity(got, ref, label="balance", tol=1e-9):
    """A device result batch against the oracle's, over the whole result record: status, iteration and
    rho-update counts and nan_legs equal; u0 and f_body within `tol` of the row's scale where the oracle has a
    solution and the same NaN pattern everywhere; rho, pri_res, dua_res and obj_val within the relative bounds
    of the solve kernels' trace test.  The measured maxima go to gpu_helpers.note."""
    np.testing.assert_array_equal(got["status"], ref["status"])
    np.testing.assert_array_equal(got["iters"], ref["iters"])
    np.testing.assert_array_equal(got["rho_updates"], ref["rho_updates"])
    np.testing.assert_array_equal(got["nan_legs"], ref["nan_legs"])
    np.testing.assert_array_equal(np.isnan(got["u0"]), np.isnan(ref["u0"]))
    np.testing.assert_array_equal(np.isnan(got["f_body"]), np.isnan(ref["f_body"]))
    ok = ~np.isnan(ref["u0"]).any(1)
    scale = np.maximum(np.abs(ref["u0"][ok]).max(1, keepdims=True), 1.0)
    e_u0 = np.abs(got["u0"][ok] - ref["u0"][ok]) / scale
    e_fb = np.abs(got["f_body"][ok] - ref["f_body"][ok]) / scale
    assert np.all(np.isnan(got["u0"][~ok]))

    def rel(name, floor, slack):
        d = np.abs(got[name] - ref[name])
        bound = tol * np.maximum(np.abs(ref[name]), floor) + slack
        return d, bound

    measured = {"u0": float(e_u0.max()) if e_u0.size else 0.0, "f_body": float(e_fb.max()) if e_fb.size else 0.0}
    checks = {}
    # NaN is the objective OSQP reports for NON_CVX decided by a residual above OSQP_INFTY
    nan_obj = np.isnan(ref["obj_val"])
    np.testing.assert_array_equal(np.isnan(got["obj_val"]), nan_obj)
    for name, floor, slack in (("rho", 0.0, 0.0), ("pri_res", 1e-12, 1e-15), ("dua_res", 1e-12, 1e-15),
                               ("obj_val", 1.0, 0.0)):
        keep = ~nan_obj if name == "obj_val" else np.ones(len(ref), bool)
        d, bound = rel(name, floor, slack)
        checks[name] = (d[keep], bound[keep])
        den = np.maximum(np.abs(ref[name][keep]), floor if floor else 1e-300)
        measured[name] = float((d[keep] / den).max()) if keep.any() else 0.0
    from gpu_helpers import note
    note(f"balance full parity: {label}", robots=int(len(ref)), **{f"max_rel_{k}": v for k, v in measured.items()})
    assert np.all(e_u0 <= tol) and np.all(e_fb <= tol), f"{label}: u0 {measured['u0']:.3e} f_body {measured['f_body']:.3e}"
    for name, (d, bound) in checks.items():
        bad = np.flatnonzero(~(d <= bound))
        assert bad.size == 0, f"{label}: {name} of rows {bad[:8]} off by {d[bad][:8]} (bound {bound[bad][:8]})"
    big = np.abs(ref["obj_val"]) == OSQP_INFTY  # a certificate's objective is the constant itself
    np.testing.assert_array_equal(got["obj_val"][big], ref["obj_val"][big])
