"""The keyword overrides of the ten default_* parameter functions go through one helper (mpcqp._lib.override):
an unknown name raises AttributeError, a c_double array field takes exactly its length, a scalar is set, ``seed``
splits into two words, ``hidden`` sets n_hidden, and with no override the structure is the C default's.  No device."""
import ctypes

import numpy as np
import pytest

import mpcqp
from mpcqp import _lib

# python function: (structure, the C default function, an array field or None, a scalar field and a value or None)
FUNCTIONS = {
    _lib.default_params: (_lib.Params, "mpcqp_default_params", "q_weights", ("max_iter", 37)),
    _lib.default_balance_params: (_lib.BalanceParams, "mpcqp_balance_default_params", "q_diag", ("mu", 0.45)),
    mpcqp.default_balance_gains: (_lib.BalanceGains, "mpcqp_balance_default_gains", "kd_angular", None),
    mpcqp.default_command_params: (_lib.CommandParams, "mpcqp_command_default_params", "kp_linear",
                                   ("body_height_max", 0.31)),
    mpcqp.default_plan_params: (_lib.PlanParams, "mpcqp_plan_default_params", "kp_foot", ("use_terrain_adapt", 0)),
    mpcqp.default_estimator_params: (_lib.EstimatorParams, "mpcqp_est_default_params", "rho_fix", ("gravity", 9.5)),
    mpcqp.default_plant_params: (_lib.PlantParams, "mpcqp_plant_default_params", "inertia", ("substeps", 3)),
    mpcqp.default_episode_params: (_lib.EpisodeParams, "mpcqp_episode_default_params", None, ("max_ticks", 123)),
    mpcqp.default_disturb_params: (_lib.DisturbParams, "mpcqp_disturb_default_params", "sigma", ("bias_acc", 0.25)),
    mpcqp.default_policy_params: (_lib.PolicyParams, "mpcqp_policy_default_params", "obs_scale", ("clip_obs", 55.0)),
}
IDS = [f.__name__ for f in FUNCTIONS]


def test_the_table_names_every_default_function():
    assert len(FUNCTIONS) == 10
    assert mpcqp.default_balance_gains is mpcqp.balance.default_balance_gains
    assert mpcqp.balance.default_balance_params is _lib.default_balance_params


@pytest.mark.parametrize("fn", list(FUNCTIONS), ids=IDS)
def test_no_override_is_the_c_default(fn):
    cls, c_name, _, _ = FUNCTIONS[fn]
    direct = cls()
    c_fn = getattr(_lib.load(), c_name)
    if fn is _lib.default_params:
        c_fn(ctypes.byref(direct), 10)
    else:
        c_fn(ctypes.byref(direct))
    p = fn()
    assert type(p) is cls and bytes(p) == bytes(direct)
    assert any(bytes(p))  # the defaults are not the zero fill of a fresh structure


@pytest.mark.parametrize("fn", list(FUNCTIONS), ids=IDS)
def test_unknown_name_raises(fn):
    with pytest.raises(AttributeError, match="no_such_field"):
        fn(no_such_field=1.0)
    cls, _, array, scalar = FUNCTIONS[fn]
    name = scalar[0] if scalar else array
    with pytest.raises(AttributeError, match=name + "s"):  # the misspelling setattr used to swallow
        fn(**{name + "s": 1.0})


@pytest.mark.parametrize("fn", [f for f in FUNCTIONS if FUNCTIONS[f][2]],
                         ids=[f.__name__ for f in FUNCTIONS if FUNCTIONS[f][2]])
def test_array_takes_exactly_its_length(fn):
    cls, _, array, _ = FUNCTIONS[fn]
    n = len(getattr(cls(), array))
    for m in (n - 1, n + 1):
        with pytest.raises(ValueError, match=f"{array}: expected {n} values, got {m}"):
            fn(**{array: np.arange(m, dtype=float)})
    want = np.arange(n, dtype=float) * 0.5 + 1.0
    p = fn(**{array: want})
    assert list(getattr(p, array)) == want.tolist()
    if n % 3 == 0:  # anything that flattens to the length: [n/3][3] as well
        p = fn(**{array: want.reshape(-1, 3)[::-1]})
        assert list(getattr(p, array)) == want.reshape(-1, 3)[::-1].ravel().tolist()
    others = {name: bytes(getattr(p, name)) if isinstance(getattr(p, name), ctypes.Array) else getattr(p, name)
              for name, _ in cls._fields_ if name != array}
    base = fn()
    assert others == {name: bytes(getattr(base, name)) if isinstance(getattr(base, name), ctypes.Array)
                      else getattr(base, name) for name, _ in cls._fields_ if name != array}


@pytest.mark.parametrize("fn", [f for f in FUNCTIONS if FUNCTIONS[f][3]],
                         ids=[f.__name__ for f in FUNCTIONS if FUNCTIONS[f][3]])
def test_scalar_lands(fn):
    name, value = FUNCTIONS[fn][3]
    assert getattr(fn(), name) != value
    assert getattr(fn(**{name: value}), name) == value


@pytest.mark.parametrize("fn", [mpcqp.default_episode_params, mpcqp.default_disturb_params],
                         ids=["default_episode_params", "default_disturb_params"])
def test_seed_splits_into_two_words(fn):
    p = fn(seed=(1 << 40) + 5)
    assert (p.seed[0], p.seed[1]) == (5, 1 << 8)
    p = fn(seed=0xFFFFFFFF_00000001)
    assert (p.seed[0], p.seed[1]) == (1, 0xFFFFFFFF)


def test_hidden_sets_n_hidden():
    p = mpcqp.default_policy_params(hidden=[64, 32])
    assert p.n_hidden == 2 and list(p.hidden) == [64, 32, 0]
    p = mpcqp.default_policy_params(hidden=[16])
    assert p.n_hidden == 1 and list(p.hidden) == [16, 0, 0]
    for bad in ([], [8, 8, 8, 8]):
        with pytest.raises(ValueError, match="hidden: expected 1 to 3 widths"):
            mpcqp.default_policy_params(hidden=bad)


def test_horizon_stays_the_first_argument():
    assert _lib.default_params(7).horizon == 7 and _lib.default_params(horizon=12, rho=0.3).rho == 0.3
