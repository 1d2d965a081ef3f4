"""Policy stage of the control tick (host side of mpcqp_policy_device): the reference's Go1 RL controller
(src/go1_rl_ctrl_cpp).

Per robot and per tick the device stage builds the 48-wide observation (observation/Go1Observation.hpp:152-166,
Go1RLController.cpp:95-96), runs the MLP that ``TorchEigen::run`` runs (:98), clips the action and forms the joint
targets (:99-109), or interpolates the servo stand (``advance_servo``, :121-146) when the robot's movement_mode
is not 1.0, and applies the motor law ``tau = Kp (target - q) - Kd dq`` to the LowCmd ``send_cmd`` would fill
(:149-166).  What the controller keeps between ticks lives in a per-robot device slot of ``policy_state_size()``
doubles, zero-filled = fresh.  The weights are packed for the kernel once, by ``Policy``.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import PolicyParams, check, load, override

OBS_DIM, ACTION_DIM = 48, 12

# the slot (include/mpcqp.h MPCQP_PS_*); flags and modes as 0.0 / 1.0
POLICY_STATE_DTYPE = np.dtype([
    ("init", "f8"), ("tick", "f8"), ("servo_motion_time", "f8"), ("mode", "f8"),
    ("prev_action", "f8", 12), ("target", "f8", 12),
])
assert POLICY_STATE_DTYPE.itemsize == 8 * _lib.PS_SIZE
# the optional output row (MPCQP_PY_*)
POLICY_OUT_DTYPE = np.dtype([
    ("obs", "f8", 48), ("raw", "f8", 12), ("action", "f8", 12), ("target", "f8", 12), ("torque", "f8", 12),
    ("status", "f8"), ("updated", "f8"), ("pad", "f8", 2),
])
assert POLICY_OUT_DTYPE.itemsize == 8 * _lib.PY_SIZE

def _set_hidden(p, v):
    widths = [int(x) for x in v]
    if not 1 <= len(widths) <= 3:
        raise ValueError(f"hidden: expected 1 to 3 widths, got {len(widths)}")
    p.n_hidden = len(widths)
    for i in range(3):
        p.hidden[i] = widths[i] if i < len(widths) else 0


def default_policy_params(**over):
    """mpcqp_policy_default_params (Go1Observation.hpp:52-63, :449; Go1RLController.hpp:84, :88;
    Go1RLController.cpp:36-37, :79-86, :122-132, :139; Go1CtrlStates.hpp:75-78) + keyword overrides.
    ``hidden`` is a sequence of 1 to 3 widths and sets n_hidden; the array fields accept sequences."""
    p = PolicyParams()
    load().mpcqp_policy_default_params(ctypes.byref(p))
    return override(p, over, {"hidden": _set_hidden})


def policy_state_size():
    """Doubles per robot of the policy slot (mpcqp_policy_state_size)."""
    return int(load().mpcqp_policy_state_size())


class Policy:
    """A network packed on one device (mpcqp_policy_create).  weights[l] is layer l's [out][in] matrix as
    torch.nn.Linear stores it, biases[l] its [out] vector; the widths must be those of ``params``."""

    def __init__(self, weights, biases, params=None, device=0):
        self._h = None
        ws = [np.ascontiguousarray(np.asarray(w), dtype=np.float32) for w in weights]
        bs = [np.ascontiguousarray(np.asarray(b), dtype=np.float32).reshape(-1) for b in biases]
        if params is None:
            params = default_policy_params(hidden=[w.shape[0] for w in ws[:-1]])
        dims = [OBS_DIM] + [params.hidden[i] for i in range(params.n_hidden)] + [ACTION_DIM]
        if len(ws) != len(dims) - 1 or len(bs) != len(ws):
            raise ValueError(f"expected {len(dims) - 1} weight matrices and as many biases, got {len(ws)} / {len(bs)}")
        for l, (w, b) in enumerate(zip(ws, bs)):
            if w.shape != (dims[l + 1], dims[l]) or b.shape != (dims[l + 1],):
                raise ValueError(f"layer {l}: expected weight {(dims[l + 1], dims[l])} and bias {(dims[l + 1],)}, "
                                 f"got {w.shape} and {b.shape}")
        self.params = params
        self.device = int(device)
        self.dims = dims
        fp = ctypes.POINTER(ctypes.c_float)
        wp = (fp * len(ws))(*[w.ctypes.data_as(fp) for w in ws])
        bp = (fp * len(bs))(*[b.ctypes.data_as(fp) for b in bs])
        h = ctypes.c_void_p()
        check(load().mpcqp_policy_create(ctypes.byref(params), wp, bp, self.device, ctypes.byref(h)), None,
              "mpcqp_policy_create")
        self._h = h

    @property
    def handle(self):
        if self._h is None:
            raise _lib.MpcQpError("policy is closed")
        return self._h

    def close(self):
        if self._h is not None:
            load().mpcqp_policy_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def policy_device(policy, d_sensors, d_states, d_plan_in, d_cmd, batch, d_policy_state, d_joint_torques,
                  d_policy_out=0, d_type=0, type=2, stream=0):
    """mpcqp_policy_device on device pointers (ints).  d_type = 0: every robot runs."""
    check(load().mpcqp_policy_device(policy.handle, d_sensors, d_states, d_plan_in, d_cmd, int(batch), d_policy_state,
                                     d_type or None, int(type), d_joint_torques, d_policy_out or None, stream or None),
          None, "mpcqp_policy_device")


def load_policy_weights(path):
    """(weights, biases) as lists of float32 arrays, from an .npz (keys w0, b0, w1, b1, ... or any keys whose
    sorted order alternates weight, bias per layer as a state_dict's does) or from a TorchScript / state_dict
    file such as the reference's resource/cpp_model.pt (read with torch on the caller's machine)."""
    path = str(path)
    if path.endswith(".npz"):
        with np.load(path) as z:
            tensors = [np.asarray(z[k]) for k in sorted(z.files, key=_layer_key)]
    else:
        import torch
        try:
            named = list(torch.jit.load(path, map_location="cpu").named_parameters())
        except RuntimeError:
            sd = torch.load(path, map_location="cpu")
            sd = sd.get("model_state_dict", sd) if isinstance(sd, dict) else sd.state_dict()
            named = list(sd.items())
        tensors = [t.detach().cpu().numpy() for _, t in named]
    ws = [np.ascontiguousarray(t, dtype=np.float32) for t in tensors if t.ndim == 2]
    bs = [np.ascontiguousarray(t, dtype=np.float32) for t in tensors if t.ndim == 1]
    if not ws or len(ws) != len(bs):
        raise ValueError(f"{path}: expected as many weight matrices as bias vectors, got {len(ws)} and {len(bs)}")
    for l, (w, b) in enumerate(zip(ws, bs)):
        if w.shape[0] != b.shape[0] or (l and w.shape[1] != ws[l - 1].shape[0]):
            raise ValueError(f"{path}: layer {l} shapes {w.shape} / {b.shape} do not chain")
    return ws, bs


def _layer_key(name):
    """Sort key of a tensor name: by the first integer in it, weights before biases."""
    import re
    m = re.search(r"\d+", name)
    return (int(m.group()) if m else 0, 0 if name.lower().startswith("w") or "weight" in name.lower() else 1, name)
