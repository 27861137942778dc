"""The pieces of a stable-baselines3 model zip that only SB3 can normally write (the reference saves with
`model.save(...)` at backend/mlagents/training.py:172-175 and reads back with `PPO.load(...)`): the `data` JSON whose non-JSON members
are base64 cloudpickle blobs, and the torch.optim.Adam state_dict of `policy.optimizer.pth`.

stable-baselines3 and gymnasium are not installed here, so the three blobs `BaseAlgorithm.load` cannot do without are produced from
their public pickle forms instead of from live objects:
  * `policy_class`     -- a class pickles BY REFERENCE: the GLOBAL opcode naming `stable_baselines3.common.policies.ActorCriticPolicy`.
  * `observation_space`, `action_space` -- gymnasium spaces pickle as `copyreg.__newobj__(cls)` + the instance `__dict__`, and
    `Space.__setstate__` restores them with `self.__dict__.update(state)`; the blob is written by pickling a stand-in object whose class
    carries gymnasium's module / qualified name (`gymnasium.spaces.box.Box`, `gymnasium.spaces.discrete.Discrete`) and whose `__dict__`
    holds the attributes gymnasium's own instances have.
Everything else SB3's `_setup_model` reads after `model.__dict__.update(data)` is a JSON scalar.  VERIFIED HERE ONLY against torch itself
(optimizer / policy state_dicts load into a torch module laid out like SB3's ActorCriticPolicy) and against a re-statement of SB3's
`json_to_data` + gymnasium's `__setstate__` (tests/test_harness_cpu.py); never against SB3, which this image does not have.
"""
from __future__ import annotations

import base64
import contextlib
import pickle
import re
import sys
import types
from typing import Any

import numpy as np

POLICY_CLASS = ("stable_baselines3.common.policies", "ActorCriticPolicy")


def class_reference_pickle(module: str, qualname: str) -> bytes:
    """pickle.dumps(cls) for an importable class: PROTO 2, GLOBAL module / name, STOP."""
    return b"\x80\x02c" + module.encode() + b"\n" + qualname.encode() + b"\n."


@contextlib.contextmanager
def _stand_in(module: str, qualname: str):
    """A class that pickles as `module.qualname`, registered under stub modules for the duration of one dumps() call."""
    made, cls = [], type(qualname, (), {"__module__": module, "__qualname__": qualname})
    parts = module.split(".")
    for depth in range(1, len(parts) + 1):
        name = ".".join(parts[:depth])
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
            made.append(name)
    had = getattr(sys.modules[module], qualname, None)
    setattr(sys.modules[module], qualname, cls)
    try:
        yield cls
    finally:
        if had is None:
            delattr(sys.modules[module], qualname)
        else:
            setattr(sys.modules[module], qualname, had)
        for name in made:
            sys.modules.pop(name, None)


def space_state(space) -> tuple[str, str, dict[str, Any]]:
    """(module, class name, instance __dict__) of the gymnasium space equal to `space` (a spaces.Box / spaces.Discrete of this package
    or gymnasium's own)."""
    if hasattr(space, "n"):
        return "gymnasium.spaces.discrete", "Discrete", {"n": np.int64(space.n), "start": np.int64(getattr(space, "start", 0)), "_shape": (),
                                                         "dtype": np.dtype(np.int64), "_np_random": None}
    low, high = np.asarray(space.low, np.float32), np.asarray(space.high, np.float32)

    def short(a):
        return str(a.flat[0]) if a.size and np.all(a == a.flat[0]) else str(a)

    return "gymnasium.spaces.box", "Box", {"dtype": np.dtype(np.float32), "_shape": tuple(int(x) for x in space.shape), "low": low, "high": high,
                                           "low_repr": short(low), "high_repr": short(high), "bounded_below": np.isfinite(low),
                                           "bounded_above": np.isfinite(high), "_np_random": None}


def space_pickle(space) -> bytes:
    module, name, state = space_state(space)
    with _stand_in(module, name) as cls:
        obj = cls()
        obj.__dict__.update(state)
        return pickle.dumps(obj, protocol=2)


def serialized(blob: bytes, type_name: str, **readable) -> dict[str, Any]:
    """One non-JSON member of `data`, as SB3's data_to_json writes it."""
    return {":type:": type_name, ":serialized:": base64.b64encode(blob).decode(), **readable}


def data_members(observation_space, action_space, policy_class: tuple[str, str] = POLICY_CLASS) -> dict[str, Any]:
    """The three members of `data` BaseAlgorithm.load needs as live objects.  policy_class: (module, name) of the class SB3 would pickle by
    reference -- ActorCriticPolicy for PPO / A2C, `("stable_baselines3.dqn.policies", "DQNPolicy")` for DQN."""
    om, on, _ = space_state(observation_space)
    am, an, _ = space_state(action_space)
    return {
        "policy_class": serialized(class_reference_pickle(*policy_class), "<class 'abc.ABCMeta'>", __module__=policy_class[0]),
        "observation_space": serialized(space_pickle(observation_space), f"<class '{om}.{on}'>", _shape=list(observation_space.shape)),
        "action_space": serialized(space_pickle(action_space), f"<class '{am}.{an}'>", _shape=list(action_space.shape)),
    }


# ---- policy_kwargs: activation_fn, log_std_init, ortho_init.  SB3's data_to_json keeps, beside the pickled blob of a non-JSON member, a str() of
# each of its items: a policy built with activation_fn=nn.ReLU leaves "activation_fn": "<class 'torch.nn.modules.activation.ReLU'>" there.
ACTIVATIONS = {"tanh": (0, "Tanh"), "relu": (1, "ReLU")}  # name -> (tma_policy_dims.activation, torch.nn class name)


def parse_activation(fn) -> str:
    """policy_kwargs["activation_fn"] -> "tanh" / "relu".  Accepted: None (SB3's default, tanh), torch.nn.Tanh, torch.nn.ReLU, "tanh", "relu"."""
    if fn is None:
        return "tanh"
    if isinstance(fn, str) and fn.lower() in ACTIVATIONS:
        return fn.lower()
    if isinstance(fn, type):
        import torch

        for name, (_, cls) in ACTIVATIONS.items():
            if fn is getattr(torch.nn, cls):
                return name
    raise ValueError(f"activation_fn must be torch.nn.Tanh or torch.nn.ReLU (or 'tanh' / 'relu'), got {fn!r}: the kernels have no other activation")


def activation_repr(name: str) -> str:
    """str(torch.nn.<cls>): what SB3's JSON shows for the member."""
    return f"<class 'torch.nn.modules.activation.{ACTIVATIONS[name][1]}'>"


def policy_kwargs_data(hidden: int, activation: str = "tanh", log_std_init: float = 0.0, ortho_init: bool = True) -> dict[str, Any]:
    """data["policy_kwargs"] of a zip: net_arch, and each of the three other supported kwargs where it is not SB3's default."""
    pk: dict[str, Any] = {"net_arch": [int(hidden), int(hidden)]}
    if activation != "tanh":
        pk["activation_fn"] = activation_repr(activation)
    if float(log_std_init) != 0.0:
        pk["log_std_init"] = float(log_std_init)
    if not ortho_init:
        pk["ortho_init"] = False
    return pk


def policy_kwargs_from_data(data: dict) -> dict[str, Any]:
    """{"activation_fn", "log_std_init", "ortho_init"} of a zip's `data`: the activation from data["tma"] (this engine's zips), else from the text
    of data["policy_kwargs"]["activation_fn"] (this engine's, or the str() SB3 keeps beside its blob), else tanh.  A name that is neither Tanh nor
    ReLU is a ValueError: such a zip would otherwise run its weights through the wrong non-linearity."""
    tma = data.get("tma") if isinstance(data.get("tma"), dict) else {}
    pk = data.get("policy_kwargs") if isinstance(data.get("policy_kwargs"), dict) else {}
    act = None
    if tma.get("activation") is not None:
        act = parse_activation(str(tma["activation"]))
    elif pk.get("activation_fn") is not None:
        text = str(pk["activation_fn"])
        words = re.findall(r"[A-Za-z_]\w*", text)  # the class name is the last identifier of "<class 'torch.nn.modules.activation.ReLU'>" (LeakyReLU is not ReLU)
        hits = [name for name, (_, cls) in ACTIVATIONS.items() if words and (words[-1] == cls or words[-1].lower() == name)]
        if len(hits) != 1:
            raise ValueError(f"policy zip with activation_fn {text!r}: the engine runs torch.nn.Tanh and torch.nn.ReLU policies only")
        act = hits[0]
    out: dict[str, Any] = {"activation_fn": act or "tanh", "log_std_init": 0.0, "ortho_init": True}
    if isinstance(pk.get("log_std_init"), (int, float)):
        out["log_std_init"] = float(pk["log_std_init"])
    if isinstance(pk.get("ortho_init"), bool):
        out["ortho_init"] = pk["ortho_init"]
    return out


# torch registers an ActorCriticPolicy's parameters in this order: the module's own (log_std) first, then the sub-modules in the order
# _build creates them -- the order torch.optim.Adam's state_dict indexes them by
def parameter_order(continuous: bool) -> list[str]:
    names = ["log_std"] if continuous else []
    for net in ("policy_net", "value_net"):
        for layer in (0, 2):
            names += [f"mlp_extractor.{net}.{layer}.weight", f"mlp_extractor.{net}.{layer}.bias"]
    return names + ["action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias"]


def adam_state_dict(order, exp_avg: dict, exp_avg_sq: dict, step: int, lr: float, eps: float = 1e-5) -> dict[str, Any]:
    """torch.optim.Adam.state_dict() for parameters `order` with the given moments (per-parameter tensors in SB3's [out][in] layout)."""
    import torch

    state = {}
    if step > 0:
        for i, name in enumerate(order):
            state[i] = {"step": torch.tensor(float(step)), "exp_avg": exp_avg[name].clone(), "exp_avg_sq": exp_avg_sq[name].clone()}
    group = {"lr": lr, "betas": (0.9, 0.999), "eps": eps, "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
             "differentiable": False, "fused": None, "params": list(range(len(order)))}
    return {"state": state, "param_groups": [group]}


def rmsprop_state_dict(order, square_avg: dict, step: int, lr: float, alpha: float = 0.99, eps: float = 1e-5) -> dict[str, Any]:
    """stable_baselines3.common.sb2_compat.rmsprop_tf_like.RMSpropTFLike.state_dict() (A2C's optimizer; no momentum, not centered: the state of a
    parameter is its step count and `square_avg`) for parameters `order`."""
    state = {}
    if step > 0:
        for i, name in enumerate(order):
            state[i] = {"step": int(step), "square_avg": square_avg[name].clone()}
    group = {"lr": lr, "alpha": alpha, "eps": eps, "weight_decay": 0, "momentum": 0, "centered": False, "params": list(range(len(order)))}
    return {"state": state, "param_groups": [group]}
