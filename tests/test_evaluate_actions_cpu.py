"""include/tma.h, ABI 210, without a GPU: tma_policy_evaluate_actions (SB3's ActorCriticPolicy.evaluate_actions on the device) and
tma_explained_variance are exported, and every refusal comes back as TMA_ERR_INVALID with a message before any HIP call."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from three_mlagents_amd import _lib

    return _lib


def test_the_symbols_are_exported_and_the_abi_is_210():
    _lib_ = _lib()
    L = _lib_.lib()
    assert hasattr(L, "tma_policy_evaluate_actions") and hasattr(L, "tma_explained_variance")
    assert "tma_policy_evaluate_actions" in _lib_.SIGNATURES and "tma_explained_variance" in _lib_.SIGNATURES
    assert L.tma_version() >= 210


def test_evaluate_actions_refuses_bad_arguments_without_touching_a_gpu():
    _lib_ = _lib()
    L = _lib_.lib()
    good = _lib_.PolicyDims(6, 256, 5, 0, 0, -1)  # (device -1: the calling thread's current device -- no HIP call to select one)
    buf = (C.c_float * 64)()  # host memory standing in for the device buffers: a refused call never reads it
    p = C.cast(buf, C.c_void_p)

    def call(dims, params, obs, actions, n, values, logp, entropy):
        return L.tma_policy_evaluate_actions(params, C.byref(dims) if dims is not None else None, obs, actions, n, values, logp, entropy, None)

    cases = {
        "null dims": (None, p, p, p, 4, p, p, p),
        "obs_dim 0": (_lib_.PolicyDims(0, 256, 5, 0, 0, -1), p, p, p, 4, p, p, p),
        "hidden 100": (_lib_.PolicyDims(6, 100, 5, 0, 0, -1), p, p, p, 4, p, p, p),
        "17 discrete actions": (_lib_.PolicyDims(6, 256, 17, 0, 0, -1), p, p, p, 4, p, p, p),
        "box dim 33": (_lib_.PolicyDims(6, 256, 33, 1, 0, -1), p, p, p, 4, p, p, p),
        "mfma_dtype 3": (_lib_.PolicyDims(6, 256, 5, 0, 3, -1), p, p, p, 4, p, p, p),
        "bf16 at hidden 64": (_lib_.PolicyDims(6, 64, 5, 0, 1, -1), p, p, p, 4, p, p, p),
        "null params": (good, None, p, p, 4, p, p, p),
        "null obs": (good, p, None, p, 4, p, p, p),
        "null actions": (good, p, p, None, 4, p, p, p),
        "n = 0": (good, p, p, p, 0, p, p, p),
        "n < 0": (good, p, p, p, -3, p, p, p),
        "all outputs null": (good, p, p, p, 4, None, None, None),
    }
    for name, args in cases.items():
        rc = call(*args)
        assert rc == _lib_.TMA_ERR_INVALID, (name, rc)
        assert _lib_.last_error(), name
        with pytest.raises(ValueError):
            _lib_.check(rc)
    call(good, p, p, p, 4, None, None, None)
    assert "all null" in _lib_.last_error()
    # a policy that names a device is refused the same way, before that device is made current
    on_dev0 = _lib_.PolicyDims(6, 256, 5, 0, 0, 0)
    assert call(on_dev0, None, p, p, 4, p, p, p) == _lib_.TMA_ERR_INVALID
    assert call(on_dev0, p, p, p, 4, None, None, None) == _lib_.TMA_ERR_INVALID


def test_explained_variance_refuses_bad_arguments_without_touching_a_gpu():
    _lib_ = _lib()
    L = _lib_.lib()
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    for args in ((None, p, 4, p, p), (p, None, 4, p, p), (p, p, 4, None, p), (p, p, 4, p, None), (p, p, 0, p, p), (p, p, -1, p, p)):
        rc = L.tma_explained_variance(*args, None)
        assert rc == _lib_.TMA_ERR_INVALID and "tma_explained_variance" in _lib_.last_error(), args
    header = open(os.path.join(ROOT, "include", "tma.h")).read()
    assert f"#define TMA_EV_SCRATCH_DOUBLES {_lib_.EV_SCRATCH_DOUBLES}\n" in header


def test_the_python_surface_exists():
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    assert callable(getattr(HipActorCriticPolicy, "evaluate_actions")) and callable(getattr(HipActorCriticPolicy, "forward"))
