"""tma_policy_evaluate_actions_vjp / tma_policy_head_vjp (include/tma.h, ABI 222) without a GPU: the symbols are exported and bound with the
documented argument lists, the two ..._backward calls keep theirs, every refusal -- the new ones and the inherited ones -- comes back as
TMA_ERR_INVALID with a message before any HIP call, tma_policy_vjp_workspace_bytes answers what it answered at ABI 221, and the Python keyword
errors and the opt-in (enable_obs_grad) are checked before anything touches a device."""
import ctypes as C
import inspect

import pytest
import torch

from three_mlagents_amd import _lib

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int
_pd = C.POINTER(_lib.PolicyDims)
NEW = {
    "tma_policy_evaluate_actions_vjp": [_vp, _pd, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "tma_policy_head_vjp": [_vp, _pd, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
}
OLD = {
    "tma_policy_evaluate_actions_backward": [_vp, _pd, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "tma_policy_head_backward": [_vp, _pd, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp],
}
# tma_policy_vjp_workspace_bytes of the ABI 221 build: (D, H, A, Box?, mfma_dtype, n) -> bytes
WORKSPACE_221 = {
    (4, 64, 5, 0, 0, 1): 38912, (4, 64, 5, 0, 0, 77): 194560, (4, 64, 5, 0, 0, 1 << 22): 39845888,
    (6, 256, 5, 0, 0, 1): 137216, (6, 256, 5, 0, 0, 77): 686080, (6, 256, 5, 0, 0, 1 << 22): 134197248,
    (6, 256, 5, 0, 2, 77): 686080,
    (105, 256, 8, 1, 0, 77): 686080, (105, 256, 8, 1, 0, 1 << 22): 134197248,
    (172, 1024, 20, 1, 0, 1): 530432, (172, 1024, 20, 1, 0, 77): 2652160, (172, 1024, 20, 1, 0, 1 << 22): 134199296,
}


def _dims(D=4, H=64, A=5, cont=0, dtype=0):
    return _lib.PolicyDims(D, H, A, cont, dtype, -1)


class _Host:
    """host memory standing in for every buffer: each case below must be refused before anything is read or launched"""

    def __init__(self, floats=4096):
        self.buf = (C.c_float * floats)()
        self.base = C.addressof(self.buf)

    def at(self, float_offset):
        return C.c_void_p(self.base + 4 * float_offset)


def _eval_vjp(d, *, params=True, obs=True, actions=True, grad_params=True, grad_obs=True, n=16, cots=(True, False, False), ws_bytes=None,
              obs_at=0, grad_obs_at=1024, ws_at=2048):
    L, h = _lib.lib(), _Host()
    need = L.tma_policy_vjp_workspace_bytes(C.byref(d), max(n, 1)) if ws_bytes is None else ws_bytes
    p = lambda on, off=3072: h.at(off) if on else None  # noqa: E731
    return L.tma_policy_evaluate_actions_vjp(p(params), C.byref(d), p(obs, obs_at), p(actions), n, p(cots[0]), p(cots[1]), p(cots[2]), p(grad_params),
                                             p(grad_obs, grad_obs_at), h.at(ws_at) if ws_at is not None else None, need, None)


def _head_vjp(d, *, params=True, obs=True, grad_params=True, grad_obs=True, n=16, cots=(True, False), ws_bytes=None, obs_at=0, grad_obs_at=1024,
              ws_at=2048):
    L, h = _lib.lib(), _Host()
    need = L.tma_policy_vjp_workspace_bytes(C.byref(d), max(n, 1)) if ws_bytes is None else ws_bytes
    p = lambda on, off=3072: h.at(off) if on else None  # noqa: E731
    return L.tma_policy_head_vjp(p(params), C.byref(d), p(obs, obs_at), n, p(cots[0]), p(cots[1]), p(grad_params), p(grad_obs, grad_obs_at),
                                 h.at(ws_at) if ws_at is not None else None, need, None)


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    assert L.tma_version() >= 222
    for name, args in {**NEW, **OLD}.items():
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        assert _lib.SIGNATURES[name] == (_i32, args), name
        assert list(getattr(L, name).argtypes) == args and getattr(L, name).restype is _i32, name


def test_the_header_declares_both_calls():
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tma.h")).read()
    flat = " ".join(header.split())
    assert ("int tma_policy_evaluate_actions_vjp(const float *params, const tma_policy_dims *d, const float *obs, const void *actions, int64_t n, "
            "const float *g_values, const float *g_logp, const float *g_entropy, float *grad_params") in flat
    assert "int tma_policy_head_vjp(const float *params, const tma_policy_dims *d, const float *obs, int64_t n, const float *g_head, const float *g_values, float *grad_params, float *grad_obs, void *workspace, int64_t workspace_bytes, void *stream);" in flat


@pytest.mark.parametrize("key,want", sorted(WORKSPACE_221.items()))
def test_workspace_bytes_did_not_move(key, want):
    D, H, A, cont, dtype, n = key
    assert _lib.lib().tma_policy_vjp_workspace_bytes(C.byref(_dims(D, H, A, cont, dtype)), n) == want


# n = 16 rows of D = 4: obs and grad_obs are 256 bytes = 64 floats each; the workspace of (4, 64, 5) at n = 16 is 38 912 bytes
NEW_REFUSALS = [
    ("both outputs NULL", dict(grad_params=False, grad_obs=False), "both null"),
    ("grad_obs is obs", dict(grad_obs_at=0), "overlaps obs"),
    ("grad_obs starts inside obs", dict(grad_obs_at=63), "overlaps obs"),
    ("grad_obs ends inside obs", dict(obs_at=1024 + 63), "overlaps obs"),
    ("grad_obs at the head of the workspace", dict(grad_obs_at=2048 - 1), "overlaps the workspace"),
    ("grad_obs inside the workspace", dict(grad_obs_at=2048 + 100), "overlaps the workspace"),
]
INHERITED = [
    ("null params", dict(params=False), None), ("null obs", dict(obs=False), None), ("n = 0", dict(n=0), "n must be >= 1"),
    ("n < 0", dict(n=-3), "n must be >= 1"), ("short workspace", dict(ws_bytes=15), "workspace"), ("null workspace", dict(ws_at=None), "workspace"),
]


@pytest.mark.parametrize("case,kw,text", NEW_REFUSALS + INHERITED + [("null actions", dict(actions=False), None),
                                                                     ("three NULL cotangents", dict(cots=(False, False, False)), "all null")])
def test_evaluate_actions_vjp_refusals_come_back_before_any_hip_call(case, kw, text):
    _lib.lib().tma_policy_param_count(None, None, None)  # leaves ANOTHER message behind: the one asserted below is this call's
    assert _eval_vjp(_dims(), **kw) == _lib.TMA_ERR_INVALID, case
    msg = _lib.last_error()
    assert "tma_policy_evaluate_actions_vjp" in msg and (text is None or text in msg), (case, msg)
    with pytest.raises(ValueError):
        _lib.check(_eval_vjp(_dims(), **kw))


@pytest.mark.parametrize("case,kw,text", NEW_REFUSALS + INHERITED + [("two NULL cotangents", dict(cots=(False, False)), "both null")])
def test_head_vjp_refusals_come_back_before_any_hip_call(case, kw, text):
    _lib.lib().tma_policy_param_count(None, None, None)
    assert _head_vjp(_dims(), **kw) == _lib.TMA_ERR_INVALID, case
    msg = _lib.last_error()
    assert "tma_policy_head_vjp" in msg and (text is None or text in msg), (case, msg)


def test_adjacent_buffers_are_not_an_overlap():
    """grad_obs ending where obs begins (and the other way round) passes the overlap checks: the call goes on to the NEXT refusal (a short
    workspace), still before any HIP call"""
    for kw in (dict(obs_at=64, grad_obs_at=0), dict(obs_at=0, grad_obs_at=64)):
        assert _eval_vjp(_dims(), ws_bytes=15, **kw) == _lib.TMA_ERR_INVALID and "reports" in _lib.last_error()
        assert _head_vjp(_dims(), ws_bytes=15, **kw) == _lib.TMA_ERR_INVALID and "reports" in _lib.last_error()


def test_one_output_alone_is_accepted_up_to_the_next_refusal():
    for kw in (dict(grad_params=False), dict(grad_obs=False)):
        assert _eval_vjp(_dims(), ws_bytes=15, **kw) == _lib.TMA_ERR_INVALID and "reports" in _lib.last_error()
        assert _head_vjp(_dims(), ws_bytes=15, **kw) == _lib.TMA_ERR_INVALID and "reports" in _lib.last_error()


@pytest.mark.parametrize("bad", [(0, 64, 5, 0, 0), (4, 96, 5, 0, 0), (4, 64, 17, 0, 0), (4, 64, 33, 1, 0), (4, 64, 5, 0, 3), (6, 128, 5, 0, 2)])
def test_bad_dims_are_refused(bad):
    assert _eval_vjp(_dims(*bad), ws_bytes=1 << 20) == _lib.TMA_ERR_INVALID and _lib.last_error()
    assert _head_vjp(_dims(*bad), ws_bytes=1 << 20) == _lib.TMA_ERR_INVALID and _lib.last_error()


def test_bf16_dims_are_refused_with_a_reason():
    d = _dims(6, 256, 5, 0, 1)
    assert _eval_vjp(d, ws_bytes=1 << 20) == _lib.TMA_ERR_INVALID and "bf16" in _lib.last_error()
    assert _head_vjp(d, ws_bytes=1 << 20) == _lib.TMA_ERR_INVALID and "bf16" in _lib.last_error()


def test_the_backward_calls_keep_their_refusals():
    L, h, d = _lib.lib(), _Host(), _dims()
    need = L.tma_policy_vjp_workspace_bytes(C.byref(d), 16)
    b = h.at(0)
    assert L.tma_policy_evaluate_actions_backward(b, C.byref(d), b, b, 16, b, None, None, None, b, need, None) == _lib.TMA_ERR_INVALID
    assert "tma_policy_evaluate_actions_backward: null buffer" in _lib.last_error()
    assert L.tma_policy_head_backward(b, C.byref(d), b, 16, b, None, None, b, need, None) == _lib.TMA_ERR_INVALID
    assert "tma_policy_head_backward: null buffer" in _lib.last_error()


# ---- the Python surface, as far as a run without a device reaches
def _shell(mfma="f32"):
    """a HipActorCriticPolicy without its device buffers: what the argument checks in front of the first library call read"""
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    pol = HipActorCriticPolicy.__new__(HipActorCriticPolicy)
    pol.mfma_dtype, pol.obs_dim, pol.act_dim, pol.continuous, pol.device, pol._leaf, pol._obs_grad = mfma, 6, 5, False, torch.device("cpu"), None, False
    return pol


def test_keyword_only_flags():
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    for name in ("evaluate_actions_backward", "head_backward"):
        par = inspect.signature(getattr(HipActorCriticPolicy, name)).parameters
        assert par["params_grad"].kind is par["obs_grad"].kind is inspect.Parameter.KEYWORD_ONLY
        assert par["params_grad"].default is True and par["obs_grad"].default is False
    pol = _shell()
    obs, actions = torch.zeros(8, 6), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(ValueError, match="both False"):
        pol.evaluate_actions_backward(obs, actions, torch.ones(8), params_grad=False, obs_grad=False)
    with pytest.raises(ValueError, match="both False"):
        pol.head_backward(obs, None, torch.ones(8), params_grad=False, obs_grad=False)


def test_a_bf16_policy_refuses_enable_obs_grad_for_the_reason_parameters_gives():
    pol = _shell("bf16")
    with pytest.raises(ValueError) as why:
        pol.parameters()
    with pytest.raises(ValueError) as mine:
        pol.enable_obs_grad()
    assert str(mine.value).split(": ", 1)[1] == str(why.value).split(": ", 1)[1]
    assert pol._obs_grad is False and pol.enable_obs_grad(False) is pol


def test_obs_gradients_are_opt_in():
    """Without enable_obs_grad() an obs that requires grad is a ValueError naming the switch wherever the call is differentiable with respect to
    the parameters -- raised before anything touches a device"""
    pol = _shell()
    assert pol.enable_obs_grad() is pol and pol._obs_grad is True and pol.enable_obs_grad(False)._obs_grad is False
    pol._leaf = torch.zeros(4, requires_grad=True)
    pol._synced_version = pol._leaf._version
    x = torch.zeros(8, 6, requires_grad=True)
    for call in (lambda: pol.evaluate_actions(x, torch.zeros(8, dtype=torch.int32)), lambda: pol.head(x), lambda: pol.get_distribution(x)):
        with pytest.raises(ValueError, match="enable_obs_grad"):
            call()
