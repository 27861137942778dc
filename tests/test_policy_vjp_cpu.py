"""tma_policy_evaluate_actions_backward / tma_policy_vjp_workspace_bytes (include/tma.h, ABI 215) without a GPU: the symbols are exported and
bound, every documented refusal comes back as TMA_ERR_INVALID with a message before any HIP call, and the workspace stays within 256 MB for
every accepted shape whatever the batch."""
import ctypes as C

import pytest

from three_mlagents_amd import _lib

NAMES = ("tma_policy_vjp_workspace_bytes", "tma_policy_evaluate_actions_backward")
SHAPES = [(4, 64, 5, 0), (172, 1024, 20, 1), (6, 256, 16, 0)]  # (D, H, A, Box?)
MB256 = 256 << 20


def _dims(D, H, A, cont, dtype=0):
    return _lib.PolicyDims(D, H, A, cont, dtype, -1)


def _backward(d, *, params=True, obs=True, actions=True, grad=True, n=16, cots=(True, False, False), ws_bytes=None):
    """The call with host memory standing in for every buffer: each case below must be refused before anything is read or launched."""
    L = _lib.lib()
    buf = (C.c_float * 16)()
    need = L.tma_policy_vjp_workspace_bytes(C.byref(d), max(n, 1))
    p = lambda on: buf if on else None  # noqa: E731
    return L.tma_policy_evaluate_actions_backward(p(params), C.byref(d) if d is not None else None, p(obs), p(actions), n, p(cots[0]), p(cots[1]), p(cots[2]),
                                                  p(grad), buf, need if ws_bytes is None else ws_bytes, None)


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    assert L.tma_version() >= 215
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.tma_policy_vjp_workspace_bytes.restype is C.c_int64


@pytest.mark.parametrize("D,H,A,cont", SHAPES)
@pytest.mark.parametrize("n", [1, 77, 1 << 22])
def test_workspace_is_bounded_independently_of_n(D, H, A, cont, n):
    b = _lib.lib().tma_policy_vjp_workspace_bytes(C.byref(_dims(D, H, A, cont)), n)
    assert 0 < b <= MB256, b
    assert b <= _lib.lib().tma_policy_vjp_workspace_bytes(C.byref(_dims(D, H, A, cont)), 1 << 30) <= MB256  # it grows with n up to the chunk, then stays


@pytest.mark.parametrize("case,kw", [
    ("null params", dict(params=False)), ("null obs", dict(obs=False)), ("null actions", dict(actions=False)), ("null grad_out", dict(grad=False)),
    ("n = 0", dict(n=0)), ("n < 0", dict(n=-3)), ("three NULL cotangents", dict(cots=(False, False, False))), ("short workspace", dict(ws_bytes=15)),
])
def test_refusals_come_back_before_any_hip_call(case, kw):
    _lib.lib().tma_policy_param_count(None, None, None)  # leaves ANOTHER message behind: the one asserted below is this call's
    d = _dims(4, 64, 5, 0)
    assert _backward(d, **kw) == _lib.TMA_ERR_INVALID, case
    msg = _lib.last_error()
    assert "tma_policy_evaluate_actions_backward" in msg, (case, msg)
    with pytest.raises(ValueError):
        _lib.check(_backward(d, **kw))


@pytest.mark.parametrize("bad", [(0, 64, 5, 0, 0), (4, 96, 5, 0, 0), (4, 2048, 5, 0, 0), (4, 64, 17, 0, 0), (4, 64, 1, 0, 0), (4, 64, 33, 1, 0), (4, 64, 5, 0, 3),
                                 (6, 128, 5, 0, 2)])
def test_bad_dims_are_refused(bad):
    d = _dims(*bad)
    assert _backward(d) == _lib.TMA_ERR_INVALID and _lib.last_error()
    assert _lib.lib().tma_policy_vjp_workspace_bytes(C.byref(d), 77) == 0 and _lib.last_error()
    assert _lib.lib().tma_policy_evaluate_actions_backward(None, None, None, None, 1, None, None, None, None, None, 0, None) == _lib.TMA_ERR_INVALID


def test_bf16_dims_are_refused_with_a_reason():
    d = _dims(6, 256, 5, 0, 1)
    nt = C.c_int64(0)
    assert _lib.lib().tma_policy_param_count(C.byref(d), C.byref(nt), None) == _lib.TMA_OK  # the shape itself is a valid policy
    assert _backward(d) == _lib.TMA_ERR_INVALID and "bf16" in _lib.last_error()
    assert _lib.lib().tma_policy_vjp_workspace_bytes(C.byref(d), 77) == 0 and "bf16" in _lib.last_error()
    assert _lib.lib().tma_policy_vjp_workspace_bytes(C.byref(_dims(6, 256, 5, 0, 2)), 77) > 0  # bf16x3 runs the exact-f32 code


def test_chunk_override_is_validated_on_every_call(monkeypatch):
    d = _dims(4, 64, 5, 0)
    for bad in ("8", "24", "abc", "-16"):
        monkeypatch.setenv("TMA_VJP_CHUNK_ROWS", bad)
        assert _backward(d) == _lib.TMA_ERR_INVALID and "TMA_VJP_CHUNK_ROWS" in _lib.last_error()
    monkeypatch.setenv("TMA_VJP_CHUNK_ROWS", "32")
    assert _lib.lib().tma_policy_vjp_workspace_bytes(C.byref(d), 1 << 22) == _lib.lib().tma_policy_vjp_workspace_bytes(C.byref(d), 1 << 23)  # not the override's business
    assert _backward(d, cots=(False, False, False)) == _lib.TMA_ERR_INVALID and "TMA_VJP_CHUNK_ROWS" not in _lib.last_error()
