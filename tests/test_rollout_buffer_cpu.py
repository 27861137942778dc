"""tma_rollout_gather (include/tma.h, ABI 221) and the Python surface built on it (three-mlagents_amd/rollout_buffer.py), without a GPU: the
symbol is exported and bound, every documented refusal comes back as TMA_ERR_INVALID with its message before any HIP call, the sample tuple
carries SB3's field names, the package exports the buffer class, and the permutation key helper is the expression PPO.train used to spell out."""
import ctypes as C

import pytest

from three_mlagents_amd import _lib


def _dims(D=4, H=64, A=5, cont=0):
    return _lib.PolicyDims(D, H, A, cont, 0, -1)


def _gather(*, rb=True, d=True, mb=True, T=5, N=3, start=0, count=4, values=True, planes=(True,) * 5, outs=(True,) * 6, dims=None):
    """The call with host memory standing in for every buffer: each case below must be refused before anything is read or launched.
    planes: obs, actions, log_probs, advantages, returns of the view; outs: obs, actions, old_values, old_log_prob, advantages, returns."""
    buf = (C.c_float * 16)()
    p = lambda on: C.cast(buf, C.c_void_p) if on else None  # noqa: E731
    view = _lib.Rollout(*(p(on) for on in planes), T, N, None)
    batch = _lib.Minibatch(None, 1, 0, start, count, 0, 0)
    dd = dims if dims is not None else _dims()
    return _lib.lib().tma_rollout_gather(C.byref(view) if rb else None, p(values), C.byref(dd) if d else None, C.byref(batch) if mb else None,
                                         *(p(on) for on in outs), None)


def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert L.tma_version() >= 221
    assert "tma_rollout_gather" in _lib.SIGNATURES and hasattr(L, "tma_rollout_gather")
    res, args = _lib.SIGNATURES["tma_rollout_gather"]
    assert res is C.c_int and len(args) == 11 and args[0] == C.POINTER(_lib.Rollout) and args[2] == C.POINTER(_lib.PolicyDims) and args[3] == C.POINTER(_lib.Minibatch)


def _only(i, n):
    return tuple(k == i for k in range(n))


@pytest.mark.parametrize("case,kw,word", [
    ("rb NULL", dict(rb=False), "null argument"),
    ("d NULL", dict(d=False), "null argument"),
    ("mb NULL", dict(mb=False), "null argument"),
    ("obs plane NULL, obs_out given", dict(planes=(False, True, True, True, True)), "source plane is null"),
    ("actions plane NULL, actions_out given", dict(planes=(True, False, True, True, True)), "source plane is null"),
    ("log_probs plane NULL, old_log_prob_out given", dict(planes=(True, True, False, True, True)), "source plane is null"),
    ("advantages plane NULL, advantages_out given", dict(planes=(True, True, True, False, True)), "source plane is null"),
    ("returns plane NULL, returns_out given", dict(planes=(True, True, True, True, False)), "source plane is null"),
    ("values NULL, old_values_out given", dict(values=False), "without a values plane"),
    ("count = 0", dict(count=0), "not inside"),
    ("count < 0", dict(count=-2), "not inside"),
    ("start < 0", dict(start=-1), "not inside"),
    ("start + count > T*N", dict(start=12, count=4), "not inside"),
    ("start past the end", dict(start=16, count=1), "not inside"),
    ("start + count overflows", dict(start=2, count=(1 << 63) - 1), "not inside"),
    ("T*N = 2^31", dict(T=1 << 15, N=1 << 16), "below 2^31"),
    ("T*N > 2^31", dict(T=3, N=1 << 31), "below 2^31"),
])
def test_refusals_come_back_before_any_hip_call(case, kw, word):
    _lib.lib().tma_policy_param_count(None, None, None)  # leaves ANOTHER message behind: the one asserted below is this call's
    assert _gather(**kw) == _lib.TMA_ERR_INVALID, case
    msg = _lib.last_error()
    assert "tma_rollout_gather" in msg and word in msg, (case, msg)
    with pytest.raises(ValueError):
        _lib.check(_gather(**kw))


def test_bad_dims_are_refused():
    for bad in (_dims(D=0), _dims(H=96), _dims(A=17), _dims(A=33, cont=1)):
        assert _gather(dims=bad) == _lib.TMA_ERR_INVALID


def test_a_null_plane_is_no_refusal_when_its_output_is_null_too():
    """... but then the call gets as far as the launch, which this machine cannot do: anything but TMA_ERR_INVALID."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("needs a machine without a device: with one the call would launch on host memory")
    assert _gather(planes=(False, True, True, True, True), outs=(False, True, True, True, True, True)) != _lib.TMA_ERR_INVALID
    assert _gather(values=False, outs=(True, True, False, True, True, True)) != _lib.TMA_ERR_INVALID


def test_samples_have_sb3s_field_names_and_the_package_exports_the_buffer():
    import three_mlagents_amd as pkg
    from three_mlagents_amd.rollout_buffer import RolloutBuffer, RolloutBufferSamples

    assert RolloutBufferSamples._fields == ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns")
    assert pkg.RolloutBuffer is RolloutBuffer and pkg.RolloutBufferSamples is RolloutBufferSamples
    assert "RolloutBuffer" in pkg.__all__ and "RolloutBufferSamples" in pkg.__all__
    for name in ("get", "observations", "actions", "rewards", "values", "log_probs", "advantages", "returns", "terminated", "truncated", "buffer_size", "n_envs"):
        assert hasattr(RolloutBuffer, name), name


def test_perm_seed_helper_is_trains_former_expression():
    from three_mlagents_amd import ppo
    from three_mlagents_amd.rollout_buffer import perm_seed

    for seed in (0, 1, 1 << 31):
        assert perm_seed(seed) == (seed * 2654435761 + 12345) & 0xFFFFFFFF
    assert ppo._perm_seed is perm_seed  # (train() and get() use the one helper)


def test_get_refuses_a_buffer_that_is_not_full_and_a_bad_batch_size():
    from three_mlagents_amd.rollout_buffer import RolloutBuffer

    class _Model:
        n_steps, n_envs = 4, 2

    rb = RolloutBuffer(_Model())
    assert rb.full is False and rb.buffer_size == 4 and rb.n_envs == 2
    with pytest.raises(ValueError, match="not full"):
        rb.get(4)
    rb.full = True
    for bad in (0, -1):
        with pytest.raises(ValueError, match="batch_size"):
            rb.get(bad)
