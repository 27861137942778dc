"""tma_policy_head / tma_policy_head_backward (include/tma.h, ABI 218) and the Python surface built on them, without a GPU: the symbols are
exported and bound, every documented refusal comes back as TMA_ERR_INVALID with a message before any HIP call, the policy class and the two
distribution classes carry SB3's member names, and the distribution wrappers on plain CPU tensors give the log-probabilities and entropies of
the CPU restatement (oracle/sb3_ref.py evaluate_actions)."""
import ctypes as C

import pytest
import torch

from oracle import sb3_ref
from three_mlagents_amd import _lib

NAMES = ("tma_policy_head", "tma_policy_head_backward")
BAD_DIMS = [(0, 64, 5, 0, 0), (4, 96, 5, 0, 0), (4, 2048, 5, 0, 0), (4, 64, 17, 0, 0), (4, 64, 1, 0, 0), (4, 64, 33, 1, 0), (4, 64, 5, 0, 3), (6, 128, 5, 0, 2)]


def _dims(D, H, A, cont, dtype=0):
    return _lib.PolicyDims(D, H, A, cont, dtype, -1)


def _head(d, *, params=True, obs=True, head=True, values=True, n=16):
    """The call with host memory standing in for every buffer: each case below must be refused before anything is read or launched."""
    buf = (C.c_float * 16)()
    p = lambda on: buf if on else None  # noqa: E731
    return _lib.lib().tma_policy_head(p(params), C.byref(d) if d is not None else None, p(obs), n, p(head), p(values), None)


def _backward(d, *, params=True, obs=True, grad=True, n=16, cots=(True, False), ws_bytes=None):
    L = _lib.lib()
    buf = (C.c_float * 16)()
    need = L.tma_policy_vjp_workspace_bytes(C.byref(d), max(n, 1))
    p = lambda on: buf if on else None  # noqa: E731
    return L.tma_policy_head_backward(p(params), C.byref(d) if d is not None else None, p(obs), n, p(cots[0]), p(cots[1]), p(grad), buf,
                                      need if ws_bytes is None else ws_bytes, None)


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    assert L.tma_version() >= 218
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert len(_lib.SIGNATURES["tma_policy_head"][1]) == 7 and len(_lib.SIGNATURES["tma_policy_head_backward"][1]) == 10


@pytest.mark.parametrize("case,kw", [("null params", dict(params=False)), ("null obs", dict(obs=False)), ("null head_out", dict(head=False)),
                                     ("n = 0", dict(n=0)), ("n < 0", dict(n=-3))])
def test_head_refusals_come_back_before_any_hip_call(case, kw):
    _lib.lib().tma_policy_param_count(None, None, None)  # leaves ANOTHER message behind: the one asserted below is this call's
    for d in (_dims(4, 64, 5, 0), _dims(6, 256, 5, 0, 1), _dims(6, 256, 5, 0, 2), _dims(105, 256, 8, 1)):  # every mfma_dtype is a valid head
        assert _head(d, **kw) == _lib.TMA_ERR_INVALID, case
        msg = _lib.last_error()
        assert "tma_policy_head" in msg and "backward" not in msg, (case, msg)
        with pytest.raises(ValueError):
            _lib.check(_head(d, **kw))


@pytest.mark.parametrize("case,kw", [
    ("null params", dict(params=False)), ("null obs", dict(obs=False)), ("null grad_out", dict(grad=False)), ("n = 0", dict(n=0)), ("n < 0", dict(n=-3)),
    ("two NULL cotangents", dict(cots=(False, False))), ("short workspace", dict(ws_bytes=15)),
])
def test_backward_refusals_come_back_before_any_hip_call(case, kw):
    _lib.lib().tma_policy_param_count(None, None, None)
    for d in (_dims(4, 64, 5, 0), _dims(6, 64, 4, 1)):
        assert _backward(d, **kw) == _lib.TMA_ERR_INVALID, case
        msg = _lib.last_error()
        assert "tma_policy_head_backward" in msg, (case, msg)
        with pytest.raises(ValueError):
            _lib.check(_backward(d, **kw))


@pytest.mark.parametrize("bad", BAD_DIMS)
def test_bad_dims_are_refused(bad):
    d = _dims(*bad)
    assert _head(d) == _lib.TMA_ERR_INVALID and _lib.last_error()
    assert _backward(d) == _lib.TMA_ERR_INVALID and _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(_head(d))
    with pytest.raises(ValueError):
        _lib.check(_backward(d))
    L = _lib.lib()
    assert L.tma_policy_head(None, None, None, 1, None, None, None) == _lib.TMA_ERR_INVALID and _lib.last_error()
    assert L.tma_policy_head_backward(None, None, None, 1, None, None, None, None, 0, None) == _lib.TMA_ERR_INVALID and _lib.last_error()


def test_backward_refuses_bf16_with_a_reason_and_takes_bf16x3():
    assert _backward(_dims(6, 256, 5, 0, 1)) == _lib.TMA_ERR_INVALID and "bf16" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(_backward(_dims(6, 256, 5, 0, 1)))
    # bf16x3 runs the exact-f32 code: its dims pass the checks, and the next refusal in line is reported instead
    assert _backward(_dims(6, 256, 5, 0, 2), cots=(False, False)) == _lib.TMA_ERR_INVALID and "both null" in _lib.last_error()


def test_chunk_override_is_validated_on_every_call(monkeypatch):
    d = _dims(4, 64, 5, 0)
    for bad in ("8", "24", "abc", "-16"):
        monkeypatch.setenv("TMA_VJP_CHUNK_ROWS", bad)
        assert _backward(d) == _lib.TMA_ERR_INVALID and "TMA_VJP_CHUNK_ROWS" in _lib.last_error()


def test_python_surface_has_sb3s_names():
    from three_mlagents_amd import distributions
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    for name in ("head", "head_backward", "get_distribution"):
        assert callable(getattr(HipActorCriticPolicy, name))
    for cls in (distributions.CategoricalDistribution, distributions.DiagGaussianDistribution):
        for name in ("log_prob", "entropy", "mode", "sample", "get_actions"):
            assert callable(getattr(cls, name)), (cls, name)
    assert isinstance(distributions.CategoricalDistribution(torch.zeros(2, 3)).distribution, torch.distributions.Categorical)
    assert isinstance(distributions.DiagGaussianDistribution(torch.zeros(2, 3), torch.zeros(3)).distribution, torch.distributions.Normal)


def _sd(D, H, A, cont, seed, dtype):
    sd = sb3_ref.init_policy(D, H, A, cont, seed)
    g = torch.Generator().manual_seed(seed)
    sd["action_net.weight"] = sd["action_net.weight"] * 40 + 0.05 * torch.randn(sd["action_net.weight"].shape, generator=g)
    sd["action_net.bias"] = 0.1 * torch.randn(A, generator=g)
    if cont:
        sd["log_std"] = torch.linspace(-0.7, 0.3, A)
    return {k: v.to(dtype) for k, v in sd.items()}


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-14)])
def test_categorical_wrapper_agrees_with_the_cpu_restatement(dtype, tol):
    """the same torch operations on the same logits: a few ulps of the format at the most"""
    from three_mlagents_amd.distributions import CategoricalDistribution

    D, H, A, n = 4, 64, 5, 77
    sd = _sd(D, H, A, False, 3, dtype)
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(n, D, generator=g).to(dtype)
    a32 = torch.randint(0, A, (n,), generator=g, dtype=torch.int32)
    logits, _ = sb3_ref.forward(sd, obs)
    _, lp_ref, ent_ref = sb3_ref.evaluate_actions(sd, obs, a32)
    dist = CategoricalDistribution(logits)
    for actions in (a32, a32.long()):  # the rollout buffer's dtype and SB3's
        lp = dist.log_prob(actions)
        assert lp.shape == (n,) and torch.allclose(lp, lp_ref, rtol=tol, atol=tol)
    assert torch.allclose(dist.entropy(), ent_ref, rtol=tol, atol=tol)
    assert torch.equal(dist.mode(), logits.argmax(dim=1)) and torch.equal(dist.get_actions(deterministic=True), dist.mode())
    s = dist.get_actions()
    assert s.shape == (n,) and int(s.min()) >= 0 and int(s.max()) < A
    kl = torch.distributions.kl_divergence(dist.distribution, CategoricalDistribution(logits + 3.0).distribution)  # a shift of the logits is the same distribution
    assert float(kl.abs().max()) <= 100 * tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-14)])
def test_gaussian_wrapper_agrees_with_the_cpu_restatement(dtype, tol):
    from three_mlagents_amd.distributions import DiagGaussianDistribution

    D, H, A, n = 6, 64, 4, 77
    sd = _sd(D, H, A, True, 3, dtype)
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(n, D, generator=g).to(dtype)
    mean, _ = sb3_ref.forward(sd, obs)
    actions = mean + sd["log_std"].exp() * torch.randn(n, A, generator=g).clamp(-3.0, 3.0).to(dtype)
    _, lp_ref, ent_ref = sb3_ref.evaluate_actions(sd, obs, actions)
    dist = DiagGaussianDistribution(mean, sd["log_std"])
    lp, ent = dist.log_prob(actions), dist.entropy()
    assert lp.shape == ent.shape == (n,)
    assert torch.allclose(lp, lp_ref, rtol=tol, atol=10 * tol) and torch.allclose(ent, ent_ref, rtol=tol, atol=tol)
    assert torch.equal(dist.mode(), mean) and torch.equal(dist.get_actions(deterministic=True), mean)
    assert dist.sample().shape == (n, A)
    assert torch.equal(dist.distribution.stddev[0], sd["log_std"].exp())
    # log_std is part of the graph the wrapper builds: its gradient flows through torch
    ls = sd["log_std"].clone().requires_grad_(True)
    DiagGaussianDistribution(mean, ls).log_prob(actions).sum().backward()
    assert ls.grad is not None and float(ls.grad.abs().max()) > 0
