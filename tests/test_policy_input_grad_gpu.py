"""tma_policy_evaluate_actions_vjp / tma_policy_head_vjp (include/tma.h, ABI 222; phase (c) of csrc/tma_vjp.hip) on the GPU: the gradient with
respect to the OBSERVATIONS, and the torch autograd binding of HipActorCriticPolicy.evaluate_actions / head / get_distribution built on it
(opt-in: policy.enable_obs_grad(); without it an `obs` that requires grad is what tests/test_policy_vjp_gpu.py and tests/test_policy_head_gpu.py
hold it to -- a ValueError where the call is differentiable with respect to the parameters, ignored where it is not).

Reference: float64 torch autograd of oracle/sb3_ref.py (tests/_relu_ref.py for ReLU) with obs.double().requires_grad_(True).
Bound of every comparison with it: max|err| <= 2e-5 max(max|ref|, 1) + 1e-6 -- the bound tests/test_policy_vjp_gpu.py and tests/test_ppo_gpu.py hold
gradients to.  Every case prints its error and the share of the bound it uses.

The _policy / _batch recipe is tests/test_policy_vjp_gpu.py's, restated.
"""
import ctypes as C

import pytest
import torch

import _policy_head_ref as head_ref
import _relu_ref
from oracle import sb3_ref

pytestmark = pytest.mark.gpu

# (D, H, A, Box?): D = 1, D not a multiple of 4 / 16, D beyond one column tile (21), beyond one pass of four (105, 172); H = 64 and wider
SHAPES = [(1, 64, 2, False), (4, 64, 5, False), (16, 64, 3, False), (17, 64, 3, False), (21, 64, 3, False), (6, 64, 4, True), (4, 128, 5, False),
          (6, 256, 5, False), (105, 256, 8, True), (4, 320, 3, False), (172, 256, 20, True)]
THREE = [(4, 64, 5, False), (6, 256, 5, False), (6, 64, 4, True)]  # H = 64, H = 256, one Box
NS = [1, 15, 16, 17, 77]


def _dev():
    return torch.device("cuda", 0)


def _policy(D, H, A, cont, seed=5, mfma="f32"):
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    pol = HipActorCriticPolicy(D, A, cont, H, _dev(), seed=seed, mfma_dtype=mfma)
    sd = pol.state_dict()
    if cont:
        sd["log_std"] = torch.linspace(-0.7, 0.3, A)
    g = torch.Generator().manual_seed(seed)
    sd["action_net.weight"] = sd["action_net.weight"] * 40 + 0.05 * torch.randn(sd["action_net.weight"].shape, generator=g)
    sd["action_net.bias"] = 0.1 * torch.randn(sd["action_net.bias"].shape, generator=g)
    for k in list(sd):
        if k.endswith("bias") and k != "action_net.bias":
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    pol.load_state_dict(sd)
    return pol, sd


def _actions(sd, obs, A, cont, g, forward=sb3_ref.forward):
    n = obs.shape[0]
    if cont:
        with torch.no_grad():
            mean, _ = forward(sd, obs)
        return (mean + sd["log_std"].exp() * torch.randn(n, A, generator=g).clamp(-3.0, 3.0)).to(torch.float32)
    return torch.randint(0, A, (n,), generator=g, dtype=torch.int32)


def _batch(sd, D, A, cont, n, seed=0):
    """observations, actions (uniform Discrete; mean + sigma z, |z| <= 3 for Box) and three randn cotangents, on the CPU"""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(n, D, generator=g)
    actions = _actions(sd, obs, A, cont, g)
    return obs, actions, [torch.randn(n, generator=g) for _ in range(3)]


def _ref(sd, obs, actions, cots, evaluate=sb3_ref.evaluate_actions):
    """float64 autograd of  sum g_v V + g_lp logp + g_ent H  with respect to the observations"""
    x = obs.double().requires_grad_(True)
    sd64 = {k: v.double() for k, v in sd.items()}
    outs = evaluate(sd64, x, actions.double() if "log_std" in sd else actions)
    loss = 0.0
    for c, out in zip(cots, outs):
        if c is not None:
            loss = loss + (c.double() * out).sum()
    if not loss.requires_grad:  # (a Gaussian's entropy does not depend on the observations at all)
        return torch.zeros_like(x)
    loss.backward()
    return x.grad


def _ref_head(sd, obs, g_head, g_values):
    x = obs.double().requires_grad_(True)
    head, values = sb3_ref.forward({k: v.double() for k, v in sd.items()}, x)
    loss = 0.0
    if g_head is not None:
        loss = loss + (g_head.double() * head).sum()
    if g_values is not None:
        loss = loss + (g_values.double() * values).sum()
    loss.backward()
    return x.grad


def _ws(pol, n):
    from three_mlagents_amd import _lib

    need = _lib.lib().tma_policy_vjp_workspace_bytes(C.byref(pol.dims), n)
    assert 0 < need <= 256 << 20
    return torch.empty(need, dtype=torch.uint8, device=_dev()), need


def _vjp(pol, obs, actions, cots, params=True, inputs=True, grad_obs=None):
    """tma_policy_evaluate_actions_vjp itself -> (grad_params or None, grad_obs or None); both outputs pre-filled with NaN (OVERWRITTEN)"""
    from three_mlagents_amd import _lib

    dev, n = _dev(), obs.shape[0]
    obs, actions = obs.to(dev).contiguous(), actions.to(dev).contiguous()
    cots = [None if c is None else c.to(dev, torch.float32).contiguous() for c in cots]
    ws, need = _ws(pol, n)
    gp = torch.full((pol.n_trainable,), float("nan"), device=dev) if params else None
    go = (torch.full((n, pol.obs_dim), float("nan"), device=dev) if grad_obs is None else grad_obs) if inputs else None
    _lib.check(_lib.lib().tma_policy_evaluate_actions_vjp(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), _lib.ptr(actions), n, _lib.ptr(cots[0]),
                                                          _lib.ptr(cots[1]), _lib.ptr(cots[2]), _lib.ptr(gp), _lib.ptr(go), _lib.ptr(ws), need,
                                                          _lib.stream_ptr()))
    return gp, go


def _old(pol, obs, actions, cots):
    from three_mlagents_amd import _lib

    dev, n = _dev(), obs.shape[0]
    obs, actions = obs.to(dev).contiguous(), actions.to(dev).contiguous()
    cots = [None if c is None else c.to(dev, torch.float32).contiguous() for c in cots]
    ws, need = _ws(pol, n)
    gp = torch.full((pol.n_trainable,), float("nan"), device=dev)
    _lib.check(_lib.lib().tma_policy_evaluate_actions_backward(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), _lib.ptr(actions), n,
                                                               _lib.ptr(cots[0]), _lib.ptr(cots[1]), _lib.ptr(cots[2]), _lib.ptr(gp), _lib.ptr(ws), need,
                                                               _lib.stream_ptr()))
    return gp


def _head_vjp(pol, obs, g_head, g_values, params=True, inputs=True, old=False):
    from three_mlagents_amd import _lib

    dev, n = _dev(), obs.shape[0]
    obs = obs.to(dev).contiguous()
    g_head, g_values = (None if c is None else c.to(dev, torch.float32).contiguous() for c in (g_head, g_values))
    ws, need = _ws(pol, n)
    gp = torch.full((pol.n_trainable,), float("nan"), device=dev) if params else None
    go = torch.full((n, pol.obs_dim), float("nan"), device=dev) if inputs else None
    L = _lib.lib()
    if old:
        _lib.check(L.tma_policy_head_backward(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), n, _lib.ptr(g_head), _lib.ptr(g_values), _lib.ptr(gp),
                                              _lib.ptr(ws), need, _lib.stream_ptr()))
        return gp, None
    _lib.check(L.tma_policy_head_vjp(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), n, _lib.ptr(g_head), _lib.ptr(g_values), _lib.ptr(gp),
                                     _lib.ptr(go), _lib.ptr(ws), need, _lib.stream_ptr()))
    return gp, go


def _within(grad, ref, what=""):
    err, scale = (grad.detach().cpu().double() - ref.double()).abs().max().item(), ref.abs().max().item()
    bound = 2e-5 * max(scale, 1.0) + 1e-6
    print(f"{what} err {err:.3e} scale {scale:.3e} share of the bound {err / bound:.3f}")
    assert err <= bound, (what, err, scale)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1
@pytest.mark.parametrize("D,H,A,cont", SHAPES)
def test_obs_gradient_matches_float64_autograd(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    for n in NS:
        obs, actions, cots = _batch(sd, D, A, cont, n, seed=n)
        _, go = _vjp(pol, obs, actions, cots)
        _within(go, _ref(sd, obs, actions, cots), f"{(D, H, A, cont)} n={n}")


@pytest.mark.parametrize("D,H,A,cont", [(21, 64, 3, False), (105, 256, 8, True)])
def test_head_obs_gradient_matches_float64_autograd(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    for n in NS:
        g = torch.Generator().manual_seed(100 + n)
        obs, g_head, g_values = torch.randn(n, D, generator=g), torch.randn(n, A, generator=g), torch.randn(n, generator=g)
        _, go = _head_vjp(pol, obs, g_head, g_values)
        _within(go, _ref_head(sd, obs, g_head, g_values), f"head {(D, H, A, cont)} n={n}")
    for alone in ((g_head, None), (None, g_values)):
        _within(_head_vjp(pol, obs, *alone, params=False)[1], _ref_head(sd, obs, *alone), f"head {(D, H, A, cont)} one cotangent")


# ---- 2
@pytest.mark.parametrize("D,H,A,cont", THREE)
def test_nothing_else_moved(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    obs, actions, cots = _batch(sd, D, A, cont, 77)
    gp_both, go_both = _vjp(pol, obs, actions, cots)
    gp_only, none = _vjp(pol, obs, actions, cots, inputs=False)
    none2, go_only = _vjp(pol, obs, actions, cots, params=False)
    assert none is None and none2 is None
    assert bool(torch.isfinite(gp_both).all()) and bool(torch.isfinite(go_both).all())
    assert _bits(gp_both, gp_only) and _bits(gp_only, _old(pol, obs, actions, cots))
    assert _bits(go_both, go_only)
    g = torch.Generator().manual_seed(9)
    g_head, g_values = torch.randn(77, A, generator=g), torch.randn(77, generator=g)
    hp_both, ho_both = _head_vjp(pol, obs, g_head, g_values)
    hp_only, _ = _head_vjp(pol, obs, g_head, g_values, inputs=False)
    _, ho_only = _head_vjp(pol, obs, g_head, g_values, params=False)
    hp_old, _ = _head_vjp(pol, obs, g_head, g_values, old=True)
    assert bool(torch.isfinite(hp_both).all()) and _bits(hp_both, hp_only) and _bits(hp_only, hp_old) and _bits(ho_both, ho_only)


# ---- 3
@pytest.mark.parametrize("D,H,A,cont", THREE)
def test_chunks_do_not_move_the_obs_gradient(D, H, A, cont, monkeypatch):
    """n = 69 at 32-row chunks (two full chunks and a ragged one): a row's gradient does not depend on the chunking; the parameter gradient's
    summation order does, which shows that the override took effect"""
    pol, sd = _policy(D, H, A, cont)
    obs, actions, cots = _batch(sd, D, A, cont, 69)
    gp1, go1 = _vjp(pol, obs, actions, cots)
    monkeypatch.setenv("TMA_VJP_CHUNK_ROWS", "32")
    gp3, go3 = _vjp(pol, obs, actions, cots)
    _, go3_only = _vjp(pol, obs, actions, cots, params=False)
    assert _bits(go1, go3) and _bits(go1, go3_only)
    assert not _bits(gp1, gp3)
    _within(go3, _ref(sd, obs, actions, cots), "chunks of 32")


@pytest.mark.parametrize("D,H,A,cont", THREE)
def test_a_row_does_not_depend_on_its_batch_and_runs_repeat(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    obs, actions, cots = _batch(sd, D, A, cont, 33)
    _, go = _vjp(pol, obs, actions, cots, params=False)
    assert _bits(go, _vjp(pol, obs, actions, cots, params=False)[1])
    for i in (0, 15, 16, 32):
        _, alone = _vjp(pol, obs[i:i + 1], actions[i:i + 1], [c[i:i + 1] for c in cots], params=False)
        assert _bits(alone[0], go[i]), i


# ---- 4
@pytest.mark.parametrize("D,H,A,cont", THREE)
def test_cotangents_alone_and_zero_rows(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    n = 77
    obs, actions, cots = _batch(sd, D, A, cont, n)
    for i in range(3):
        alone = [c if j == i else None for j, c in enumerate(cots)]
        _within(_vjp(pol, obs, actions, alone, params=False)[1], _ref(sd, obs, actions, alone), f"{(D, H, A, cont)} cotangent {i} alone")
    zero_rows = [0, 15, 16, 40, 76]
    for c in cots:
        c[zero_rows] = 0.0
    _, go = _vjp(pol, obs, actions, cots)
    nz = (go != 0).any(dim=1).cpu()
    assert not bool(nz[zero_rows].any()) and bool((go[zero_rows] == 0.0).all())
    assert bool(nz[[r for r in range(n) if r not in zero_rows]].all())
    _within(go, _ref(sd, obs, actions, cots), "with zero rows")


def test_out_of_range_action_never_matters_where_its_cotangent_is_zero():
    D, H, A = 4, 64, 5
    pol, sd = _policy(D, H, A, False)
    obs, actions, cots = _batch(sd, D, A, False, 77)
    row = 33
    cots[1][row] = 0.0
    wild, tame = actions.clone(), actions.clone()
    wild[row], tame[row] = A + 3, 0
    _, g_wild = _vjp(pol, obs, wild, cots)
    _, g_tame = _vjp(pol, obs, tame, cots)
    assert bool(torch.isfinite(g_wild).all()) and _bits(g_wild[row], g_tame[row]) and _bits(g_wild, g_tame)
    _within(g_tame, _ref(sd, obs, tame, cots), "row with a zero log-prob cotangent")


# ---- 5
def test_extent_and_alignment():
    D, H, A, n = 4, 64, 5, 17
    pol, sd = _policy(D, H, A, False)
    obs, actions, cots = _batch(sd, D, A, False, n)
    guarded = torch.full((n + 2, D), float("nan"), device=_dev())
    _vjp(pol, obs, actions, cots, params=False, grad_obs=guarded[1:n + 1])
    assert bool(torch.isnan(guarded[0]).all()) and bool(torch.isnan(guarded[n + 1]).all()) and not bool(torch.isnan(guarded[1:n + 1]).any())
    flat = torch.full((n * D + 2,), float("nan"), device=_dev())
    assert flat.data_ptr() % 16 == 0
    shifted = flat[1:1 + n * D].view(n, D)  # base offset by one float: not 16-byte aligned
    _vjp(pol, obs, actions, cots, params=False, grad_obs=shifted)
    assert _bits(shifted, guarded[1:n + 1]) and bool(torch.isnan(flat[0])) and bool(torch.isnan(flat[-1]))


# ---- 6
@pytest.mark.parametrize("D,H,A", [(4, 64, 5), (6, 256, 5)])
def test_relu(D, H, A):
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    sd = _relu_ref.policy_sd(D, H, A, False)
    pol = HipActorCriticPolicy(D, A, False, H, _dev(), seed=5, activation="relu")
    pol.load_state_dict(sd)
    for n in NS:
        obs = _relu_ref.clear_obs(sd, D, n, seed=n)
        assert _relu_ref.kink_margin(sd, obs) >= _relu_ref.KINK_MARGIN  # BEFORE any device result is looked at
        g = torch.Generator().manual_seed(1000 + n)
        actions = torch.randint(0, A, (n,), generator=g, dtype=torch.int32)
        cots = [torch.randn(n, generator=g) for _ in range(3)]
        _, go = _vjp(pol, obs, actions, cots, params=False)
        _within(go, _ref(sd, obs, actions, cots, evaluate=lambda s, x, a: _relu_ref.evaluate_actions(s, x, a, "relu")), f"relu {(D, H, A)} n={n}")


# ---- 7
def test_a_bf16x3_policy_runs_the_exact_f32_code():
    pol, sd = _policy(6, 256, 5, False, mfma="bf16x3")
    pol0, _ = _policy(6, 256, 5, False)
    for n in (17, 77):
        obs, actions, cots = _batch(sd, 6, 5, False, n, seed=n)
        _, go = _vjp(pol, obs, actions, cots)
        _within(go, _ref(sd, obs, actions, cots), f"bf16x3 n={n}")
        assert _bits(go, _vjp(pol0, obs, actions, cots)[1])


# ---- 8
@pytest.mark.parametrize("D,H,A,cont", THREE)
def test_autograd_binding(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    n = 77
    obs, actions, cots = _batch(sd, D, A, cont, n)
    obs_d, act_d = obs.to(_dev()), actions.to(_dev())
    g_v, g_lp, g_ent = (c.to(_dev()) for c in cots)
    plain = pol.evaluate_actions(obs_d, act_d)
    gp_lib, go_lib = _vjp(pol, obs, actions, cots)
    # off by default: a forward-only policy ignores obs.requires_grad, as it always has
    x = obs_d.clone().requires_grad_(True)
    assert all(t.grad_fn is None for t in pol.evaluate_actions(x, act_d)) and pol.head(x)[0].grad_fn is None
    assert pol.enable_obs_grad() is pol
    # a fresh policy: obs.grad is filled, no leaf is made
    out = pol.evaluate_actions(x, act_d)
    assert all(t.requires_grad for t in out) and all(_bits(a.detach(), b) for a, b in zip(out, plain))
    ((g_v * out[0]).sum() + (g_lp * out[1]).sum() + (g_ent * out[2]).sum()).backward()
    assert pol._leaf is None and _bits(x.grad, go_lib)
    with torch.no_grad():
        assert all(t.grad_fn is None and not t.requires_grad for t in pol.evaluate_actions(x, act_d))
    # head of the frozen policy
    x = obs_d.clone().requires_grad_(True)
    head, values = pol.head(x)
    g = torch.Generator().manual_seed(4)
    g_head = torch.randn(n, A, generator=g)
    ((g_head.to(_dev()) * head).sum() + (g_v * values).sum()).backward()
    assert pol._leaf is None and _bits(x.grad, _head_vjp(pol, obs, g_head, cots[0], params=False)[1])
    plain_head = pol.head(obs_d)
    assert _bits(head.detach(), plain_head[0]) and _bits(values.detach(), plain_head[1]) and plain_head[0].grad_fn is None
    # both gradients from one backward
    (leaf,) = pol.parameters()
    x = obs_d.clone().requires_grad_(True)
    out = pol.evaluate_actions(x, act_d)
    ((g_v * out[0]).sum() + (g_lp * out[1]).sum() + (g_ent * out[2]).sum()).backward()
    assert _bits(x.grad, go_lib) and _bits(leaf.grad, gp_lib)
    # an output the loss does not use reaches the library as NULL
    x = obs_d.clone().requires_grad_(True)
    (pol.evaluate_actions(x, act_d)[1] * g_lp).sum().backward()
    assert _bits(x.grad, _vjp(pol, obs, actions, [None, cots[1], None], params=False)[1])
    # float64 observations get a float64 gradient: the conversion is part of the graph
    x64 = obs_d.double().requires_grad_(True)
    out = pol.evaluate_actions(x64, act_d)
    ((g_v * out[0]).sum() + (g_lp * out[1]).sum() + (g_ent * out[2]).sum()).backward()
    assert x64.grad.dtype == torch.float64 and torch.equal(x64.grad, go_lib.double())
    # second order is torch's to refuse
    x = obs_d.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(pol.evaluate_actions(x, act_d)[0].sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    # the keyword surface of the explicit calls
    both = pol.evaluate_actions_backward(obs_d, act_d, g_v, g_lp, g_ent, params_grad=True, obs_grad=True)
    assert isinstance(both, tuple) and _bits(both[0], gp_lib) and _bits(both[1], go_lib)
    assert _bits(pol.evaluate_actions_backward(obs_d, act_d, g_v, g_lp, g_ent), gp_lib)
    assert _bits(pol.evaluate_actions_backward(obs_d, act_d, g_v, g_lp, g_ent, params_grad=False, obs_grad=True), go_lib)
    assert tuple(pol.head_backward(obs_d, g_head, None, params_grad=False, obs_grad=True).shape) == (n, D)
    with pytest.raises(ValueError):
        pol.evaluate_actions_backward(obs_d, act_d, g_v, params_grad=False, obs_grad=False)
    # switched off again: with a leaf that requires grad an obs that requires grad is the ValueError it was
    pol.enable_obs_grad(False)
    for call in (lambda: pol.evaluate_actions(x, act_d), lambda: pol.head(x), lambda: pol.get_distribution(x)):
        with pytest.raises(ValueError, match="enable_obs_grad"):
            call()
    assert all(t.requires_grad for t in pol.evaluate_actions(obs_d, act_d))


def test_a_bf16_policy_refuses_enable_obs_grad_as_it_refuses_parameters():
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    pol = HipActorCriticPolicy(6, 5, False, 256, _dev(), seed=1, mfma_dtype="bf16")
    with pytest.raises(ValueError, match="bf16"):
        pol.enable_obs_grad()
    x = torch.randn(8, 6).to(_dev()).requires_grad_(True)
    head, _ = pol.head(x)  # forward-only, as ever
    assert head.grad_fn is None and bool(torch.isfinite(head).all())


# ---- 9
def test_a_module_in_front_of_the_policy():
    D, H, A, n = 4, 64, 5, 64
    pol, sd = _policy(D, H, A, False)
    pol.enable_obs_grad()
    torch.manual_seed(3)
    enc = torch.nn.Linear(7, D).to(_dev())
    g = torch.Generator().manual_seed(6)
    x = torch.randn(n, 7, generator=g)
    actions = torch.randint(0, A, (n,), generator=g, dtype=torch.int32)
    cots = [torch.randn(n, generator=g) for _ in range(3)]
    x_d, act_d = x.to(_dev()), actions.to(_dev())
    out = pol.evaluate_actions(enc(x_d), act_d)
    sum(((c.to(_dev()) * o).sum() for c, o in zip(cots, out))).backward()
    assert pol._leaf is None
    w64, b64 = enc.weight.detach().cpu().double().requires_grad_(True), enc.bias.detach().cpu().double().requires_grad_(True)
    ref_out = sb3_ref.evaluate_actions({k: v.double() for k, v in sd.items()}, torch.nn.functional.linear(x.double(), w64, b64), actions)
    sum(((c.double() * o).sum() for c, o in zip(cots, ref_out))).backward()
    _within(enc.weight.grad, w64.grad, "encoder weight")
    _within(enc.bias.grad, b64.grad, "encoder bias")
    # five Adam steps on encoder + policy leaf decrease a behaviour-cloning loss on the fixed batch
    opt = torch.optim.Adam(list(enc.parameters()) + pol.parameters(), lr=1e-3)
    nll = lambda: -pol.evaluate_actions(enc(x_d), act_d)[1].mean()  # noqa: E731
    first = nll().item()
    w0, p0 = enc.weight.detach().clone(), pol.params[: pol.n_trainable].clone()
    for _ in range(5):
        opt.zero_grad()
        nll().backward()
        opt.step()
    with torch.no_grad():
        last = nll().item()
    print(f"BC through an encoder: {first:.6f} -> {last:.6f}")
    assert last < first
    assert not torch.equal(enc.weight.detach(), w0) and not torch.equal(pol.params[: pol.n_trainable], p0)  # both halves were stepped


# ---- 10
@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 64, 4, True)])
def test_kl_between_two_policies_fills_obs_grad(D, H, A, cont):
    student, s_sd = _policy(D, H, A, cont)
    teacher, t_sd = _policy(D, H, A, cont, seed=11)
    if cont:
        t_sd["log_std"] = t_sd["log_std"] + 0.2
        teacher.load_state_dict(t_sd)
    obs = torch.randn(77, D, generator=torch.Generator().manual_seed(0))
    x = obs.to(_dev()).requires_grad_(True)
    teacher.enable_obs_grad(), student.enable_obs_grad()
    kl = torch.distributions.kl_divergence(teacher.get_distribution(x).distribution, student.get_distribution(x).distribution)
    if cont:
        kl = kl.sum(dim=1)
    kl.sum().backward()
    assert teacher._leaf is None and student._leaf is None
    x64 = obs.double().requires_grad_(True)
    ref = torch.distributions.kl_divergence(head_ref.distribution(head_ref.double(t_sd), x64), head_ref.distribution(head_ref.double(s_sd), x64))
    ref.sum().backward()
    _within(x.grad, x64.grad, f"dKL/dobs {(D, H, A, cont)}")
