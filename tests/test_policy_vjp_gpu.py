"""tma_policy_evaluate_actions_backward on the GPU and the torch autograd binding of HipActorCriticPolicy.evaluate_actions built on it.

  * the VJP against float64 torch autograd of the CPU restatement (oracle/sb3_ref.py evaluate_actions) for every head and width family, at
    batch sizes around the 16-row tile, across chunk boundaries, with NULL cotangents;
  * determinism: equal inputs give equal bits;
  * tied to the trained kernels: with the cotangents of PPO's loss it reproduces tma_ppo_minibatch_grad;
  * the binding: opt-in through parameters(), same forward bits, leaf.grad = the library call, derived weight copies rebuilt after a torch
    optimizer stepped the leaf, and a behaviour-cloning loop that lands where the CPU reference lands.

Bound of every comparison with a reference gradient: max|err| <= 2e-5 max(max|ref|, 1) + 1e-6, the bound tests/test_ppo_gpu.py
test_minibatch_gradient_matches_autograd holds the PPO gradient to (float32 torch autograd itself stays within 7e-7 of the float64 scale on
these shapes).
"""
import ctypes as C

import pytest
import torch

from oracle import sb3_ref
from test_evaluate_actions_gpu import H64_MORE

pytestmark = pytest.mark.gpu

V_TOL = dict(rtol=1e-5, atol=1e-5)   # tests/test_evaluate_actions_gpu.py
LP_TOL = dict(rtol=1e-5, atol=5e-5)

# (D, H, A, Box?): H = 64 image family, generic, column-parallel 128 / 256, generic 320, two-pass Box shapes, and the head edges
SHAPES = [(4, 64, 5, False), (21, 64, 3, False), (6, 64, 4, True), (4, 128, 5, False), (6, 256, 5, False), (105, 256, 8, True), (4, 320, 3, False),
          (172, 256, 20, True), (4, 64, 2, False), (4, 64, 16, False), (6, 64, 32, True)]
SHAPES += H64_MORE  # (and every shorter list below that holds (4, 64, 5): the image path at 6, 7 and 16 observations)
NS = [1, 15, 16, 17, 77]


def _dev():
    return torch.device("cuda", 0)


def _policy(D, H, A, cont, seed=5, mfma="f32"):
    """tests/test_evaluate_actions_gpu.py _policy: heads made non-trivial (gain 0.01 init gives almost uniform logits), non-zero biases and log_std."""
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


def _batch(sd, D, A, cont, n, seed=0):
    """observations, actions (uniform Discrete; mean + sigma z, |z| <= 3 for Box) and three randn cotangents, on the CPU"""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(n, D, generator=g)
    if cont:
        mean, _ = sb3_ref.forward(sd, obs)
        actions = (mean + sd["log_std"].exp() * torch.randn(n, A, generator=g).clamp(-3.0, 3.0)).to(torch.float32)
    else:
        actions = torch.randint(0, A, (n,), generator=g, dtype=torch.int32)
    return obs, actions, [torch.randn(n, generator=g) for _ in range(3)]


def _flat(pol, named, dtype=torch.float64):
    """SB3-named tensors ([out][in]) -> the engine's flat [in][out] layout, at `dtype`"""
    flat = torch.zeros(pol.n_trainable, dtype=dtype)
    for key, off, shape in pol._segments():
        gk = named[key].reshape(shape)
        gk = gk.t().contiguous() if len(shape) == 2 else gk
        flat[off:off + gk.numel()] = gk.reshape(-1)
    if pol.continuous:
        flat[pol.offsets[12]:pol.offsets[12] + pol.act_dim] = named["log_std"]
    return flat


def _ref(pol, sd, obs, actions, cots):
    """float64 autograd of sum g_v V + g_lp logp + g_ent H through oracle/sb3_ref.py"""
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    v, lp, ent = sb3_ref.evaluate_actions(sd64, obs.double(), actions.double() if pol.continuous else actions)
    loss = 0.0
    for c, out in zip(cots, (v, lp, ent)):
        if c is not None:
            loss = loss + (c.double() * out).sum()
    loss.backward()
    return _flat(pol, {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in sd64.items()})


def _vjp(pol, obs, actions, cots, grad=None):
    """the library call itself (cots: three CPU / device tensors or None)"""
    from three_mlagents_amd import _lib

    L, dev, n = _lib.lib(), _dev(), obs.shape[0]
    obs, actions = obs.to(dev).contiguous(), actions.to(dev).contiguous()
    cots = [None if c is None else c.to(dev, torch.float32).contiguous() for c in cots]
    need = L.tma_policy_vjp_workspace_bytes(C.byref(pol.dims), n)
    assert 0 < need <= 256 << 20
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    grad = torch.full((pol.n_trainable,), float("nan"), device=dev) if grad is None else grad  # OVERWRITTEN: no element may stay NaN
    _lib.check(L.tma_policy_evaluate_actions_backward(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), _lib.ptr(actions), n, _lib.ptr(cots[0]),
                                                      _lib.ptr(cots[1]), _lib.ptr(cots[2]), _lib.ptr(grad), _lib.ptr(ws), need, _lib.stream_ptr()))
    return grad


def _within(grad, ref, what=""):
    err, scale = (grad.detach().cpu().double() - ref.double()).abs().max().item(), ref.abs().max().item()
    print(f"{what} err {err:.3e} scale {scale:.3e}")
    assert err <= 2e-5 * max(scale, 1.0) + 1e-6, (what, err, scale)


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1
@pytest.mark.parametrize("D,H,A,cont", SHAPES)
def test_vjp_matches_float64_autograd(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    for n in NS:
        obs, actions, cots = _batch(sd, D, A, cont, n, seed=n)
        _within(_vjp(pol, obs, actions, cots), _ref(pol, sd, obs, actions, cots), f"{(D, H, A, cont)} n={n}")


def test_vjp_of_a_bf16x3_policy_runs_the_exact_f32_code():
    pol, sd = _policy(6, 256, 5, False, mfma="bf16x3")
    pol0, _ = _policy(6, 256, 5, False)
    for n in NS:
        obs, actions, cots = _batch(sd, 6, 5, False, n, seed=n)
        grad = _vjp(pol, obs, actions, cots)
        _within(grad, _ref(pol, sd, obs, actions, cots), f"bf16x3 n={n}")
        assert _bits(grad, _vjp(pol0, obs, actions, cots))


# ---- 2
@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 256, 5, False), (6, 64, 4, True)] + H64_MORE)
def test_chunk_boundaries(D, H, A, cont, monkeypatch):
    """n = 69 at 32-row chunks: two full chunks and a ragged one, added to the gradient chunk after chunk"""
    pol, sd = _policy(D, H, A, cont)
    obs, actions, cots = _batch(sd, D, A, cont, 69)
    one_chunk = _vjp(pol, obs, actions, cots)
    monkeypatch.setenv("TMA_VJP_CHUNK_ROWS", "32")
    a, b = _vjp(pol, obs, actions, cots), _vjp(pol, obs, actions, cots)
    ref = _ref(pol, sd, obs, actions, cots)
    _within(a, ref, "chunks of 32")
    assert _bits(a, b)
    assert not _bits(a, one_chunk)  # (the override took effect: another summation order)
    _within(one_chunk, ref, "one chunk")


# ---- 3
@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 64, 4, True), (6, 256, 5, False)] + H64_MORE)
def test_null_cotangents_are_zeros(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    n = 77
    obs, actions, cots = _batch(sd, D, A, cont, n)
    zero = torch.zeros(n)
    total = torch.zeros(pol.n_trainable, dtype=torch.float64)
    for i in range(3):
        alone = [c if j == i else None for j, c in enumerate(cots)]
        explicit = [c if j == i else zero for j, c in enumerate(cots)]
        g_null = _vjp(pol, obs, actions, alone)
        assert _bits(g_null, _vjp(pol, obs, actions, explicit)), i
        _within(g_null, _ref(pol, sd, obs, actions, alone), f"cotangent {i} alone")
        total += g_null.cpu().double()
    joint = _vjp(pol, obs, actions, cots)
    _within(total, joint.cpu().double(), "sum of the three against the joint call")


# ---- 4
@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 256, 5, False)] + H64_MORE)
def test_reproducible(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    obs, actions, cots = _batch(sd, D, A, cont, 1000)
    first = _vjp(pol, obs, actions, cots)
    assert bool(torch.isfinite(first).all())
    for _ in range(4):
        assert _bits(first, _vjp(pol, obs, actions, cots))


# ---- 5
def _rollout(pol, sd, D, A, cont, T, N, seed=0):
    """tests/test_ppo_gpu.py _rollout: old log-probs spread around the current ones, every sample clear of the clip boundary"""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(T, N, D, generator=g)
    flat = obs.reshape(T * N, D)
    if cont:
        actions = torch.randn(T, N, A, generator=g) * 0.7
        act_flat = actions.reshape(T * N, A)
    else:
        actions = torch.randint(0, A, (T, N), generator=g, dtype=torch.int32)
        act_flat = actions.reshape(T * N)
    with torch.no_grad():
        _, lp, _ = sb3_ref.evaluate_actions(sd, flat, act_flat)
    old_lp = lp + 0.25 * torch.randn(T * N, generator=g)
    for _ in range(3):
        ratio = torch.exp(lp.double() - old_lp.double())
        near = ((ratio - 1.0).abs() - 0.2).abs() < 5e-3
        old_lp = torch.where(near, old_lp + 0.03, old_lp)
    return obs, actions, old_lp.reshape(T, N), torch.randn(T, N, generator=g), torch.randn(T, N, generator=g)


@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 64, 4, True)] + H64_MORE)
def test_ppo_cotangents_reproduce_the_trained_gradient_kernel(D, H, A, cont):
    from three_mlagents_amd import _lib

    T, N, B, dev = 16, 24, 77, _dev()
    clip, ent_coef, vf_coef = 0.2, 0.01, 0.5
    pol, sd = _policy(D, H, A, cont)
    obs, actions, old_lp, adv, ret = _rollout(pol, sd, D, A, cont, T, N)
    idx = torch.randperm(T * N, generator=torch.Generator().manual_seed(2))[37:37 + B]
    d = {k: v.to(dev).contiguous() for k, v in dict(obs=obs, actions=actions, old_lp=old_lp, adv=adv, ret=ret).items()}
    rv = _lib.Rollout(_lib.ptr(d["obs"]), _lib.ptr(d["actions"]), _lib.ptr(d["old_lp"]), _lib.ptr(d["adv"]), _lib.ptr(d["ret"]), T, N)
    idx_dev = idx.to(dev)
    mb = _lib.Minibatch(_lib.ptr(idx_dev), 0, 0, 0, B)
    hpar = _lib.PPOHParams(clip, ent_coef, vf_coef, 0)  # normalize_advantage = False
    ppo_grad = torch.zeros(pol.n_trainable, device=dev)
    ws = torch.zeros(int(_lib.lib().tma_ppo_workspace_bytes(C.byref(pol.dims))), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().tma_ppo_minibatch_grad(_lib.ptr(pol.params), C.byref(pol.dims), C.byref(rv), C.byref(mb), C.byref(hpar), _lib.ptr(ppo_grad),
                                                 _lib.ptr(ws), _lib.stream_ptr()))
    f = lambda x: x.transpose(0, 1).reshape(T * N, *x.shape[2:])[idx]  # noqa: E731  (RolloutBuffer.swap_and_flatten, then the minibatch rows)
    o, a, olp, ad, rt = f(obs), f(actions), f(old_lp), f(adv), f(ret)
    V, lp, _ = (t.cpu() for t in pol.evaluate_actions(o.to(dev), a.to(dev)))
    ratio = torch.exp(lp - olp)
    unclipped = ad * ratio <= ad * ratio.clamp(1 - clip, 1 + clip)  # the surrogate's min() takes the unclipped term
    assert 0.05 < 1.0 - unclipped.float().mean().item() < 0.95  # both branches
    g_lp = torch.where(unclipped, -ad * ratio / B, torch.zeros(B))
    g_ent = torch.full((B,), -ent_coef / B)
    g_v = 2.0 * vf_coef * (V - rt) / B
    _within(_vjp(pol, o, a, [g_v, g_lp, g_ent]), ppo_grad.cpu().double(), "against tma_ppo_minibatch_grad")


# ---- 6
def test_out_of_range_action_never_matters_where_its_cotangent_is_zero():
    D, H, A = 4, 64, 5
    pol, sd = _policy(D, H, A, False)
    obs, actions, cots = _batch(sd, D, A, False, 77)
    row = 33
    cots[1][row] = 0.0
    wild, tame = actions.clone(), actions.clone()
    wild[row], tame[row] = A + 3, 0
    g_wild, g_tame = _vjp(pol, obs, wild, cots), _vjp(pol, obs, tame, cots)
    assert bool(torch.isfinite(g_wild).all()) and _bits(g_wild, g_tame)
    _within(g_tame, _ref(pol, sd, obs, tame, cots), "row with a zero log-prob cotangent")


# ---- 7
@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 64, 4, True), (6, 256, 5, False)] + H64_MORE)
def test_autograd_binding(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    n = 77
    obs, actions, cots = _batch(sd, D, A, cont, n)
    obs_d, act_d = obs.to(_dev()), actions.to(_dev())
    before = pol.evaluate_actions(obs_d, act_d)
    assert pol._leaf is None and not any(t.requires_grad for t in before)  # parameters() never called: forward-only, as ever
    (leaf,) = pol.parameters()
    assert pol.parameters()[0] is leaf and leaf.is_leaf and leaf.requires_grad and leaf.data_ptr() == pol.params.data_ptr() and leaf.numel() == pol.n_trainable
    out = pol.evaluate_actions(obs_d, act_d)
    assert all(t.requires_grad for t in out) and all(_bits(x.detach(), y) for x, y in zip(out, before))
    g_v, g_lp, g_ent = (c.to(_dev()) for c in cots)
    loss = (g_v * out[0]).sum() + (g_lp * out[1]).sum() + (g_ent * out[2]).sum()
    loss.backward()
    assert _bits(leaf.grad, _vjp(pol, obs, actions, cots))
    # an output the loss does not use reaches the library as NULL; a broadcast (non-contiguous) cotangent is handled
    leaf.grad = None
    out = pol.evaluate_actions(obs_d, act_d)
    seen = []
    out[1].register_hook(seen.append)
    (-out[1].mean()).backward()
    assert not seen[0].is_contiguous() or seen[0].stride() == (1,)
    assert _bits(leaf.grad, _vjp(pol, obs, actions, [None, seen[0], None]))
    with torch.no_grad():
        assert not any(t.requires_grad for t in pol.evaluate_actions(obs_d, act_d))
    with pytest.raises(ValueError):
        pol.evaluate_actions(obs_d.clone().requires_grad_(True), act_d)
    leaf.requires_grad_(False)
    assert not any(t.requires_grad for t in pol.evaluate_actions(obs_d, act_d))


def test_parameters_of_a_bf16_policy_are_refused():
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    pol = HipActorCriticPolicy(6, 5, False, 256, _dev(), seed=1, mfma_dtype="bf16")
    with pytest.raises(ValueError):
        pol.parameters()
    v, lp, ent = pol.evaluate_actions(torch.randn(8, 6).to(_dev()), torch.zeros(8, dtype=torch.int32, device=_dev()))
    assert not v.requires_grad and bool(torch.isfinite(lp).all())


# ---- 8
@pytest.mark.parametrize("D,H,A", [(4, 64, 5), (6, 256, 5)] + [c[:3] for c in H64_MORE])
def test_derived_copies_follow_a_torch_optimizer_step(D, H, A):
    pol, sd = _policy(D, H, A, False)
    obs, actions, _ = _batch(sd, D, A, False, 77)
    obs_d, act_d = obs.to(_dev()), actions.to(_dev())
    opt = torch.optim.SGD(pol.parameters(), lr=0.1)
    v, lp, ent = pol.evaluate_actions(obs_d, act_d)
    (v.mean() - lp.mean() + ent.mean()).backward()
    opt.step()
    stepped = pol.state_dict()
    logits_ref, values_ref = sb3_ref.forward(stepped, obs)
    assert (values_ref - sb3_ref.forward(sd, obs)[1]).abs().max().item() > 1e-2  # the step moved the outputs far beyond the tolerances below
    a, values, logp = pol.act(obs_d, deterministic=True)
    assert torch.allclose(values.cpu(), values_ref, **V_TOL), (values.cpu() - values_ref).abs().max().item()
    assert torch.equal(a.cpu().long(), logits_ref.argmax(dim=1))
    assert torch.allclose(logp.cpu(), torch.log_softmax(logits_ref, dim=1).gather(1, a.cpu().long()[:, None])[:, 0], **LP_TOL)
    # ... and once more, with predict_values as the first call after the step
    opt.zero_grad()
    (pol.evaluate_actions(obs_d, act_d)[0].mean()).backward()
    opt.step()
    assert torch.allclose(pol.predict_values(obs_d).cpu(), sb3_ref.forward(pol.state_dict(), obs)[1], **V_TOL)


# ---- 9
def _bc_reference(sd0, obs, labels, dtype, steps):
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd0.items()}
    opt = torch.optim.Adam(list(sd.values()), lr=1e-3)
    nll = lambda: -sb3_ref.evaluate_actions(sd, obs.to(dtype), labels)[1].mean()  # noqa: E731
    first = nll().item()
    for _ in range(steps):
        opt.zero_grad()
        nll().backward()
        opt.step()
    with torch.no_grad():
        return first, nll().item()


def test_behaviour_cloning_lands_where_the_cpu_reference_lands():
    """50 Adam(lr = 1e-3) steps on the negative log-likelihood of a second policy's greedy actions, (4, 64, 5), 256 fixed observations.  The
    yardstick is the CPU restatement's own float32 - float64 gap of the final loss from the same start; the device (float32, other summation
    orders) must end within ten times that gap of the float64 run, and below where it started.
    Measured on an MI355X: initial loss 1.545612, final loss device 0.499041764, CPU float32 0.499041796, CPU float64 0.499041724 -- the
    float32 - float64 gap is 7.2e-8 (so the bound is 7.2e-7) and the device ends 4.0e-8 from the float64 run."""
    D, H, A, n, steps = 4, 64, 5, 256, 50
    pol, sd = _policy(D, H, A, False)
    teacher, _ = _policy(D, H, A, False, seed=11)
    obs = torch.randn(n, D, generator=torch.Generator().manual_seed(3))
    obs_d = obs.to(_dev())
    labels_d, _, _ = teacher.act(obs_d, deterministic=True)
    labels = labels_d.cpu()
    first32, last32 = _bc_reference(sd, obs, labels, torch.float32, steps)
    first64, last64 = _bc_reference(sd, obs, labels, torch.float64, steps)
    gap = abs(last32 - last64)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    nll = lambda: -pol.evaluate_actions(obs_d, labels_d)[1].mean()  # noqa: E731
    first = nll().item()
    for _ in range(steps):
        opt.zero_grad()
        nll().backward()
        opt.step()
    with torch.no_grad():
        last = -pol.evaluate_actions(obs_d, labels_d)[1].double().mean().item()
    print(f"BC: initial {first:.9f} (f64 {first64:.9f}); final device {last:.9f}, cpu f32 {last32:.9f}, cpu f64 {last64:.9f}; f32-f64 gap {gap:.3e}, "
          f"device-f64 {abs(last - last64):.3e}")
    assert last < first
    assert abs(last - last64) <= 10.0 * gap, (last, last64, gap)


# ---- a model keeps training after a foreign step
@pytest.mark.parametrize("algo,hidden", [("ppo", 64), ("ppo", 256), ("a2c", 64)])
def test_a_model_stepped_by_a_torch_optimizer_keeps_training(algo, hidden):
    """PPO / A2C do not use the autograd path, but their drivers read the derived weight copies: after a torch optimizer stepped
    model.policy.parameters() the next rollout must run on the stepped weights (audited as tests/test_evaluate_actions_gpu.py test_rollout_audit
    does: what the rollout kernels wrote against what the policy gives for those rows), and learn() goes on from there."""
    from three_mlagents_amd.a2c import A2C
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv

    T, N = 16, 64
    env = HipVecEnv("gridworld", N, seed=3)
    try:
        cls = PPO if algo == "ppo" else A2C
        kw = dict(batch_size=256, n_epochs=2) if algo == "ppo" else {}
        model = cls("MlpPolicy", env, n_steps=T, seed=7, policy_kwargs={"net_arch": [hidden, hidden]}, **kw)
        assert model.collect_rollouts()
        pol, buf = model.policy, model.buf
        obs, actions = buf["obs"][:T].flatten(0, 1).clone(), buf["actions"].flatten(0, 1).clone()
        values_before = buf["values"].flatten().clone()
        opt = torch.optim.SGD(pol.parameters(), lr=0.1)
        v, lp, ent = pol.evaluate_actions(obs, actions)
        (v.mean() - lp.mean()).backward()
        opt.step()
        assert model.collect_rollouts()  # on the stepped weights
        v, lp, _ = pol.evaluate_actions(buf["obs"][:T].flatten(0, 1), buf["actions"].flatten(0, 1))
        assert torch.allclose(v, buf["values"].flatten(), **V_TOL) and torch.allclose(lp, buf["log_probs"].flatten(), **LP_TOL)
        with torch.no_grad():
            assert (pol.predict_values(obs) - values_before).abs().max().item() > 1e-2  # (the step had moved the value net far beyond that tolerance)
        model.train()
        model.learn(2 * T * N)
        assert bool(torch.isfinite(pol.params).all())
    finally:
        env.close()
