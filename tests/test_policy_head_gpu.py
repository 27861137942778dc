"""tma_policy_head / tma_policy_head_backward on the GPU and HipActorCriticPolicy.head / get_distribution built on them.

  1 the head (logits / mean) and the values against float64 (oracle/sb3_ref.py forward) for every head and width family, at batch sizes around
    the 16-row tile, with NaN guard rows behind the batch; the bf16 kernels' own head against the emulation of tests/test_bf16_gpu.py;
  2 the bits of the kernels it shares: values = act's = evaluate_actions', a Box head = act(deterministic)'s actions, a Discrete head's argmax =
    the deterministic action, the dispatch id = act's, for every forward family and above its grid cap; values_out = NULL;
  3 get_distribution's log_prob / entropy against the evaluate_actions kernel;
  4 the backward against float64 autograd: every shape and n, NULL cotangents, chunk boundaries, equal bits from equal inputs;
  5 tied to tma_policy_evaluate_actions_backward through the head cotangent its three cotangents imply;
  6 the autograd binding: KL between two policies, log_std through torch, a torch optimizer step, a bf16 policy forward-only;
  7 distillation of a 256-wide teacher into a 64-wide student lands where the CPU reference lands.

Bound of every comparison with a reference gradient: tests/test_policy_vjp_gpu.py's, max|err| <= 2e-5 max(max|ref|, 1) + 1e-6.
"""
import ctypes as C

import pytest
import torch

import _policy_head_ref as ref
from test_bf16_gpu import _emulated_forward
from test_evaluate_actions_gpu import CAPPED, FAMILIES, _dispatch_value, _last_fwd_dispatch
from test_policy_vjp_gpu import H64_MORE, LP_TOL, NS, SHAPES, V_TOL, _batch, _bits, _dev, _flat, _policy, _vjp, _within

pytestmark = pytest.mark.gpu

GUARD = 16


def _head(pol, obs, values=True):
    """the library call itself: (head [n, A], values [n] or None); 16 guard rows of NaN behind row n must stay NaN"""
    from three_mlagents_amd import _lib

    dev, n = _dev(), obs.shape[0]
    obs = obs.to(dev).contiguous()
    head = torch.full((n + GUARD, pol.act_dim), float("nan"), device=dev)
    vals = torch.full((n + GUARD,), float("nan"), device=dev) if values else None
    _lib.check(_lib.lib().tma_policy_head(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), n, _lib.ptr(head), _lib.ptr(vals), _lib.stream_ptr()))
    assert bool(torch.isnan(head[n:]).all()) and (vals is None or bool(torch.isnan(vals[n:]).all())), "a row behind n was stored"
    return head[:n], (None if vals is None else vals[:n])


def _head_vjp(pol, obs, g_head, g_values):
    """the library call itself (CPU / device cotangents or None); grad_out starts as NaN: it is OVERWRITTEN, no element may stay NaN"""
    from three_mlagents_amd import _lib

    L, dev, n = _lib.lib(), _dev(), obs.shape[0]
    obs = obs.to(dev).contiguous()
    g_head, g_values = (None if c is None else c.to(dev, torch.float32).contiguous() for c in (g_head, g_values))
    need = L.tma_policy_vjp_workspace_bytes(C.byref(pol.dims), n)
    assert 0 < need <= 256 << 20
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    grad = torch.full((pol.n_trainable,), float("nan"), device=dev)
    _lib.check(L.tma_policy_head_backward(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), n, _lib.ptr(g_head), _lib.ptr(g_values), _lib.ptr(grad),
                                          _lib.ptr(ws), need, _lib.stream_ptr()))
    assert not bool(torch.isnan(grad).any())
    if pol.continuous:
        o = pol.offsets[12]
        assert bool((grad[o:o + pol.act_dim] == 0).all()), "the head does not depend on log_std"
    return grad


def _cots(n, A, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(n, A, generator=g), torch.randn(n, generator=g)


def _obs(n, D, seed):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(seed))


# ---- 1
@pytest.mark.parametrize("D,H,A,cont", SHAPES)
def test_head_and_values_match_float64(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    for n in NS:
        obs = _obs(n, D, n)
        head, values = _head(pol, obs)
        head_ref, values_ref = ref.forward64(sd, obs)
        eh, ev = (head.cpu().double() - head_ref).abs().max().item(), (values.cpu().double() - values_ref).abs().max().item()
        print(f"{(D, H, A, cont)} n={n}: max |dhead| {eh:.3e} (scale {head_ref.abs().max().item():.3e})  max |dv| {ev:.3e}")
        assert head.shape == (n, A) and values.shape == (n,)
        assert torch.allclose(head.cpu().double(), head_ref, **V_TOL), eh
        assert torch.allclose(values.cpu().double(), values_ref, **V_TOL), ev


@pytest.mark.parametrize("D,H,A,cont", [(6, 256, 5, False), (105, 256, 8, True)])
def test_bf16_head_matches_the_bf16_emulation(D, H, A, cont):
    """tests/test_bf16_gpu.py test_bf16_forward: the same rounding points, f32 sums in another order -- 4e-3; against the f32 restatement 3e-2"""
    pol, sd = _policy(D, H, A, cont, mfma="bf16")
    for n in NS:
        obs = _obs(n, D, n)
        head, values = _head(pol, obs)
        head_emu, values_emu = _emulated_forward(sd, obs)
        head_ref, values_ref = ref.forward64(sd, obs)
        eh, ev = (head.cpu() - head_emu).abs().max().item(), (values.cpu() - values_emu).abs().max().item()
        print(f"bf16 {(D, H, A, cont)} n={n}: max |dhead| {eh:.3e}  max |dv| {ev:.3e} against the emulation")
        assert torch.allclose(head.cpu(), head_emu, rtol=4e-3, atol=4e-3), eh
        assert torch.allclose(values.cpu(), values_emu, rtol=4e-3, atol=4e-3), ev
        assert torch.allclose(head.cpu().double(), head_ref, rtol=3e-2, atol=3e-2) and torch.allclose(values.cpu().double(), values_ref, rtol=3e-2, atol=3e-2)


# ---- 2
def _check_same_bits(pol, cont, obs_d, expect_dispatch):
    a_det, v_act, _ = pol.act(obs_d, deterministic=True)
    d_act = _last_fwd_dispatch()
    head, values = _head(pol, obs_d)
    d_head = _last_fwd_dispatch()
    assert d_head == d_act, (d_head, d_act)  # the family `act` ran, under its existing id
    if "|" in expect_dispatch or not expect_dispatch.endswith("GENERIC"):
        assert d_head == _dispatch_value(expect_dispatch), (d_head, expect_dispatch)
    assert _bits(values, v_act)
    if cont:
        assert _bits(head, a_det)
        v_eval, _, _ = pol.evaluate_actions(obs_d, a_det)
    else:
        assert torch.equal(head.argmax(dim=1).to(torch.int32), a_det)
        v_eval, _, _ = pol.evaluate_actions(obs_d, a_det)
    assert _bits(values, v_eval)
    head_alone, none = _head(pol, obs_d, values=False)
    assert none is None and _bits(head_alone, head)
    h2, v2 = pol.head(obs_d)  # the method: the same call
    assert _bits(h2, head) and _bits(v2, values) and h2.shape == head.shape and not h2.requires_grad


@pytest.mark.parametrize("D,H,A,cont,mfma,family", FAMILIES, ids=[f"{f[0]}x{f[1]}x{f[2]}{'C' if f[3] else 'D'}-{f[4]}" for f in FAMILIES])
def test_same_bits_as_the_kernels_it_shares(D, H, A, cont, mfma, family):
    pol, _ = _policy(D, H, A, cont, mfma=mfma)
    for n in (1, 17, 101, 1000):
        _check_same_bits(pol, cont, _obs(n, D, n).to(_dev()), family)


@pytest.mark.parametrize("D,H,A,cont,mfma,n,dispatch", CAPPED, ids=[f"{c[0]}x{c[1]}x{c[2]}{'C' if c[3] else 'D'}-{c[4]}-{c[5]}" for c in CAPPED])
def test_same_bits_above_the_grid_caps(D, H, A, cont, mfma, n, dispatch):
    pol, _ = _policy(D, H, A, cont, mfma=mfma)
    _check_same_bits(pol, cont, _obs(n, D, 3).to(_dev()), dispatch)


# ---- 3
@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 64, 4, True), (6, 256, 5, False), (105, 256, 8, True)] + H64_MORE)
def test_distribution_is_consistent_with_evaluate_actions(D, H, A, cont):
    from three_mlagents_amd.distributions import CategoricalDistribution, DiagGaussianDistribution

    pol, sd = _policy(D, H, A, cont)
    obs, actions, _ = _batch(sd, D, A, cont, 77)
    obs_d, act_d = obs.to(_dev()), actions.to(_dev())
    _, lp, ent = pol.evaluate_actions(obs_d, act_d)
    dist = pol.get_distribution(obs_d)
    assert isinstance(dist, DiagGaussianDistribution if cont else CategoricalDistribution)
    dlp, dent = dist.log_prob(act_d), dist.entropy()
    print(f"{(D, H, A, cont)}: max |dlogp| {(dlp - lp).abs().max().item():.3e}  max |dent| {(dent - ent).abs().max().item():.3e}")
    assert dlp.shape == dent.shape == (77,) and dlp.is_cuda
    assert torch.allclose(dlp, lp, **LP_TOL) and torch.allclose(dent, ent, **LP_TOL)
    if not cont:
        assert torch.allclose(dist.log_prob(act_d.long()), lp, **LP_TOL)  # SB3's dtype
    det, _, _ = pol.act(obs_d, deterministic=True)
    assert torch.equal(dist.mode().to(det.dtype), det) and dist.sample().shape == det.shape


# ---- 4
@pytest.mark.parametrize("D,H,A,cont", SHAPES)
def test_backward_matches_float64_autograd(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    for n in NS:
        obs = _obs(n, D, n)
        g_head, g_values = _cots(n, A, n)
        _within(_head_vjp(pol, obs, g_head, g_values), _flat(pol, ref.head_grad(sd, obs, g_head, g_values)), f"{(D, H, A, cont)} n={n}")


def test_backward_of_a_bf16x3_policy_runs_the_exact_f32_code():
    pol, sd = _policy(6, 256, 5, False, mfma="bf16x3")
    pol0, _ = _policy(6, 256, 5, False)
    obs = _obs(77, 6, 0)
    g_head, g_values = _cots(77, 5, 0)
    grad = _head_vjp(pol, obs, g_head, g_values)
    _within(grad, _flat(pol, ref.head_grad(sd, obs, g_head, g_values)), "bf16x3")
    assert _bits(grad, _head_vjp(pol0, obs, g_head, g_values))


@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 64, 4, True), (6, 256, 5, False)] + H64_MORE)
def test_null_cotangents_are_zeros(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    n = 77
    obs = _obs(n, D, 0)
    g_head, g_values = _cots(n, A, 0)
    only_head, only_values = _head_vjp(pol, obs, g_head, None), _head_vjp(pol, obs, None, g_values)
    assert _bits(only_head, _head_vjp(pol, obs, g_head, torch.zeros(n)))
    assert _bits(only_values, _head_vjp(pol, obs, torch.zeros(n, A), g_values))
    _within(only_head, _flat(pol, ref.head_grad(sd, obs, g_head, None)), "g_head alone")
    _within(only_values, _flat(pol, ref.head_grad(sd, obs, None, g_values)), "g_values alone")
    v0 = pol.offsets[6]  # the two nets share nothing: each call leaves the other net's gradient exactly zero
    assert bool((only_head[v0:] == 0).all()) and bool((only_values[:v0] == 0).all())
    joint = _head_vjp(pol, obs, g_head, g_values)
    assert _bits(joint[:v0], only_head[:v0]) and _bits(joint[v0:], only_values[v0:])


@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 256, 5, False), (6, 64, 4, True)] + H64_MORE)
def test_chunk_boundaries(D, H, A, cont, monkeypatch):
    """n = 69 at 32-row chunks: two full chunks and a ragged one, added to the gradient chunk after chunk"""
    pol, sd = _policy(D, H, A, cont)
    obs = _obs(69, D, 0)
    g_head, g_values = _cots(69, A, 0)
    one_chunk = _head_vjp(pol, obs, g_head, g_values)
    monkeypatch.setenv("TMA_VJP_CHUNK_ROWS", "32")
    a, b = _head_vjp(pol, obs, g_head, g_values), _head_vjp(pol, obs, g_head, g_values)
    want = _flat(pol, ref.head_grad(sd, obs, g_head, g_values))
    _within(a, want, "chunks of 32")
    assert _bits(a, b)
    assert not _bits(a, one_chunk)  # (the override took effect: another summation order)
    _within(one_chunk, want, "one chunk")


@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 256, 5, False)] + H64_MORE)
def test_reproducible(D, H, A, cont):
    pol, _ = _policy(D, H, A, cont)
    obs = _obs(1000, D, 0)
    g_head, g_values = _cots(1000, A, 0)
    first = _head_vjp(pol, obs, g_head, g_values)
    assert bool(torch.isfinite(first).all()) and _bits(first, _head_vjp(pol, obs, g_head, g_values))


# ---- 5
@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 256, 5, False), (6, 64, 4, True), (105, 256, 8, True)] + H64_MORE)
def test_implied_head_cotangent_reproduces_the_evaluate_actions_vjp(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    obs, actions, (g_v, g_lp, g_ent) = _batch(sd, D, A, cont, 77)
    existing = _vjp(pol, obs, actions, [g_v, g_lp, g_ent])
    mine = _head_vjp(pol, obs, ref.implied_head_cotangent(sd, obs, actions, g_lp, g_ent), g_v)
    keep = pol.offsets[12] if cont else pol.n_trainable  # (all but log_std: the Gaussian's dependence on it is not the head's)
    _within(mine[:keep], existing[:keep].cpu().double(), f"{(D, H, A, cont)} against tma_policy_evaluate_actions_backward")


# ---- 6
def test_head_is_plain_without_parameters():
    pol, _ = _policy(4, 64, 5, False)
    head, values = pol.head(_obs(33, 4, 0).to(_dev()))
    assert pol._leaf is None and not head.requires_grad and not values.requires_grad
    assert head.shape == (33, 5) and values.shape == (33,) and head.is_cuda
    dist = pol.get_distribution(_obs(33, 4, 0).to(_dev()))
    assert not dist.distribution.logits.requires_grad


@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 64, 4, True)] + H64_MORE)
def test_kl_between_two_policies_backpropagates_to_the_leaf(D, H, A, cont):
    student, s_sd = _policy(D, H, A, cont)
    teacher, t_sd = _policy(D, H, A, cont, seed=11)
    if cont:  # another log_std as well
        t_sd["log_std"] = t_sd["log_std"] + 0.2
        teacher.load_state_dict(t_sd)
    obs = _obs(77, D, 0)
    obs_d = obs.to(_dev())
    (leaf,) = student.parameters()
    before = student._head(obs_d)
    t_dist, s_dist = teacher.get_distribution(obs_d), student.get_distribution(obs_d)
    s_head = s_dist.distribution.mean if cont else s_dist.distribution.logits
    assert s_head.requires_grad and not (t_dist.distribution.mean if cont else t_dist.distribution.logits).requires_grad
    head, values = student.head(obs_d)
    assert head.requires_grad and values.requires_grad and _bits(head.detach(), before[0]) and _bits(values.detach(), before[1])
    loss = torch.distributions.kl_divergence(t_dist.distribution, s_dist.distribution).mean()
    loss.backward()
    loss_ref, g_ref = ref.kl_grad(t_sd, s_sd, obs)
    assert abs(loss.item() - loss_ref) <= 1e-5 * max(abs(loss_ref), 1.0), (loss.item(), loss_ref)
    _within(leaf.grad, _flat(student, g_ref), f"KL {(D, H, A, cont)}")
    if cont:
        o = student.offsets[12]
        assert float(leaf.grad[o:o + A].abs().min()) > 0  # log_std: through torch alone, non-zero here
    # values alone: the head's cotangent reaches the library as NULL
    leaf.grad = None
    student.head(obs_d)[1].sum().backward()
    assert _bits(leaf.grad, _head_vjp(student, obs, None, torch.ones(77)))
    with torch.no_grad():
        assert not student.head(obs_d)[0].requires_grad
    with pytest.raises(ValueError):
        student.head(obs_d.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        student.get_distribution(obs_d.clone().requires_grad_(True))
    leaf.requires_grad_(False)
    assert not student.head(obs_d)[0].requires_grad


@pytest.mark.parametrize("D,H,A,cont", [(4, 64, 5, False), (6, 256, 5, False), (6, 64, 4, True)] + H64_MORE)
def test_head_follows_a_torch_optimizer_step(D, H, A, cont):
    pol, sd = _policy(D, H, A, cont)
    obs = _obs(77, D, 0)
    obs_d = obs.to(_dev())
    opt = torch.optim.SGD(pol.parameters(), lr=0.1)
    head, values = pol.head(obs_d)
    (values.mean() + head[:, 0].mean()).backward()
    opt.step()
    stepped = pol.state_dict()
    head_ref, values_ref = ref.forward64(stepped, obs)
    assert (values_ref - ref.forward64(sd, obs)[1]).abs().max().item() > 1e-2  # the step moved the outputs far beyond the tolerance below
    head, values = pol.head(obs_d)
    assert torch.allclose(head.detach().cpu().double(), head_ref, **V_TOL) and torch.allclose(values.detach().cpu().double(), values_ref, **V_TOL)


def test_a_bf16_policy_gives_its_distribution_forward_only():
    pol, sd = _policy(6, 256, 5, False, mfma="bf16")
    obs = _obs(33, 6, 0)
    dist = pol.get_distribution(obs.to(_dev()))
    assert not dist.distribution.logits.requires_grad and bool(torch.isfinite(dist.entropy()).all())
    logits_emu, _ = _emulated_forward(sd, obs)
    assert torch.allclose(dist.distribution.logits.cpu(), torch.log_softmax(logits_emu, dim=1), rtol=4e-3, atol=4e-3)
    with pytest.raises(ValueError):
        pol.parameters()
    with pytest.raises(ValueError):
        pol.head_backward(obs.to(_dev()), torch.zeros(33, 5), None)


# ---- 7
def test_distillation_lands_where_the_cpu_reference_lands():
    """50 Adam(lr = 1e-3) steps on the full KL(teacher || student) from a fixed (4, 256, 5) teacher into a (4, 64, 5) student, 256 fixed
    observations.  As tests/test_policy_vjp_gpu.py test_behaviour_cloning_lands_where_the_cpu_reference_lands: the yardstick is the CPU
    restatement's own float32 - float64 gap of the final loss from the same start; the device (float32, other summation orders) must end within
    ten times that gap of the float64 run, and below where it started.
    Measured on an MI355X: initial loss 0.039113738, final loss device 0.000228950, CPU float32 0.000228953, CPU float64 0.000228950 -- the
    float32 - float64 gap is 2.7e-9 (so the bound is 2.7e-8) and the device ends 6.2e-13 from the float64 run."""
    D, A, n, steps = 4, 5, 256, 50
    student, s_sd = _policy(D, 64, A, False)
    teacher, t_sd = _policy(D, 256, A, False, seed=11)
    obs = _obs(n, D, 3)
    obs_d = obs.to(_dev())
    first32, last32 = ref.distill(t_sd, s_sd, obs, torch.float32, steps)
    first64, last64 = ref.distill(t_sd, s_sd, obs, torch.float64, steps)
    gap = abs(last32 - last64)
    opt = torch.optim.Adam(student.parameters(), lr=1e-3)
    with torch.no_grad():
        t_dist = teacher.get_distribution(obs_d).distribution
    kl = lambda: torch.distributions.kl_divergence(t_dist, student.get_distribution(obs_d).distribution).mean()  # noqa: E731
    first = kl().item()
    for _ in range(steps):
        opt.zero_grad()
        kl().backward()
        opt.step()
    with torch.no_grad():
        s_logits = student.get_distribution(obs_d).distribution.logits.double()
        t64 = torch.distributions.Categorical(logits=t_dist.logits.double())
        last = torch.distributions.kl_divergence(t64, torch.distributions.Categorical(logits=s_logits)).mean().item()
    print(f"distillation: initial {first:.9f} (f64 {first64:.9f}); final device {last:.9f}, cpu f32 {last32:.9f}, cpu f64 {last64:.9f}; "
          f"f32-f64 gap {gap:.3e}, device-f64 {abs(last - last64):.3e}")
    assert last < first
    assert abs(last - last64) <= 10.0 * gap, (last, last64, gap)
