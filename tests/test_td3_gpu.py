"""csrc/tma_td3.hip and three_mlagents_amd/td3.py on the GPU (include/tma.h ABI 227).

  * tma_td3_act: all three modes against the float64 restatement (tests/_td3_ref.py) with the kernel's OWN noise_out, a sigma large enough
    that the reference itself shows clipped elements (asserted first); NULL optional outputs; canaries behind every output; the head bits of both
    gradient kernels' forwards; the generated noise against N(0, 1) with tests/_sampling_stats.py; the collect and the target stream differ.
  * tma_td3_critic_grad / tma_td3_actor_grad against float64 autograd with noise_in given, on batches whose properties (both sides of
    target_noise_clip, both sides of the +-1 action clamp, both winners of the target min, no ReLU pre-activation within the margin) are asserted
    first from the reference.  Bound, the project's SAC convention: ten times the max-abs gap between the restatement run in torch float32 and in
    float64 on the same batch, floored at four float32 ulps of max|ref|; computed in the test and printed with the error.  The batches are built by
    per-row rejection, so no case is ever skipped for a ReLU kink.
  * run-to-run bit equality of both gradients; a row's head bits at n = 1 against the same row inside n = 67.
  * six gradient steps with policy_delay = 2 against the restatement at float64; the actor and its target bit-unchanged after odd steps.
  * tma_td3_iterations_local against the same sequence issued one C-ABI call at a time: every buffer and counter bit-equal.
  * the TD3 class on `ant` (105 + 8).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _sampling_stats as ss
import _td3_ref as ref
from three_mlagents_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(8, 256, 2), (105, 64, 8), (5, 128, 1), (21, 128, 3)]  # (D, H, A)
ROWS = [1, 15, 16, 17, 67]
TANH_CASE = ((8, 128, 2), 35, "tanh")
GRID_CAP_ROWS = _lib.SAC_GRID_CAP * 16  # workgroups of one 16-row tile each
GRAD_CASES = [(s, n, "relu") for s in SHAPES for n in ROWS] + [TANH_CASE, ((5, 128, 1), GRID_CAP_ROWS + 1, "relu")]
PN, CLIP = ref.POLICY_NOISE, ref.NOISE_CLIP
ULP4 = 4 * 2.0 ** -23  # four float32 ulps of 1: the floor of a bound, times max|ref|
p = _lib.ptr


def _dims(D, H, A, act):
    from three_mlagents_amd.td3 import sac_dims

    return sac_dims(D, A, H, act, 0)


def _tables(D, H, A, act):
    from three_mlagents_amd.td3 import actor_tensors, critic_tensors, param_offsets

    off = param_offsets(_dims(D, H, A, act))
    return off, actor_tensors(off, D, A, H), critic_tensors(off, D, A, H)


def _flats(sd, D, H, A, act):
    """(actor, actor_target, critic, critic_target) flat device buffers of SB3-named weights"""
    from three_mlagents_amd.td3 import flat_from_named

    off, at, ct = _tables(D, H, A, act)
    return (flat_from_named(sd, at, "actor", off.n_actor).to(DEV), flat_from_named(sd, at, "actor_target", off.n_actor).to(DEV),
            flat_from_named(sd, ct, "critic", off.n_critic).to(DEV), flat_from_named(sd, ct, "critic_target", off.n_critic).to(DEV))


def _named(flat, D, H, A, act, which):
    from three_mlagents_amd.td3 import named_from_flat

    _, at, ct = _tables(D, H, A, act)
    return named_from_flat(flat, at if which == "actor" else ct, which)


def _canary(shape, dtype=torch.float32, pad=64):
    """a buffer of prod(shape) + pad elements filled with 777: the pad must come back untouched"""
    n = int(np.prod(shape))
    return torch.full((n + pad,), 777.0, dtype=dtype, device=DEV), n


def _take(buf_n, shape):
    buf, n = buf_n
    assert bool((buf[n:] == 777.0).all()), "canary"
    return buf[:n].view(shape).cpu()


def _noise(A, mean, sigma):
    from three_mlagents_amd.td3 import NormalActionNoise, noise_struct

    return noise_struct(NormalActionNoise(mean, sigma), A)


def _act(actor, d, obs, mode, seed=0, draw=0, offset=0, *, an=None, noise_in=None, want=("noise", "head")):
    """One tma_td3_act call -> dict(actions, noise, head) (those asked for; canaries checked)."""
    n, A = obs.shape[0], d.act_dim
    bufs = dict(actions=_canary((n, A)), noise=_canary((n, A)) if "noise" in want else None, head=_canary((n, A)) if "head" in want else None)
    ptr = lambda k: p(bufs[k][0]) if bufs[k] is not None else None  # noqa: E731
    _lib.check(_lib.lib().tma_td3_act(p(actor), C.byref(d), p(obs), n, mode, C.byref(an) if an is not None else None, seed, draw, offset, p(noise_in),
                                      ptr("actions"), ptr("noise"), ptr("head"), _lib.stream_ptr(DEV)))
    return {k: _take(v, (n, A)) for k, v in bufs.items() if v is not None}


@functools.lru_cache(maxsize=None)
def _case(D, H, A, n, act):
    """Weights, batch (properties asserted FIRST, from the reference), device copies and the float64 / float32 references: computed once, shared."""
    sd = ref.make_sd(D, H, A, act, seed=3)
    batch, relu_rejected = ref.make_batch(sd, D, A, n, act, seed=100 + n)
    ref.check_batch(sd, batch, act)
    out = dict(sd=sd, batch=batch, flats=_flats(sd, D, H, A, act), dev={k: v.to(DEV).contiguous() for k, v in batch.items()}, relu_rejected=relu_rejected)
    for name, fn in (("critic", lambda dtype: ref.critic_grad(sd, batch, PN, CLIP, act, dtype)), ("actor", lambda dtype: ref.actor_grad(sd, batch, act, dtype))):
        g64, stats, x, y = fn(torch.float64)
        g32 = fn(torch.float32)[0]
        out[name] = dict(g64=g64, stats=stats, x=x, y=y, gap=max(float((g64[k] - g32[k].double()).abs().max()) for k in g64),
                         ref_max=max(float(v.abs().max()) for v in g64.values()))
    return out


def _workspace(d, n):
    need = int(_lib.lib().tma_td3_workspace_bytes(C.byref(d), n))
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device=DEV), need


def _poison(ws, need):
    ws.view(torch.int32)[: need // 4].fill_(0x7FC00000)  # quiet NaNs where the slabs and the partials go
    _lib.check(_lib.lib().tma_debug_poison_lds(0, _lib.stream_ptr(DEV)))


def _critic(c, d, n, *, actor_target=None, target=None, noise_in="batch", outs=True, poison=False, seed=7, draw=3, pn=PN, clip=CLIP):
    """One tma_td3_critic_grad call on case c -> dict(grad, stats, q, y, noise, head)."""
    L, b = _lib.lib(), c["dev"]
    _, a_tgt, critic, tgt = c["flats"]
    A = d.act_dim
    ws, need = _workspace(d, n)
    if poison:
        _poison(ws, need)
    grad, stats = _canary((critic.numel(),)), _canary((4,), torch.float64, 4)
    q, y, noise, head = (_canary(s) if outs else None for s in ((n, 2), (n,), (n, A), (n, A)))
    ptr = lambda t: p(t[0]) if t is not None else None  # noqa: E731
    _lib.check(L.tma_td3_critic_grad(p(a_tgt if actor_target is None else actor_target), p(critic), p(tgt if target is None else target), C.byref(d), p(b["obs"]),
                                     p(b["actions"]), p(b["next_obs"]), p(b["dones"]), p(b["rewards"]), p(b["discounts"]), n, pn, clip, seed, draw,
                                     p(b["noise"]) if isinstance(noise_in, str) else p(noise_in), p(grad[0]), p(stats[0]), ptr(q), ptr(y), ptr(noise), ptr(head),
                                     p(ws), need, _lib.stream_ptr(DEV)))
    out = dict(grad=_take(grad, (critic.numel(),)), stats=_take(stats, (4,)))
    if outs:
        out.update(q=_take(q, (n, 2)), y=_take(y, (n,)), noise=_take(noise, (n, A)), head=_take(head, (n, A)))
    return out


def _actor(c, d, n, *, critic=None, outs=True, poison=False):
    """One tma_td3_actor_grad call on case c -> dict(grad, stats, actions, head)."""
    L, b = _lib.lib(), c["dev"]
    actor, _, crit, _ = c["flats"]
    A = d.act_dim
    ws, need = _workspace(d, n)
    if poison:
        _poison(ws, need)
    grad, stats = _canary((actor.numel(),)), _canary((2,), torch.float64, 4)
    acts, head = (_canary((n, A)) if outs else None for _ in range(2))
    ptr = lambda t: p(t[0]) if t is not None else None  # noqa: E731
    _lib.check(L.tma_td3_actor_grad(p(actor), p(crit if critic is None else critic), C.byref(d), p(b["obs"]), n, p(grad[0]), p(stats[0]), ptr(acts), ptr(head),
                                    p(ws), need, _lib.stream_ptr(DEV)))
    out = dict(grad=_take(grad, (actor.numel(),)), stats=_take(stats, (2,)))
    if outs:
        out.update(actions=_take(acts, (n, A)), head=_take(head, (n, A)))
    return out


def _grad_error(got_flat, c, which, shape, act):
    D, H, A = shape
    named = _named(got_flat, D, H, A, act, which)
    g64 = c[which]["g64"]
    return max(float((named[k].double() - g64[k]).abs().max()) for k in g64)


def _bound(kind, shape, n, act, err, c):
    bound = max(10.0 * c["gap"], ULP4 * c["ref_max"])
    print(f"{kind} grad {shape} n={n} {act}: error {err:.3e}, bound {bound:.3e} (10 x f32-f64 gap {10.0 * c['gap']:.3e}, floor {ULP4 * c['ref_max']:.3e}), "
          f"max|ref| {c['ref_max']:.3e}")
    return bound


# ---- tma_td3_act
@pytest.mark.parametrize("shape,n,act", [(SHAPES[0], 67, "relu"), (SHAPES[1], 17, "relu"), (SHAPES[2], 1, "relu"), (SHAPES[3], 16, "relu"), TANH_CASE])
def test_act_matches_float64_in_all_three_modes(shape, n, act):
    D, H, A = shape
    sd = ref.make_sd(D, H, A, act, seed=3)
    actor = _flats(sd, D, H, A, act)[0]
    d = _dims(D, H, A, act)
    obs = torch.randn(n, D, generator=torch.Generator().manual_seed(n))
    mean, sigma = np.linspace(-0.2, 0.2, A), np.full(A, 1.5)  # sigma 1.5 on tanh(mu) in (-1, 1): the clamp is hit often
    an = _noise(A, mean, sigma)
    got = _act(actor, d, obs.to(DEV), _lib.TD3_NOISY, 11, 5, 1000, an=an)
    z = got["noise"]
    assert bool(torch.isfinite(z).all()) and (n * A < 8 or float(z.std()) > 0.3)

    def restated(dtype):
        mu = ref.actor_mu(ref.to_dtype(sd, dtype), "actor", obs.to(dtype), act)
        return mu, ref.act(mu), ref.act(mu, z.to(dtype), torch.as_tensor(mean, dtype=torch.float32).to(dtype), torch.as_tensor(sigma, dtype=torch.float32).to(dtype))

    (mu64, det64, a64), (mu32, det32, a32) = restated(torch.float64), restated(torch.float32)
    clipped = a64.abs() == 1.0
    if n * A >= 16:  # the reference itself shows clipped elements on both sides, and free ones
        assert bool((a64 == 1.0).any()) and bool((a64 == -1.0).any()) and bool((~clipped).any())
    gaps = dict(head=float((mu32.double() - mu64).abs().max()), det=float((det32.double() - det64).abs().max()), a=float((a32.double() - a64).abs().max()))
    errs = dict(head=float((got["head"].double() - mu64).abs().max()), a=float((got["actions"].double() - a64).abs().max()))
    # deterministic: tanh(mu), zero noise, no action_noise needed
    det = _act(actor, d, obs.to(DEV), _lib.TD3_DETERMINISTIC)
    errs["det"] = float((det["actions"].double() - det64).abs().max())
    print(f"act {shape} n={n} {act}: errors {errs}, float32-float64 gaps of the restatement {gaps}, clipped {int(clipped.sum())} of {clipped.numel()}")
    # bounds: ten times the restatement's own float32 - float64 gap, floored at a few float32 ulps of the values' size (a tiny batch can have a
    # gap of zero by luck): mu is a sum of up to 256 terms of order 1 (2e-5), actions lie in [-1, 1] and carry the noise's rounding (1e-6)
    assert errs["head"] <= max(10.0 * gaps["head"], 2e-5) and errs["a"] <= max(10.0 * gaps["a"], 1e-6) and errs["det"] <= max(10.0 * gaps["det"], 1e-6)
    assert float(got["actions"].abs().max()) <= 1.0 and torch.equal(got["actions"][clipped], a64[clipped].float())
    assert not bool(det["noise"].any()) and torch.equal(det["head"], got["head"]) and float(det["actions"].abs().max()) <= 1.0
    # its own noise fed back: equal bits everywhere; NULL optional outputs: the same actions
    again = _act(actor, d, obs.to(DEV), _lib.TD3_NOISY, 999, 999, 0, an=an, noise_in=z.to(DEV))
    for k in ("actions", "noise", "head"):
        assert torch.equal(again[k], got[k]), k
    bare = _act(actor, d, obs.to(DEV), _lib.TD3_NOISY, 11, 5, 1000, an=an, want=())
    assert torch.equal(bare["actions"], got["actions"])
    assert torch.equal(_act(actor, d, obs.to(DEV), _lib.TD3_DETERMINISTIC, want=())["actions"], det["actions"])
    # sigma 0 and mean 0: the noisy mode gives the deterministic bits
    quiet = _act(actor, d, obs.to(DEV), _lib.TD3_NOISY, 11, 5, 1000, an=_noise(A, 0.0, 0.0))
    assert torch.equal(quiet["actions"], det["actions"]) and torch.equal(quiet["noise"], z)


def test_act_uniform_mode_and_the_two_noise_streams():
    L = _lib.lib()
    D, H, A, n = 21, 128, 3, 4096
    d = _dims(D, H, A, "relu")
    buf = _canary((n, A))
    draws = []
    for draw in (0, 1):
        _lib.check(L.tma_td3_act(None, C.byref(d), None, n, _lib.TD3_UNIFORM, None, 5, draw, 0, None, p(buf[0]), None, None, _lib.stream_ptr(DEV)))
        draws.append(_take(buf, (n, A)).clone())
    u = draws[0]
    assert float(u.min()) >= -1.0 and float(u.max()) < 1.0 and float(u.std()) > 0.5 and abs(float(u.mean())) < 0.05
    assert not torch.equal(draws[0], draws[1]) and not torch.equal(u[0], u[1]) and not torch.equal(u[:, 0], u[:, 1])
    _lib.check(L.tma_td3_act(None, C.byref(d), None, n, _lib.TD3_UNIFORM, None, 5, 0, 7, None, p(buf[0]), None, None, _lib.stream_ptr(DEV)))
    assert torch.equal(_take(buf, (n, A))[:-7], u[7:])  # row_offset shifts the row id
    # SAC's warm-up arithmetic: the bits tma_sac_act gives for equal (seed, draw, row_offset)
    _lib.check(L.tma_sac_act(None, C.byref(d), None, n, _lib.SAC_UNIFORM, 5, 0, 0, None, p(buf[0]), None, None, None, _lib.stream_ptr(DEV)))
    assert torch.equal(_take(buf, (n, A)), u)
    # the two streams, from equal (seed, draw, rows): collect (act) and target smoothing (critic)
    c = _case(D, H, A, 67, "relu")
    an = _noise(A, 0.0, 0.1)
    z_act = _act(c["flats"][0], d, c["dev"]["obs"], _lib.TD3_NOISY, 7, 3, 0, an=an)["noise"]
    z_tgt = _critic(c, d, 67, noise_in=None)["noise"]
    assert not torch.equal(z_act, z_tgt)
    z_tgt2 = _critic(c, d, 67, noise_in=None, draw=4)["noise"]
    assert not torch.equal(z_tgt, z_tgt2) and not torch.equal(z_tgt[0], z_tgt[1]) and torch.equal(_critic(c, d, 67, noise_in=None)["noise"], z_tgt)
    assert not torch.equal(_act(c["flats"][0], d, c["dev"]["obs"], _lib.TD3_NOISY, 7, 4, 0, an=an)["noise"], z_act)
    for z in (z_act, z_tgt):
        assert bool(torch.isfinite(z).all()) and 0.7 < float(z.std()) < 1.3


@pytest.mark.parametrize("stream", ["collect", "target"])
def test_generated_noise_is_standard_normal(stream):
    """T draws x N rows x A columns of either stream against N(0, 1): the statistics of tests/_sampling_stats.py, one family level split
    Bonferroni over them."""
    D, H, A, T, N = 5, 64, 8, 24, 2048
    sd = ref.make_sd(D, H, A, "relu", seed=3)
    flats, d = _flats(sd, D, H, A, "relu"), _dims(D, H, A, "relu")
    if stream == "collect":
        obs, an = torch.zeros(N, D, device=DEV), _noise(A, 0.0, 0.1)
        z = np.stack([_act(flats[0], d, obs, _lib.TD3_NOISY, 21, t, 0, an=an, want=("noise",))["noise"].numpy() for t in range(T)])
    else:
        L = _lib.lib()
        ws, need = _workspace(d, N)
        zero = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
        grad, out = torch.empty(flats[2].numel(), device=DEV), torch.empty(N, A, device=DEV)
        obs, acts, vec = zero(N, D), zero(N, A), zero(N)
        rows = []
        for t in range(T):
            _lib.check(L.tma_td3_critic_grad(p(flats[1]), p(flats[2]), p(flats[3]), C.byref(d), p(obs), p(acts), p(obs), p(vec), p(vec), p(vec), N, 0.2, 0.5, 21, t,
                                             None, p(grad), None, None, None, p(out), None, p(ws), need, _lib.stream_ptr(DEV)))
            rows.append(out.cpu().numpy().copy())
        z = np.stack(rows)
    pvals = ss.normal(z.astype(np.float64))
    level = ss.FAMILY_ALPHA / len(ss.normal_names(A))
    bad = {k: v for k, v in pvals.items() if not v > level}
    assert not bad, bad


# ---- the two gradient calls
@pytest.mark.parametrize("shape,n,act", GRAD_CASES)
def test_critic_grad_matches_float64_autograd(shape, n, act):
    D, H, A = shape
    c, d = _case(D, H, A, n, act), _dims(D, H, A, act)
    got = _critic(c, d, n, poison=True)
    err = _grad_error(got["grad"], c, "critic", shape, act)
    bound = _bound("critic", shape, n, act, err, c["critic"])
    assert err <= bound, (err, bound)
    st, want = got["stats"].tolist(), c["critic"]["stats"]
    tol = lambda v: 2e-5 * max(abs(v), float(n))  # noqa: E731  (sums of n float32 values of order 1 to 10)
    assert st[3] == n and abs(st[0] - want["loss_sum"]) <= tol(want["loss_sum"]) and abs(st[1] - want["q0_sum"]) <= tol(want["q0_sum"])
    assert abs(st[2] - want["q1_sum"]) <= tol(want["q1_sum"])
    assert float((got["q"].double() - c["critic"]["x"]).abs().max()) <= 2e-5 and float((got["y"].double() - c["critic"]["y"]).abs().max()) <= 1e-4
    assert torch.equal(got["noise"], c["batch"]["noise"])
    # equal inputs, equal bits; the optional outputs change nothing
    again = _critic(c, d, n, outs=False)
    assert torch.equal(again["grad"], got["grad"]) and torch.equal(again["stats"], got["stats"])
    # the head of the critic's forward (the TARGET actor on next_obs): tma_td3_act's bits on the same rows
    if n <= 67:
        head = _act(c["flats"][1], d, c["dev"]["next_obs"], _lib.TD3_DETERMINISTIC, want=("head",))["head"]
        assert torch.equal(head, got["head"])


@pytest.mark.parametrize("shape,n,act", GRAD_CASES)
def test_actor_grad_matches_float64_autograd(shape, n, act):
    D, H, A = shape
    c, d = _case(D, H, A, n, act), _dims(D, H, A, act)
    got = _actor(c, d, n, poison=True)
    err = _grad_error(got["grad"], c, "actor", shape, act)
    bound = _bound("actor", shape, n, act, err, c["actor"])
    assert err <= bound, (err, bound)
    st, want = got["stats"].tolist(), c["actor"]["stats"]
    assert st[1] == n and abs(st[0] - want["loss_sum"]) <= 2e-5 * max(abs(want["loss_sum"]), float(n))
    assert float((got["actions"].double() - c["actor"]["x"]).abs().max()) <= 1e-5
    again = _actor(c, d, n, outs=False)
    assert torch.equal(again["grad"], got["grad"]) and torch.equal(again["stats"], got["stats"])
    # the actor forward is ONE device function: the head bits of tma_td3_act on the same rows, in another batch
    k = min(n, 5)
    head = _act(c["flats"][0], d, c["dev"]["obs"][:k].contiguous(), _lib.TD3_DETERMINISTIC, want=("head",))["head"]
    assert torch.equal(head, got["head"][:k])


def test_a_row_does_not_depend_on_its_batch_and_inputs_matter():
    shape, n, act = SHAPES[3], 67, "relu"
    D, H, A = shape
    c, d = _case(D, H, A, n, act), _dims(D, H, A, act)
    base_c, base_a = _critic(c, d, n), _actor(c, d, n)
    # head bits at n = 1 against the same row inside n = 67: rows 0, 16 (the second tile's first) and 66 (the last, in a partial tile)
    for row in (0, 16, 66):
        one = _act(c["flats"][0], d, c["dev"]["obs"][row:row + 1].contiguous(), _lib.TD3_DETERMINISTIC)
        assert torch.equal(one["head"][0], base_a["head"][row]) and torch.equal(one["actions"][0], base_a["actions"][row])
        one = _act(c["flats"][1], d, c["dev"]["next_obs"][row:row + 1].contiguous(), _lib.TD3_DETERMINISTIC)
        assert torch.equal(one["head"][0], base_c["head"][row])
    # NULL noise_in: generated; its noise_out as noise_in: equal bits everywhere; the batch's own noise is another one
    gen = _critic(c, d, n, noise_in=None)
    fed = _critic(c, d, n, noise_in=gen["noise"].to(DEV))
    for k in gen:
        assert torch.equal(gen[k], fed[k]), k
    assert not torch.equal(gen["grad"], base_c["grad"])
    # only the targets change: y and the critic gradient change, Q does not
    for kw in (dict(target=(c["flats"][3] * 1.5).contiguous()), dict(actor_target=c["flats"][0])):
        other = _critic(c, d, n, **kw)
        assert not torch.equal(other["grad"], base_c["grad"]) and not torch.equal(other["y"], base_c["y"]) and torch.equal(other["q"], base_c["q"])
    # the smoothing parameters reach the kernel: no noise, and a clip of zero, give the same y; another clip gives another
    y0 = _critic(c, d, n, pn=0.0)["y"]
    assert torch.equal(_critic(c, d, n, clip=0.0)["y"], y0) and not torch.equal(y0, base_c["y"]) and not torch.equal(_critic(c, d, n, clip=0.1)["y"], base_c["y"])
    # the actor gradient reads qf0 alone: another qf1 changes nothing, another qf0 moves it
    crit = c["flats"][2]
    nq = crit.numel() // 2
    other = crit.clone()
    other[nq:] *= 1.5
    same = _actor(c, d, n, critic=other)
    assert torch.equal(same["grad"], base_a["grad"]) and torch.equal(same["stats"], base_a["stats"])
    other = crit.clone()
    other[:nq] *= 1.5
    moved = _actor(c, d, n, critic=other)
    assert not torch.equal(moved["grad"], base_a["grad"]) and torch.equal(moved["actions"], base_a["actions"])


# ---- six full gradient steps
def test_six_gradient_steps_with_policy_delay_two_land_where_float64_torch_lands():
    """sample -> critic step -> (even steps) actor step -> both polyak updates, six times from a small ReplayBuffer, through TD3.train one step at
    a time; the same loop in torch (tests/_td3_ref.py Trainer) at float32 and at float64 on the rows and the noise the device used.  Compared: the
    four parameter sets after the sixth step, element by element.  Bound: ten times the same maximum between the two torch runs, floored at four
    float32 ulps of the largest parameter.  After odd steps the actor and its target are bit-unchanged."""
    from three_mlagents_amd.replay_buffer import ReplayBuffer
    from three_mlagents_amd.td3 import TD3, HipTD3Policy

    D, H, A, R, N, B, steps, lr, tau = 21, 128, 3, 40, 2, 64, 6, 1e-3, 0.05
    sd0 = ref.make_sd(D, H, A, "relu", seed=8)
    model = TD3("MlpPolicy", None, learning_rate=lr, batch_size=B, tau=tau, policy_delay=2, target_policy_noise=PN, target_noise_clip=CLIP, seed=4,
                policy_kwargs=dict(net_arch=[H, H]))
    model.device = DEV
    model._make_policy(D, A, H, "relu", DEV)
    pol = model.policy
    assert isinstance(pol, HipTD3Policy)
    pol.load_state_dict(sd0)
    g = torch.Generator().manual_seed(7)
    rb = model.replay_buffer = ReplayBuffer(R * N, D, (A, True), DEV, n_envs=N, seed=13)
    for _ in range(R):
        rb.add(torch.randn(N, D, generator=g).to(DEV), torch.randn(N, D, generator=g).to(DEV), (torch.rand(N, A, generator=g) * 2 - 1).to(DEV),
               torch.randn(N, generator=g).to(DEV), (torch.rand(N, generator=g) < 0.2).to(torch.uint8).to(DEV), torch.zeros(N, dtype=torch.uint8, device=DEV))
    L = _lib.lib()
    ws, need = _workspace(pol.dims, B)
    model.buf = dict(ws=ws, critic_stats=torch.zeros(4, dtype=torch.float64, device=DEV), actor_stats=torch.zeros(2, dtype=torch.float64, device=DEV))
    batches = []
    for k in range(steps):
        # the rows and the noise of step k, from the counters train() is about to use (draw = rb._draw, seed = model.seed)
        draw = rb._draw
        s = rb.sample(B)
        rb._draw = draw  # (train() draws the same batch again)
        z, grad = torch.empty((B, A), dtype=torch.float32, device=DEV), torch.empty(pol.n_critic, dtype=torch.float32, device=DEV)
        _lib.check(L.tma_td3_critic_grad(p(pol.actor_target), p(pol.critic), p(pol.critic_target), C.byref(pol.dims), p(s.observations), p(s.actions),
                                         p(s.next_observations), p(s.dones), p(s.rewards), p(s.discounts), B, PN, CLIP, model.seed, draw, None, p(grad), None, None,
                                         None, p(z), None, p(ws), need, _lib.stream_ptr(DEV)))
        batches.append(dict(obs=s.observations.cpu(), actions=s.actions.cpu(), next_obs=s.next_observations.cpu(), dones=s.dones.cpu(),
                            rewards=s.rewards.cpu(), discounts=s.discounts.cpu(), noise=z.cpu()))
        before = [t.clone() for t in (pol.actor, pol.actor_target, pol.critic, pol.critic_target)]
        model.train(gradient_steps=1, batch_size=B)
        moved = [not torch.equal(x, y) for x, y in zip(before, (pol.actor, pol.actor_target, pol.critic, pol.critic_target))]
        assert moved == ([False, False, True, False] if k % 2 == 0 else [True, True, True, True]), (k, moved)  # (k = 0 is the first, an odd, step)
        assert "train/critic_loss" in model.pop_train_stats() and ("train/actor_loss" in model.pop_train_stats()) == (k >= 1)
    assert model._n_updates == steps == model._adam_step and model._actor_adam_step == steps // 2 and rb._draw == steps

    def torch_run(dtype):
        t = ref.Trainer(sd0, lr=lr, tau=tau, policy_delay=2, policy_noise=PN, noise_clip=CLIP, dtype=dtype)
        for b in batches:
            t.step(b)
        return {k: v.detach().double() for k, v in t.sd.items()}

    w32, w64 = torch_run(torch.float32), torch_run(torch.float64)
    dev_sd = {k: v.double() for k, v in pol.state_dict().items()}
    for name, keys in (("actor", ref.actor_keys()), ("actor_target", ref.actor_keys("actor_target")), ("critic", ref.critic_keys()),
                       ("critic_target", ref.critic_keys("critic_target"))):
        gap = max(float((w32[k] - w64[k]).abs().max()) for k in keys)
        err = max(float((dev_sd[k] - w64[k]).abs().max()) for k in keys)
        moved = max(float((w64[k] - sd0[k].double()).abs().max()) for k in keys)
        floor = ULP4 * max(float(w64[k].abs().max()) for k in keys)
        print(f"six steps, {name}: device-f64 {err:.3e}, torch f32-f64 {gap:.3e}, floor {floor:.3e}, moved {moved:.3e}")
        assert moved > 1e-4 and err <= max(10.0 * gap, floor), (name, err, gap)


# ---- the native loop against the same calls issued one at a time
def _loop_model(n_envs, gradient_steps, policy_delay, noisy):
    from three_mlagents_amd.td3 import TD3, NormalActionNoise
    from three_mlagents_amd.vec_env import HipVecEnv

    env = HipVecEnv("ant", n_envs, seed=1)
    m = TD3("MlpPolicy", env, learning_rate=1e-3, learning_starts=8 * n_envs, buffer_size=24 * n_envs, batch_size=32, train_freq=2, gradient_steps=gradient_steps,
            policy_delay=policy_delay, tau=0.05, seed=5, action_noise=NormalActionNoise(np.zeros(8), 0.1 * np.ones(8)) if noisy else None,
            policy_kwargs=dict(net_arch=[64, 64]))
    with torch.no_grad():  # targets that differ from their nets from the start
        m.policy.critic_target.mul_(1.25)
        m.policy.actor_target.mul_(0.75)
    return m, env


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("n_envs,gradient_steps,policy_delay", [(1, 1, 2), (3, -1, 3)])
def test_native_loop_equals_the_calls_issued_one_by_one(monkeypatch, n_envs, gradient_steps, policy_delay, noisy):
    """32 vector steps of ant through tma_td3_iterations_local (one call, on a side stream, torch.Tensor.cpu disabled) and through the same
    C-ABI calls issued from Python in the order tests/_td3_ref.py iteration_events gives: across the learning_starts boundary (8 warm-up vector
    steps), with the action noise on and off.  Ring of 24 rows: it wraps."""
    L, N, ITERS = _lib.lib(), n_envs, 16
    native, env1 = _loop_model(n_envs, gradient_steps, policy_delay, noisy)
    manual, env2 = _loop_model(n_envs, gradient_steps, policy_delay, noisy)
    assert torch.equal(native.policy.actor, manual.policy.actor) and not torch.equal(native.policy.critic, native.policy.critic_target)
    a0 = native.policy.actor.clone()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with monkeypatch.context() as mp, torch.cuda.stream(side):
        def no_host_copy(self, *a, **k):
            raise AssertionError("the native loop copied a tensor to the host")

        mp.setattr(torch.Tensor, "cpu", no_host_copy)
        native._run_iterations(ITERS)
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    m, rb, b, pol, st = manual, manual.replay_buffer, manual.buf, manual.policy, _lib.stream_ptr(DEV)
    ao, co, d = m.actor_opt, m.critic_opt, C.byref(manual.policy.dims)
    eng = env2.engine
    rb.start(env2.reset_device())
    c = ref.new_counters()
    kinds, uniform, delayed = [], 0, 0
    mode = _lib.TD3_NOISY if noisy else _lib.TD3_DETERMINISTIC
    for ev in ref.iteration_events(c, ITERS, n_envs=N, capacity=24, train_freq=2, gradient_steps=gradient_steps, learning_starts=8 * N, policy_delay=policy_delay):
        kinds.append(ev[0])
        if ev[0] == "step":
            _, warm, draw, pos = ev
            uniform += warm
            _lib.check(L.tma_td3_act(None if warm else p(pol.actor), d, None if warm else p(rb.last_obs), N, _lib.TD3_UNIFORM if warm else mode, C.byref(m._noise),
                                     5, draw, eng.env_offset, None, p(b["actions"]), None, None, st))
            _lib.check(L.tma_env_step(eng._h, p(b["actions"]), _lib.ACT_F32, 0, 0, 1, p(b["step_obs"]), p(b["rewards"]), p(b["term"]), p(b["trunc"]),
                                      p(b["term_obs"]), None, None, st))
            _lib.check(L.tma_replay_add(C.byref(rb._view), pos, p(rb.last_obs), p(b["actions"]), p(b["step_obs"]), p(b["rewards"]), p(b["term"]), p(b["trunc"]),
                                        p(b["term_obs"]), st))
        else:
            _, size, newest, draw, t_c, t_a = ev
            _lib.check(L.tma_replay_sample(C.byref(rb._view), size, newest, 1, 0.99, rb.seed, draw, 32, p(b["s_obs"]), p(b["s_actions"]), p(b["s_next_obs"]),
                                           p(b["s_dones"]), p(b["s_rewards"]), p(b["s_discounts"]), None, None, st))
            _lib.check(L.tma_td3_critic_grad(p(pol.actor_target), p(pol.critic), p(pol.critic_target), d, p(b["s_obs"]), p(b["s_actions"]), p(b["s_next_obs"]),
                                             p(b["s_dones"]), p(b["s_rewards"]), p(b["s_discounts"]), 32, 0.2, 0.5, 5, draw, None, p(co.grad), p(b["critic_stats"]),
                                             None, None, None, None, p(b["ws"]), b["ws"].numel(), st))
            _lib.check(L.tma_adam_step_flat(p(pol.critic), p(co.grad), p(co.exp_avg), p(co.exp_avg_sq), pol.n_critic, t_c, 1e-3, 0.9, 0.999, 1e-8, st))
            if t_a is not None:
                delayed += 1
                _lib.check(L.tma_td3_actor_grad(p(pol.actor), p(pol.critic), d, p(b["s_obs"]), 32, p(ao.grad), p(b["actor_stats"]), None, None, p(b["ws"]),
                                                b["ws"].numel(), st))
                _lib.check(L.tma_adam_step_flat(p(pol.actor), p(ao.grad), p(ao.exp_avg), p(ao.exp_avg_sq), pol.n_actor, t_a, 1e-3, 0.9, 0.999, 1e-8, st))
                _lib.check(L.tma_polyak_update(p(pol.critic), p(pol.critic_target), pol.n_critic, 0.05, st))
                _lib.check(L.tma_polyak_update(p(pol.actor), p(pol.actor_target), pol.n_actor, 0.05, st))
    assert kinds.count("step") == 32 and uniform == 8 and kinds.count("train") > delayed > 0
    nrb, npol = native.replay_buffer, native.policy
    got = dict(num_timesteps=native.num_timesteps, n_calls=native._n_calls, pos=nrb.pos, full=nrb.full, draw=nrb._draw, collect_step=nrb._collect_step,
               critic_adam_step=native._adam_step, actor_adam_step=native._actor_adam_step, n_updates=native._n_updates)
    assert got == c and c["full"] and c["num_timesteps"] == 32 * N and c["actor_adam_step"] == c["n_updates"] // policy_delay
    pairs = [("actor", npol.actor, pol.actor), ("actor_target", npol.actor_target, pol.actor_target), ("critic", npol.critic, pol.critic),
             ("critic_target", npol.critic_target, pol.critic_target), ("last_obs", nrb.last_obs, rb.last_obs),
             ("critic_stats", native.buf["critic_stats"], b["critic_stats"]), ("actor_stats", native.buf["actor_stats"], b["actor_stats"])]
    for name in ("actor_opt", "critic_opt"):
        pairs += [(f"{name}.{k}", getattr(getattr(native, name), k), getattr(getattr(m, name), k)) for k in ("grad", "exp_avg", "exp_avg_sq")]
    pairs += [(name, getattr(nrb, name), getattr(rb, name)) for name in ("observations", "next_observations", "actions", "rewards", "terminated", "truncated")]
    for name, x, y in pairs:
        assert torch.equal(x, y), name
    assert not torch.equal(npol.actor, a0) and all(bool(torch.isfinite(t).all()) for t in (npol.actor, npol.actor_target, npol.critic, npol.critic_target))
    assert float(nrb.actions.abs().max()) <= 1.0
    env1.close()
    env2.close()


def test_action_noise_changes_what_the_loop_collects():
    off, env1 = _loop_model(1, 1, 2, False)
    on, env2 = _loop_model(1, 1, 2, True)
    off._run_iterations(8)
    on._run_iterations(8)
    a_off, a_on = off.replay_buffer.actions[:16].cpu(), on.replay_buffer.actions[:16].cpu()
    assert torch.equal(a_off[:8], a_on[:8]) and not torch.equal(a_off[8:], a_on[8:])  # the warm-up is the same uniform draw; then the noise enters
    assert float((a_on[8] - a_off[8]).abs().max()) < 0.6  # the first step behind the warm-up: equal obs and actor, N(0, 0.1) apart
    env1.close()
    env2.close()


# ---- the class (ant: 105 observations, 8 actions in [-1, 1])
def _class_model(env, **kw):
    from three_mlagents_amd.td3 import TD3

    return TD3("MlpPolicy", env, learning_starts=100, buffer_size=1000, batch_size=64, policy_kwargs=dict(net_arch=[64, 64]), **kw)


def test_the_class_learns_predicts_saves_and_goes_on(tmp_path):
    """Two histories from equal seeds: A learns 1100 + 61 steps; B learns 1100, is saved (zip + replay buffer), loaded onto its env where it stands,
    and learns the 61.  Everything after the load equals what was saved; A and B end bit-equal.  1100 steps: ant ends an episode at its 1000th step at
    the latest (csrc/tma_tasks.h), so learn() has written a log row; the ring of 1000 rows has wrapped.  61 more steps from an even _n_updates end
    on an odd one, so the delayed step continues from the loaded counters."""
    import zipfile

    from three_mlagents_amd.td3 import TD3, NormalActionNoise, plan_iterations
    from three_mlagents_amd.vec_env import HipVecEnv

    noise = lambda: NormalActionNoise(np.zeros(8), 0.1 * np.ones(8))  # noqa: E731
    env_a, env_b = HipVecEnv("ant", 1), HipVecEnv("ant", 1)
    a, b = _class_model(env_a, action_noise=noise()), _class_model(env_b, action_noise=noise())
    start = {k: v.clone() for k, v in b.policy.state_dict().items()}
    assert torch.equal(b.critic_target, b.critic) and torch.equal(b.actor_target, b.actor) and b.policy.activation == "relu" and b.learning_rate == 1e-3
    a.learn(1100, log_interval=1)
    b.learn(1100, log_interval=1)
    plan = plan_iterations(0, 0, 1100, 1, 1, 1, 100, 2)
    assert b.num_timesteps == 1100 == plan["num_timesteps"] and b._n_calls == 1100 and plan["uniform_steps"] == 100
    assert b._n_updates == plan["n_updates"] == 1000 == b._adam_step and b._actor_adam_step == plan["actor_updates"] == 500
    rb = b.replay_buffer
    assert (rb.pos, rb.full, rb._draw, rb._collect_step) == (100, True, 1000, 1100)
    for x, y in ((a.actor, b.actor), (a.actor_target, b.actor_target), (a.critic, b.critic), (a.critic_target, b.critic_target)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())  # the run is reproducible
    now = b.policy.state_dict()
    assert all(not torch.equal(now[k], start[k]) for k in start) and not torch.equal(b.critic_target, b.critic) and not torch.equal(b.actor_target, b.actor)
    stats = b.pop_train_stats()
    assert set(stats) == {"train/actor_loss", "train/critic_loss"} and all(np.isfinite(v) for v in stats.values()) and stats["train/critic_loss"] >= 0.0
    log = b.logger_values  # the last row learn() wrote: an episode has finished by step 1000
    for key in ("rollout/ep_rew_mean", "rollout/ep_len_mean", "train/n_updates", "train/critic_loss", "train/actor_loss", "train/learning_rate",
                "time/total_timesteps"):
        assert key in log and np.isfinite(log[key]), key
    assert log["train/learning_rate"] == 1e-3 and 0 < log["train/n_updates"] <= 1000 and "train/ent_coef" not in log
    # predict: tanh(mu), `deterministic` makes no difference; one row or many; inside the bounds
    obs = torch.randn(40, 105, generator=torch.Generator().manual_seed(2))
    act, state = b.predict(obs.numpy(), deterministic=True)
    mu = ref.actor_mu(ref.to_dtype(now, torch.float64), "actor", obs.double())
    assert state is None and act.dtype == np.float32 and act.shape == (40, 8) and np.abs(act - torch.tanh(mu).numpy()).max() <= 1e-5
    assert np.all(act >= env_b.action_space.low) and np.all(act <= env_b.action_space.high)
    one, _ = b.predict(obs[0].numpy(), deterministic=True)
    assert one.shape == (8,) and np.array_equal(one, act[0]) and np.array_equal(b.predict(obs.numpy(), deterministic=False)[0], act)
    # save / load onto the env where it stands
    b.save(tmp_path / "td3")
    b.save_replay_buffer(tmp_path / "replay.pt")
    with zipfile.ZipFile(tmp_path / "td3.zip") as z:
        assert {"data", "policy.pth", "actor.optimizer.pth", "critic.optimizer.pth"} <= set(z.namelist())
        import io
        import json

        data = json.loads(z.read("data").decode())
        sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
        opt = torch.load(io.BytesIO(z.read("actor.optimizer.pth")), map_location="cpu", weights_only=True)
    assert data["tma"]["algorithm"] == "td3" and data["policy_delay"] == 2
    assert list(sd) == ref.actor_keys() + ref.actor_keys("actor_target") + ref.critic_keys() + ref.critic_keys("critic_target")
    assert sd["actor.mu.4.weight"].shape == (8, 64) and sd["critic_target.qf1.0.weight"].shape == (64, 113)
    assert len(opt["state"]) == 6 and float(opt["state"][0]["step"]) == 500.0 and opt["state"][4]["exp_avg"].shape == (8, 64)
    loaded = TD3.load(tmp_path / "td3", env=env_b, force_reset=False)
    loaded.load_replay_buffer(tmp_path / "replay.pt")
    for name in ("learning_rate", "buffer_size", "learning_starts", "batch_size", "tau", "gamma", "train_freq", "gradient_steps", "n_steps", "policy_delay",
                 "target_policy_noise", "target_noise_clip", "seed", "num_timesteps", "_n_updates", "_adam_step", "_actor_adam_step", "_n_calls",
                 "_total_timesteps"):
        assert getattr(loaded, name) == getattr(b, name), name
    assert np.array_equal(loaded.action_noise.sigma, b.action_noise.sigma) and np.array_equal(loaded.action_noise.mean, b.action_noise.mean)
    pairs = [(loaded.actor, b.actor), (loaded.actor_target, b.actor_target), (loaded.critic, b.critic), (loaded.critic_target, b.critic_target),
             (loaded.replay_buffer.observations, b.replay_buffer.observations), (loaded.replay_buffer.actions, b.replay_buffer.actions),
             (loaded.replay_buffer.last_obs, b.replay_buffer.last_obs)]
    pairs += [(getattr(getattr(loaded, o), k), getattr(getattr(b, o), k)) for o in ("actor_opt", "critic_opt") for k in ("exp_avg", "exp_avg_sq")]
    for x, y in pairs:
        assert torch.equal(x, y)
    lr_, br = loaded.replay_buffer, b.replay_buffer
    assert (lr_.pos, lr_.full, lr_._draw, lr_._collect_step) == (br.pos, br.full, br._draw, br._collect_step) and loaded.policy.activation == "relu"
    assert np.array_equal(loaded.predict(obs.numpy())[0], act)  # identical predict bits
    a.learn(61, reset_num_timesteps=False)
    loaded.learn(61, reset_num_timesteps=False)
    assert a.num_timesteps == loaded.num_timesteps == 1161 and a._n_updates == loaded._n_updates == 1061 and a._actor_adam_step == loaded._actor_adam_step == 530
    for x, y in ((a.actor, loaded.actor), (a.actor_target, loaded.actor_target), (a.critic, loaded.critic), (a.critic_target, loaded.critic_target),
                 (a.actor_opt.exp_avg_sq, loaded.actor_opt.exp_avg_sq), (a.critic_opt.exp_avg, loaded.critic_opt.exp_avg)):
        assert torch.equal(x, y)
    assert not torch.equal(a.actor, b.actor)  # (b itself stayed at 1100)
    # train() as a public method: from _n_updates = 1000, three steps run the delayed block once (at 1002)
    before = [b.actor.clone(), b.critic.clone()]
    b.train(gradient_steps=3, batch_size=16)
    assert b._n_updates == 1003 and b._adam_step == 1003 and b._actor_adam_step == 501 and not torch.equal(b.actor, before[0]) and not torch.equal(b.critic, before[1])
    # without an env the model predicts
    bare = TD3.load(tmp_path / "td3")
    assert np.array_equal(bare.predict(obs.numpy(), deterministic=True)[0], act)
    # no actor step yet: train/actor_loss is absent
    fresh = _class_model(env_a, policy_delay=1000)
    first = [t.clone() for t in (fresh.actor, fresh.critic)]
    fresh.learn(140)
    assert fresh._n_updates == 40 and fresh._actor_adam_step == 0 and set(fresh.pop_train_stats()) == {"train/critic_loss"}
    assert torch.equal(fresh.actor, first[0]) and torch.equal(fresh.actor_target, first[0])  # only the critics have stepped: no target has moved
    assert torch.equal(fresh.critic_target, first[1]) and not torch.equal(fresh.critic, first[1])
    env_a.close()
    env_b.close()
    # a Discrete task and a shape outside the kernels' are refused
    for task, word in (("gridworld", "Box action space"), ("crawler", "act_dim 20")):
        env = HipVecEnv(task, 1)
        with pytest.raises(ValueError, match=word):
            _class_model(env)
        env.close()
