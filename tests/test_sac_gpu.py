"""csrc/tma_sac.hip and three_mlagents_amd/sac.py on the GPU (include/tma.h ABI 226).

  * tma_sac_act: actions / logp against the float64 restatement (tests/_sac_ref.py) with the kernel's OWN noise_out; the deterministic and the
    uniform mode; NULL optional outputs; canaries behind every output; the head bits of the gradient kernels' forward; the generated noise
    against N(0, 1) with the statistics and the family level of tests/_sampling_stats.py; the three streams.
  * tma_sac_critic_grad / tma_sac_actor_grad against float64 autograd with noise_in given, on batches whose properties are asserted first from
    the reference.  Bound: ten times the max-abs gap between the restatement run in torch float32 and in float64 on the same batch, computed in
    the test (log(1 - a^2 + 1e-6) amplifies float32 rounding of a by up to about 100 at |u| = 3, so no fixed bound is taken); the error, the
    bound, max|ref| and whether DQN's 2e-5 max(max|ref|, 1) + 1e-6 would have held are printed.
  * tma_adam_step_flat against torch Adam, tma_polyak_update bit-equal to three torch ops.
  * six full gradient steps against the restatement at float64, the bound ten times the float32 - float64 gap of the torch runs.
  * tma_sac_iterations_local against the same sequence issued one C-ABI call at a time: every buffer and counter bit-equal.
  * the SAC class and the harness on `ant`, the one Box task whose shape the kernels take (105 + 8; ball3d's action space is Discrete).
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import _sac_ref as ref
import _sampling_stats as ss
from three_mlagents_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(8, 256, 2), (105, 64, 8), (5, 128, 1), (21, 128, 3)]  # (D, H, A)
ROWS = [1, 15, 16, 17, 67]
TANH_CASE = ((8, 128, 2), 35, "tanh")
GRID_CAP_ROWS = _lib.SAC_GRID_CAP * 16  # workgroups of one 16-row tile each
GRAD_CASES = [(s, n, "relu") for s in SHAPES for n in ROWS] + [TANH_CASE, ((5, 128, 1), GRID_CAP_ROWS + 1, "relu")]
LOG_ALPHA = float(np.log(0.2))
p = _lib.ptr


def _dims(D, H, A, act):
    from three_mlagents_amd.sac import sac_dims

    return sac_dims(D, A, H, act, 0)


def _tables(D, H, A, act):
    from three_mlagents_amd.sac import actor_tensors, critic_tensors, param_offsets

    off = param_offsets(_dims(D, H, A, act))
    return off, actor_tensors(off, D, A, H), critic_tensors(off, D, A, H)


def _flats(sd, D, H, A, act):
    """(actor, critic, critic_target) flat device buffers of SB3-named weights"""
    from three_mlagents_amd.sac import flat_from_named

    off, at, ct = _tables(D, H, A, act)
    return (flat_from_named(sd, at, "actor", off.n_actor).to(DEV), flat_from_named(sd, ct, "critic", off.n_critic).to(DEV),
            flat_from_named(sd, ct, "critic_target", off.n_critic).to(DEV))


def _named(flat, D, H, A, act, which):
    from three_mlagents_amd.sac import named_from_flat

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


def _act(actor, d, obs, mode, seed, draw, offset, *, noise_in=None, want=("logp", "noise", "head")):
    """One tma_sac_act call -> dict(actions, logp, noise, head) (those asked for; canaries checked)."""
    n, A = obs.shape[0], d.act_dim
    bufs = dict(actions=_canary((n, A)), logp=_canary((n,)) if "logp" in want else None, noise=_canary((n, A)) if "noise" in want else None,
                head=_canary((n, 2 * A)) if "head" in want else None)
    ptr = lambda k: p(bufs[k][0]) if bufs[k] is not None else None  # noqa: E731
    _lib.check(_lib.lib().tma_sac_act(p(actor), C.byref(d), p(obs), n, mode, seed, draw, offset, p(noise_in), ptr("actions"), ptr("logp"), ptr("noise"),
                                      ptr("head"), _lib.stream_ptr(DEV)))
    shapes = dict(actions=(n, A), logp=(n,), noise=(n, A), head=(n, 2 * A))
    return {k: _take(v, shapes[k]) for k, v in bufs.items() if v is not None}


@functools.lru_cache(maxsize=None)
def _case(D, H, A, n, act):
    """Weights, batch (properties asserted FIRST, from the reference), device copies and the float64 / float32 references: computed once, shared."""
    sd = ref.make_sd(D, H, A, act, seed=3)
    batch = ref.make_batch(sd, D, A, n, act, seed=100 + n, log_ent_coef=LOG_ALPHA)
    ref.check_batch(sd, batch, act, LOG_ALPHA)
    out = dict(sd=sd, batch=batch, flats=_flats(sd, D, H, A, act), dev={k: v.to(DEV).contiguous() for k, v in batch.items()},
               log_alpha=torch.tensor([LOG_ALPHA], dtype=torch.float32, device=DEV))
    for name, fn in (("critic", ref.critic_grad), ("actor", ref.actor_grad)):
        g64, stats, x, y = fn(sd, batch, LOG_ALPHA, act, dtype=torch.float64)
        g32 = fn(sd, batch, LOG_ALPHA, act, dtype=torch.float32)[0]
        out[name] = dict(g64=g64, stats=stats, x=x, y=y, gap=max(float((g64[k] - g32[k].double()).abs().max()) for k in g64),
                         ref_max=max(float(v.abs().max()) for v in g64.values()))
    return out


def _workspace(d, n):
    need = int(_lib.lib().tma_sac_workspace_bytes(C.byref(d), n))
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device=DEV), need


def _critic(c, d, n, *, target=None, log_alpha=None, noise_in="batch", outs=True, poison=False, seed=7, draw=3):
    """One tma_sac_critic_grad call on case c -> dict(grad, stats, q, y, noise, head)."""
    L, b = _lib.lib(), c["dev"]
    actor, critic, tgt = c["flats"]
    A = d.act_dim
    ws, need = _workspace(d, n)
    if poison:
        ws.view(torch.int32)[: need // 4].fill_(0x7FC00000)  # quiet NaNs where the slabs and the partials go
        _lib.check(L.tma_debug_poison_lds(0, _lib.stream_ptr(DEV)))
    grad, stats = _canary((critic.numel(),)), _canary((4,), torch.float64, 4)
    q, y, noise, head = (_canary(s) if outs else None for s in ((n, 2), (n,), (n, A), (n, 2 * A)))
    ptr = lambda t: p(t[0]) if t is not None else None  # noqa: E731
    _lib.check(L.tma_sac_critic_grad(p(actor), p(critic), p(tgt if target is None else target), p(c["log_alpha"] if log_alpha is None else log_alpha),
                                     C.byref(d), p(b["obs"]), p(b["actions"]), p(b["next_obs"]), p(b["dones"]), p(b["rewards"]), p(b["discounts"]), n, seed, draw,
                                     p(b["noise_next"]) if isinstance(noise_in, str) else p(noise_in), p(grad[0]), p(stats[0]), ptr(q), ptr(y), ptr(noise),
                                     ptr(head), p(ws), need, _lib.stream_ptr(DEV)))
    out = dict(grad=_take(grad, (critic.numel(),)), stats=_take(stats, (4,)))
    if outs:
        out.update(q=_take(q, (n, 2)), y=_take(y, (n,)), noise=_take(noise, (n, A)), head=_take(head, (n, 2 * A)))
    return out


def _actor(c, d, n, *, critic=None, log_alpha=None, noise_in="batch", outs=True, poison=False, seed=7, draw=3):
    """One tma_sac_actor_grad call on case c -> dict(grad, stats, actions, logp, noise, head)."""
    L, b = _lib.lib(), c["dev"]
    actor, crit, _ = c["flats"]
    A = d.act_dim
    ws, need = _workspace(d, n)
    if poison:
        ws.view(torch.int32)[: need // 4].fill_(0x7FC00000)
        _lib.check(L.tma_debug_poison_lds(0, _lib.stream_ptr(DEV)))
    grad, stats = _canary((actor.numel(),)), _canary((3,), torch.float64, 4)
    acts, logp, noise, head = (_canary(s) if outs else None for s in ((n, A), (n,), (n, A), (n, 2 * A)))
    ptr = lambda t: p(t[0]) if t is not None else None  # noqa: E731
    _lib.check(L.tma_sac_actor_grad(p(actor), p(crit if critic is None else critic), p(c["log_alpha"] if log_alpha is None else log_alpha), C.byref(d),
                                    p(b["obs"]), n, seed, draw, p(b["noise_pi"]) if isinstance(noise_in, str) else p(noise_in), p(grad[0]), p(stats[0]),
                                    ptr(acts), ptr(logp), ptr(noise), ptr(head), p(ws), need, _lib.stream_ptr(DEV)))
    out = dict(grad=_take(grad, (actor.numel(),)), stats=_take(stats, (3,)))
    if outs:
        out.update(actions=_take(acts, (n, A)), logp=_take(logp, (n,)), noise=_take(noise, (n, A)), head=_take(head, (n, 2 * A)))
    return out


def _grad_error(got_flat, c, which, shape, act):
    D, H, A = shape
    named = _named(got_flat, D, H, A, act, which)
    g64 = c[which]["g64"]
    return max(float((named[k].double() - g64[k]).abs().max()) for k in g64)


def _report(kind, shape, n, act, err, c):
    bound, ref_max = 10.0 * c["gap"], c["ref_max"]
    dqn = 2e-5 * max(ref_max, 1.0) + 1e-6
    print(f"{kind} grad {shape} n={n} {act}: error {err:.3e}, bound (10 x f32-f64 gap) {bound:.3e}, max|ref| {ref_max:.3e}; DQN's bound {dqn:.3e} "
          f"{'would have held' if err <= dqn else 'would NOT have held'}")
    return bound


# ---- tma_sac_act
@pytest.mark.parametrize("shape,n,act", [(SHAPES[0], 67, "relu"), (SHAPES[1], 17, "relu"), (SHAPES[2], 1, "relu"), (SHAPES[3], 16, "relu"), TANH_CASE])
def test_act_matches_float64_with_its_own_noise(shape, n, act):
    D, H, A = shape
    sd = ref.make_sd(D, H, A, act, seed=3)
    sd["actor.log_std.weight"][0] *= 0.25  # column 0 (mean -2.5, std 3) still leaves the clamp above 2, with fewer rows whose tanh is 1 in float32
    sd["actor.log_std.bias"][0] = sd["actor.log_std.bias"][0] * 0.25 - 1.0
    actor = _flats(sd, D, H, A, act)[0]
    d = _dims(D, H, A, act)
    obs = torch.randn(n, D, generator=torch.Generator().manual_seed(n))
    got = _act(actor, d, obs.to(DEV), _lib.SAC_SAMPLE, 11, 5, 1000)
    z = got["noise"]
    assert bool(torch.isfinite(z).all()) and (n * A < 8 or float(z.std()) > 0.3)

    def restated(dtype):
        mu, ls = ref.actor_head(ref.to_dtype(sd, dtype), obs.to(dtype), act)
        a, logp, u = ref.squash(mu, ls, z.to(dtype))
        return mu, ls, a, logp

    (mu64, ls64, a64, lp64), (mu32, ls32, a32, lp32) = restated(torch.float64), restated(torch.float32)
    head64 = torch.cat([mu64, ls64], dim=1)
    gaps = dict(head=float((torch.cat([mu32, ls32], dim=1).double() - head64).abs().max()), a=float((a32.double() - a64).abs().max()),
                logp=float((lp32.double() - lp64).abs().max()))
    errs = dict(head=float((got["head"].double() - head64).abs().max()), a=float((got["actions"].double() - a64).abs().max()),
                logp=float((got["logp"].double() - lp64).abs().max()))
    print(f"act {shape} n={n} {act}: errors {errs}, float32-float64 gaps of the restatement {gaps}")
    # bounds: ten times the restatement's own float32 - float64 gap, and never below a few float32 ulps of the values' size (a tiny batch can
    # have a gap of zero by luck): head and logp are sums of up to 256 terms of order 1 to 30 (2e-5), actions lie in [-1, 1] (1e-6)
    assert errs["head"] <= max(10.0 * gaps["head"], 2e-5) and errs["a"] <= max(10.0 * gaps["a"], 1e-6) and errs["logp"] <= max(10.0 * gaps["logp"], 2e-5)
    assert float(got["actions"].abs().max()) <= 1.0
    # its own noise fed back: equal bits everywhere; NULL optional outputs: the same actions
    again = _act(actor, d, obs.to(DEV), _lib.SAC_SAMPLE, 999, 999, 0, noise_in=z.to(DEV))
    for k in ("actions", "logp", "noise", "head"):
        assert torch.equal(again[k], got[k]), k
    bare = _act(actor, d, obs.to(DEV), _lib.SAC_SAMPLE, 11, 5, 1000, want=())
    assert torch.equal(bare["actions"], got["actions"])
    # deterministic: tanh(mu), zero noise, the logp of z = 0
    det = _act(actor, d, obs.to(DEV), _lib.SAC_DETERMINISTIC, 11, 5, 1000)
    a_det, lp_det, _ = ref.squash(mu64, ls64, torch.zeros_like(mu64))
    assert not bool(det["noise"].any()) and torch.equal(det["head"], got["head"])
    assert float((det["actions"].double() - a_det).abs().max()) <= max(10.0 * gaps["head"], 1e-6)
    assert float((det["logp"].double() - lp_det).abs().max()) <= max(10.0 * gaps["logp"], 2e-5)


def test_act_uniform_mode_and_the_three_noise_streams():
    L = _lib.lib()
    D, H, A, n = 21, 128, 3, 4096
    d = _dims(D, H, A, "relu")
    buf = _canary((n, A))
    draws = []
    for draw in (0, 1):
        _lib.check(L.tma_sac_act(None, C.byref(d), None, n, _lib.SAC_UNIFORM, 5, draw, 0, None, p(buf[0]), None, None, None, _lib.stream_ptr(DEV)))
        draws.append(_take(buf, (n, A)).clone())
    u = draws[0]
    assert float(u.min()) >= -1.0 and float(u.max()) < 1.0 and float(u.std()) > 0.5 and abs(float(u.mean())) < 0.05
    assert not torch.equal(draws[0], draws[1]) and not torch.equal(u[0], u[1]) and not torch.equal(u[:, 0], u[:, 1])
    _lib.check(L.tma_sac_act(None, C.byref(d), None, n, _lib.SAC_UNIFORM, 5, 0, 7, None, p(buf[0]), None, None, None, _lib.stream_ptr(DEV)))
    assert torch.equal(_take(buf, (n, A))[:-7], u[7:])  # row_offset shifts the row id
    # the three streams, from equal (seed, draw, rows): collect (act), next action (critic), pi action (actor)
    c = _case(D, H, A, 67, "relu")
    z_act = _act(c["flats"][0], d, c["dev"]["obs"], _lib.SAC_SAMPLE, 7, 3, 0)["noise"]
    z_next = _critic(c, d, 67, noise_in=None)["noise"]
    z_pi = _actor(c, d, 67, noise_in=None)["noise"]
    assert not torch.equal(z_act, z_next) and not torch.equal(z_act, z_pi) and not torch.equal(z_next, z_pi)
    z_pi2 = _actor(c, d, 67, noise_in=None, draw=4)["noise"]
    assert not torch.equal(z_pi, z_pi2) and not torch.equal(z_pi[0], z_pi[1]) and torch.equal(_actor(c, d, 67, noise_in=None)["noise"], z_pi)
    for z in (z_act, z_next, z_pi):
        assert bool(torch.isfinite(z).all()) and 0.7 < float(z.std()) < 1.3


def test_generated_noise_is_standard_normal():
    """T draws x N rows x A columns of the collect stream against N(0, 1): the statistics of tests/_sampling_stats.py, one family level split
    Bonferroni over them."""
    D, H, A, T, N = 5, 64, 8, 24, 2048
    sd = ref.make_sd(D, H, A, "relu", seed=3)
    actor, d = _flats(sd, D, H, A, "relu")[0], _dims(D, H, A, "relu")
    obs = torch.zeros(N, D, device=DEV)
    z = np.stack([_act(actor, d, obs, _lib.SAC_SAMPLE, 21, t, 0, want=("noise",))["noise"].numpy() for t in range(T)]).astype(np.float64)
    pvals = ss.normal(z)
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
    bound = _report("critic", shape, n, act, err, c["critic"])
    assert err <= bound, (err, bound)
    st, want = got["stats"].tolist(), c["critic"]["stats"]
    tol = lambda v: 2e-5 * max(abs(v), float(n))  # noqa: E731  (sums of n float32 values of order 1 to 10)
    assert st[3] == n and abs(st[0] - want["loss_sum"]) <= tol(want["loss_sum"]) and abs(st[1] - want["q0_sum"]) <= tol(want["q0_sum"])
    assert abs(st[2] - want["q1_sum"]) <= tol(want["q1_sum"])
    assert float((got["q"].double() - c["critic"]["x"]).abs().max()) <= 2e-5 and float((got["y"].double() - c["critic"]["y"]).abs().max()) <= 1e-4
    assert torch.equal(got["noise"], c["batch"]["noise_next"])
    # equal inputs, equal bits; the optional outputs change nothing
    again = _critic(c, d, n, outs=False)
    assert torch.equal(again["grad"], got["grad"]) and torch.equal(again["stats"], got["stats"])


@pytest.mark.parametrize("shape,n,act", GRAD_CASES)
def test_actor_grad_matches_float64_autograd(shape, n, act):
    D, H, A = shape
    c, d = _case(D, H, A, n, act), _dims(D, H, A, act)
    got = _actor(c, d, n, poison=True)
    err = _grad_error(got["grad"], c, "actor", shape, act)
    bound = _report("actor", shape, n, act, err, c["actor"])
    assert err <= bound, (err, bound)
    st, want = got["stats"].tolist(), c["actor"]["stats"]
    tol = lambda v: 2e-5 * max(abs(v), float(n))  # noqa: E731
    assert st[2] == n and abs(st[0] - want["loss_sum"]) <= tol(want["loss_sum"]) and abs(st[1] - want["logp_sum"]) <= tol(want["logp_sum"])
    assert float((got["actions"].double() - c["actor"]["x"]).abs().max()) <= 1e-5 and float((got["logp"].double() - c["actor"]["y"]).abs().max()) <= 1e-4
    assert torch.equal(got["noise"], c["batch"]["noise_pi"])
    again = _actor(c, d, n, outs=False)
    assert torch.equal(again["grad"], got["grad"]) and torch.equal(again["stats"], got["stats"])
    # the actor forward is ONE device function: the head bits of tma_sac_act on the same rows, in another batch
    k = min(n, 5)
    head = _act(c["flats"][0], d, c["dev"]["obs"][:k].contiguous(), _lib.SAC_DETERMINISTIC, 0, 0, 0, want=("head",))["head"]
    assert torch.equal(head, got["head"][:k])
    if n <= 67:
        head_next = _act(c["flats"][0], d, c["dev"]["next_obs"], _lib.SAC_DETERMINISTIC, 0, 0, 0, want=("head",))["head"]
        assert torch.equal(head_next, _critic(c, d, n)["head"])


def test_generated_noise_fed_back_gives_equal_bits_and_inputs_matter():
    shape, n, act = SHAPES[3], 67, "relu"
    D, H, A = shape
    c, d = _case(D, H, A, n, act), _dims(D, H, A, act)
    # NULL noise_in: generated; its noise_out as noise_in: equal bits everywhere
    for run in (_critic, _actor):
        gen = run(c, d, n, noise_in=None)
        fed = run(c, d, n, noise_in=gen["noise"].to(DEV))
        for k in gen:
            assert torch.equal(gen[k], fed[k]), (run.__name__, k)
        assert not torch.equal(gen["grad"], run(c, d, n)["grad"])  # (the batch's own noise is another one)
    base = _critic(c, d, n)
    # only the target critics change: y and the critic gradient change
    other = _critic(c, d, n, target=(c["flats"][2] * 1.5).contiguous())
    assert not torch.equal(other["grad"], base["grad"]) and not torch.equal(other["y"], base["y"]) and torch.equal(other["q"], base["q"])
    # only alpha changes: the same
    alpha2 = torch.tensor([float(np.log(0.7))], dtype=torch.float32, device=DEV)
    other = _critic(c, d, n, log_alpha=alpha2)
    assert not torch.equal(other["grad"], base["grad"]) and torch.equal(other["q"], base["q"])
    a_base = _actor(c, d, n)
    a_other = _actor(c, d, n, log_alpha=alpha2)
    assert not torch.equal(a_other["grad"], a_base["grad"]) and torch.equal(a_other["actions"], a_base["actions"])
    # the actor gradient reads the critics, not the target: other critics move it, and its signature takes no target at all
    a_crit = _actor(c, d, n, critic=c["flats"][2])
    assert not torch.equal(a_crit["grad"], a_base["grad"]) and torch.equal(a_crit["actions"], a_base["actions"])


# ---- optimizer and polyak
@pytest.mark.parametrize("n", [1, 257])
def test_adam_step_flat_follows_torch_adam(n):
    L = _lib.lib()
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * s for s in (1.0, 0.01, 3.0, 1e-4)]
    w = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=3e-4, eps=1e-8)
    params, m, v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    tail = _canary((n,))
    for t, gr in enumerate(grads, 1):
        w.grad = gr.clone()
        opt.step()
        tail[0][:n].copy_(params)
        _lib.check(L.tma_adam_step_flat(p(tail[0]), p(gr.to(DEV)), p(m), p(v), n, t, 3e-4, 0.9, 0.999, 1e-8, _lib.stream_ptr(DEV)))
        params = _take(tail, (n,)).to(DEV)
        st = opt.state[w]
        # one float32 ulp (1.2e-7 relative) of the largest operand per step taken so far: of the largest parameter; for exp_avg of the largest
        # |grad| seen (a small exp_avg is the rounded difference of terms that size); for exp_avg_sq of the largest grad^2 (1 - beta2) seen
        gmax = max(float(x.abs().max()) for x in grads[:t])
        assert float((params.cpu() - w.detach()).abs().max()) <= t * 1.2e-7 * max(1.0, float(w.detach().abs().max()))
        assert float((m.cpu() - st["exp_avg"]).abs().max()) <= t * 1.2e-7 * gmax
        assert float((v.cpu() - st["exp_avg_sq"]).abs().max()) <= t * 1.2e-7 * 1e-3 * gmax * gmax
    assert not torch.equal(params.cpu(), p0)


def test_polyak_update_is_three_torch_ops():
    L, n = _lib.lib(), 1000
    g = torch.Generator().manual_seed(1)
    params, target = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    buf = _canary((n,))
    buf[0][:n].copy_(target)
    tau = 0.005
    _lib.check(L.tma_polyak_update(p(params), p(buf[0]), n, tau, _lib.stream_ptr(DEV)))
    want = torch.tensor(tau, dtype=torch.float32, device=DEV) * params + torch.tensor(1.0 - tau, dtype=torch.float32, device=DEV) * target
    assert torch.equal(_take(buf, (n,)), want.cpu())
    _lib.check(L.tma_polyak_update(p(params), p(buf[0]), n, 1.0, _lib.stream_ptr(DEV)))
    assert torch.equal(_take(buf, (n,)), params.cpu())


# ---- six full gradient steps
def test_six_gradient_steps_land_where_float64_torch_lands():
    """sample -> critic step -> actor step -> ent_coef step -> polyak, six times from a small ReplayBuffer, through SAC.train; the same loop in
    torch (tests/_sac_ref.py Trainer) at float32 and at float64 on the rows and the noise the device used.  Compared: the three parameter sets
    and log_ent_coef after the sixth step, element by element.  Bound: ten times the same maximum between the two torch runs.
    Measured on an MI355X (printed): device - float64 6.96e-3 / 2.82e-3 / 5.00e-4 (actor / critic / target), torch float32 - float64 6.96e-3 /
    2.82e-3 / 5.00e-4, while the parameters moved by 6.0e-3 / 6.0e-3 / 0.70.  The gap is lr-sized because Adam divides a gradient by its own
    size: an element whose gradient is of rounding size (a ReLU unit alive on one row whose tanh is saturated) moves by lr in a direction the
    precision decides.  The float32 run shows it from the first step on one element per matrix, so here the bound is a loose one; the tight
    statement about the arithmetic is the two gradient tests above."""
    from three_mlagents_amd.replay_buffer import ReplayBuffer
    from three_mlagents_amd.sac import SAC, HipSACPolicy, _OptState

    D, H, A, R, N, B, steps, lr, tau = 21, 128, 3, 40, 2, 64, 6, 1e-3, 0.05
    sd0 = ref.make_sd(D, H, A, "relu", seed=8)
    model = SAC("MlpPolicy", None, learning_rate=lr, batch_size=B, tau=tau, ent_coef="auto_0.3", seed=4, policy_kwargs=dict(net_arch=[H, H]))
    model.device = DEV
    model._make_policy(D, A, H, "relu", DEV)
    pol = model.policy
    assert isinstance(pol, HipSACPolicy) and isinstance(model.ent_coef_optimizer, _OptState)
    pol.load_state_dict(sd0)
    g = torch.Generator().manual_seed(7)
    rb = model.replay_buffer = ReplayBuffer(R * N, D, (A, True), DEV, n_envs=N, seed=13)
    for _ in range(R):
        rb.add(torch.randn(N, D, generator=g).to(DEV), torch.randn(N, D, generator=g).to(DEV), (torch.rand(N, A, generator=g) * 2 - 1).to(DEV),
               torch.randn(N, generator=g).to(DEV), (torch.rand(N, generator=g) < 0.2).to(torch.uint8).to(DEV), torch.zeros(N, dtype=torch.uint8, device=DEV))
    L = _lib.lib()
    ws, need = _workspace(pol.dims, B)
    model.buf = dict(ws=ws, critic_stats=torch.zeros(4, dtype=torch.float64, device=DEV), actor_stats=torch.zeros(3, dtype=torch.float64, device=DEV))
    batches = []
    for k in range(steps):
        # the rows and the noise of step k, from the counters train() is about to use (draw = rb._draw, seed = model.seed)
        draw = rb._draw
        s = rb.sample(B)
        rb._draw = draw  # (train() draws the same batch again)
        z = {}
        for name, fn in (("noise_next", "critic"), ("noise_pi", "actor")):
            buf = torch.empty((B, A), dtype=torch.float32, device=DEV)
            grad = torch.empty(pol.n_critic if fn == "critic" else pol.n_actor, dtype=torch.float32, device=DEV)
            if fn == "critic":
                _lib.check(L.tma_sac_critic_grad(p(pol.actor), p(pol.critic), p(pol.critic_target), p(pol.log_ent_coef), C.byref(pol.dims), p(s.observations),
                                                 p(s.actions), p(s.next_observations), p(s.dones), p(s.rewards), p(s.discounts), B, model.seed, draw, None, p(grad),
                                                 None, None, None, p(buf), None, p(ws), need, _lib.stream_ptr(DEV)))
            else:
                _lib.check(L.tma_sac_actor_grad(p(pol.actor), p(pol.critic), p(pol.log_ent_coef), C.byref(pol.dims), p(s.observations), B, model.seed, draw, None,
                                                p(grad), None, None, None, p(buf), None, p(ws), need, _lib.stream_ptr(DEV)))
            z[name] = buf.cpu()
        batches.append(dict(obs=s.observations.cpu(), actions=s.actions.cpu(), next_obs=s.next_observations.cpu(), dones=s.dones.cpu(),
                            rewards=s.rewards.cpu(), discounts=s.discounts.cpu(), **z))
        model.train(gradient_steps=1, batch_size=B)
    assert model._n_updates == steps and rb._draw == steps

    def torch_run(dtype):
        t = ref.Trainer(sd0, float(np.log(0.3)), lr=lr, tau=tau, target_entropy=-float(A), dtype=dtype)
        for b in batches:
            t.step(b)
        return {k: v.detach().double() for k, v in t.sd.items()}, float(t.log_ent_coef.detach()[0])

    (w32, e32), (w64, e64) = torch_run(torch.float32), torch_run(torch.float64)
    dev_sd, e_dev = {k: v.double() for k, v in pol.state_dict().items()}, float(pol.log_ent_coef.cpu()[0])
    for name, keys in (("actor", ref.actor_keys()), ("critic", ref.critic_keys()), ("critic_target", ref.critic_keys("critic_target"))):
        gap = max(float((w32[k] - w64[k]).abs().max()) for k in keys)
        err = max(float((dev_sd[k] - w64[k]).abs().max()) for k in keys)
        moved = max(float((w64[k] - sd0[k].double()).abs().max()) for k in keys)
        print(f"six steps, {name}: device-f64 {err:.3e}, torch f32-f64 {gap:.3e}, moved {moved:.3e}")
        assert moved > 1e-3 and err <= 10.0 * gap, (name, err, gap)
    print(f"six steps, log_ent_coef: device {e_dev:.9f}, f32 {e32:.9f}, f64 {e64:.9f}")
    assert abs(e64 - float(np.log(0.3))) > 1e-3 and abs(e_dev - e64) <= 10.0 * abs(e32 - e64) + 1.2e-7  # (+ one float32 ulp of 1: a scalar's gap can cancel)


# ---- the native loop against the same calls issued one at a time
def _loop_model(n_envs, gradient_steps):
    from three_mlagents_amd.sac import SAC
    from three_mlagents_amd.vec_env import HipVecEnv

    env = HipVecEnv("ant", n_envs, seed=1)
    m = SAC("MlpPolicy", env, learning_rate=1e-3, learning_starts=8 * n_envs, buffer_size=24 * n_envs, batch_size=32, train_freq=2, gradient_steps=gradient_steps,
            target_update_interval=2, tau=0.05, seed=5, policy_kwargs=dict(net_arch=[64, 64]))
    with torch.no_grad():  # a target that differs from the critics from the start
        m.policy.critic_target.mul_(1.25)
    return m, env


@pytest.mark.parametrize("n_envs,gradient_steps", [(1, 1), (3, -1)])
def test_native_loop_equals_the_calls_issued_one_by_one(monkeypatch, n_envs, gradient_steps):
    """32 vector steps of ant through tma_sac_iterations_local (one call, on a side stream, torch.Tensor.cpu disabled) and through the same
    C-ABI calls issued from Python in the order tests/_sac_ref.py iteration_events gives.  Ring of 24 rows: it wraps."""
    L, N, ITERS = _lib.lib(), n_envs, 16
    native, env1 = _loop_model(n_envs, gradient_steps)
    manual, env2 = _loop_model(n_envs, gradient_steps)
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
    ao, co, eo, d = m.actor_opt, m.critic_opt, m.ent_opt, C.byref(manual.policy.dims)
    eng = env2.engine
    rb.start(env2.reset_device())
    c = ref.new_counters()
    kinds, uniform, polyaks = [], 0, 0
    for ev in ref.iteration_events(c, ITERS, n_envs=N, capacity=24, train_freq=2, gradient_steps=gradient_steps, learning_starts=8 * N, target_update_interval=2):
        kinds.append(ev[0])
        if ev[0] == "step":
            _, warm, draw, pos = ev
            uniform += warm
            _lib.check(L.tma_sac_act(None if warm else p(pol.actor), d, None if warm else p(rb.last_obs), N, _lib.SAC_UNIFORM if warm else _lib.SAC_SAMPLE, 5, draw,
                                     eng.env_offset, None, p(b["actions"]), None, None, None, st))
            _lib.check(L.tma_env_step(eng._h, p(b["actions"]), _lib.ACT_F32, 0, 0, 1, p(b["step_obs"]), p(b["rewards"]), p(b["term"]), p(b["trunc"]),
                                      p(b["term_obs"]), None, None, st))
            _lib.check(L.tma_replay_add(C.byref(rb._view), pos, p(rb.last_obs), p(b["actions"]), p(b["step_obs"]), p(b["rewards"]), p(b["term"]), p(b["trunc"]),
                                        p(b["term_obs"]), st))
        else:
            _, size, newest, draw, t, polyak = ev
            polyaks += polyak
            _lib.check(L.tma_replay_sample(C.byref(rb._view), size, newest, 1, 0.99, rb.seed, draw, 32, p(b["s_obs"]), p(b["s_actions"]), p(b["s_next_obs"]),
                                           p(b["s_dones"]), p(b["s_rewards"]), p(b["s_discounts"]), None, None, st))
            _lib.check(L.tma_sac_critic_grad(p(pol.actor), p(pol.critic), p(pol.critic_target), p(pol.log_ent_coef), d, p(b["s_obs"]), p(b["s_actions"]),
                                             p(b["s_next_obs"]), p(b["s_dones"]), p(b["s_rewards"]), p(b["s_discounts"]), 32, 5, draw, None, p(co.grad),
                                             p(b["critic_stats"]), None, None, None, None, p(b["ws"]), b["ws"].numel(), st))
            _lib.check(L.tma_adam_step_flat(p(pol.critic), p(co.grad), p(co.exp_avg), p(co.exp_avg_sq), pol.n_critic, t, 1e-3, 0.9, 0.999, 1e-8, st))
            _lib.check(L.tma_sac_actor_grad(p(pol.actor), p(pol.critic), p(pol.log_ent_coef), d, p(b["s_obs"]), 32, 5, draw, None, p(ao.grad), p(b["actor_stats"]),
                                            None, None, None, None, p(b["ws"]), b["ws"].numel(), st))
            _lib.check(L.tma_adam_step_flat(p(pol.actor), p(ao.grad), p(ao.exp_avg), p(ao.exp_avg_sq), pol.n_actor, t, 1e-3, 0.9, 0.999, 1e-8, st))
            _lib.check(L.tma_sac_ent_coef_grad(p(b["actor_stats"]), -8.0, p(eo.grad), st))
            _lib.check(L.tma_adam_step_flat(p(pol.log_ent_coef), p(eo.grad), p(eo.exp_avg), p(eo.exp_avg_sq), 1, t, 1e-3, 0.9, 0.999, 1e-8, st))
            if polyak:
                _lib.check(L.tma_polyak_update(p(pol.critic), p(pol.critic_target), pol.n_critic, 0.05, st))
    assert kinds.count("step") == 32 and uniform == 8 and kinds.count("train") > polyaks > 0
    nrb, npol = native.replay_buffer, native.policy
    got = dict(num_timesteps=native.num_timesteps, n_calls=native._n_calls, pos=nrb.pos, full=nrb.full, draw=nrb._draw, collect_step=nrb._collect_step,
               adam_step=native._adam_step, n_updates=native._n_updates)
    assert got == c and c["full"] and c["num_timesteps"] == 32 * N
    pairs = [("actor", npol.actor, pol.actor), ("critic", npol.critic, pol.critic), ("critic_target", npol.critic_target, pol.critic_target),
             ("log_ent_coef", npol.log_ent_coef, pol.log_ent_coef), ("last_obs", nrb.last_obs, rb.last_obs),
             ("critic_stats", native.buf["critic_stats"], b["critic_stats"]), ("actor_stats", native.buf["actor_stats"], b["actor_stats"])]
    for name in ("actor_opt", "critic_opt", "ent_opt"):
        pairs += [(f"{name}.{k}", getattr(getattr(native, name), k), getattr(getattr(m, name), k)) for k in ("exp_avg", "exp_avg_sq")]
    pairs += [(name, getattr(nrb, name), getattr(rb, name)) for name in ("observations", "next_observations", "actions", "rewards", "terminated", "truncated")]
    for name, x, y in pairs:
        assert torch.equal(x, y), name
    assert not torch.equal(npol.actor, a0) and all(bool(torch.isfinite(t).all()) for t in (npol.actor, npol.critic, npol.critic_target, npol.log_ent_coef))
    assert float(npol.log_ent_coef.cpu()[0]) != 0.0 and float(nrb.actions.abs().max()) <= 1.0
    env1.close()
    env2.close()


# ---- the class and the harness (ant: 105 observations, 8 actions in [-1, 1])
def _class_model(env, **kw):
    from three_mlagents_amd.sac import SAC

    return SAC("MlpPolicy", env, learning_starts=100, buffer_size=1000, batch_size=64, policy_kwargs=dict(net_arch=[64, 64]), **kw)


def test_the_class_learns_predicts_saves_and_goes_on(tmp_path):
    """Two histories from equal seeds: A learns 1100 + 60 steps; B learns 1100, is saved (zip + replay buffer), loaded onto its env where it
    stands, and learns the 60.  Everything after the load equals what was saved; A and B end bit-equal.  1100 steps: ant ends an episode at its
    1000th step at the latest (csrc/tma_tasks.h), so at least one episode has finished and learn() has written a log row; the ring of 1000 rows
    has wrapped."""
    from three_mlagents_amd.evaluation import evaluate_policy
    from three_mlagents_amd.sac import SAC, plan_iterations
    from three_mlagents_amd.vec_env import HipVecEnv

    env_a, env_b = HipVecEnv("ant", 1), HipVecEnv("ant", 1)
    a, b = _class_model(env_a), _class_model(env_b)
    start = {k: v.clone() for k, v in b.policy.state_dict().items()}
    assert torch.equal(b.critic_target, b.critic) and b.policy.activation == "relu" and b._target_entropy == -8.0 and float(b.log_ent_coef.cpu()[0]) == 0.0
    a.learn(1100, log_interval=1)
    b.learn(1100, log_interval=1)
    plan = plan_iterations(0, 0, 1100, 1, 1, 1, 100, 1)
    assert b.num_timesteps == 1100 == plan["num_timesteps"] and b._n_calls == 1100 and plan["uniform_steps"] == 100
    assert b._n_updates == plan["n_updates"] == 1000 == b._adam_step == plan["target_updates"]
    rb = b.replay_buffer
    assert (rb.pos, rb.full, rb._draw, rb._collect_step) == (100, True, 1000, 1100)
    for x, y in ((a.actor, b.actor), (a.critic, b.critic), (a.critic_target, b.critic_target), (a.log_ent_coef, b.log_ent_coef)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())  # the run is reproducible
    now = b.policy.state_dict()
    assert all(not torch.equal(now[k], start[k]) for k in start) and not torch.equal(b.critic_target, b.critic)
    stats = b.pop_train_stats()
    assert set(stats) == {"train/actor_loss", "train/critic_loss", "train/ent_coef", "train/ent_coef_loss"} and all(np.isfinite(v) for v in stats.values())
    assert stats["train/ent_coef"] != 1.0
    log = b.logger_values  # the last row learn() wrote: an episode has finished by step 1000
    for key in ("rollout/ep_rew_mean", "rollout/ep_len_mean", "train/actor_loss", "train/critic_loss", "train/ent_coef", "train/ent_coef_loss",
                "train/n_updates", "train/learning_rate", "time/fps", "time/total_timesteps", "time/episodes", "time/time_elapsed"):
        assert key in log, key
    assert all(np.isfinite(log[k]) for k in log if k.startswith(("train/", "rollout/"))), log
    assert log["train/learning_rate"] == 3e-4 and log["time/episodes"] >= 1 and 1 <= log["rollout/ep_len_mean"] <= 1000
    assert 0 < log["train/n_updates"] <= 1000 and log["time/total_timesteps"] <= 1100 and log["train/ent_coef"] > 0.0
    # predict: tanh(mu) when deterministic, a sample otherwise; one row or many
    obs = torch.randn(40, 105, generator=torch.Generator().manual_seed(2))
    act, state = b.predict(obs.numpy(), deterministic=True)
    mu, _ = ref.actor_head(ref.to_dtype(now, torch.float64), obs.double())
    assert state is None and act.dtype == np.float32 and act.shape == (40, 8) and np.abs(act - torch.tanh(mu).numpy()).max() <= 1e-5
    one, _ = b.predict(obs[0].numpy(), deterministic=True)
    assert one.shape == (8,) and np.array_equal(one, act[0])
    sampled, _ = b.predict(obs.numpy())
    assert sampled.shape == (40, 8) and np.abs(sampled).max() <= 1.0 and not np.array_equal(sampled, act)
    eval_env = HipVecEnv("ant", 4, seed=77)
    mean_r, std_r = evaluate_policy(b, eval_env, 4)
    assert np.isfinite(mean_r) and np.isfinite(std_r)
    eval_env.close()
    # save / load onto the env where it stands
    b.save(tmp_path / "sac")
    b.save_replay_buffer(tmp_path / "replay.pt")
    loaded = SAC.load(tmp_path / "sac", env=env_b, force_reset=False)
    loaded.load_replay_buffer(tmp_path / "replay.pt")
    for name in ("learning_rate", "buffer_size", "learning_starts", "batch_size", "tau", "gamma", "train_freq", "gradient_steps", "n_steps",
                 "target_update_interval", "ent_coef", "_target_entropy", "_auto_ent", "seed", "num_timesteps", "_n_updates", "_adam_step", "_n_calls",
                 "_total_timesteps"):
        assert getattr(loaded, name) == getattr(b, name), name
    pairs = [(loaded.actor, b.actor), (loaded.critic, b.critic), (loaded.critic_target, b.critic_target), (loaded.log_ent_coef, b.log_ent_coef),
             (loaded.replay_buffer.observations, b.replay_buffer.observations), (loaded.replay_buffer.actions, b.replay_buffer.actions),
             (loaded.replay_buffer.last_obs, b.replay_buffer.last_obs)]
    pairs += [(getattr(getattr(loaded, o), k), getattr(getattr(b, o), k)) for o in ("actor_opt", "critic_opt", "ent_opt") for k in ("exp_avg", "exp_avg_sq")]
    for x, y in pairs:
        assert torch.equal(x, y)
    lr_, br = loaded.replay_buffer, b.replay_buffer
    assert (lr_.pos, lr_.full, lr_._draw, lr_._collect_step) == (br.pos, br.full, br._draw, br._collect_step) and loaded.policy.activation == "relu"
    a.learn(60, reset_num_timesteps=False)
    loaded.learn(60, reset_num_timesteps=False)
    assert a.num_timesteps == loaded.num_timesteps == 1160 and a._n_updates == loaded._n_updates == 1060
    for x, y in ((a.actor, loaded.actor), (a.critic, loaded.critic), (a.critic_target, loaded.critic_target), (a.log_ent_coef, loaded.log_ent_coef),
                 (a.actor_opt.exp_avg_sq, loaded.actor_opt.exp_avg_sq), (a.critic_opt.exp_avg, loaded.critic_opt.exp_avg)):
        assert torch.equal(x, y)
    assert not torch.equal(a.actor, b.actor)  # (b itself stayed at 1100)
    # train() as a public method; without an env the model predicts
    n0 = b._n_updates
    before = b.actor.clone()
    b.train(gradient_steps=2, batch_size=16)
    assert b._n_updates == n0 + 2 and not torch.equal(b.actor, before)
    bare = SAC.load(tmp_path / "sac")
    assert np.array_equal(bare.predict(obs.numpy(), deterministic=True)[0], act)
    # a fixed ent_coef never steps log_ent_coef; a Discrete task and a shape outside the kernels' are refused
    fixed = _class_model(env_a, ent_coef=0.1)
    fixed.learn(140)
    assert float(fixed.log_ent_coef.cpu()[0]) == float(np.float32(np.log(0.1))) and fixed._n_updates == 40
    # its zip has no ent_coef_optimizer.pth: an absent member is fine, a member that is there but does not load is an error
    import zipfile

    fixed.save(tmp_path / "fixed")
    with zipfile.ZipFile(tmp_path / "fixed.zip") as z:
        assert "ent_coef_optimizer.pth" not in z.namelist()
    refixed = SAC.load(tmp_path / "fixed")
    assert not refixed._auto_ent and refixed.ent_coef_optimizer is None and torch.equal(refixed.log_ent_coef, fixed.log_ent_coef)
    assert torch.equal(refixed.actor, fixed.actor)
    with zipfile.ZipFile(tmp_path / "sac.zip") as zin, zipfile.ZipFile(tmp_path / "bad.zip", "w") as zout:
        for name in zin.namelist():
            zout.writestr(name, b"not a torch file" if name == "critic.optimizer.pth" else zin.read(name))
    with pytest.raises(Exception) as info:
        SAC.load(tmp_path / "bad")
    assert not isinstance(info.value, (KeyError, AssertionError))
    env_a.close()
    env_b.close()
    for task, word in (("gridworld", "Box action space"), ("crawler", "act_dim 20")):
        env = HipVecEnv(task, 1)
        with pytest.raises(ValueError, match=word):
            _class_model(env)
        env.close()


def test_the_harness_trains_and_evaluates_sac(tmp_path, monkeypatch):
    from three_mlagents_amd import harness

    monkeypatch.chdir(tmp_path)
    cfg = harness.TrainConfig("ant", algorithm="sac", total_timesteps=600, n_envs=8, eval_episodes=2, eval_freq=400, run_name="sac_run", verbose=0)
    result = harness.train_task(cfg, model_kwargs=dict(learning_starts=100, batch_size=64, buffer_size=2000, policy_kwargs=dict(net_arch=[64, 64])))
    assert result.algorithm == "sac" and result.total_timesteps == 600 and np.isfinite(result.mean_reward)
    with open(result.metadata_path, encoding="utf-8") as fh:
        meta = json.load(fh)
    assert meta["algorithm"] == "sac" and meta["substituted_for"] is None
    assert meta["schedule"] == dict(batch_size=64, train_freq=1, gradient_steps=1, learning_starts=100, buffer_size=2000, n_envs=1)  # n_envs forced to 1
    out = harness.evaluate_model("ant", result.model_filename, episodes=2)
    assert out["episodes"] == 2 and np.isfinite(out["mean_reward"]) and len(out["episode_rewards"]) == 2
    action = harness.predict_action("ant", np.zeros(105, dtype=np.float32), result.model_filename)
    assert isinstance(action, list) and len(action) == 8 and all(-1.0 <= x <= 1.0 for x in action)
    with pytest.raises(ValueError, match="Box action space"):
        harness.train_task(harness.TrainConfig("gridworld", algorithm="sac", total_timesteps=100, verbose=0))
