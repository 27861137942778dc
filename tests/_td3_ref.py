"""torch / plain-Python restatement of csrc/tma_td3.hip and of the loop of three_mlagents_amd/td3.py (include/tma.h, ABI 227) -- TEST
INFRASTRUCTURE ONLY, importable without a GPU, at the dtype it is called with, in SB3's names (stable_baselines3/td3/td3.py).

  * actor_mu / act / q_value: the deterministic actor (actor.mu, one Sequential) before its tanh, tma_td3_act's three-line arithmetic, one critic
    over obs | action, for ReLU / tanh, on SB3-named tensors ([out][in] weights: what HipTD3Policy.state_dict() gives);
  * critic_loss / actor_loss with their autograd gradients, and critic_grad_by_hand / actor_grad_by_hand: the same gradients from cotangents
    written out the way the kernels form them (2 (Q - y) / n; -1 / n through qf0 alone, down to the action rows, through the tanh);
  * Trainer: TD3.train's gradient step in SB3's own order with two torch Adams, the delayed actor step and both polyak updates;
  * sb3_train_plan: a literal loop of SB3's train() for the delayed update;  iteration_events: the loop of one tma_td3_iterations_local call;
  * make_sd / make_batch / check_batch: weights whose heads are scaled from data, a batch built by per-row rejection on the float64 reference so
    that it holds both sides of target_noise_clip, both sides of the action clamp and both winners of the target min, and the properties asserted
    first.
"""
from __future__ import annotations

import math

import torch

from _relu_ref import KINK_MARGIN  # noqa: F401  (the ReLU screen's margin, the one tests/_sac_ref.py uses)
from _sac_ref import _cast_batch, _f, critic_keys, q_value, to_dtype  # noqa: F401

ACTOR_LAYERS = ("mu.0", "mu.2", "mu.4")
Q_GAP, EDGE_GAP = 1e-3, 1e-3
POLICY_NOISE, NOISE_CLIP = 0.4, 0.5  # the gradient tests' smoothing: |0.4 z| passes 0.5 on one row in five (SB3's 0.2 / 0.5: one in eighty)


def actor_keys(prefix="actor"):
    return [f"{prefix}.{layer}.{p}" for layer in ACTOR_LAYERS for p in ("weight", "bias")]


def tensor_shapes(D, A, H):
    """{SB3 name: shape} of the four nets, in SB3's state_dict order."""
    out = {}
    for prefix in ("actor", "actor_target"):
        out.update({f"{prefix}.mu.0.weight": (H, D), f"{prefix}.mu.0.bias": (H,), f"{prefix}.mu.2.weight": (H, H), f"{prefix}.mu.2.bias": (H,),
                    f"{prefix}.mu.4.weight": (A, H), f"{prefix}.mu.4.bias": (A,)})
    for prefix in ("critic", "critic_target"):
        for i in range(2):
            out.update({f"{prefix}.qf{i}.0.weight": (H, D + A), f"{prefix}.qf{i}.0.bias": (H,), f"{prefix}.qf{i}.2.weight": (H, H),
                        f"{prefix}.qf{i}.2.bias": (H,), f"{prefix}.qf{i}.4.weight": (1, H), f"{prefix}.qf{i}.4.bias": (1,)})
    return out


# ---- the nets
def actor_mu(sd, prefix, obs, activation="relu", pre=None):
    """mu [B, A] BEFORE the tanh of `prefix` in ("actor", "actor_target"); `pre`: a list the two hidden pre-activations are appended to."""
    lin, f = torch.nn.functional.linear, _f(activation)
    z1 = lin(obs, sd[f"{prefix}.mu.0.weight"], sd[f"{prefix}.mu.0.bias"])
    z2 = lin(f(z1), sd[f"{prefix}.mu.2.weight"], sd[f"{prefix}.mu.2.bias"])
    if pre is not None:
        pre += [z1, z2]
    return lin(f(z2), sd[f"{prefix}.mu.4.weight"], sd[f"{prefix}.mu.4.bias"])


def act(mu, z=None, mean=None, sigma=None):
    """tma_td3_act on a head: tanh(mu), or with noise z clamp(tanh(mu) + (mean + sigma z), -1, 1)."""
    a = torch.tanh(mu)
    return a if z is None else torch.clamp(a + (mean + sigma * z), -1.0, 1.0)


# ---- the losses (TD3.train)
def critic_parts(sd, batch, policy_noise=POLICY_NOISE, noise_clip=NOISE_CLIP, activation="relu", pre=None):
    """-> (q0, q1, y, a_next, qt0, qt1, raw, mu_next): raw = policy_noise z before its clamp.  batch: obs, actions, next_obs, dones, rewards,
    discounts, noise."""
    with torch.no_grad():
        mu = actor_mu(sd, "actor_target", batch["next_obs"], activation, pre)
        raw = policy_noise * batch["noise"]
        a_next = torch.clamp(torch.tanh(mu) + torch.clamp(raw, -noise_clip, noise_clip), -1.0, 1.0)
        qt0 = q_value(sd, "critic_target", 0, batch["next_obs"], a_next, activation, pre)
        qt1 = q_value(sd, "critic_target", 1, batch["next_obs"], a_next, activation, pre)
        y = batch["rewards"] + (1.0 - batch["dones"]) * batch["discounts"] * torch.min(qt0, qt1)
    q0 = q_value(sd, "critic", 0, batch["obs"], batch["actions"], activation, pre)
    q1 = q_value(sd, "critic", 1, batch["obs"], batch["actions"], activation, pre)
    return q0, q1, y, a_next, qt0, qt1, raw, mu


def critic_loss(sd, batch, policy_noise=POLICY_NOISE, noise_clip=NOISE_CLIP, activation="relu"):
    q0, q1, y, *_ = critic_parts(sd, batch, policy_noise, noise_clip, activation)
    return torch.nn.functional.mse_loss(q0, y) + torch.nn.functional.mse_loss(q1, y)  # SB3: sum(F.mse_loss(q, target) for q in current_q_values)


def actor_loss(sd, batch, activation="relu", pre=None):
    """-mean(Q0(obs, tanh(mu(obs)))): SB3's -critic.q1_forward(obs, actor(obs)).mean().  -> (loss, a_pi, q0)"""
    a_pi = torch.tanh(actor_mu(sd, "actor", batch["obs"], activation, pre))
    q0 = q_value(sd, "critic", 0, batch["obs"], a_pi, activation, pre)
    return -q0.mean(), a_pi, q0


def critic_grad(sd, batch, policy_noise=POLICY_NOISE, noise_clip=NOISE_CLIP, activation="relu", dtype=torch.float64):
    """autograd in `dtype`: ({SB3 name: gradient} over the critic tensors, stats dict(loss_sum, q0_sum, q1_sum), q [B, 2], y [B])."""
    keys = critic_keys()
    sd_t = {k: v.requires_grad_(k in keys) for k, v in to_dtype(sd, dtype).items()}
    q0, q1, y, *_ = critic_parts(sd_t, _cast_batch(batch, dtype), policy_noise, noise_clip, activation)
    loss = torch.nn.functional.mse_loss(q0, y) + torch.nn.functional.mse_loss(q1, y)
    loss.backward()
    stats = dict(loss_sum=float(loss.detach()) * len(y), q0_sum=float(q0.detach().sum()), q1_sum=float(q1.detach().sum()))
    return {k: sd_t[k].grad for k in keys}, stats, torch.stack([q0.detach(), q1.detach()], dim=1), y


def actor_grad(sd, batch, activation="relu", dtype=torch.float64):
    """autograd in `dtype`: ({SB3 name: gradient} over the actor tensors, stats dict(loss_sum), a_pi [B, A], q0 [B])."""
    keys = actor_keys()
    sd_t = {k: v.requires_grad_(k in keys) for k, v in to_dtype(sd, dtype).items()}
    loss, a_pi, q0 = actor_loss(sd_t, _cast_batch(batch, dtype), activation)
    loss.backward()
    return {k: sd_t[k].grad for k in keys}, dict(loss_sum=float(loss.detach()) * len(q0)), a_pi.detach(), q0.detach()


# ---- the same gradients by hand: the cotangents the kernels form
def _mlp_forward(x, w, activation):
    """w: [(W [out][in], b)] x 3 -> (out, [x, h1, h2]) with the hidden activations kept"""
    f = _f(activation)
    h1 = f(torch.nn.functional.linear(x, *w[0]))
    h2 = f(torch.nn.functional.linear(h1, *w[1]))
    return torch.nn.functional.linear(h2, *w[2]), [x, h1, h2]


def _act_bwd(g, h, activation):
    return g * (h > 0).to(g.dtype) if activation == "relu" else g * (1.0 - h * h)


def _mlp_backward(dout, w, hs, activation, weights=True):
    """cotangent dout [B, out] -> ([(dW, db)] x 3 or None, dx [B, in])"""
    x, h1, h2 = hs
    dz2 = _act_bwd(dout @ w[2][0], h2, activation)
    dz1 = _act_bwd(dz2 @ w[1][0], h1, activation)
    grads = [(dz1.t() @ x, dz1.sum(0)), (dz2.t() @ h1, dz2.sum(0)), (dout.t() @ h2, dout.sum(0))] if weights else None
    return grads, dz1 @ w[0][0]


def _layers(sd, prefix, names):
    return [(sd[f"{prefix}.{k}.weight"], sd[f"{prefix}.{k}.bias"]) for k in names]


def critic_grad_by_hand(sd, batch, policy_noise=POLICY_NOISE, noise_clip=NOISE_CLIP, activation="relu", dtype=torch.float64):
    """{SB3 name: gradient} of critic_loss with the cotangent written out: dQ_i = 2 (Q_i - y) / n (the sum of two means of squares; no 1/2)."""
    sd_t, b = to_dtype(sd, dtype), _cast_batch(batch, dtype)
    y = critic_parts(sd_t, b, policy_noise, noise_clip, activation)[2]
    x, n, out = torch.cat([b["obs"], b["actions"]], dim=1), len(y), {}
    for i in range(2):
        w = _layers(sd_t, f"critic.qf{i}", (0, 2, 4))
        q, hs = _mlp_forward(x, w, activation)
        grads, _ = _mlp_backward((2.0 * (q.flatten() - y) / n)[:, None], w, hs, activation)
        for k, (dw, db) in zip((0, 2, 4), grads):
            out[f"critic.qf{i}.{k}.weight"], out[f"critic.qf{i}.{k}.bias"] = dw, db
    return out


def actor_grad_by_hand(sd, batch, activation="relu", dtype=torch.float64):
    """{SB3 name: gradient} of actor_loss: -1 / n into qf0 ALONE, its input gradient at the action columns (no critic weight gradient), times
    1 - a^2, then the actor's backward."""
    sd_t, b = to_dtype(sd, dtype), _cast_batch(batch, dtype)
    wa = _layers(sd_t, "actor", ACTOR_LAYERS)
    mu, hs_a = _mlp_forward(b["obs"], wa, activation)
    a = torch.tanh(mu)
    wq = _layers(sd_t, "critic.qf0", (0, 2, 4))
    q, hs_q = _mlp_forward(torch.cat([b["obs"], a], dim=1), wq, activation)
    n, D = len(q), b["obs"].shape[1]
    _, dx = _mlp_backward(torch.full_like(q, -1.0 / n), wq, hs_q, activation, weights=False)
    grads, _ = _mlp_backward(dx[:, D:] * (1.0 - a * a), wa, hs_a, activation)
    out = {}
    for k, (dw, db) in zip(ACTOR_LAYERS, grads):
        out[f"actor.{k}.weight"], out[f"actor.{k}.bias"] = dw, db
    return out


class Trainer:
    """TD3.train's gradient step in SB3's own order on leaf tensors of `dtype`, with two torch Adams (eps 1e-8), the delayed actor step and both
    polyak updates."""

    def __init__(self, sd, *, lr, tau, policy_delay, policy_noise, noise_clip, activation="relu", dtype=torch.float64, device="cpu"):
        self.sd = {k: v.detach().to(device, dtype).clone().requires_grad_("_target" not in k) for k, v in sd.items()}
        self.tau, self.delay, self.pn, self.clip, self.act, self.dtype = tau, policy_delay, policy_noise, noise_clip, activation, dtype
        self.opt_a = torch.optim.Adam([self.sd[k] for k in actor_keys()], lr=lr, eps=1e-8)
        self.opt_c = torch.optim.Adam([self.sd[k] for k in critic_keys()], lr=lr, eps=1e-8)
        self.n_updates = 0

    def step(self, batch):
        b = _cast_batch(batch, self.dtype)
        self.n_updates += 1
        loss_c = critic_loss(self.sd, b, self.pn, self.clip, self.act)
        self.opt_c.zero_grad()
        loss_c.backward()
        self.opt_c.step()
        loss_a = None
        if self.n_updates % self.delay == 0:
            loss_a, _, _ = actor_loss(self.sd, b, self.act)  # the critics AFTER their step
            self.opt_a.zero_grad()
            loss_a.backward()
            self.opt_a.step()
            with torch.no_grad():
                for k in critic_keys() + actor_keys():
                    t = self.sd[k.replace("critic.", "critic_target.", 1).replace("actor.", "actor_target.", 1)]
                    t.copy_(self.tau * self.sd[k] + (1.0 - self.tau) * t)
            loss_a = loss_a.detach()
        return loss_c.detach(), loss_a


# ---- the loop
def sb3_train_plan(n_updates, gradient_steps, policy_delay):
    """A literal loop of SB3's TD3.train: -> (per optimizer step: does the delayed block run, _n_updates afterwards)."""
    delayed = []
    for _ in range(gradient_steps):
        n_updates += 1
        # (sample; critic loss; critic optimizer step)
        if n_updates % policy_delay == 0:
            delayed.append(True)  # actor loss; actor optimizer step; polyak_update(critic); polyak_update(actor)
        else:
            delayed.append(False)
    return delayed, n_updates


def new_counters(**kw):
    c = dict(num_timesteps=0, n_calls=0, pos=0, full=False, draw=0, collect_step=0, critic_adam_step=0, actor_adam_step=0, n_updates=0)
    c.update(kw)
    return c


def iteration_events(c, n_iters, *, n_envs, capacity, train_freq, gradient_steps, learning_starts, policy_delay):
    """Generator over the calls of `n_iters` iterations, updating the counter dict `c` in place as tma_td3_iterations_local does:
    ("step", uniform, draw, pos) -> act + env step + replay add;  ("train", size, newest, draw, critic Adam step, actor Adam step or None)."""
    for _ in range(n_iters):
        for _ in range(train_freq):
            yield ("step", c["num_timesteps"] < learning_starts, c["collect_step"], c["pos"])
            c["collect_step"] += 1
            c["pos"] += 1
            if c["pos"] == capacity:
                c["pos"], c["full"] = 0, True
            c["num_timesteps"] += n_envs
            c["n_calls"] += 1
        if c["num_timesteps"] > learning_starts:
            for _ in range(train_freq if gradient_steps < 0 else gradient_steps):
                c["n_updates"] += 1
                size = capacity if c["full"] else c["pos"]
                delayed = c["n_updates"] % policy_delay == 0
                c["critic_adam_step"] += 1
                if delayed:
                    c["actor_adam_step"] += 1
                yield ("train", size, (c["pos"] - 1) % capacity, c["draw"], c["critic_adam_step"], c["actor_adam_step"] if delayed else None)
                c["draw"] += 1


# ---- weights and batches for the gradient tests
def make_sd(D, H, A, activation="relu", seed=0):
    """float32 SB3-named weights (torch's Linear init; the targets are nets of their own) with the heads rescaled FROM DATA (4096 randn rows,
    float64): both actors' mu to mean 0, std 1.2 (tanh(mu) comes within target_noise_clip of +-1 on many rows and stays away on many); every
    critic's Q to mean 0, std 1 (so either target wins the min)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in tensor_shapes(D, A, H).items():
        if len(shape) == 2:  # (a weight; its bias takes the same bound)
            bound = 1.0 / math.sqrt(shape[1])
            sd[k] = (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * bound
            sd[k.replace("weight", "bias")] = (torch.rand(shape[0], generator=g, dtype=torch.float64) * 2 - 1) * bound
    obs, acts = torch.randn(4096, D, generator=g, dtype=torch.float64), torch.rand(4096, A, generator=g, dtype=torch.float64) * 2 - 1

    def rescale(wk, bk, values, mean, std):  # values [B, out] of the head as it stands -> affine map of the head per column
        m, s = values.mean(dim=0), values.std(dim=0).clamp_min(1e-12)
        scale = std / s
        sd[wk] = sd[wk] * scale[:, None]
        sd[bk] = (sd[bk] - m) * scale + mean

    for prefix in ("actor", "actor_target"):
        rescale(f"{prefix}.mu.4.weight", f"{prefix}.mu.4.bias", actor_mu(sd, prefix, obs, activation), 0.0, 1.2)
    for prefix in ("critic", "critic_target"):
        for i in range(2):
            rescale(f"{prefix}.qf{i}.4.weight", f"{prefix}.qf{i}.4.bias", q_value(sd, prefix, i, obs, acts, activation)[:, None], 0.0, 1.0)
    return {k: v.to(torch.float32) for k, v in sd.items()}


def _row_screen(sd64, cand, policy_noise, noise_clip, activation):
    """Per candidate row (float64): ok mask, the ReLU-margin mask alone, and the class: (noise regime: 0 no column clipped / 1 some column at
    +clip / 2 some column at -clip, by the first clipped column; action regime: 0 no column clamped / 1 some column at +1 / 2 some at -1, by the
    first clamped column; which target wins at a')."""
    pre = []
    q0, q1, y, a_next, qt0, qt1, raw, mu = critic_parts(sd64, cand, policy_noise, noise_clip, activation, pre)
    actor_loss(sd64, cand, activation, pre)
    unclamped = torch.tanh(mu) + torch.clamp(raw, -noise_clip, noise_clip)
    ok = (qt0 - qt1).abs() >= Q_GAP
    ok &= ((raw.abs() - noise_clip).abs().min(dim=1).values >= EDGE_GAP) & ((unclamped.abs() - 1.0).abs().min(dim=1).values >= EDGE_GAP)
    relu_ok = torch.ones_like(ok)
    if activation == "relu":
        for z in pre:
            relu_ok &= z.abs().min(dim=1).values >= KINK_MARGIN

    def regime(v, bound):  # by the first column outside [-bound, bound]
        out = v.abs() > bound
        first = torch.argmax(out.to(torch.int64), dim=1)
        sign = torch.gather(v, 1, first[:, None]).flatten()
        return torch.where(out.any(dim=1), torch.where(sign > 0, 1, 2), 0)

    return ok & relu_ok, relu_ok, regime(raw, noise_clip), regime(unclamped, 1.0), (qt1 < qt0).long()


def wanted_classes(A, n):
    """The class of row i: the feasible (noise regime, action regime, target winner) triples in turn.  With one action column a row whose noise
    sits at +clip cannot be clamped at -1 (tanh > -1 and clip <= 1), nor the mirror image."""
    feasible = [(c, k, w) for w in range(2) for k in range(3) for c in range(3) if not (A == 1 and {c, k} == {1, 2})]
    return [feasible[i % len(feasible)] for i in range(n)], feasible


def make_batch(sd, D, A, n, activation="relu", seed=0, policy_noise=POLICY_NOISE, noise_clip=NOISE_CLIP):
    """n rows built by PER-ROW rejection on the float64 reference, no row ever skipped afterwards: row i is the next unused candidate of class
    wanted_classes(A, n)[i] that passes every screen of check_batch.  -> (batch, fraction of candidates the ReLU margin alone rejected).
    dones alternate in pairs; discounts alternate between 0.99^3 and 0.99."""
    g = torch.Generator().manual_seed(seed)
    sd64 = to_dtype(sd, torch.float64)
    want, _ = wanted_classes(A, n)
    pools: dict = {}
    rows = [None] * n
    missing = set(range(n))
    keys = ("obs", "actions", "next_obs", "noise", "rewards")
    seen = rejected = 0
    for _ in range(400):
        m = 4096
        cand = dict(obs=torch.randn(m, D, generator=g), actions=torch.rand(m, A, generator=g) * 2 - 1, next_obs=torch.randn(m, D, generator=g),
                    noise=torch.randn(m, A, generator=g), rewards=torch.randn(m, generator=g), dones=torch.zeros(m), discounts=torch.full((m,), 0.99))
        ok, relu_ok, c_reg, k_reg, win = _row_screen(sd64, _cast_batch(cand, torch.float64), policy_noise, noise_clip, activation)
        seen, rejected = seen + m, rejected + int((~relu_ok).sum())
        for j in torch.nonzero(ok).flatten().tolist():
            pools.setdefault((int(c_reg[j]), int(k_reg[j]), int(win[j])), []).append({k: cand[k][j] for k in keys})
        for i in sorted(missing):
            pool = pools.get(want[i])
            if pool:
                rows[i] = pool.pop(0)
                missing.discard(i)
        if not missing:
            break
    assert not missing, f"no candidate rows for classes {sorted({want[i] for i in missing})}"
    i = torch.arange(n)
    batch = {k: torch.stack([r[k] for r in rows]).contiguous() for k in keys}
    batch["dones"] = ((i // 2) % 2).to(torch.float32) if n > 1 else torch.zeros(1)
    batch["discounts"] = torch.where(i % 3 == 0, torch.tensor(0.99 ** 3), torch.tensor(0.99)).to(torch.float32)
    return batch, rejected / seen


def check_batch(sd, batch, activation="relu", policy_noise=POLICY_NOISE, noise_clip=NOISE_CLIP):
    """The properties the gradient tests assert FIRST, from the float64 reference, on every row: no hidden pre-activation of any of the six net
    passes (target actor on next_obs, the targets at a', the critics at a_replay, the actor on obs, qf0 at tanh(mu)) within KINK_MARGIN of 0
    (ReLU); |Qt0 - Qt1| >= 1e-3 at a'; no smoothing noise within 1e-3 of +-clip and no unclamped a' within 1e-3 of +-1.  And, as far as n rows can
    hold them: noise inside, at +clip and at -clip; a' inside, at +1 and at -1; both targets winning the min; dones 0 and 1; two discounts."""
    sd64, b = to_dtype(sd, torch.float64), _cast_batch(batch, torch.float64)
    ok, _, c_reg, k_reg, win = _row_screen(sd64, b, policy_noise, noise_clip, activation)
    assert bool(ok.all()), torch.nonzero(~ok).flatten().tolist()
    n, A = len(win), batch["actions"].shape[1]
    want, feasible = wanted_classes(A, n)
    got = list(zip(c_reg.tolist(), k_reg.tolist(), win.tolist()))
    assert got == want
    assert len(set(got)) == min(n, len(feasible))
    if n >= len(feasible):
        assert set(c_reg.tolist()) == {0, 1, 2} and set(k_reg.tolist()) == {0, 1, 2} and set(win.tolist()) == {0, 1}
        a_next = critic_parts(sd64, b, policy_noise, noise_clip, activation)[3]
        assert float(a_next.max()) == 1.0 and float(a_next.min()) == -1.0 and bool((a_next.abs() < 1.0).any())
    if n >= 3:
        assert set(batch["dones"].tolist()) == {0.0, 1.0}
    if n >= 2:
        assert len(set(batch["discounts"].tolist())) >= 2
    return got
