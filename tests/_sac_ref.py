"""torch / plain-Python restatement of csrc/tma_sac.hip and of the loop of three_mlagents_amd/sac.py (include/tma.h, ABI 226) -- TEST
INFRASTRUCTURE ONLY, importable without a GPU, float64-capable, in SB3's names (stable_baselines3/sac/sac.py, SquashedDiagGaussianDistribution).

  * actor_head / squash / q_value: the actor (latent_pi -> mu, log_std), the squashed Gaussian with given noise, one critic over obs | action,
    for ReLU / tanh, on SB3-named tensors ([out][in] weights: what HipSACPolicy.state_dict() gives);
  * critic_loss / actor_loss / ent_coef_loss and their autograd gradients;
  * Trainer: one SAC.train gradient step in SB3's own order with three torch Adams and the polyak update;
  * iteration_events: the loop of one tma_sac_iterations_local call as plain Python;
  * make_sd / make_batch / check_batch: weights whose heads are scaled from data so that a batch can hold every regime, a batch built by per-row
    rejection on the float64 reference (the style of _relu_ref.clear_obs and _dqn_ref.check_batch), and the properties asserted first.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from _relu_ref import KINK_MARGIN  # noqa: F401  (the ReLU screen's margin)

LOG_STD_MIN, LOG_STD_MAX, EPS = -20.0, 2.0, 1e-6
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
ACTOR_LAYERS = ("latent_pi.0", "latent_pi.2", "mu", "log_std")
U_MAX, Q_GAP, CLAMP_GAP = 3.0, 1e-3, 1e-3


def _f(name):
    return {"tanh": torch.tanh, "relu": torch.relu}[name]


def actor_keys():
    return [f"actor.{layer}.{p}" for layer in ACTOR_LAYERS for p in ("weight", "bias")]


def critic_keys(prefix="critic"):
    return [f"{prefix}.qf{i}.{k}.{p}" for i in range(2) for k in (0, 2, 4) for p in ("weight", "bias")]


def tensor_shapes(D, A, H):
    """{SB3 name: shape} of the three nets."""
    out = {"actor.latent_pi.0.weight": (H, D), "actor.latent_pi.0.bias": (H,), "actor.latent_pi.2.weight": (H, H), "actor.latent_pi.2.bias": (H,),
           "actor.mu.weight": (A, H), "actor.mu.bias": (A,), "actor.log_std.weight": (A, H), "actor.log_std.bias": (A,)}
    for prefix in ("critic", "critic_target"):
        for i in range(2):
            out.update({f"{prefix}.qf{i}.0.weight": (H, D + A), f"{prefix}.qf{i}.0.bias": (H,), f"{prefix}.qf{i}.2.weight": (H, H),
                        f"{prefix}.qf{i}.2.bias": (H,), f"{prefix}.qf{i}.4.weight": (1, H), f"{prefix}.qf{i}.4.bias": (1,)})
    return out


def to_dtype(sd, dtype):
    return {k: v.detach().to(dtype).clone() for k, v in sd.items()}


# ---- the nets
def actor_head(sd, obs, activation="relu", pre=None):
    """-> (mu [B, A], log_std before the clamp [B, A]); `pre`: a list the two hidden pre-activations are appended to."""
    lin, f = torch.nn.functional.linear, _f(activation)
    z1 = lin(obs, sd["actor.latent_pi.0.weight"], sd["actor.latent_pi.0.bias"])
    z2 = lin(f(z1), sd["actor.latent_pi.2.weight"], sd["actor.latent_pi.2.bias"])
    if pre is not None:
        pre += [z1, z2]
    h = f(z2)
    return lin(h, sd["actor.mu.weight"], sd["actor.mu.bias"]), lin(h, sd["actor.log_std.weight"], sd["actor.log_std.bias"])


def squash(mu, log_std_raw, z):
    """-> (a, logp, u): ls = clamp(log_std, -20, 2); u = mu + exp(ls) z; a = tanh(u);
    logp = sum_j (-z_j^2 / 2 - ls_j - log sqrt(2 pi)) - sum_j log(1 - a_j^2 + 1e-6)."""
    ls = torch.clamp(log_std_raw, LOG_STD_MIN, LOG_STD_MAX)
    u = mu + torch.exp(ls) * z
    a = torch.tanh(u)
    logp = (-(z * z) * 0.5 - ls - HALF_LOG_2PI).sum(dim=1) - torch.log(1.0 - a * a + EPS).sum(dim=1)
    return a, logp, u


def q_value(sd, prefix, i, obs, actions, activation="relu", pre=None):
    """Q_i(obs, actions) [B] of `prefix` in ("critic", "critic_target"): SB3's ContinuousCritic on cat(obs, actions)."""
    lin, f = torch.nn.functional.linear, _f(activation)
    x = torch.cat([obs, actions], dim=1)
    z1 = lin(x, sd[f"{prefix}.qf{i}.0.weight"], sd[f"{prefix}.qf{i}.0.bias"])
    z2 = lin(f(z1), sd[f"{prefix}.qf{i}.2.weight"], sd[f"{prefix}.qf{i}.2.bias"])
    if pre is not None:
        pre += [z1, z2]
    return lin(f(z2), sd[f"{prefix}.qf{i}.4.weight"], sd[f"{prefix}.qf{i}.4.bias"]).flatten()


# ---- the losses (SAC.train)
def critic_parts(sd, batch, alpha, activation="relu", pre=None):
    """-> (q0, q1, y, logp_next, next_actions, qt0, qt1).  batch: obs, actions, next_obs, dones, rewards, discounts, noise_next."""
    with torch.no_grad():
        mu, ls = actor_head(sd, batch["next_obs"], activation, pre)
        a_next, logp_next, _ = squash(mu, ls, batch["noise_next"])
        qt0 = q_value(sd, "critic_target", 0, batch["next_obs"], a_next, activation, pre)
        qt1 = q_value(sd, "critic_target", 1, batch["next_obs"], a_next, activation, pre)
        y = batch["rewards"] + (1.0 - batch["dones"]) * batch["discounts"] * (torch.min(qt0, qt1) - alpha * logp_next)
    q0 = q_value(sd, "critic", 0, batch["obs"], batch["actions"], activation, pre)
    q1 = q_value(sd, "critic", 1, batch["obs"], batch["actions"], activation, pre)
    return q0, q1, y, logp_next, a_next, qt0, qt1


def critic_loss(sd, batch, alpha, activation="relu"):
    q0, q1, y, *_ = critic_parts(sd, batch, alpha, activation)
    return 0.5 * (torch.nn.functional.mse_loss(q0, y) + torch.nn.functional.mse_loss(q1, y))


def actor_parts(sd, batch, activation="relu", pre=None):
    """-> (a_pi, logp_pi, q0, q1, u) on batch obs / noise_pi."""
    mu, ls = actor_head(sd, batch["obs"], activation, pre)
    a_pi, logp_pi, u = squash(mu, ls, batch["noise_pi"])
    q0 = q_value(sd, "critic", 0, batch["obs"], a_pi, activation, pre)
    q1 = q_value(sd, "critic", 1, batch["obs"], a_pi, activation, pre)
    return a_pi, logp_pi, q0, q1, u


def actor_loss(sd, batch, alpha, activation="relu"):
    _, logp_pi, q0, q1, _ = actor_parts(sd, batch, activation)
    return (alpha * logp_pi - torch.min(q0, q1)).mean(), logp_pi


def ent_coef_loss(log_ent_coef, logp_pi, target_entropy):
    return -(log_ent_coef * (logp_pi.detach() + target_entropy)).mean()


def _cast_batch(batch, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in batch.items()}


def critic_grad(sd, batch, log_ent_coef, activation="relu", dtype=torch.float64):
    """autograd in `dtype`: ({SB3 name: gradient} over the critic tensors, stats dict(loss_sum, q0_sum, q1_sum), q [B, 2], y [B])."""
    keys = critic_keys()
    sd_t = {k: v.requires_grad_(k in keys) for k, v in to_dtype(sd, dtype).items()}
    b = _cast_batch(batch, dtype)
    alpha = torch.exp(torch.tensor(float(log_ent_coef), dtype=torch.float32)).to(dtype)  # the kernels' alpha: expf of the stored float
    q0, q1, y, *_ = critic_parts(sd_t, b, alpha, activation)
    loss = 0.5 * (torch.nn.functional.mse_loss(q0, y) + torch.nn.functional.mse_loss(q1, y))
    loss.backward()
    stats = dict(loss_sum=float(loss.detach()) * len(y), q0_sum=float(q0.detach().sum()), q1_sum=float(q1.detach().sum()))
    return {k: sd_t[k].grad for k in keys}, stats, torch.stack([q0.detach(), q1.detach()], dim=1), y


def actor_grad(sd, batch, log_ent_coef, activation="relu", dtype=torch.float64):
    """autograd in `dtype`: ({SB3 name: gradient} over the actor tensors, stats dict(loss_sum, logp_sum), a_pi, logp_pi)."""
    keys = actor_keys()
    sd_t = {k: v.requires_grad_(k in keys) for k, v in to_dtype(sd, dtype).items()}
    b = _cast_batch(batch, dtype)
    alpha = torch.exp(torch.tensor(float(log_ent_coef), dtype=torch.float32)).to(dtype)
    a_pi, logp_pi, q0, q1, _ = actor_parts(sd_t, b, activation)
    loss = (alpha * logp_pi - torch.min(q0, q1)).mean()
    loss.backward()
    stats = dict(loss_sum=float(loss.detach()) * len(logp_pi), logp_sum=float(logp_pi.detach().sum()))
    return {k: sd_t[k].grad for k in keys}, stats, a_pi.detach(), logp_pi.detach()


class Trainer:
    """SAC.train's gradient step in SB3's own order on leaf tensors of `dtype`, with three torch Adams (eps 1e-8) and the polyak update."""

    def __init__(self, sd, log_ent_coef, *, lr, tau, target_entropy, activation="relu", dtype=torch.float64, auto_ent=True, target_update_interval=1,
                 device="cpu"):
        self.sd = {k: v.detach().to(device, dtype).clone().requires_grad_(not k.startswith("critic_target")) for k, v in sd.items()}
        self.log_ent_coef = torch.tensor([float(log_ent_coef)], dtype=dtype, device=device, requires_grad=True)
        self.tau, self.te, self.act, self.dtype, self.auto, self.every = tau, target_entropy, activation, dtype, auto_ent, target_update_interval
        self.opt_a = torch.optim.Adam([self.sd[k] for k in actor_keys()], lr=lr, eps=1e-8)
        self.opt_c = torch.optim.Adam([self.sd[k] for k in critic_keys()], lr=lr, eps=1e-8)
        self.opt_e = torch.optim.Adam([self.log_ent_coef], lr=lr, eps=1e-8)
        self.n_updates = 0

    def step(self, batch):
        b = _cast_batch(batch, self.dtype)
        alpha = torch.exp(self.log_ent_coef.detach())[0]  # read before any step of this iteration
        loss_c = critic_loss(self.sd, b, alpha, self.act)
        self.opt_c.zero_grad()
        loss_c.backward()
        self.opt_c.step()
        loss_a, logp = actor_loss(self.sd, b, alpha, self.act)  # the critics AFTER their step
        self.opt_a.zero_grad()
        self.opt_c.zero_grad()
        loss_a.backward()
        self.opt_a.step()
        if self.auto:
            loss_e = ent_coef_loss(self.log_ent_coef, logp, self.te)
            self.opt_e.zero_grad()
            loss_e.backward()
            self.opt_e.step()
        if self.n_updates % self.every == 0:
            with torch.no_grad():
                for k in critic_keys():
                    t = self.sd[k.replace("critic.", "critic_target.", 1)]
                    t.copy_(self.tau * self.sd[k] + (1.0 - self.tau) * t)
        self.n_updates += 1
        return loss_c.detach(), loss_a.detach()


# ---- the loop
def new_counters(**kw):
    c = dict(num_timesteps=0, n_calls=0, pos=0, full=False, draw=0, collect_step=0, adam_step=0, n_updates=0)
    c.update(kw)
    return c


def iteration_events(c, n_iters, *, n_envs, capacity, train_freq, gradient_steps, learning_starts, target_update_interval):
    """Generator over the calls of `n_iters` iterations, updating the counter dict `c` in place as tma_sac_iterations_local does:
    ("step", uniform, draw, pos) -> act + env step + replay add;  ("train", size, newest, draw, adam_step_index, polyak)."""
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
                size = capacity if c["full"] else c["pos"]
                yield ("train", size, (c["pos"] - 1) % capacity, c["draw"], c["adam_step"] + 1, c["n_updates"] % target_update_interval == 0)
                c["draw"] += 1
                c["adam_step"] += 1
                c["n_updates"] += 1


# ---- weights and batches for the gradient tests
def make_sd(D, H, A, activation="relu", seed=0):
    """float32 SB3-named weights (torch's Linear init) with the heads rescaled FROM DATA (4096 randn rows, float64) so that a batch can hold
    every regime: column 0 of the log_std head spreads to mean -6, std 12 (rows leave the clamp on both sides), its other columns to mean -1.5,
    std 0.7; mu to mean 0, std 0.8; every critic's Q to mean 0, std 1 (so either critic wins the min)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in tensor_shapes(D, A, H).items():
        if len(shape) == 2:  # (a weight; its bias takes the same bound)
            bound = 1.0 / math.sqrt(shape[1])
            sd[k] = (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * bound
            sd[k.replace("weight", "bias")] = (torch.rand(shape[0], generator=g, dtype=torch.float64) * 2 - 1) * bound
    obs, act = torch.randn(4096, D, generator=g, dtype=torch.float64), torch.rand(4096, A, generator=g, dtype=torch.float64) * 2 - 1

    def rescale(wk, bk, values, mean, std):  # values [B, out] of the head as it stands -> affine map of the head per column
        m, s = values.mean(dim=0), values.std(dim=0).clamp_min(1e-12)
        scale = torch.as_tensor(std, dtype=torch.float64) / s
        sd[wk] = sd[wk] * scale[:, None]
        sd[bk] = (sd[bk] - m) * scale + torch.as_tensor(mean, dtype=torch.float64)

    mu, ls = actor_head(sd, obs, activation)
    rescale("actor.mu.weight", "actor.mu.bias", mu, [0.0] * A, [0.8] * A)
    rescale("actor.log_std.weight", "actor.log_std.bias", ls, [-6.0] + [-1.5] * (A - 1), [12.0] + [0.7] * (A - 1))
    for prefix in ("critic", "critic_target"):
        for i in range(2):
            q = q_value(sd, prefix, i, obs, act, activation)[:, None]
            rescale(f"{prefix}.qf{i}.4.weight", f"{prefix}.qf{i}.4.bias", q, [0.0], [1.0])
    return {k: v.to(torch.float32) for k, v in sd.items()}


def _row_screen(sd64, cand, log_ent_coef, activation):
    """Per candidate row (float64): ok mask and the class (clamp regime of log_std column 0 at obs: 0 inside / 1 above / 2 below; which critic
    wins at a_pi; which target wins at a')."""
    pre = []
    alpha = math.exp(log_ent_coef)
    q0, q1, y, _, _, qt0, qt1 = critic_parts(sd64, cand, alpha, activation, pre)
    _, _, p0, p1, u_pi = actor_parts(sd64, cand, activation, pre)
    mu_n, ls_n = actor_head(sd64, cand["next_obs"], activation)
    _, _, u_n = squash(mu_n, ls_n, cand["noise_next"])
    _, ls_o = actor_head(sd64, cand["obs"], activation)
    ok = (u_pi.abs().max(dim=1).values <= U_MAX) & (u_n.abs().max(dim=1).values <= U_MAX)
    ok &= ((p0 - p1).abs() >= Q_GAP) & ((qt0 - qt1).abs() >= Q_GAP)
    for ls in (ls_o, ls_n):
        ok &= ((ls - LOG_STD_MIN).abs().min(dim=1).values >= CLAMP_GAP) & ((ls - LOG_STD_MAX).abs().min(dim=1).values >= CLAMP_GAP)
    if activation == "relu":
        for z in pre:
            ok &= z.abs().min(dim=1).values >= KINK_MARGIN
    regime = torch.where(ls_o[:, 0] > LOG_STD_MAX, 1, torch.where(ls_o[:, 0] < LOG_STD_MIN, 2, 0))
    return ok, regime, (p1 < p0).long(), (qt1 < qt0).long()


def make_batch(sd, D, A, n, activation="relu", seed=0, log_ent_coef=0.0):
    """n rows built by PER-ROW rejection on the float64 reference, no row ever skipped afterwards: row i is the next unused candidate of class
    (i % 3, (i // 3) % 2, (i // 6) % 2) = (clamp regime, critic winning at a_pi, target winning at a') that passes every screen of check_batch.
    Noise is 0.5 randn (|u| <= 3 must hold at exp(2) as well); dones alternate in pairs; discounts alternate between 0.99^3 and 0.99."""
    g = torch.Generator().manual_seed(seed)
    sd64 = to_dtype(sd, torch.float64)
    want = [(i % 3, (i // 3) % 2, (i // 6) % 2) for i in range(n)]
    pools: dict = {}
    rows = [None] * n
    missing = set(range(n))
    keys = ("obs", "actions", "next_obs", "noise_next", "noise_pi", "rewards")
    for _ in range(400):
        m = 4096
        cand = dict(obs=torch.randn(m, D, generator=g), actions=torch.rand(m, A, generator=g) * 2 - 1, next_obs=torch.randn(m, D, generator=g),
                    noise_next=0.5 * torch.randn(m, A, generator=g), noise_pi=0.5 * torch.randn(m, A, generator=g), rewards=torch.randn(m, generator=g),
                    dones=torch.zeros(m), discounts=torch.full((m,), 0.99))
        ok, regime, win_pi, win_t = _row_screen(sd64, _cast_batch(cand, torch.float64), log_ent_coef, activation)
        for j in torch.nonzero(ok).flatten().tolist():
            pools.setdefault((int(regime[j]), int(win_pi[j]), int(win_t[j])), []).append({k: cand[k][j] for k in keys})
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
    return batch


def check_batch(sd, batch, activation="relu", log_ent_coef=0.0):
    """The properties the gradient tests assert FIRST, from the float64 reference, on every row: no hidden pre-activation of any of the five net
    passes (actor on obs and on next_obs, the critics at a_replay and at a_pi, the targets at a') within KINK_MARGIN of 0 (ReLU); |Q0 - Q1| >=
    1e-3 at a_pi and at a'; |u| <= 3; no log_std before the clamp within 1e-3 of -20 or 2.  And, as far as n rows can hold them: all three clamp
    regimes, dones 0 and 1, two discounts, both critics (and both targets) winning the min."""
    sd64, b = to_dtype(sd, torch.float64), _cast_batch(batch, torch.float64)
    ok, regime, win_pi, win_t = _row_screen(sd64, b, log_ent_coef, activation)
    assert bool(ok.all()), torch.nonzero(~ok).flatten().tolist()
    n = len(regime)
    assert len(set(regime.tolist())) == min(n, 3)
    if n >= 6:
        assert set(win_pi.tolist()) == {0, 1}
    if n >= 12:
        assert set(win_t.tolist()) == {0, 1}
    if n >= 3:
        assert set(batch["dones"].tolist()) == {0.0, 1.0}
    if n >= 2:
        assert len(set(batch["discounts"].tolist())) >= 2
    return dict(regime=np.asarray(regime), win_pi=np.asarray(win_pi), win_t=np.asarray(win_t))
