"""torch / plain-Python restatement of csrc/tma_dqn.hip and of the loop of three_mlagents_amd/dqn.py (include/tma.h, ABI 225) -- TEST
INFRASTRUCTURE ONLY, importable without a GPU, float64-capable.

  * q_values: the Q forward of the `pi` segment (SB3's QNetwork features -> H -> H -> A) for ReLU / tanh, on SB3-named tensors
    (oracle.sb3_ref.KEYS[0:6], what HipActorCriticPolicy.state_dict() gives);
  * td_loss / td_grad: y = r + (1 - done) * discount * max_a Q_target(s', a) without gradient, mean smooth_l1(Q(s, a) - y), beta = 1, and its
    autograd gradient in SB3 names (the vf.* tensors get zeros);
  * linear_schedule / epsilon: SB3's get_linear_fn and the uniform warm-up below learning_starts;
  * iteration_events: the loop of one tma_dqn_iterations_local call as plain Python -- the calls in order, with the counters each one takes.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.sb3_ref import KEYS
from _relu_ref import KINK_MARGIN, clear_obs, preactivations  # noqa: F401  (re-exported: the ReLU screen of the online net)
from _replay_ref import egreedy  # noqa: F401

PI_KEYS = KEYS[:6]


def q_values(sd, obs, activation="relu"):
    f = {"tanh": torch.tanh, "relu": torch.relu}[activation]
    lin = torch.nn.functional.linear
    return lin(f(lin(f(lin(obs, sd[KEYS[0]], sd[KEYS[1]])), sd[KEYS[2]], sd[KEYS[3]])), sd[KEYS[4]], sd[KEYS[5]])


def td_parts(sd, target_sd, batch, activation="relu"):
    """(q_taken, y, delta) of a batch dict obs / actions / next_obs / dones / rewards / discounts (tensors of sd's dtype; actions integer)."""
    with torch.no_grad():
        nxt = q_values(target_sd, batch["next_obs"], activation).max(dim=1).values
        y = batch["rewards"] + (1.0 - batch["dones"]) * batch["discounts"] * nxt
    q = q_values(sd, batch["obs"], activation)
    q_taken = q.gather(1, batch["actions"].long()[:, None]).squeeze(1)
    return q_taken, y, q_taken - y


def td_loss(sd, target_sd, batch, activation="relu"):
    q_taken, y, _ = td_parts(sd, target_sd, batch, activation)
    return torch.nn.functional.smooth_l1_loss(q_taken, y)  # beta = 1, mean


def to_dtype(sd, dtype):
    return {k: v.detach().to(dtype).clone() for k, v in sd.items()}


def td_grad(sd, target_sd, batch, activation="relu", dtype=torch.float64):
    """float64 (or `dtype`) autograd: ({SB3 name: gradient} with zeros for every tensor outside the pi segment, loss, sum of Q taken)."""
    sd_t = {k: v.requires_grad_(k in PI_KEYS) for k, v in to_dtype(sd, dtype).items()}
    b = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in batch.items()}
    q_taken, y, _ = td_parts(sd_t, to_dtype(target_sd, dtype), b, activation)
    loss = torch.nn.functional.smooth_l1_loss(q_taken, y)
    loss.backward()
    grads = {k: (v.grad if k in PI_KEYS else torch.zeros_like(v)) for k, v in sd_t.items()}
    return grads, float(loss.detach()), float(q_taken.detach().sum())


# ---- the schedule (SB3 common/utils.py get_linear_fn; DQN._on_step / _sample_action)
def linear_schedule(progress_remaining, start, end, end_fraction):
    if (1 - progress_remaining) > end_fraction:
        return end
    return start + (1 - progress_remaining) * (end - start) / end_fraction


def epsilon(num_timesteps, total_timesteps, learning_starts, fraction, initial, final):
    """the exploration rate of the vector step taken at num_timesteps (taken BEFORE the step): 1 below learning_starts"""
    if num_timesteps < learning_starts:
        return 1.0
    return linear_schedule(1.0 - num_timesteps / total_timesteps, initial, final, fraction)


# ---- the loop
def new_counters(**kw):
    c = dict(num_timesteps=0, n_calls=0, pos=0, full=False, draw=0, collect_step=0, adam_step=0, n_updates=0)
    c.update(kw)
    return c


def iteration_events(c, n_iters, *, n_envs, capacity, train_freq, gradient_steps, learning_starts, target_update_interval, total_timesteps,
                     exploration_fraction, exploration_initial_eps, exploration_final_eps):
    """Generator over the calls of `n_iters` iterations, updating the counter dict `c` in place as tma_dqn_iterations_local does:
    ("step", eps, rng_step, pos) -> act + env step + replay add;  ("target",);  ("train", size, newest, draw, adam_step_index)."""
    every = max(target_update_interval // n_envs, 1)
    for _ in range(n_iters):
        for _ in range(train_freq):
            eps = epsilon(c["num_timesteps"], total_timesteps, learning_starts, exploration_fraction, exploration_initial_eps, exploration_final_eps)
            yield ("step", eps, c["collect_step"], c["pos"])
            c["collect_step"] += 1
            c["pos"] += 1
            if c["pos"] == capacity:
                c["pos"], c["full"] = 0, True
            c["num_timesteps"] += n_envs
            c["n_calls"] += 1
            if c["n_calls"] % every == 0:
                yield ("target",)
        if c["num_timesteps"] > learning_starts:
            for _ in range(train_freq if gradient_steps < 0 else gradient_steps):
                size = capacity if c["full"] else c["pos"]
                yield ("train", size, (c["pos"] - 1) % capacity, c["draw"], c["adam_step"] + 1)
                c["draw"] += 1
                c["adam_step"] += 1
                c["n_updates"] += 1


def count_events(n_iters, **kw):
    c = new_counters(**{k: kw.pop(k) for k in list(kw) if k in new_counters()})
    ev = list(iteration_events(c, n_iters, **kw))
    return c, sum(e[0] == "train" for e in ev), sum(e[0] == "target" for e in ev), ev


# ---- batches for the TD-gradient tests
def make_batch(sd, target_sd, obs, next_obs, A, activation, seed):
    """A batch on `obs` / `next_obs` (float32 CPU) whose float64 |delta| is 0.4 on even rows and 2.5 on odd ones, with both signs: actions walk
    the columns, dones alternate in pairs, discounts alternate between 0.99 and 0.99 ** 3, and the reward of a row is what puts its delta there
    (rounded to float32, which moves delta by one part in 10^7)."""
    n = obs.shape[0]
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(n)
    actions = ((i + int(torch.randint(0, A, (1,), generator=g))) % A).to(torch.int32)
    dones = ((i // 2) % 2).to(torch.float32) if n > 1 else torch.zeros(1)
    discounts = torch.where(i % 3 == 0, torch.tensor(0.99 ** 3), torch.tensor(0.99)).to(torch.float32)
    want = torch.where(i % 2 == 0, torch.tensor(0.4), torch.tensor(2.5)).double() * torch.where((i // 2) % 2 == 0, 1.0, -1.0).double()
    zero = dict(obs=obs.double(), next_obs=next_obs.double(), actions=actions, dones=dones.double(), rewards=torch.zeros(n, dtype=torch.float64),
                discounts=discounts.double())
    q_taken, y0, _ = td_parts(to_dtype(sd, torch.float64), to_dtype(target_sd, torch.float64), zero, activation)
    rewards = (q_taken.detach() - y0 - want).to(torch.float32)
    return dict(obs=obs, next_obs=next_obs, actions=actions, dones=dones, rewards=rewards, discounts=discounts)


def check_batch(sd, target_sd, batch, A, activation):
    """The properties the TD-gradient tests assert FIRST, from the float64 reference: no row within 1e-3 of the Huber kink; and, as far as n
    rows can hold them (n rows hold at most n distinct values), both Huber regimes, dones 0 and 1, two discounts, every action column."""
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    _, _, delta = td_parts(to_dtype(sd, torch.float64), to_dtype(target_sd, torch.float64), b64, activation)
    ad = delta.abs().detach().numpy()
    n = len(ad)
    assert np.all(np.abs(ad - 1.0) > 1e-3), ad
    if n >= 2:
        assert (ad < 1.0).any() and (ad > 1.0).any()
        assert len(set(batch["discounts"].tolist())) >= 2
    if n >= 3:
        assert set(batch["dones"].tolist()) == {0.0, 1.0}
    assert len(set(batch["actions"].tolist())) == min(n, A)
