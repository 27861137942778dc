"""Restatement of the Stable-Baselines3 2.9 pieces A2C adds to the PPO half (oracle/sb3_ref.py) -- TEST INFRASTRUCTURE ONLY.

stable-baselines3 is not installable here, so what the HIP kernels are compared with is restated from the published algorithm:
  * `rmsprop_tflike`: clip_grad_norm_ + RMSpropTFLike.step() on one flat parameter vector, float64 numpy (tests/test_a2c_cpu.py checks it against
    the literal torch sequence of RMSpropTFLike.step);
  * `a2c_loss`: the loss of A2C.train();
  * `RefA2C`: torch f32 autograd of that loss + clip_grad_norm_ + the literal RMSpropTFLike sequence, per SB3-named parameter.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import sb3_ref

ALPHA, EPS, LR, MAX_GRAD_NORM = 0.99, 1e-5, 7e-4, 0.5  # SB3's A2C defaults


def clip_coef(grad, max_norm):
    """torch.nn.utils.clip_grad_norm_: (total norm, min(1, max_norm / (norm + 1e-6))), float64."""
    norm = float(np.sqrt(np.sum(np.asarray(grad, np.float64) ** 2)))
    return norm, min(1.0, float(max_norm) / (norm + 1e-6))


def rmsprop_tflike(p, g, square_avg, *, lr=LR, alpha=ALPHA, eps=EPS, max_norm=MAX_GRAD_NORM, grad_scale=1.0):
    """One step in float64: -> (p', square_avg', norm).  State starts at ONES (the caller's business); eps INSIDE the root."""
    p, g, sq = (np.asarray(x, np.float64) for x in (p, g, square_avg))
    g = g * float(grad_scale)
    norm, coef = clip_coef(g, max_norm)
    g = g * coef
    sq = alpha * sq + (1.0 - alpha) * g * g
    return p - lr * g / np.sqrt(sq + eps), sq, norm


def torch_rmsprop_tflike_(p: torch.Tensor, g: torch.Tensor, square_avg: torch.Tensor, *, lr=LR, alpha=ALPHA, eps=EPS) -> None:
    """The literal sequence of RMSpropTFLike.step() (no weight decay, momentum or centering), in place, in the tensors' dtype."""
    square_avg.mul_(alpha).addcmul_(g, g, value=1 - alpha)
    avg = square_avg.add(eps).sqrt_()
    p.addcdiv_(g, avg, value=-lr)


def a2c_loss(sd, obs, actions, advantages, returns, *, ent_coef=0.0, vf_coef=0.5, normalize_advantage=False):
    """A2C.train(): -> (loss, dict of the three logged losses)."""
    values, log_prob, entropy = sb3_ref.evaluate_actions(sd, obs, actions)
    adv = advantages
    if normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    policy_loss = -(adv * log_prob).mean()
    value_loss = torch.nn.functional.mse_loss(returns, values)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    return loss, dict(policy_loss=float(policy_loss.detach()), value_loss=float(value_loss.detach()), entropy_loss=float(entropy_loss.detach()))


class RefA2C:
    """Parameters + RMSpropTFLike(lr, alpha, eps) + clip_grad_norm_(max_grad_norm) as A2C.train applies them (torch f32)."""

    def __init__(self, sd, lr=LR, max_grad_norm=MAX_GRAD_NORM, alpha=ALPHA, eps=EPS):
        self.sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        self.square_avg = {k: torch.ones_like(v) for k, v in sd.items()}
        self.lr, self.max_grad_norm, self.alpha, self.eps = lr, max_grad_norm, alpha, eps

    def step(self, obs, actions, advantages, returns, **hp):
        loss, stats = a2c_loss(self.sd, obs, actions, advantages, returns, **hp)
        for v in self.sd.values():
            v.grad = None
        loss.backward()
        grads = {k: v.grad.clone() for k, v in self.sd.items()}
        stats["grad_norm"] = float(torch.nn.utils.clip_grad_norm_(list(self.sd.values()), self.max_grad_norm))
        with torch.no_grad():
            for k, v in self.sd.items():
                torch_rmsprop_tflike_(v, v.grad, self.square_avg[k], lr=self.lr, alpha=self.alpha, eps=self.eps)
        return stats, grads
