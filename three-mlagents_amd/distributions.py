"""The action distributions `HipActorCriticPolicy.get_distribution(obs)` returns, under the member names of SB3's
`stable_baselines3.common.distributions` (CategoricalDistribution / DiagGaussianDistribution): `.distribution` is the torch distribution built on
the head the device kernels computed (`HipActorCriticPolicy.head`: the logits of a Discrete policy, the mean of a Box policy), so everything a
loss does with it -- `torch.distributions.kl_divergence`, cross-entropies, probabilities -- is plain torch on device tensors, and its gradient
reaches the policy's flat parameter leaf through `head`'s autograd node (and, for log_std, through torch alone).

This is a few lines of torch arithmetic on n x act_dim numbers, not a hot path: the nets are the kernels'.
"""
from __future__ import annotations

import torch


class CategoricalDistribution:
    """SB3's CategoricalDistribution: Categorical(logits = action_net's output)."""

    def __init__(self, logits: torch.Tensor):
        self.action_dim = int(logits.shape[-1])
        self.distribution = torch.distributions.Categorical(logits=logits)

    def log_prob(self, actions: torch.Tensor) -> torch.Tensor:
        """actions: int32 (the rollout buffer's dtype) or int64 (SB3's), shape [n]"""
        return self.distribution.log_prob(actions.to(self.distribution.logits.device, torch.int64))

    def entropy(self) -> torch.Tensor:
        return self.distribution.entropy()

    def sample(self) -> torch.Tensor:
        return self.distribution.sample()

    def mode(self) -> torch.Tensor:
        return torch.argmax(self.distribution.probs, dim=1)

    def get_actions(self, deterministic: bool = False) -> torch.Tensor:
        return self.mode() if deterministic else self.sample()


class DiagGaussianDistribution:
    """SB3's DiagGaussianDistribution: Normal(mean, exp(log_std)) with a state-independent log_std; log_prob and entropy are summed over the
    action dimensions."""

    def __init__(self, mean: torch.Tensor, log_std: torch.Tensor):
        self.action_dim = int(mean.shape[-1])
        self.distribution = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp())

    def log_prob(self, actions: torch.Tensor) -> torch.Tensor:
        """actions: float32 [n, act_dim], unclipped (the rollout buffer's layout)"""
        mean = self.distribution.mean
        return self.distribution.log_prob(actions.to(mean.device, mean.dtype)).sum(dim=1)

    def entropy(self) -> torch.Tensor:
        return self.distribution.entropy().sum(dim=1)

    def sample(self) -> torch.Tensor:
        return self.distribution.rsample()

    def mode(self) -> torch.Tensor:
        return self.distribution.mean

    def get_actions(self, deterministic: bool = False) -> torch.Tensor:
        return self.mode() if deterministic else self.sample()
