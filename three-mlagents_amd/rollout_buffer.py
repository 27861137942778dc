"""SB3's `RolloutBuffer` surface on the engine's device planes: `model.rollout_buffer.get(batch_size)`.

The native update (PPO.train / A2C.train) never forms a minibatch in memory: its gradient kernels gather their rows themselves.  A caller who
writes the update in torch -- a loss on the differentiable `policy.evaluate_actions` / `get_distribution`, stepped by a torch optimizer on
`policy.parameters()` -- needs the rows, and needs the ones the engine's own epoch would have used.  `get` yields them: one
`tma_rollout_gather` launch (include/tma.h, csrc/tma_gather.hip) per minibatch, in the order of the on-device permutation the gradient
kernels evaluate.

Deviations from SB3's buffer:
  * `episode_starts` is not kept: the engine's GAE (tma_gae_flags) works from the `terminated` / `truncated` planes, which are exposed instead.
  * Discrete actions are int32 `[B]` -- what `evaluate_actions` takes -- not SB3's float `[B, 1]` column; Box actions are float32 `[B, A]`.
  * the minibatch order is the engine's counter-based permutation of (perm_seed, perm_epoch), not `np.random.permutation`.
  * the attributes are views of the engine's planes (no copies), float32 / int32 / uint8 device tensors, not numpy arrays.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib


def perm_seed(seed: int) -> int:
    """Key of the minibatch permutation of a model seeded with `seed`: what PPO.train hands the native epoch calls and `RolloutBuffer.get`
    hands tma_rollout_gather (the permutation itself: include/tma.h tma_ppo_permutation)."""
    return (int(seed) * 2654435761 + 12345) & 0xFFFFFFFF


class RolloutBufferSamples(NamedTuple):
    observations: torch.Tensor  # f32 [B, D]
    actions: torch.Tensor       # i32 [B] (Discrete) | f32 [B, A] (Box)
    old_values: torch.Tensor    # f32 [B]
    old_log_prob: torch.Tensor  # f32 [B]
    advantages: torch.Tensor    # f32 [B]
    returns: torch.Tensor       # f32 [B]


class RolloutBuffer:
    """`model.rollout_buffer` of a PPO / A2C model: SB3-shaped views of the planes the native rollout driver fills, and `get`.

    Under VecNormalize the planes hold normalised observations and rewards, as the native update sees them.  `full` is True after a complete
    `collect_rollouts()` and False after one a callback interrupted (and before the first).  `episode_starts` is not kept (module docstring).
    """

    def __init__(self, model):
        self._model = model
        self.full = False

    # -- SB3's attributes: views, not copies ---------------------------------------------------
    @property
    def buffer_size(self) -> int:
        return self._model.n_steps

    @property
    def n_envs(self) -> int:
        return self._model.n_envs

    @property
    def observations(self) -> torch.Tensor:  # [T, N, D]: the first T slots of the engine's [T + 1, N, D] plane (slot T is the final new_obs)
        return self._model.buf["obs"][: self._model.n_steps]

    @property
    def actions(self) -> torch.Tensor:  # [T, N] int32 | [T, N, A] float32
        return self._model.buf["actions"]

    @property
    def rewards(self) -> torch.Tensor:  # [T, N], timeout bootstrap applied
        return self._model.buf["rewards"]

    @property
    def values(self) -> torch.Tensor:
        return self._model.buf["values"]

    @property
    def log_probs(self) -> torch.Tensor:
        return self._model.buf["log_probs"]

    @property
    def advantages(self) -> torch.Tensor:
        return self._model.buf["advantages"]

    @property
    def returns(self) -> torch.Tensor:
        return self._model.buf["returns"]

    @property
    def terminated(self) -> torch.Tensor:  # [T, N] uint8
        return self._model.buf["terminated"]

    @property
    def truncated(self) -> torch.Tensor:
        return self._model.buf["truncated"]

    # -- RolloutBuffer.get ------------------------------------------------------------------
    def get(self, batch_size: int | None = None, *, perm_epoch: int | None = None):
        """Generator over the minibatches of one pass: ceil(T*N / batch_size) `RolloutBufferSamples` of fresh device tensors (the last one short
        when batch_size does not divide T*N; None: one sample of everything), each from one tma_rollout_gather launch on the current stream.

        The pass is permutation (perm_seed(model.seed), perm_epoch).  perm_epoch defaults to the model's epoch counter, read when the pass
        starts, and a pass that runs to its end advances the counter by one: n passes see the minibatches of the n epochs the next train()
        would have run, in their order, and train() then goes on with fresh permutations.  A pass that is abandoned (a target_kl early stop)
        does not advance it; an explicit perm_epoch leaves it alone.  Raises ValueError when the buffer is not full or batch_size < 1."""
        m = self._model
        total = m.n_steps * m.n_envs
        if not self.full:
            raise ValueError("rollout_buffer.get: the buffer is not full (call collect_rollouts() first; a rollout a callback interrupted does not fill it)")
        if batch_size is None:
            batch_size = total
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f"rollout_buffer.get: batch_size must be at least 1 (got {batch_size})")
        return self._passes(batch_size, total, perm_epoch)

    def _passes(self, batch_size: int, total: int, perm_epoch):
        m, L = self._model, _lib.lib()
        pol, b, dev = m.policy, m.buf, m.device
        epoch = m._epoch_counter if perm_epoch is None else int(perm_epoch)
        seed = perm_seed(m.seed)
        D, A = pol.dims.obs_dim, pol.dims.act_dim
        for start in range(0, total, batch_size):
            n = min(batch_size, total - start)
            out = RolloutBufferSamples(
                torch.empty((n, D), dtype=torch.float32, device=dev),
                torch.empty((n, A), dtype=torch.float32, device=dev) if pol.dims.continuous else torch.empty((n,), dtype=torch.int32, device=dev),
                *(torch.empty((n,), dtype=torch.float32, device=dev) for _ in range(4)))
            mb = _lib.Minibatch(None, seed, epoch & 0xFFFFFFFF, start, n, 0, 0)
            _lib.check(L.tma_rollout_gather(C.byref(m._rollout_view), _lib.ptr(b["values"]), C.byref(pol.dims), C.byref(mb), *(_lib.ptr(t) for t in out),
                                            m._stream()))
            yield out
        if perm_epoch is None:
            m._epoch_counter += 1
