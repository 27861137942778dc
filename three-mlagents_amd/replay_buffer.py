"""SB3's `ReplayBuffer` / `NStepReplayBuffer` surface on device planes: the data half of an off-policy loop over the device environments.

The planes live in HBM and are written without a copy to the host (`add_step`: one tma_replay_add launch per vector step, taking the dict
`HipVecEnv.step_device` returns) and sampled as dense tensors in one launch (`sample`: tma_replay_sample, index draw and n-step returns
included).  `collect` strings Q-function -> epsilon-greedy pick (tma_egreedy_actions) -> env step -> add together with no host round trip.
The Q-network is the caller's: a Discrete `HipActorCriticPolicy.head(obs)[0]` is one on the engine's kernels (tools/dqn_example.py).
include/tma.h and csrc/tma_replay.hip hold the kernels' contracts, DESIGN.md section 16 the layout and the deviations from SB3:
  * Discrete actions are int32 `[B]`, scalars float32 `[B]` (not SB3's `[B, 1]` columns): the deviations rollout_buffer.py documents.
  * the index draw is the engine's counter-based hash of (seed, draw counter), not `np.random.randint`; with `n_envs > 1` the env index is
    drawn per sample, as SB3 does.
  * `terminated` and `truncated` are kept as two planes instead of SB3's `dones` and `timeouts`; `dones` of a sample is `terminated`.
  * `handle_timeout_termination=False` and `optimize_memory_usage=True` are not built (ValueError).
  * an n-step window ends at the write head instead of wrapping into older data, and `discounts` is gamma ** (steps included).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib

MAX_N_STEPS = 64  # csrc/tma_replay.hip REPLAY_MAX_N_STEP


class ReplayBufferSamples(NamedTuple):
    observations: torch.Tensor       # f32 [B, D]
    actions: torch.Tensor            # i32 [B] (Discrete) | f32 [B, A] (Box)
    next_observations: torch.Tensor  # f32 [B, D]
    dones: torch.Tensor              # f32 [B]: terminated (a time-out is not a done)
    rewards: torch.Tensor            # f32 [B]: the n-step discounted sum
    discounts: torch.Tensor          # f32 [B]: gamma ** (steps included), what the bootstrap term is scaled by


def _action_geometry(action_space) -> tuple[int, bool]:
    """(num_actions | act_dim, continuous) of a Discrete / Box space, of an int (Discrete) or of that pair itself."""
    if isinstance(action_space, tuple) and len(action_space) == 2:
        n, cont = int(action_space[0]), bool(action_space[1])
    elif isinstance(action_space, int):
        n, cont = action_space, False
    elif hasattr(action_space, "n"):
        n, cont = int(action_space.n), False
    elif getattr(action_space, "shape", None) is not None and len(action_space.shape) == 1:
        n, cont = int(action_space.shape[0]), True
    else:
        raise ValueError(f"action_space must be a Discrete or one-dimensional Box space, an int, or (n, continuous); got {action_space!r}")
    if n < 1:
        raise ValueError(f"the action space needs at least one action / dimension (got {n})")
    return n, cont


class ReplayBuffer:
    """SB3's `ReplayBuffer(buffer_size, observation_space, action_space, device, n_envs, ...)` with the observation space given by its width
    and, from SB3 2.7's `NStepReplayBuffer`, `n_steps` and `gamma`.  Rows: `max(buffer_size // n_envs, 1)`, as in SB3.

    `observations`, `next_observations`, `actions`, `rewards`, `terminated`, `truncated` are the planes themselves, `[rows, n_envs, ...]` device
    tensors; `pos` and `full` are SB3's.  The buffer owns `last_obs`, the observation the next action is chosen from: `start(obs)` sets it from a
    reset, every `add_step` replaces it with the stepped observation."""

    def __init__(self, buffer_size: int, obs_dim: int, action_space, device, n_envs: int = 1, handle_timeout_termination: bool = True,
                 n_steps: int = 1, gamma: float = 0.99, seed: int = 0, *, optimize_memory_usage: bool = False):
        if not handle_timeout_termination:
            raise ValueError("ReplayBuffer: handle_timeout_termination=False is not built (a time-out is never a done here)")
        if optimize_memory_usage:
            raise ValueError("ReplayBuffer: optimize_memory_usage=True is not built (next_observations is a plane of its own)")
        buffer_size, obs_dim, n_envs, n_steps = int(buffer_size), int(obs_dim), int(n_envs), int(n_steps)
        if buffer_size < 1 or n_envs < 1 or obs_dim < 1:
            raise ValueError(f"ReplayBuffer: buffer_size, obs_dim and n_envs must be at least 1 (got {buffer_size}, {obs_dim}, {n_envs})")
        if not 1 <= n_steps <= MAX_N_STEPS:
            raise ValueError(f"ReplayBuffer: n_steps must be in [1, {MAX_N_STEPS}] (got {n_steps})")
        self.act_dim, self.continuous = _action_geometry(action_space)
        self.buffer_size = max(buffer_size // n_envs, 1)
        if self.buffer_size * n_envs >= 1 << 31:
            raise ValueError(f"ReplayBuffer: rows * n_envs must be below 2^31 (got {self.buffer_size} x {n_envs})")
        self.obs_dim, self.n_envs, self.n_steps, self.gamma = obs_dim, n_envs, n_steps, float(gamma)
        self.seed = int(seed) & 0xFFFFFFFF
        self.device = torch.device(device)
        R, N, D, dev = self.buffer_size, n_envs, obs_dim, self.device
        self.observations = torch.zeros((R, N, D), dtype=torch.float32, device=dev)
        self.next_observations = torch.zeros((R, N, D), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((R, N, self.act_dim), dtype=torch.float32, device=dev) if self.continuous else torch.zeros((R, N), dtype=torch.int32, device=dev)
        self.rewards = torch.zeros((R, N), dtype=torch.float32, device=dev)
        self.terminated = torch.zeros((R, N), dtype=torch.uint8, device=dev)
        self.truncated = torch.zeros((R, N), dtype=torch.uint8, device=dev)
        self.last_obs = torch.zeros((N, D), dtype=torch.float32, device=dev)
        self._view = _lib.Replay(*(_lib.ptr(t) for t in (self.observations, self.next_observations, self.actions, self.rewards, self.terminated,
                                                         self.truncated)), R, N, D, self.act_dim, 1 if self.continuous else 0)
        self.device = self.last_obs.device  # (with its index: what the tensors handed in are compared against)
        self.pos, self.full = 0, False
        self._draw = 0          # sample(): one index draw per call
        self._collect_step = 0  # collect(): one epsilon-greedy coin per env and step

    # -- SB3's bookkeeping ----------------------------------------------------------------------
    def size(self) -> int:
        return self.buffer_size if self.full else self.pos

    def reset(self) -> None:
        self.pos, self.full = 0, False

    def _stream(self):
        return _lib.stream_ptr(self.device)

    def _rows(self, name: str, t, shape: tuple, dtype) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device:
            raise ValueError(f"{name} must be a {dtype} tensor of shape {list(shape)} on {self.device}, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))} on {getattr(t, 'device', None)}")
        return t.contiguous()

    def _actions(self, actions) -> torch.Tensor:
        if self.continuous:
            return self._rows("actions", actions, (self.n_envs, self.act_dim), torch.float32)
        if isinstance(actions, torch.Tensor) and actions.dtype == torch.int64:  # (what torch.argmax gives)
            actions = actions.to(torch.int32)
        return self._rows("actions", actions, (self.n_envs,), torch.int32)

    def _flags(self, name: str, t) -> torch.Tensor:
        if isinstance(t, torch.Tensor) and t.dtype == torch.bool:
            t = t.view(torch.uint8)
        return self._rows(name, t, (self.n_envs,), torch.uint8)

    # -- writing -----------------------------------------------------------------------------------
    def start(self, obs: torch.Tensor) -> torch.Tensor:
        """Copy a reset observation `[n_envs, obs_dim]` into the owned `last_obs` (the env's own tensor may be overwritten by its next step)."""
        self.last_obs.copy_(self._rows("obs", obs, (self.n_envs, self.obs_dim), torch.float32))
        return self.last_obs

    def _add(self, actions, step_obs, rewards, term, trunc, term_obs) -> None:
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tma_replay_add(C.byref(self._view), self.pos, _lib.ptr(self.last_obs), _lib.ptr(actions), _lib.ptr(step_obs),
                                                 _lib.ptr(rewards), _lib.ptr(term), _lib.ptr(trunc), _lib.ptr(term_obs), self._stream()))
        self.pos += 1
        if self.pos == self.buffer_size:
            self.pos, self.full = 0, True

    def add_step(self, actions: torch.Tensor, out: dict) -> None:
        """Store one vector step: `actions` chosen from `last_obs`, `out` the dict `step_device(actions)` returned for it (n_steps = 1: `obs`,
        `rew`, `term`, `trunc`, `term_obs` with a leading axis of one).  One launch; `last_obs` becomes the stepped observation."""
        N, D = self.n_envs, self.obs_dim
        self._add(self._actions(actions), self._rows("out['obs']", out["obs"], (1, N, D), torch.float32),
                  self._rows("out['rew']", out["rew"], (1, N), torch.float32), self._rows("out['term']", out["term"], (1, N), torch.uint8),
                  self._rows("out['trunc']", out["trunc"], (1, N), torch.uint8), self._rows("out['term_obs']", out["term_obs"], (1, N, D), torch.float32))

    def add(self, obs, next_obs, actions, rewards, terminated, truncated) -> None:
        """SB3's `add` for callers with tensors of their own: `next_obs` is stored as given (the caller has put the terminal observation where
        an episode ended).  `last_obs` is set to `obs` and leaves as `next_obs`."""
        N, D = self.n_envs, self.obs_dim
        args = (self._actions(actions), self._rows("next_obs", next_obs, (N, D), torch.float32), self._rows("rewards", rewards, (N,), torch.float32),
                self._flags("terminated", terminated), self._flags("truncated", truncated))
        self.start(obs)
        self._add(*args, None)

    def collect(self, env, q_fn, n_steps: int, eps: float) -> None:
        """`n_steps` vector steps of epsilon-greedy data collection: per step `q_fn(last_obs)` -> f32 [n_envs, num_actions], tma_egreedy_actions,
        `env.step_device`, `add_step`.  Nothing synchronises with the host.  Call `start(env.reset_device())` first.  The coin of env i at this
        buffer's k-th collected step is counter (seed, env.engine.env_offset + i, k)."""
        if self.continuous:
            raise ValueError("collect: epsilon-greedy needs a Discrete buffer")
        if not 2 <= self.act_dim <= 16:
            raise ValueError(f"collect: tma_egreedy_actions covers 2 to 16 actions (got {self.act_dim})")
        eps = float(eps)
        if not 0.0 <= eps <= 1.0:
            raise ValueError(f"collect: eps must be in [0, 1] (got {eps})")
        L, N = _lib.lib(), self.n_envs
        offset = int(getattr(getattr(env, "engine", None), "env_offset", 0)) & 0xFFFFFFFF
        actions = torch.empty((N,), dtype=torch.int32, device=self.device)
        for _ in range(int(n_steps)):
            with torch.no_grad():
                q = self._rows("q_fn(last_obs)", q_fn(self.last_obs), (N, self.act_dim), torch.float32)
            with torch.cuda.device(self.device):
                _lib.check(L.tma_egreedy_actions(_lib.ptr(q), N, self.act_dim, eps, self.seed, self._collect_step & 0xFFFFFFFF, offset, _lib.ptr(actions),
                                                 self._stream()))
            self._collect_step += 1
            self.add_step(actions, env.step_device(actions))

    # -- sampling ----------------------------------------------------------------------------------
    def sample(self, batch_size: int, *, return_indices: bool = False):
        """`ReplayBufferSamples` of `batch_size` transitions drawn with replacement, fresh device tensors from one tma_replay_sample launch on
        the current stream; every call advances the draw counter, so equal seeds and call sequences give equal batches.  With
        `return_indices` the result is `(samples, rows, envs)`, int32 `[B]` each.  ValueError: an empty buffer, batch_size < 1."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f"ReplayBuffer.sample: batch_size must be at least 1 (got {batch_size})")
        size = self.size()
        if size < 1:
            raise ValueError("ReplayBuffer.sample: the buffer is empty")
        B, dev, f32 = batch_size, self.device, torch.float32
        out = ReplayBufferSamples(
            torch.empty((B, self.obs_dim), dtype=f32, device=dev),
            torch.empty((B, self.act_dim), dtype=f32, device=dev) if self.continuous else torch.empty((B,), dtype=torch.int32, device=dev),
            torch.empty((B, self.obs_dim), dtype=f32, device=dev), *(torch.empty((B,), dtype=f32, device=dev) for _ in range(3)))
        idx = tuple(torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(2)) if return_indices else (None, None)
        newest = (self.pos - 1) % self.buffer_size
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tma_replay_sample(C.byref(self._view), size, newest, self.n_steps, self.gamma, self.seed, self._draw & 0xFFFFFFFF, B,
                                                    *(_lib.ptr(t) for t in out), _lib.ptr(idx[0]), _lib.ptr(idx[1]), self._stream()))
        self._draw += 1
        return (out, *idx) if return_indices else out
