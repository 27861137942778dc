"""What the off-policy classes (dqn.py, sac.py, td3.py) share: the constructor's common arguments and refusals, the counters a native iteration call
hands back, the frame of `_run_iterations`, the one `learn()` and the replay-buffer files.  A class adds its nets, its `_setup_model`, the four
hooks `_hparams`, `_counters`, `_native_iterations` and `pop_train_stats`, and `train` / `predict` / `save` / `load`."""
from __future__ import annotations

import collections
import json
import time

import numpy as np
import torch

from . import _lib
from .ppo import PPO
from .replay_buffer import ReplayBuffer

ADAM_EPS = 1e-8          # torch.optim.Adam's default, which SB3's DQN, SAC and TD3 policies use
NATIVE_ITERATIONS = 256  # iterations per tma_*_iterations_local call of a learn() without a callback (the episode log is popped in between)


def pol_space(model, name: str):
    """The model's observation / action space, or the one its policy's shape implies (a model loaded without an env)."""
    from .spaces import Box, Discrete

    space = getattr(model, name, None) or getattr(model.env, name, None)
    if space is not None:
        return space
    return Box(-np.inf, np.inf, (model.policy.obs_dim,), np.float32) if name == "observation_space" else Discrete(model.policy.act_dim)


class OffPolicyAlgorithm(PPO):
    """An SB3-shaped off-policy algorithm whose iterations (collect train_freq vector steps into the replay ring, then gradient_steps optimizer
    steps) the library issues natively.  `ALGORITHM` names the class in messages; `ADAM_COUNTERS` maps its optimizer-step attributes to the
    fields of its counters struct."""

    ADAM_COUNTERS = {"_adam_step": "adam_step"}

    def __init__(self, policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq, gradient_steps, optimize_memory_usage,
                 n_steps, target_update_interval, stats_window_size, tensorboard_log, policy_kwargs, verbose, seed, _init_setup_model):
        """The arguments the three constructors share (target_update_interval None: the class has none).  A class checks and stores its own
        arguments first: this ends in `_setup_model()`."""
        from . import dist as _dist

        name = self.ALGORITHM.upper()
        if policy not in ("MlpPolicy", "MultiInputPolicy"):
            raise ValueError(f"three-mlagents_amd {name} supports MlpPolicy (vector observations), got '{policy}'")
        if callable(learning_rate):
            raise ValueError("schedules are not supported: pass a constant learning_rate (the reference does)")
        if isinstance(train_freq, (tuple, list)):
            if len(train_freq) != 2 or str(train_freq[1]) != "step":
                raise ValueError(f"train_freq per episode is not supported: pass a number of steps (got {train_freq!r})")
            train_freq = train_freq[0]
        if optimize_memory_usage:
            raise ValueError("optimize_memory_usage=True is not built (next_observations is a plane of its own)")
        sizes = [int(train_freq), int(batch_size), int(buffer_size)] + ([] if target_update_interval is None else [int(target_update_interval)])
        if min(sizes) < 1 or int(learning_starts) < 0:
            listed = "train_freq, batch_size and buffer_size" if target_update_interval is None else "train_freq, batch_size, target_update_interval and buffer_size"
            raise ValueError(f"{listed} must be at least 1, learning_starts at least 0")
        if int(gradient_steps) == 0 or int(gradient_steps) < -1:
            raise ValueError(f"gradient_steps must be at least 1, or -1 for as many as the vector steps collected (got {gradient_steps})")
        if not 0.0 < float(tau) <= 1.0:
            raise ValueError(f"tau must be in (0, 1] (got {tau})")
        self.policy_class, self.env = policy, env
        self.stats_window_size = int(stats_window_size) if stats_window_size else 0
        self._ep_info_r = collections.deque(maxlen=max(self.stats_window_size, 1))
        self._ep_info_l = collections.deque(maxlen=max(self.stats_window_size, 1))
        self.learning_rate, self.buffer_size, self.learning_starts, self.batch_size = float(learning_rate), int(buffer_size), int(learning_starts), int(batch_size)
        self.tau, self.gamma, self.train_freq, self.gradient_steps, self.n_steps = float(tau), float(gamma), int(train_freq), int(gradient_steps), int(n_steps)
        self.optimize_memory_usage = False
        if target_update_interval is not None:
            self.target_update_interval = int(target_update_interval)
        self.policy_kwargs = dict(policy_kwargs or {})
        self.tensorboard_log, self.verbose = tensorboard_log, int(verbose)
        self.seed = 0 if seed is None else int(seed)
        self.num_timesteps = self._n_updates = self._n_calls = self._total_timesteps = 0
        for attr in self.ADAM_COUNTERS:
            setattr(self, attr, 0)
        self.logger_values: dict[str, float] = {}
        self.policy = None
        self.replay_buffer: ReplayBuffer | None = None
        self._last_obs_valid = False
        self._native_comm = None
        self.world_size, self.rank = _dist.world_size(), _dist.rank()
        if env is not None and _init_setup_model:
            self._setup_model()

    # -- the native loop --------------------------------------------------------------------
    def _take_counters(self, c) -> None:
        rb = self.replay_buffer
        self.num_timesteps, self._n_calls, self._n_updates = int(c.num_timesteps), int(c.n_calls), int(c.n_updates)
        for attr, field in self.ADAM_COUNTERS.items():
            setattr(self, attr, int(getattr(c, field)))
        rb.pos, rb.full = int(c.pos), bool(c.full)
        rb._draw += (int(c.draw) - rb._draw) & 0xFFFFFFFF            # (the 32-bit counters wrap; the host ones do not)
        rb._collect_step += (int(c.collect_step) - rb._collect_step) & 0xFFFFFFFF

    def _run_iterations(self, n_iters: int) -> None:
        if not self._last_obs_valid:
            self.replay_buffer.start(self.env.reset_device())
            self._last_obs_valid = True
        c, hp = self._counters(), self._hparams()
        with torch.cuda.device(self.device):
            _lib.check(self._native_iterations(hp, c, int(n_iters)))
        self._take_counters(c)
        self._mark_update_done()

    def _log_row(self, common: dict) -> dict:
        """The log row of a class from the keys every class logs: here with the losses of the last optimizer step behind them."""
        return {**common, **(self.pop_train_stats() if self._n_updates > 0 else {})}

    def learn(self, total_timesteps: int, callback=None, log_interval: int = 4, tb_log_name: str | None = None, reset_num_timesteps: bool = True,
              progress_bar: bool = False):
        """SB3's learn.  Without a callback the iterations run in native calls of up to NATIVE_ITERATIONS; after each call the episode log is
        popped and a log row is dumped once at least `log_interval` episodes have finished since the last row (SB3 dumps at that episode).  With a
        callback: one iteration per native call, its train_freq vector steps reported through callbacks.BaseCallback.on_steps afterwards -- a
        callback that stops training does so at the end of the iteration, whose steps the envs have taken."""
        from .callbacks import as_callback

        cb = as_callback(callback)
        if reset_num_timesteps:
            self.num_timesteps = 0
        else:
            total_timesteps = int(total_timesteps) + self.num_timesteps
        self._total_timesteps = int(total_timesteps)
        eng, N = self.env.engine, self.n_envs
        per_iter = self.train_freq * N
        if getattr(eng, "_log_cap", 0) == 0:
            eng.episode_log(max(4096, 2 * NATIVE_ITERATIONS * per_iter))
        cb.init_callback(self)
        cb.on_training_start(locals(), globals())
        t0 = t_prev = time.time()
        episodes = since_row = 0
        first_timestep = self.num_timesteps
        try:
            while self.num_timesteps < total_timesteps:
                remaining = -(-(total_timesteps - self.num_timesteps) // per_iter)
                n = 1 if callback is not None else min(remaining, NATIVE_ITERATIONS)
                cb.on_rollout_start()
                start = self.num_timesteps
                self._run_iterations(n)
                keep_going = True
                if callback is not None:
                    end, self.num_timesteps = self.num_timesteps, start
                    _, keep_going = cb.on_steps(self.train_freq, N)
                    self.num_timesteps = end
                cb.on_rollout_end()
                cb.on_update_queued()
                r, l, e, seen = eng.pop_episode_log()
                s_ret, s_len, cnt = float(np.sum(r)), float(np.sum(l)), len(r)
                window = self._episode_window(r, l, s_ret, s_len, cnt)
                episodes += seen
                since_row += seen
                now = time.time()
                self._write_monitor(s_ret, s_len, cnt, t_prev - t0, now - t0, t0, log=(r, l, e, seen))
                t_prev = now
                if log_interval and since_row >= log_interval:
                    since_row = 0
                    stats = self._log_row({"rollout/ep_rew_mean": window[0], "rollout/ep_len_mean": window[1], "train/n_updates": self._n_updates,
                                           "train/learning_rate": self.learning_rate, "time/episodes": episodes,
                                           "time/fps": (self.num_timesteps - first_timestep) / max(now - t0, 1e-9), "time/time_elapsed": now - t0,
                                           "time/total_timesteps": self.num_timesteps})
                    self.logger_values = stats
                    self._write_progress(stats, self.num_timesteps)
                    if self.verbose >= 1:
                        print(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in stats.items()}), flush=True)
                if not keep_going:
                    break
        except BaseException:
            self._join_monitor_writer(reraise=False)
            flush = getattr(cb, "flush", None)
            if callable(flush):
                try:
                    flush()
                except Exception:  # noqa: BLE001 -- never mask the exception that is unwinding
                    pass
            raise
        self._join_monitor_writer()
        cb.on_training_end()
        return self

    # -- the replay buffer's files ------------------------------------------------------------
    def save_replay_buffer(self, path) -> None:
        """SB3's save_replay_buffer: the planes, the ring position and `last_obs` (torch.save; SB3 pickles its buffer object)."""
        rb = self.replay_buffer
        torch.save({"observations": rb.observations.cpu(), "next_observations": rb.next_observations.cpu(), "actions": rb.actions.cpu(),
                    "rewards": rb.rewards.cpu(), "terminated": rb.terminated.cpu(), "truncated": rb.truncated.cpu(), "last_obs": rb.last_obs.cpu(),
                    "pos": rb.pos, "full": bool(rb.full), "last_obs_valid": bool(self._last_obs_valid)}, str(path))

    def load_replay_buffer(self, path) -> None:
        """SB3's load_replay_buffer, for a file save_replay_buffer wrote for a buffer of the same geometry.  Where the model was loaded with
        force_reset=False (the env vector goes on where it stands) `last_obs` is restored as well and the next learn() continues from it."""
        rb = self.replay_buffer
        d = torch.load(str(path), map_location="cpu", weights_only=True)
        for name in ("observations", "next_observations", "actions", "rewards", "terminated", "truncated", "last_obs"):
            dst = getattr(rb, name)
            if tuple(d[name].shape) != tuple(dst.shape) or d[name].dtype != dst.dtype:
                raise ValueError(f"load_replay_buffer: {name} is {d[name].dtype} {list(d[name].shape)}, the buffer holds {dst.dtype} {list(dst.shape)}")
        for name in ("observations", "next_observations", "actions", "rewards", "terminated", "truncated", "last_obs"):
            getattr(rb, name).copy_(d[name])
        rb.pos, rb.full = int(d["pos"]), bool(d["full"])
        self._last_obs_valid = bool(d["last_obs_valid"]) and bool(getattr(self, "_keep_env_state", False))
