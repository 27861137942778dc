"""TD3 with the Stable-Baselines3 `TD3` surface: the deterministic-policy algorithm of the reference's table (algorithm table
backend/mlagents/training.py:31-37; it shares SAC's hyper-parameter table, training.py:392-403).

Four flat `[in][out]` float buffers in SB3's tensor order -- the actor (`actor.mu.{0,2,4}`), the actor target, the critic pair (`critic.qf0`,
`critic.qf1`, each over obs | action) and the critic target.  The hot path is csrc/tma_td3.hip: tma_td3_act (actor forward + tanh + action noise,
one launch), tma_td3_critic_grad and tma_td3_actor_grad (forwards, loss and backward, two launches each), with csrc/tma_sac.hip's
tma_adam_step_flat and tma_polyak_update, and tma_td3_iterations_local, which issues whole iterations natively with no host round trip.  The data
half is `ReplayBuffer` (replay_buffer.py).  Semantics follow SB3 2.9; DESIGN.md section 19 lists the deviations: the default net_arch is [256, 256]
(SB3: [400, 300]; the kernels take two equal layers of 64, 128 or 256), the noise and the index draws are the engine's counter-based hashes,
gradient_steps = -1 means one optimizer step per vector step collected (SB3: per env step; equal at one env), a log row is written after the native
call in which the log_interval-th episode finished, scalars are `[B]` not `[B, 1]`.  Not built: Ornstein-Uhlenbeck noise, more than two critics,
act_dim > 8, VecNormalize, data-parallel runs, the harness entry (`harness.ALGORITHMS` has no "td3").
"""
from __future__ import annotations

import ctypes as C
import io
import json
import math
import os
import time
import zipfile

import numpy as np
import torch

from . import _lib
from .off_policy import ADAM_EPS, OffPolicyAlgorithm, pol_space
from .replay_buffer import ReplayBuffer
from .sac import SAC, _OptState, critic_tensors, flat_from_named, named_from_flat, sac_dims
from .vec_env import HipVecEnv

SUPPORTED_WIDTHS = (64, 128, 256)


class NormalActionNoise:
    """SB3's NormalActionNoise(mean, sigma): Gaussian noise added to the squashed action while collecting.  The draw itself happens in
    tma_td3_act from the engine's counter-based generator; this object carries the two vectors."""

    def __init__(self, mean, sigma, dtype=np.float32):
        self._mu, self._sigma = np.asarray(mean, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
        self._dtype = dtype

    @property
    def mean(self):
        return self._mu

    @property
    def sigma(self):
        return self._sigma

    def reset(self) -> None:
        pass

    def __repr__(self) -> str:
        return f"NormalActionNoise(mu={self._mu}, sigma={self._sigma})"


def noise_struct(action_noise, act_dim: int) -> "_lib.TD3Noise":
    """tma_td3_noise of an action_noise (None: zeros): scalars are broadcast over the action columns."""
    out = _lib.TD3Noise()
    if action_noise is None:
        return out
    for name, dst in (("mean", out.mean), ("sigma", out.sigma)):
        v = np.asarray(getattr(action_noise, name), dtype=np.float64).reshape(-1)
        if v.size not in (1, act_dim):
            raise ValueError(f"action_noise.{name} has {v.size} elements, the action space {act_dim}")
        v = np.broadcast_to(v, (act_dim,))
        if not np.all(np.isfinite(v)) or (name == "sigma" and np.any(v < 0.0)):
            raise ValueError(f"action_noise.{name} must be finite{' and at least 0' if name == 'sigma' else ''} (got {v.tolist()})")
        for j in range(act_dim):
            dst[j] = float(v[j])
    return out


def param_offsets(dims: "_lib.SACDims") -> "_lib.TD3Offsets":
    off = _lib.TD3Offsets()
    _lib.check(_lib.lib().tma_td3_param_offsets(C.byref(dims), C.byref(off)))
    return off


def actor_tensors(off, D: int, A: int, H: int) -> list[tuple[str, int, int, int, int]]:
    """(SB3 name, weight offset, bias offset, in, out) of the actor buffer's layers, in buffer order: actor.mu is one Sequential."""
    return [("mu.0", off.a_W1, off.a_b1, D, H), ("mu.2", off.a_W2, off.a_b2, H, H), ("mu.4", off.a_Wmu, off.a_bmu, H, A)]


def plan_updates(n_updates: int, gradient_steps: int, policy_delay: int) -> list[bool]:
    """SB3's TD3.train, the delayed update: for each of `gradient_steps` optimizer steps taken from `_n_updates == n_updates`, whether the actor
    step and the two target updates follow the critic step.  SB3 increments `_n_updates` first and then tests `_n_updates % policy_delay == 0`."""
    return [(n_updates + k + 1) % policy_delay == 0 for k in range(int(gradient_steps))]


def plan_iterations(num_timesteps: int, n_updates: int, n_iters: int, n_envs: int, train_freq: int, gradient_steps: int, learning_starts: int,
                    policy_delay: int) -> dict:
    """What `n_iters` iterations of tma_td3_iterations_local do, from the counters alone (host arithmetic, no GPU): the counters afterwards, the
    warm-up (uniform) vector steps, the critic steps and the actor steps (each with both target updates) issued."""
    per = train_freq if gradient_steps < 0 else gradient_steps
    critic = actor = uniform = n_calls = 0
    for _ in range(n_iters):
        for _ in range(train_freq):
            uniform += num_timesteps < learning_starts
            num_timesteps += n_envs
            n_calls += 1
        if num_timesteps > learning_starts:
            actor += sum(plan_updates(n_updates + critic, per, policy_delay))
            critic += per
    return {"num_timesteps": num_timesteps, "n_calls": n_calls, "n_updates": critic, "actor_updates": actor, "uniform_steps": uniform}


class HipTD3Policy:
    """SB3's TD3Policy as four flat device buffers: `actor`, `actor_target`, `critic`, `critic_target`.  Initialised like torch's Linear (SB3's TD3
    nets are not re-initialised): U(-1 / sqrt(in), 1 / sqrt(in)) for weights and biases; the targets start equal to their nets."""

    def __init__(self, obs_dim: int, act_dim: int, hidden: int, device, seed: int = 0, activation: str = "relu"):
        self.obs_dim, self.act_dim, self.hidden, self.activation = int(obs_dim), int(act_dim), int(hidden), activation
        self.device = torch.device(device)
        self.dims = sac_dims(obs_dim, act_dim, hidden, activation, self.device.index if self.device.index is not None else -1)
        self.off = param_offsets(self.dims)  # (refuses unsupported shapes with the library's message)
        self.n_actor, self.n_critic = int(self.off.n_actor), int(self.off.n_critic)
        g = torch.Generator().manual_seed(int(seed))
        bufs = []
        for table, n in ((self.actor_table, self.n_actor), (self.critic_table, self.n_critic)):
            flat = torch.zeros(n, dtype=torch.float32)
            for _, w, b, n_in, n_out in table:
                bound = 1.0 / math.sqrt(n_in)
                flat[w:w + n_in * n_out] = (torch.rand(n_in * n_out, generator=g) * 2.0 - 1.0) * bound
                flat[b:b + n_out] = (torch.rand(n_out, generator=g) * 2.0 - 1.0) * bound
            bufs.append(flat.to(self.device))
        self.actor, self.critic = bufs
        self.actor_target, self.critic_target = self.actor.clone(), self.critic.clone()

    @property
    def actor_table(self):
        return actor_tensors(self.off, self.obs_dim, self.act_dim, self.hidden)

    @property
    def critic_table(self):
        return critic_tensors(self.off, self.obs_dim, self.act_dim, self.hidden)

    def act(self, obs, rng_seed: int = 0, rng_step: int = 0, env_offset: int = 0, deterministic: bool = True):
        """-> (actions f32 [n, A], None, None): tanh(mu) in one tma_td3_act launch.  The signature of HipActorCriticPolicy.act, so
        evaluate_policy_stepwise runs either; a TD3 policy is deterministic, so the generator's arguments and `deterministic` change nothing."""
        obs = torch.as_tensor(obs, dtype=torch.float32) if not torch.is_tensor(obs) else obs
        obs = obs.to(self.device, torch.float32).contiguous()
        if obs.dim() != 2 or obs.shape[1] != self.obs_dim:
            raise ValueError(f"obs must have shape [n, {self.obs_dim}], got {list(obs.shape)}")
        n = obs.shape[0]
        actions = torch.empty((n, self.act_dim), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tma_td3_act(_lib.ptr(self.actor), C.byref(self.dims), _lib.ptr(obs), n, _lib.TD3_DETERMINISTIC, None, 0, 0, 0, None,
                                              _lib.ptr(actions), None, None, _lib.stream_ptr(self.device)))
        return actions, None, None

    def state_dict(self) -> dict[str, torch.Tensor]:
        """SB3's TD3Policy.state_dict(): actor.*, actor_target.*, critic.*, critic_target.* in [out][in] layout."""
        return {**named_from_flat(self.actor, self.actor_table, "actor"), **named_from_flat(self.actor_target, self.actor_table, "actor_target"),
                **named_from_flat(self.critic, self.critic_table, "critic"), **named_from_flat(self.critic_target, self.critic_table, "critic_target")}

    def load_state_dict(self, sd: dict) -> None:
        with torch.no_grad():
            self.actor.copy_(flat_from_named(sd, self.actor_table, "actor", self.n_actor).to(self.device))
            self.actor_target.copy_(flat_from_named(sd, self.actor_table, "actor_target", self.n_actor).to(self.device))
            self.critic.copy_(flat_from_named(sd, self.critic_table, "critic", self.n_critic).to(self.device))
            self.critic_target.copy_(flat_from_named(sd, self.critic_table, "critic_target", self.n_critic).to(self.device))


class TD3(SAC):
    """SB3-shaped TD3 whose compute is libtma_hip.so.  Constructor / learn / train / predict / save / load keep SB3's names and defaults, except the
    default net_arch ([256, 256]).  learn(), the frame of the native loop and the replay-buffer files are OffPolicyAlgorithm's; the SB3 attribute
    names of the parts, the actor / critic optimizer states and the saved action space are SAC's."""

    ALGORITHM = "td3"
    ADAM_COUNTERS = {"_adam_step": "critic_adam_step", "_actor_adam_step": "actor_adam_step"}  # (_adam_step: the critic's)

    def __init__(self, policy: str = "MlpPolicy", env=None, learning_rate: float = 1e-3, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 256, tau: float = 0.005, gamma: float = 0.99, train_freq=1, gradient_steps: int = 1, action_noise=None,
                 optimize_memory_usage: bool = False, n_steps: int = 1, policy_delay: int = 2, target_policy_noise: float = 0.2,
                 target_noise_clip: float = 0.5, stats_window_size: int = 100, tensorboard_log: str | None = None, policy_kwargs: dict | None = None,
                 verbose: int = 0, seed: int | None = None, device="auto", _init_setup_model: bool = True):
        if action_noise is not None and not isinstance(action_noise, NormalActionNoise):
            raise ValueError(f"action_noise must be None or a three_mlagents_amd NormalActionNoise (got {type(action_noise).__name__}): "
                             "Ornstein-Uhlenbeck and other noises are not built")
        if int(policy_delay) < 1:
            raise ValueError(f"policy_delay must be at least 1 (got {policy_delay})")
        if not float(target_policy_noise) >= 0.0:
            raise ValueError(f"target_policy_noise must be at least 0 (got {target_policy_noise})")
        if not float(target_noise_clip) >= 0.0:
            raise ValueError(f"target_noise_clip must be at least 0 (got {target_noise_clip})")
        pk = dict(policy_kwargs or {})
        if int(pk.get("n_critics", 2)) != 2:
            raise ValueError(f"n_critics must be 2 (got {pk.get('n_critics')})")
        self._arch(pk)  # (an unsupported net_arch is refused here, before any env is looked at)
        self.policy_delay, self.target_policy_noise, self.target_noise_clip = int(policy_delay), float(target_policy_noise), float(target_noise_clip)
        self.action_noise, self.use_sde = action_noise, False
        OffPolicyAlgorithm.__init__(self, policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq, gradient_steps,
                                    optimize_memory_usage, n_steps, None, stats_window_size, tensorboard_log, pk, verbose, seed, _init_setup_model)

    # ------------------------------------------------------------------------------------
    @staticmethod
    def _arch(pk: dict) -> tuple[int, str]:
        """(hidden width, activation).  SB3's TD3 default is [400, 300]; the kernels take two equal layers of 64, 128 or 256, so the default here is
        [256, 256] and everything else is refused."""
        from . import sb3_format

        arch = pk.get("net_arch")
        arch = [256, 256] if arch is None else arch
        if isinstance(arch, dict):
            if list(arch.get("pi", [])) != list(arch.get("qf", [])):
                raise ValueError(f"three-mlagents_amd TD3 supports one net_arch for the actor and the critics, got {arch}")
            arch = arch["pi"]
        arch = list(arch)
        if len(arch) != 2 or arch[0] != arch[1] or int(arch[0]) not in SUPPORTED_WIDTHS:
            raise ValueError(f"three-mlagents_amd TD3 supports net_arch with two equal hidden layers of width 64, 128 or 256 (the default is [256, 256], "
                             f"not SB3's [400, 300]), got {pk.get('net_arch')}")
        fn = pk.get("activation_fn")
        return int(arch[0]), ("relu" if fn is None else sb3_format.parse_activation(fn))  # SB3's TD3Policy: nn.ReLU

    def _make_policy(self, D: int, A: int, H: int, act: str, dev) -> None:
        self.policy = HipTD3Policy(D, A, H, dev, seed=self.seed, activation=act)
        pol = self.policy
        self.actor_opt, self.critic_opt = _OptState(pol.n_actor, dev), _OptState(pol.n_critic, dev)
        self._noise = noise_struct(self.action_noise, A)

    def _setup_model(self) -> None:
        from .vec_normalize import VecNormalize

        env = self.env
        if not isinstance(env, HipVecEnv):
            raise ValueError("env must be a three_mlagents_amd HipVecEnv (use training.make_vector_env)")
        if isinstance(env, VecNormalize):
            raise ValueError("TD3 with a VecNormalize env is not supported: its native iteration loop has no normalised form")
        if self.world_size > 1:
            raise ValueError("data-parallel TD3 is not supported (world_size > 1)")
        eng = env.engine
        if eng.num_actions != 0:
            raise ValueError("TD3 needs a Box action space (the task has a Discrete one)")
        space = env.action_space
        if not (np.all(np.asarray(space.low) == -1.0) and np.all(np.asarray(space.high) == 1.0)):
            raise ValueError("TD3 needs action bounds [-1, 1] (SB3's rescaling of the squashed action is not built)")
        H, act = self._arch(self.policy_kwargs)
        D, A = eng.obs_dim, eng.act_dim
        dims = sac_dims(D, A, H, act)
        ws_bytes = int(_lib.lib().tma_td3_workspace_bytes(C.byref(dims), self.batch_size))  # the shapes csrc/tma_td3.hip takes, asked before anything else
        if ws_bytes <= 0:
            raise ValueError(f"unsupported TD3 shape: {_lib.last_error()}")
        self.device, self.n_envs = eng.device, env.num_envs
        self.observation_space, self.action_space = env.observation_space, env.action_space
        N, dev = self.n_envs, self.device
        self._make_policy(D, A, H, act, dev)
        if not getattr(self, "_keep_env_state", False):
            env.seed(self.seed)
        self.replay_buffer = ReplayBuffer(self.buffer_size, D, self.action_space, dev, n_envs=N, n_steps=self.n_steps, gamma=self.gamma, seed=self.seed)
        f32, B = torch.float32, self.batch_size
        z = lambda shape, dtype=f32: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
        self.buf = dict(actions=z((N, A)), step_obs=z((N, D)), rewards=z((N,)), term=z((N,), torch.uint8), trunc=z((N,), torch.uint8), term_obs=z((N, D)),
                        s_obs=z((B, D)), s_actions=z((B, A)), s_next_obs=z((B, D)), s_dones=z((B,)), s_rewards=z((B,)), s_discounts=z((B,)),
                        critic_stats=z((4,), torch.float64), actor_stats=z((2,), torch.float64), ws=z((ws_bytes,), torch.uint8))
        b, rb, ao, co = self.buf, self.replay_buffer, self.actor_opt, self.critic_opt
        self._buffers = _lib.TD3Buffers(*(_lib.ptr(t) for t in (rb.last_obs, b["actions"], b["step_obs"], b["rewards"], b["term"], b["trunc"], b["term_obs"],
                                                                b["s_obs"], b["s_actions"], b["s_next_obs"], b["s_dones"], b["s_rewards"], b["s_discounts"],
                                                                ao.grad, ao.exp_avg, ao.exp_avg_sq, co.grad, co.exp_avg, co.exp_avg_sq, b["critic_stats"],
                                                                b["actor_stats"], b["ws"])), ws_bytes)

    @property
    def actor_target(self) -> torch.Tensor:
        return self.policy.actor_target

    @property
    def log_ent_coef(self):
        raise AttributeError("TD3 has no entropy coefficient")

    @property
    def ent_coef_optimizer(self):
        raise AttributeError("TD3 has no entropy coefficient")

    # -- counters and hyper-parameters as the native loop takes them ------------------------------
    def _hparams(self) -> "_lib.TD3HParams":
        eng = self.env.engine
        return _lib.TD3HParams(self.learning_starts, self.batch_size, self.policy_delay, self.train_freq, self.gradient_steps, self.n_steps,
                               0 if self.action_noise is None else 1, self.tau, self.gamma, self.learning_rate, self.target_policy_noise,
                               self.target_noise_clip, self._noise, self.seed & 0xFFFFFFFF, self.replay_buffer.seed, eng.env_offset & 0xFFFFFFFF)

    def _counters(self) -> "_lib.TD3Counters":
        rb = self.replay_buffer
        return _lib.TD3Counters(self.num_timesteps, self._n_calls, rb.pos, 1 if rb.full else 0, rb._draw & 0xFFFFFFFF, rb._collect_step & 0xFFFFFFFF,
                                self._adam_step, self._actor_adam_step, self._n_updates)

    def _native_iterations(self, hp, c, n_iters: int) -> int:
        pol = self.policy
        return _lib.lib().tma_td3_iterations_local(self.env.engine._h, _lib.ptr(pol.actor), _lib.ptr(pol.actor_target), _lib.ptr(pol.critic),
                                                   _lib.ptr(pol.critic_target), C.byref(pol.dims), C.byref(self.replay_buffer._view), C.byref(self._buffers),
                                                   C.byref(hp), C.byref(c), n_iters, self._stream())

    # -- update ---------------------------------------------------------------------------
    def train(self, gradient_steps: int = 1, batch_size: int | None = None) -> None:
        """SB3 TD3.train: `gradient_steps` times sample -> critic step -> (where plan_updates says so) actor step on the stepped critics -> both
        polyak updates, on the current stream: the calls tma_td3_iterations_local issues, one by one."""
        L, pol, rb, b, st = _lib.lib(), self.policy, self.replay_buffer, self.buf, self._stream()
        B = self.batch_size if batch_size is None else int(batch_size)
        if int(gradient_steps) < 1 or B < 1:
            raise ValueError(f"train: gradient_steps and batch_size must be at least 1 (got {gradient_steps}, {B})")
        ws, need = b["ws"], int(L.tma_td3_workspace_bytes(C.byref(pol.dims), B))
        if ws.numel() < need:
            ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        ao, co, d, lr = self.actor_opt, self.critic_opt, C.byref(pol.dims), self.learning_rate
        p = _lib.ptr
        for delayed in plan_updates(self._n_updates, int(gradient_steps), self.policy_delay):
            self._n_updates += 1
            draw = rb._draw & 0xFFFFFFFF
            s = rb.sample(B)
            with torch.cuda.device(self.device):
                _lib.check(L.tma_td3_critic_grad(p(pol.actor_target), p(pol.critic), p(pol.critic_target), d, p(s.observations), p(s.actions),
                                                 p(s.next_observations), p(s.dones), p(s.rewards), p(s.discounts), B, self.target_policy_noise,
                                                 self.target_noise_clip, self.seed & 0xFFFFFFFF, draw, None, p(co.grad), p(b["critic_stats"]), None, None, None,
                                                 None, p(ws), ws.numel(), st))
                _lib.check(L.tma_adam_step_flat(p(pol.critic), p(co.grad), p(co.exp_avg), p(co.exp_avg_sq), pol.n_critic, self._adam_step + 1, lr, 0.9, 0.999,
                                                ADAM_EPS, st))
                self._adam_step += 1
                if delayed:
                    _lib.check(L.tma_td3_actor_grad(p(pol.actor), p(pol.critic), d, p(s.observations), B, p(ao.grad), p(b["actor_stats"]), None, None, p(ws),
                                                    ws.numel(), st))
                    _lib.check(L.tma_adam_step_flat(p(pol.actor), p(ao.grad), p(ao.exp_avg), p(ao.exp_avg_sq), pol.n_actor, self._actor_adam_step + 1, lr, 0.9,
                                                    0.999, ADAM_EPS, st))
                    self._actor_adam_step += 1
                    _lib.check(L.tma_polyak_update(p(pol.critic), p(pol.critic_target), pol.n_critic, self.tau, st))
                    _lib.check(L.tma_polyak_update(p(pol.actor), p(pol.actor_target), pol.n_actor, self.tau, st))
        self._mark_update_done()

    def pop_train_stats(self) -> dict[str, float]:
        """The losses of the last optimizer steps (SB3 logs the mean over one train() call; with gradient_steps = 1 the two coincide).
        train/actor_loss is absent until an actor step has run."""
        cs, as_ = self.buf["critic_stats"].cpu().tolist(), self.buf["actor_stats"].cpu().tolist()
        out = {"train/critic_loss": cs[0] / cs[3] if cs[3] else float("nan")}
        if self._actor_adam_step > 0 and as_[1]:
            out["train/actor_loss"] = as_[0] / as_[1]
        return out

    # -- inference ------------------------------------------------------------------------
    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """SB3 TD3.predict: tanh(mu(obs)); `deterministic` makes no difference, as in SB3 (the action noise belongs to collection).  One
        tma_td3_act launch; actions in [-1, 1]."""
        obs = torch.as_tensor(np.asarray(observation, dtype=np.float32) if not torch.is_tensor(observation) else observation)
        single = obs.dim() == 1
        if single:
            obs = obs.unsqueeze(0)
        pol = self.policy
        if obs.dim() != 2 or obs.shape[1] != pol.obs_dim:
            raise ValueError(f"observation must have shape [{pol.obs_dim}] or [n, {pol.obs_dim}], got {tuple(np.shape(observation))}")
        actions, _, _ = pol.act(obs)
        a = actions.cpu().numpy()
        return (a[0] if single else a), None

    # -- artefacts: SB3's TD3 zip (policy.pth: actor.* actor_target.* critic.* critic_target.*; actor.optimizer.pth, critic.optimizer.pth).  Parity
    #    with a real SB3 load is unpinned: no SB3 is installed where the tests run. ----------------------------------------------------------------
    def _data(self) -> dict:
        from . import sb3_format

        pol, rb, an = self.policy, self.replay_buffer, self.action_noise
        data = {
            "policy_kwargs": {**sb3_format.policy_kwargs_data(pol.hidden, "tanh", 0.0, True),
                              **({"activation_fn": sb3_format.activation_repr("tanh")} if pol.activation == "tanh" else {})},
            "num_timesteps": self.num_timesteps, "_total_timesteps": self._total_timesteps, "_num_timesteps_at_start": 0, "seed": self.seed,
            "action_noise": None if an is None else repr(an), "start_time": time.time_ns(), "learning_rate": self.learning_rate,
            "tensorboard_log": self.tensorboard_log, "_last_obs": None, "_last_episode_starts": None, "_last_original_obs": None, "_episode_num": 0,
            "use_sde": False, "sde_sample_freq": -1, "_current_progress_remaining": 0.0, "_stats_window_size": self.stats_window_size,
            "ep_info_buffer": None, "ep_success_buffer": None, "_n_updates": self._n_updates, "n_envs": getattr(self, "n_envs", 1),
            "buffer_size": self.buffer_size, "batch_size": self.batch_size, "learning_starts": self.learning_starts, "tau": self.tau, "gamma": self.gamma,
            "gradient_steps": self.gradient_steps, "optimize_memory_usage": False, "replay_buffer_class": None, "replay_buffer_kwargs": {},
            "n_steps": self.n_steps, "train_freq": self.train_freq, "use_sde_at_warmup": False, "policy_delay": self.policy_delay,
            "target_policy_noise": self.target_policy_noise, "target_noise_clip": self.target_noise_clip, "verbose": self.verbose, "_custom_logger": False,
            "tma": {"engine": "three-mlagents_amd", "algorithm": "td3", "task_id": getattr(self.env, "task_id", None), "mfma_dtype": "f32",
                    "activation": pol.activation, "adam_step": self._adam_step, "actor_adam_step": self._actor_adam_step, "obs_dim": pol.obs_dim,
                    "act_dim": pol.act_dim, "continuous": True, "hidden": pol.hidden, "n_calls": self._n_calls, "replay_pos": rb.pos if rb else 0,
                    "replay_full": bool(rb.full) if rb else False, "replay_draw": rb._draw if rb else 0, "collect_step": rb._collect_step if rb else 0,
                    "action_noise": None if an is None else {"mean": np.asarray(an.mean).reshape(-1).tolist(), "sigma": np.asarray(an.sigma).reshape(-1).tolist()}},
        }
        data.update(sb3_format.data_members(pol_space(self, "observation_space"), self._action_space_for_save(),
                                            policy_class=("stable_baselines3.td3.policies", "TD3Policy")))
        return data

    def save(self, path, exclude=None, include=None, _frozen: dict | None = None) -> None:
        """SB3's TD3 zip.  The replay buffer is not part of it (SB3: save_replay_buffer); the engine's counters sit under data["tma"]."""
        from . import sb3_format

        path = str(path)
        if not os.path.splitext(path)[1]:
            path += ".zip"
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

        def _pth(obj) -> bytes:
            bio = io.BytesIO()
            torch.save(obj, bio)
            return bio.getvalue()

        pol = self.policy

        def _opt(opt: _OptState, table, prefix: str, step: int) -> dict:
            order = [f"{prefix}.{name}.{part}" for name, *_ in table for part in ("weight", "bias")]
            m, v = (named_from_flat(t, table, prefix) for t in (opt.exp_avg, opt.exp_avg_sq))
            return sb3_format.adam_state_dict(order, m, v, step, self.learning_rate, eps=ADAM_EPS)

        with zipfile.ZipFile(path, "w") as z:
            z.writestr("data", json.dumps(self._data(), indent=2, default=str))
            z.writestr("policy.pth", _pth(pol.state_dict()))
            z.writestr("actor.optimizer.pth", _pth(_opt(self.actor_opt, pol.actor_table, "actor", self._actor_adam_step)))
            z.writestr("critic.optimizer.pth", _pth(_opt(self.critic_opt, pol.critic_table, "critic", self._adam_step)))
            z.writestr("pytorch_variables.pth", _pth({}))
            z.writestr("_stable_baselines3_version", "2.9.0+three-mlagents_amd")

    @classmethod
    def load(cls, path, env=None, device="auto", **kwargs) -> "TD3":
        """TD3.load(path, env): the zips this class writes.  Without an env the model predicts; with one it trains on.  The replay buffer starts
        empty, as after SB3's load: load_replay_buffer(path) puts back what save_replay_buffer(path) wrote."""
        path = str(path)
        if not os.path.exists(path) and os.path.exists(path + ".zip"):
            path += ".zip"
        if not os.path.exists(path):
            raise FileNotFoundError(f"Model not found: {path}")
        with zipfile.ZipFile(path) as z:
            data = json.loads(z.read("data").decode())
            sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
            opts = {k: torch.load(io.BytesIO(z.read(f"{k}.pth")), map_location="cpu", weights_only=True) for k in ("actor.optimizer", "critic.optimizer")}
        tma = data.get("tma") if isinstance(data.get("tma"), dict) else {}
        if str(tma.get("algorithm", "td3")) != "td3" or "actor.mu.0.weight" not in sd or "actor_target.mu.0.weight" not in sd:
            raise ValueError(f"{path} does not hold a TD3 model")
        w1, wmu = sd["actor.mu.0.weight"], sd["actor.mu.4.weight"]
        H, D, A = int(w1.shape[0]), int(w1.shape[1]), int(wmu.shape[0])
        num = lambda key, default: default if isinstance(data.get(key, default), dict) or data.get(key) is None else data[key]  # noqa: E731
        act = str(tma.get("activation", "relu"))
        an = tma.get("action_noise")
        noise = NormalActionNoise(np.asarray(an["mean"]), np.asarray(an["sigma"])) if isinstance(an, dict) else None
        model = cls("MlpPolicy", None, learning_rate=num("learning_rate", 1e-3), buffer_size=num("buffer_size", 1_000_000),
                    learning_starts=num("learning_starts", 100), batch_size=num("batch_size", 256), tau=num("tau", 0.005), gamma=num("gamma", 0.99),
                    train_freq=num("train_freq", 1), gradient_steps=num("gradient_steps", 1), action_noise=noise, n_steps=num("n_steps", 1),
                    policy_delay=num("policy_delay", 2), target_policy_noise=num("target_policy_noise", 0.2), target_noise_clip=num("target_noise_clip", 0.5),
                    stats_window_size=num("_stats_window_size", 100), policy_kwargs={"net_arch": [H, H], "activation_fn": act}, seed=num("seed", 0),
                    _init_setup_model=False)
        model.num_timesteps, model._n_updates = int(data.get("num_timesteps", 0)), int(data.get("_n_updates", 0))
        model._total_timesteps = int(data.get("_total_timesteps", 0))
        model._adam_step, model._actor_adam_step, model._n_calls = int(tma.get("adam_step", 0)), int(tma.get("actor_adam_step", 0)), int(tma.get("n_calls", 0))
        if env is not None:
            model.env = env
            model._keep_env_state = not kwargs.get("force_reset", True)
            model._setup_model()
            rb = model.replay_buffer
            rb._draw, rb._collect_step = int(tma.get("replay_draw", 0)), int(tma.get("collect_step", 0))  # (counters are never reused across a save / load)
        else:
            from .vec_env import _require_gpu

            dev = _require_gpu(None if device == "auto" else device)
            model.device = dev
            model._make_policy(D, A, H, act, dev)
        pol = model.policy
        pol.load_state_dict(sd)
        for key, opt, table, prefix, n in (("actor.optimizer", model.actor_opt, pol.actor_table, "actor", pol.n_actor),
                                           ("critic.optimizer", model.critic_opt, pol.critic_table, "critic", pol.n_critic)):
            state = (opts[key].get("state") or {}) if isinstance(opts[key], dict) else {}
            order = [f"{prefix}.{name}.{part}" for name, *_ in table for part in ("weight", "bias")]
            if len(state) == len(order):
                with torch.no_grad():
                    for moment, vec in (("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)):
                        vec.copy_(flat_from_named({name: state[i][moment] for i, name in enumerate(order)}, table, prefix, n).to(pol.device))
        return model
