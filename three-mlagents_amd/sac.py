"""SAC with the Stable-Baselines3 `SAC` surface: the reference's off-policy algorithm for its Box tasks (algorithm table
backend/mlagents/training.py:31-37; hyper-parameter table training.py:392-403).

Three flat `[in][out]` float buffers in SB3's tensor order -- the actor (`actor.latent_pi`, `actor.mu`, `actor.log_std`), the critic pair (`critic.qf0`,
`critic.qf1`, each over obs | action) and the critic target -- plus one device float `log_ent_coef`.  The hot path is csrc/tma_sac.hip:
tma_sac_act (actor forward + squash, one launch), tma_sac_critic_grad and tma_sac_actor_grad (forwards, loss and backward, two launches each),
tma_adam_step_flat, tma_polyak_update and tma_sac_iterations_local, which issues whole iterations natively with no host round trip.  The data half
is `ReplayBuffer` (replay_buffer.py), whose planes the native loop writes.  Semantics follow SB3 2.9; DESIGN.md section 18 lists the deviations: the
noise and the index draws are the engine's counter-based hashes, the polyak update is decided on `_n_updates` (SB3: on the index of the gradient step
inside one train() call; the two coincide at gradient_steps = 1), gradient_steps = -1 means one optimizer step per vector step collected (SB3: per env
step; equal at one env), a log row is written after the native call in which the log_interval-th episode
finished, scalars are `[B]` not `[B, 1]`.  Not built: use_sde, action_noise, more than two critics, act_dim > 8, VecNormalize, data-parallel runs.
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
from .off_policy import ADAM_EPS, NATIVE_ITERATIONS, OffPolicyAlgorithm, pol_space  # noqa: F401  (the names this module has always had)
from .replay_buffer import ReplayBuffer
from .vec_env import HipVecEnv

ACTIVATIONS = {"tanh": 0, "relu": 1}


def sac_dims(obs_dim: int, act_dim: int, hidden: int, activation: str = "relu", device: int = -1) -> "_lib.SACDims":
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation_fn must be tanh or relu (got {activation!r})")
    return _lib.SACDims(int(obs_dim), int(act_dim), int(hidden), ACTIVATIONS[activation], int(device))


def param_offsets(dims: "_lib.SACDims") -> "_lib.SACOffsets":
    off = _lib.SACOffsets()
    _lib.check(_lib.lib().tma_sac_param_offsets(C.byref(dims), C.byref(off)))
    return off


def actor_tensors(off, D: int, A: int, H: int) -> list[tuple[str, int, int, int, int]]:
    """(SB3 name, weight offset, bias offset, in, out) of the actor buffer's layers, in buffer order."""
    return [("latent_pi.0", off.a_W1, off.a_b1, D, H), ("latent_pi.2", off.a_W2, off.a_b2, H, H), ("mu", off.a_Wmu, off.a_bmu, H, A),
            ("log_std", off.a_Wls, off.a_bls, H, A)]


def critic_tensors(off, D: int, A: int, H: int) -> list[tuple[str, int, int, int, int]]:
    """The same for the critic pair: qf0, then qf1 at n_q."""
    return [(f"qf{i}.{k}", i * off.n_q + w, i * off.n_q + b, n_in, n_out) for i in range(2)
            for k, w, b, n_in, n_out in ((0, off.q_W1, off.q_b1, D + A, H), (2, off.q_W2, off.q_b2, H, H), (4, off.q_W3, off.q_b3, H, 1))]


def named_from_flat(flat: torch.Tensor, table, prefix: str) -> dict[str, torch.Tensor]:
    """SB3's state-dict tensors ([out][in] weights) of a flat [in][out] buffer, as CPU copies."""
    flat, out = flat.detach().cpu(), {}
    for name, w, b, n_in, n_out in table:
        out[f"{prefix}.{name}.weight"] = flat[w:w + n_in * n_out].view(n_in, n_out).t().contiguous()
        out[f"{prefix}.{name}.bias"] = flat[b:b + n_out].clone()
    return out


def flat_from_named(named: dict, table, prefix: str, n: int) -> torch.Tensor:
    flat = torch.zeros(n, dtype=torch.float32)
    for name, w, b, n_in, n_out in table:
        wt, bt = named[f"{prefix}.{name}.weight"], named[f"{prefix}.{name}.bias"]
        if tuple(wt.shape) != (n_out, n_in) or tuple(bt.shape) != (n_out,):
            raise ValueError(f"{prefix}.{name}: weight {list(wt.shape)} / bias {list(bt.shape)}, expected [{n_out}, {n_in}] / [{n_out}]")
        flat[w:w + n_in * n_out] = wt.to(torch.float32).t().contiguous().view(-1)
        flat[b:b + n_out] = bt.to(torch.float32)
    return flat


def plan_iterations(num_timesteps: int, n_updates: int, n_iters: int, n_envs: int, train_freq: int, gradient_steps: int, learning_starts: int,
                    target_update_interval: int) -> dict:
    """What `n_iters` iterations of tma_sac_iterations_local do, from the counters alone (host arithmetic, no GPU): the counters afterwards, the
    warm-up (uniform) vector steps, the optimizer steps and the polyak updates issued."""
    per = train_freq if gradient_steps < 0 else gradient_steps
    updates = targets = uniform = n_calls = 0
    for _ in range(n_iters):
        for _ in range(train_freq):
            uniform += num_timesteps < learning_starts
            num_timesteps += n_envs
            n_calls += 1
        if num_timesteps > learning_starts:
            for _ in range(per):
                targets += (n_updates + updates) % target_update_interval == 0
                updates += 1
    return {"num_timesteps": num_timesteps, "n_calls": n_calls, "n_updates": updates, "target_updates": targets, "uniform_steps": uniform}


class HipSACPolicy:
    """SB3's SACPolicy as three flat device buffers and one float: `actor`, `critic`, `critic_target`, `log_ent_coef`.  Initialised like torch's
    Linear (SB3's SAC nets are not re-initialised): U(-1 / sqrt(in), 1 / sqrt(in)) for weights and biases; the target starts equal to the critic."""

    def __init__(self, obs_dim: int, act_dim: int, hidden: int, device, seed: int = 0, activation: str = "relu", log_ent_coef: float = 0.0):
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
        self.critic_target = self.critic.clone()
        self.log_ent_coef = torch.full((1,), float(log_ent_coef), dtype=torch.float32, device=self.device)

    @property
    def actor_table(self):
        return actor_tensors(self.off, self.obs_dim, self.act_dim, self.hidden)

    @property
    def critic_table(self):
        return critic_tensors(self.off, self.obs_dim, self.act_dim, self.hidden)

    def _rows(self, obs) -> torch.Tensor:
        obs = torch.as_tensor(obs, dtype=torch.float32) if not torch.is_tensor(obs) else obs
        return obs.to(self.device, torch.float32).contiguous()

    def act(self, obs, rng_seed: int = 0, rng_step: int = 0, env_offset: int = 0, deterministic: bool = False):
        """-> (actions f32 [n, A], None, log_prob f32 [n]): one tma_sac_act launch (there is no value head).  The signature of
        HipActorCriticPolicy.act, so evaluate_policy_stepwise runs either."""
        obs = self._rows(obs)
        if obs.dim() != 2 or obs.shape[1] != self.obs_dim:
            raise ValueError(f"obs must have shape [n, {self.obs_dim}], got {list(obs.shape)}")
        n = obs.shape[0]
        actions = torch.empty((n, self.act_dim), dtype=torch.float32, device=self.device)
        logp = torch.empty((n,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tma_sac_act(_lib.ptr(self.actor), C.byref(self.dims), _lib.ptr(obs), n, _lib.SAC_DETERMINISTIC if deterministic else _lib.SAC_SAMPLE,
                                              int(rng_seed) & 0xFFFFFFFF, int(rng_step) & 0xFFFFFFFF, int(env_offset) & 0xFFFFFFFF, None, _lib.ptr(actions),
                                              _lib.ptr(logp), None, None, _lib.stream_ptr(self.device)))
        return actions, None, logp

    def state_dict(self) -> dict[str, torch.Tensor]:
        """SB3's SACPolicy.state_dict(): actor.*, critic.*, critic_target.* in [out][in] layout."""
        return {**named_from_flat(self.actor, self.actor_table, "actor"), **named_from_flat(self.critic, self.critic_table, "critic"),
                **named_from_flat(self.critic_target, self.critic_table, "critic_target")}

    def load_state_dict(self, sd: dict) -> None:
        with torch.no_grad():
            self.actor.copy_(flat_from_named(sd, self.actor_table, "actor", self.n_actor).to(self.device))
            self.critic.copy_(flat_from_named(sd, self.critic_table, "critic", self.n_critic).to(self.device))
            self.critic_target.copy_(flat_from_named(sd, self.critic_table, "critic_target", self.n_critic).to(self.device))


class _OptState:
    """The moments of one torch Adam, flat like the buffer it steps."""

    def __init__(self, n: int, device):
        self.grad, self.exp_avg, self.exp_avg_sq = (torch.zeros(n, dtype=torch.float32, device=device) for _ in range(3))


class SAC(OffPolicyAlgorithm):
    """SB3-shaped SAC whose compute is libtma_hip.so.  Constructor / learn / train / predict / save / load keep SB3's names and defaults; learn(),
    the frame of the native loop and the replay-buffer files are OffPolicyAlgorithm's."""

    ALGORITHM = "sac"

    def __init__(self, policy: str = "MlpPolicy", env=None, learning_rate: float = 3e-4, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 256, tau: float = 0.005, gamma: float = 0.99, train_freq=1, gradient_steps: int = 1, action_noise=None,
                 optimize_memory_usage: bool = False, n_steps: int = 1, ent_coef="auto", target_update_interval: int = 1, target_entropy="auto",
                 use_sde: bool = False, sde_sample_freq: int = -1, use_sde_at_warmup: bool = False, stats_window_size: int = 100,
                 tensorboard_log: str | None = None, policy_kwargs: dict | None = None, verbose: int = 0, seed: int | None = None, device="auto",
                 _init_setup_model: bool = True):
        if use_sde:
            raise ValueError("use_sde=True is not built (generalised state-dependent exploration has no kernel)")
        if action_noise is not None:
            raise ValueError("action_noise is not built: SAC explores through its own policy noise")
        pk = dict(policy_kwargs or {})
        if int(pk.get("n_critics", 2)) != 2:
            raise ValueError(f"n_critics must be 2 (got {pk.get('n_critics')})")
        # ent_coef: "auto" (initial value 1), "auto_<initial>", or a fixed number
        if isinstance(ent_coef, str):
            if not ent_coef.startswith("auto"):
                raise ValueError(f"ent_coef must be 'auto', 'auto_<initial value>' or a number (got {ent_coef!r})")
            init = float(ent_coef.split("_")[1]) if "_" in ent_coef else 1.0
            if not init > 0.0:
                raise ValueError("the initial value of ent_coef must be greater than 0")
            self._auto_ent = True
        else:
            init = float(ent_coef)
            if not init > 0.0:
                raise ValueError(f"a fixed ent_coef must be greater than 0 (got {ent_coef})")
            self._auto_ent = False
        self.ent_coef, self._log_ent_coef_init = ent_coef, math.log(init)
        if isinstance(target_entropy, str) and target_entropy != "auto":
            raise ValueError(f"target_entropy must be 'auto' or a number (got {target_entropy!r})")
        self.target_entropy = target_entropy
        self.action_noise, self.use_sde = None, False
        super().__init__(policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq, gradient_steps, optimize_memory_usage,
                         n_steps, target_update_interval, stats_window_size, tensorboard_log, pk, verbose, seed, _init_setup_model)

    # ------------------------------------------------------------------------------------
    @staticmethod
    def _arch(pk: dict) -> tuple[int, str]:
        from . import sb3_format

        arch = pk.get("net_arch")
        arch = [256, 256] if arch is None else arch
        if isinstance(arch, dict):
            if list(arch.get("pi", [])) != list(arch.get("qf", [])):
                raise ValueError(f"three-mlagents_amd SAC supports one net_arch for the actor and the critics, got {arch}")
            arch = arch["pi"]
        arch = list(arch)
        if len(arch) != 2 or arch[0] != arch[1]:
            raise ValueError(f"three-mlagents_amd SAC supports net_arch with two equal hidden layers, got {pk.get('net_arch')}")
        fn = pk.get("activation_fn")
        return int(arch[0]), ("relu" if fn is None else sb3_format.parse_activation(fn))  # SB3's SACPolicy: nn.ReLU

    def _make_policy(self, D: int, A: int, H: int, act: str, dev) -> None:
        self.policy = HipSACPolicy(D, A, H, dev, seed=self.seed, activation=act, log_ent_coef=self._log_ent_coef_init)
        pol = self.policy
        self.actor_opt, self.critic_opt, self.ent_opt = _OptState(pol.n_actor, dev), _OptState(pol.n_critic, dev), _OptState(1, dev)
        self._target_entropy = float(-A) if self.target_entropy == "auto" else float(self.target_entropy)

    def _setup_model(self) -> None:
        from .vec_normalize import VecNormalize

        env = self.env
        if not isinstance(env, HipVecEnv):
            raise ValueError("env must be a three_mlagents_amd HipVecEnv (use training.make_vector_env)")
        if isinstance(env, VecNormalize):
            raise ValueError("SAC with a VecNormalize env is not supported: its native iteration loop has no normalised form")
        if self.world_size > 1:
            raise ValueError("data-parallel SAC is not supported (world_size > 1)")
        eng = env.engine
        if eng.num_actions != 0:
            raise ValueError("SAC needs a Box action space (the task has a Discrete one)")
        space = env.action_space
        if not (np.all(np.asarray(space.low) == -1.0) and np.all(np.asarray(space.high) == 1.0)):
            raise ValueError("SAC needs action bounds [-1, 1] (SB3's rescaling of the squashed action is not built)")
        H, act = self._arch(self.policy_kwargs)
        D, A = eng.obs_dim, eng.act_dim
        dims = sac_dims(D, A, H, act)
        ws_bytes = int(_lib.lib().tma_sac_workspace_bytes(C.byref(dims), self.batch_size))  # the shapes csrc/tma_sac.hip takes, asked before anything else
        if ws_bytes <= 0:
            raise ValueError(f"unsupported SAC shape: {_lib.last_error()}")
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
                        critic_stats=z((4,), torch.float64), actor_stats=z((3,), torch.float64), ws=z((ws_bytes,), torch.uint8))
        b, rb, ao, co, eo = self.buf, self.replay_buffer, self.actor_opt, self.critic_opt, self.ent_opt
        self._buffers = _lib.SACBuffers(*(_lib.ptr(t) for t in (rb.last_obs, b["actions"], b["step_obs"], b["rewards"], b["term"], b["trunc"], b["term_obs"],
                                                                b["s_obs"], b["s_actions"], b["s_next_obs"], b["s_dones"], b["s_rewards"], b["s_discounts"],
                                                                ao.grad, ao.exp_avg, ao.exp_avg_sq, co.grad, co.exp_avg, co.exp_avg_sq, eo.grad, eo.exp_avg,
                                                                eo.exp_avg_sq, b["critic_stats"], b["actor_stats"], b["ws"])), ws_bytes)

    # SB3's attribute names for the parts
    @property
    def actor(self) -> torch.Tensor:
        return self.policy.actor

    @property
    def critic(self) -> torch.Tensor:
        return self.policy.critic

    @property
    def critic_target(self) -> torch.Tensor:
        return self.policy.critic_target

    @property
    def log_ent_coef(self) -> torch.Tensor:
        return self.policy.log_ent_coef

    @property
    def ent_coef_optimizer(self):
        """The moments of the log_ent_coef step (SB3: a torch Adam); None with a fixed ent_coef."""
        return self.ent_opt if self._auto_ent else None

    def side_stream(self):
        """None: EvalCallback evaluates a SAC model on the compute stream (the deferred evaluation snapshots a tma_policy_dims parameter buffer)."""
        return None

    # -- counters and hyper-parameters as the native loop takes them ------------------------------
    def _hparams(self) -> "_lib.SACHParams":
        eng = self.env.engine
        return _lib.SACHParams(self.learning_starts, self.batch_size, self.target_update_interval, self.train_freq, self.gradient_steps, self.n_steps,
                               1 if self._auto_ent else 0, self.tau, self.gamma, self.learning_rate, self._target_entropy, self.seed & 0xFFFFFFFF,
                               self.replay_buffer.seed, eng.env_offset & 0xFFFFFFFF)

    def _counters(self) -> "_lib.SACCounters":
        rb = self.replay_buffer
        return _lib.SACCounters(self.num_timesteps, self._n_calls, rb.pos, 1 if rb.full else 0, rb._draw & 0xFFFFFFFF, rb._collect_step & 0xFFFFFFFF,
                                self._adam_step, self._n_updates)

    def _native_iterations(self, hp, c, n_iters: int) -> int:
        pol = self.policy
        return _lib.lib().tma_sac_iterations_local(self.env.engine._h, _lib.ptr(pol.actor), _lib.ptr(pol.critic), _lib.ptr(pol.critic_target),
                                                   _lib.ptr(pol.log_ent_coef), C.byref(pol.dims), C.byref(self.replay_buffer._view), C.byref(self._buffers),
                                                   C.byref(hp), C.byref(c), n_iters, self._stream())

    # -- update ---------------------------------------------------------------------------
    def train(self, gradient_steps: int = 1, batch_size: int | None = None) -> None:
        """SB3 SAC.train: `gradient_steps` times sample -> critic step -> actor step (on the stepped critics) -> ent_coef step -> polyak, on the
        current stream: the calls tma_sac_iterations_local issues, one by one."""
        L, pol, rb, b, st = _lib.lib(), self.policy, self.replay_buffer, self.buf, self._stream()
        B = self.batch_size if batch_size is None else int(batch_size)
        if int(gradient_steps) < 1 or B < 1:
            raise ValueError(f"train: gradient_steps and batch_size must be at least 1 (got {gradient_steps}, {B})")
        ws, need = b["ws"], int(L.tma_sac_workspace_bytes(C.byref(pol.dims), B))
        if ws.numel() < need:
            ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        ao, co, eo, d, lr = self.actor_opt, self.critic_opt, self.ent_opt, C.byref(pol.dims), self.learning_rate
        p = _lib.ptr
        for _ in range(int(gradient_steps)):
            draw = rb._draw & 0xFFFFFFFF
            s = rb.sample(B)
            t = self._adam_step + 1
            with torch.cuda.device(self.device):
                _lib.check(L.tma_sac_critic_grad(p(pol.actor), p(pol.critic), p(pol.critic_target), p(pol.log_ent_coef), d, p(s.observations), p(s.actions),
                                                 p(s.next_observations), p(s.dones), p(s.rewards), p(s.discounts), B, self.seed & 0xFFFFFFFF, draw, None,
                                                 p(co.grad), p(b["critic_stats"]), None, None, None, None, p(ws), ws.numel(), st))
                _lib.check(L.tma_adam_step_flat(p(pol.critic), p(co.grad), p(co.exp_avg), p(co.exp_avg_sq), pol.n_critic, t, lr, 0.9, 0.999, ADAM_EPS, st))
                _lib.check(L.tma_sac_actor_grad(p(pol.actor), p(pol.critic), p(pol.log_ent_coef), d, p(s.observations), B, self.seed & 0xFFFFFFFF, draw, None,
                                                p(ao.grad), p(b["actor_stats"]), None, None, None, None, p(ws), ws.numel(), st))
                _lib.check(L.tma_adam_step_flat(p(pol.actor), p(ao.grad), p(ao.exp_avg), p(ao.exp_avg_sq), pol.n_actor, t, lr, 0.9, 0.999, ADAM_EPS, st))
                if self._auto_ent:
                    _lib.check(L.tma_sac_ent_coef_grad(p(b["actor_stats"]), self._target_entropy, p(eo.grad), st))
                    _lib.check(L.tma_adam_step_flat(p(pol.log_ent_coef), p(eo.grad), p(eo.exp_avg), p(eo.exp_avg_sq), 1, t, lr, 0.9, 0.999, ADAM_EPS, st))
                if self._n_updates % self.target_update_interval == 0:
                    _lib.check(L.tma_polyak_update(p(pol.critic), p(pol.critic_target), pol.n_critic, self.tau, st))
            self._adam_step += 1
            self._n_updates += 1
        self._mark_update_done()

    def pop_train_stats(self) -> dict[str, float]:
        """The losses of the last optimizer step (SB3 logs the mean over one train() call; with gradient_steps = 1 the two coincide).  ent_coef is
        the value AFTER that step, ent_coef_loss the one SB3 computes before it, from the pre-step log_ent_coef."""
        cs, as_ = self.buf["critic_stats"].cpu().tolist(), self.buf["actor_stats"].cpu().tolist()
        log_alpha = float(self.policy.log_ent_coef.cpu()[0])
        out = {"train/critic_loss": cs[0] / cs[3] if cs[3] else float("nan"), "train/actor_loss": as_[0] / as_[2] if as_[2] else float("nan"),
               "train/ent_coef": math.exp(log_alpha)}
        if self._auto_ent and as_[2]:
            g = -(as_[1] / as_[2] + self._target_entropy)
            # the pre-step value of log_ent_coef is not kept: the loss is reported with the post-step one (they differ by at most one lr-sized step)
            out["train/ent_coef_loss"] = log_alpha * g
        return out

    # -- inference ------------------------------------------------------------------------
    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """SB3 SAC.predict: tanh(mu) when deterministic, else a sample of the squashed Gaussian.  One tma_sac_act launch; actions in [-1, 1]."""
        obs = torch.as_tensor(np.asarray(observation, dtype=np.float32) if not torch.is_tensor(observation) else observation)
        single = obs.dim() == 1
        if single:
            obs = obs.unsqueeze(0)
        pol = self.policy
        if obs.dim() != 2 or obs.shape[1] != pol.obs_dim:
            raise ValueError(f"observation must have shape [{pol.obs_dim}] or [n, {pol.obs_dim}], got {tuple(np.shape(observation))}")
        self._predict_counter = getattr(self, "_predict_counter", 0) + 1
        actions, _, _ = pol.act(obs, rng_seed=self.seed ^ 0x5EED, rng_step=self._predict_counter, env_offset=0, deterministic=deterministic)
        a = actions.cpu().numpy()
        return (a[0] if single else a), None

    # -- artefacts: SB3's SAC zip (policy.pth: actor.* critic.* critic_target.*; actor.optimizer.pth, critic.optimizer.pth, ent_coef_optimizer.pth;
    #    pytorch_variables.pth: log_ent_coef).  Parity with a real SB3 load is unpinned: no SB3 is installed where the tests run. -------------------
    def _data(self) -> dict:
        from . import sb3_format

        pol, rb = self.policy, self.replay_buffer
        data = {
            "policy_kwargs": {**sb3_format.policy_kwargs_data(pol.hidden, "tanh", 0.0, True), "use_sde": False,
                              **({"activation_fn": sb3_format.activation_repr("tanh")} if pol.activation == "tanh" else {})},
            "num_timesteps": self.num_timesteps, "_total_timesteps": self._total_timesteps, "_num_timesteps_at_start": 0, "seed": self.seed,
            "action_noise": None, "start_time": time.time_ns(), "learning_rate": self.learning_rate, "tensorboard_log": self.tensorboard_log,
            "_last_obs": None, "_last_episode_starts": None, "_last_original_obs": None, "_episode_num": 0, "use_sde": False, "sde_sample_freq": -1,
            "_current_progress_remaining": 0.0, "_stats_window_size": self.stats_window_size, "ep_info_buffer": None, "ep_success_buffer": None,
            "_n_updates": self._n_updates, "n_envs": getattr(self, "n_envs", 1), "buffer_size": self.buffer_size, "batch_size": self.batch_size,
            "learning_starts": self.learning_starts, "tau": self.tau, "gamma": self.gamma, "gradient_steps": self.gradient_steps,
            "optimize_memory_usage": False, "replay_buffer_class": None, "replay_buffer_kwargs": {}, "n_steps": self.n_steps, "train_freq": self.train_freq,
            "use_sde_at_warmup": False, "target_entropy": self._target_entropy, "ent_coef": self.ent_coef,
            "target_update_interval": self.target_update_interval, "verbose": self.verbose, "_custom_logger": False,
            "tma": {"engine": "three-mlagents_amd", "algorithm": "sac", "task_id": getattr(self.env, "task_id", None), "mfma_dtype": "f32",
                    "activation": pol.activation, "adam_step": self._adam_step, "obs_dim": pol.obs_dim, "act_dim": pol.act_dim, "continuous": True,
                    "hidden": pol.hidden, "n_calls": self._n_calls, "replay_pos": rb.pos if rb else 0, "replay_full": bool(rb.full) if rb else False,
                    "replay_draw": rb._draw if rb else 0, "collect_step": rb._collect_step if rb else 0, "auto_ent_coef": self._auto_ent},
        }
        data.update(sb3_format.data_members(pol_space(self, "observation_space"), self._action_space_for_save(),
                                            policy_class=("stable_baselines3.sac.policies", "SACPolicy")))
        return data

    def _action_space_for_save(self):
        from .spaces import Box

        space = getattr(self, "action_space", None) or getattr(self.env, "action_space", None)
        return space if space is not None else Box(-1.0, 1.0, (self.policy.act_dim,), np.float32)

    def save(self, path, exclude=None, include=None, _frozen: dict | None = None) -> None:
        """SB3's SAC zip.  The replay buffer is not part of it (SB3: save_replay_buffer); the engine's counters sit under data["tma"]."""
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

        def _opt(opt: _OptState, table, prefix: str) -> dict:
            order = [f"{prefix}.{name}.{part}" for name, *_ in table for part in ("weight", "bias")]
            m, v = (named_from_flat(t, table, prefix) for t in (opt.exp_avg, opt.exp_avg_sq))
            return sb3_format.adam_state_dict(order, m, v, self._adam_step, self.learning_rate, eps=ADAM_EPS)

        with zipfile.ZipFile(path, "w") as z:
            z.writestr("data", json.dumps(self._data(), indent=2, default=str))
            z.writestr("policy.pth", _pth(pol.state_dict()))
            z.writestr("actor.optimizer.pth", _pth(_opt(self.actor_opt, pol.actor_table, "actor")))
            z.writestr("critic.optimizer.pth", _pth(_opt(self.critic_opt, pol.critic_table, "critic")))
            if self._auto_ent:
                eo = self.ent_opt
                z.writestr("ent_coef_optimizer.pth", _pth(sb3_format.adam_state_dict(["log_ent_coef"], {"log_ent_coef": eo.exp_avg.cpu()},
                                                                                      {"log_ent_coef": eo.exp_avg_sq.cpu()}, self._adam_step,
                                                                                      self.learning_rate, eps=ADAM_EPS)))
            z.writestr("pytorch_variables.pth", _pth({"log_ent_coef": pol.log_ent_coef.detach().cpu()}))
            z.writestr("_stable_baselines3_version", "2.9.0+three-mlagents_amd")

    @classmethod
    def load(cls, path, env=None, device="auto", **kwargs) -> "SAC":
        """SAC.load(path, env): the zips this class writes.  Without an env the model predicts; with one it trains on.  The replay buffer starts
        empty, as after SB3's load: load_replay_buffer(path) puts back what save_replay_buffer(path) wrote."""
        path = str(path)
        if not os.path.exists(path) and os.path.exists(path + ".zip"):
            path += ".zip"
        if not os.path.exists(path):
            raise FileNotFoundError(f"Model not found: {path}")

        def _member(z, name, default):
            try:
                blob = z.read(name)
            except KeyError:  # a zip without the member (a fixed ent_coef has no ent_coef_optimizer.pth); one that is there must load
                return default
            return torch.load(io.BytesIO(blob), map_location="cpu", weights_only=True)

        with zipfile.ZipFile(path) as z:
            data = json.loads(z.read("data").decode())
            sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
            opts = {k: _member(z, f"{k}.pth", {}) for k in ("actor.optimizer", "critic.optimizer", "ent_coef_optimizer")}
            variables = _member(z, "pytorch_variables.pth", {})
        tma = data.get("tma") if isinstance(data.get("tma"), dict) else {}
        if str(tma.get("algorithm", "sac")) != "sac" or "actor.latent_pi.0.weight" not in sd:
            raise ValueError(f"{path} does not hold a SAC model")
        w1, wmu = sd["actor.latent_pi.0.weight"], sd["actor.mu.weight"]
        H, D, A = int(w1.shape[0]), int(w1.shape[1]), int(wmu.shape[0])
        num = lambda key, default: default if isinstance(data.get(key, default), dict) or data.get(key) is None else data[key]  # noqa: E731
        act = str(tma.get("activation", "relu"))
        model = cls("MlpPolicy", None, learning_rate=num("learning_rate", 3e-4), buffer_size=num("buffer_size", 1_000_000),
                    learning_starts=num("learning_starts", 100), batch_size=num("batch_size", 256), tau=num("tau", 0.005), gamma=num("gamma", 0.99),
                    train_freq=num("train_freq", 1), gradient_steps=num("gradient_steps", 1), n_steps=num("n_steps", 1), ent_coef=num("ent_coef", "auto"),
                    target_update_interval=num("target_update_interval", 1), target_entropy=num("target_entropy", "auto"),
                    stats_window_size=num("_stats_window_size", 100), policy_kwargs={"net_arch": [H, H], "activation_fn": act}, seed=num("seed", 0),
                    _init_setup_model=False)
        model.num_timesteps, model._n_updates = int(data.get("num_timesteps", 0)), int(data.get("_n_updates", 0))
        model._total_timesteps = int(data.get("_total_timesteps", 0))
        model._adam_step, model._n_calls = int(tma.get("adam_step", 0)), int(tma.get("n_calls", 0))
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
        if "log_ent_coef" in variables:
            with torch.no_grad():
                pol.log_ent_coef.copy_(variables["log_ent_coef"].to(torch.float32).view(1))
        for key, opt, table, prefix, n in (("actor.optimizer", model.actor_opt, pol.actor_table, "actor", pol.n_actor),
                                           ("critic.optimizer", model.critic_opt, pol.critic_table, "critic", pol.n_critic)):
            state = (opts[key].get("state") or {}) if isinstance(opts[key], dict) else {}
            order = [f"{prefix}.{name}.{part}" for name, *_ in table for part in ("weight", "bias")]
            if len(state) == len(order):
                with torch.no_grad():
                    for moment, vec in (("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)):
                        vec.copy_(flat_from_named({name: state[i][moment] for i, name in enumerate(order)}, table, prefix, n).to(pol.device))
        state = (opts["ent_coef_optimizer"].get("state") or {}) if isinstance(opts["ent_coef_optimizer"], dict) else {}
        if len(state) == 1:
            with torch.no_grad():
                model.ent_opt.exp_avg.copy_(state[0]["exp_avg"].to(torch.float32).view(1))
                model.ent_opt.exp_avg_sq.copy_(state[0]["exp_avg_sq"].to(torch.float32).view(1))
        return model
