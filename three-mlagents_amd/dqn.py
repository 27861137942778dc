"""DQN with the Stable-Baselines3 `DQN` surface: the reference's default algorithm for its Discrete tasks (backend/mlagents/registry.py:59,91,107,123;
hyper-parameter table backend/mlagents/training.py:343-360).

The Q-network is the `pi.*` segment of a Discrete `HipActorCriticPolicy` (SB3's QNetwork features -> H -> H -> A; the value net rides along unused
and untouched), the target net a second policy over a buffer of the same layout.  The hot path is csrc/tma_dqn.hip: tma_dqn_act (Q forward +
epsilon-greedy pick, one launch), tma_dqn_td_grad (both forwards, the Huber loss and the backward, two launches), tma_dqn_target_update, Adam
through tma_ppo_adam_step_local, and tma_dqn_iterations_local, which issues whole iterations natively with no host round trip.  The data half is
`ReplayBuffer` (replay_buffer.py), whose planes the native loop writes.  Semantics follow SB3 2.9; DESIGN.md section 17 lists the deviations:
the epsilon coin is per env (SB3 tosses one per predict call), sampling is the engine's counter-based hash, a log row is written after the native
call in which the log_interval-th episode finished (SB3: at that episode), scalars are `[B]` not `[B, 1]`.
"""
from __future__ import annotations

import ctypes as C
import io
import json
import os
import time
import zipfile

import numpy as np
import torch

from . import _lib
from .off_policy import ADAM_EPS, NATIVE_ITERATIONS, OffPolicyAlgorithm, pol_space  # noqa: F401  (the names this module has always had)
from .ppo import HipActorCriticPolicy
from .replay_buffer import ReplayBuffer
from .vec_env import HipVecEnv

Q_KEYS = [f"q_net.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]          # SB3's QNetwork: Sequential(Linear, act, Linear, act, Linear)
PI_KEYS = ["mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight",
           "mlp_extractor.policy_net.2.bias", "action_net.weight", "action_net.bias"]  # the same six tensors in HipActorCriticPolicy's names


def linear_epsilon(num_timesteps: int, total_timesteps: int, fraction: float, initial: float, final: float) -> float:
    """SB3's get_linear_fn(initial, final, fraction) at progress_remaining = 1 - num_timesteps / total_timesteps (the arithmetic of
    tma_dqn_epsilon, in the same order)."""
    total = float(total_timesteps) if total_timesteps > 0 else 1.0
    progress = 1.0 - (1.0 - float(num_timesteps) / total)
    if progress > fraction:
        return float(final)
    return float(initial) + progress * (float(final) - float(initial)) / float(fraction)


def epsilon_at(num_timesteps: int, total_timesteps: int, learning_starts: int, fraction: float, initial: float, final: float) -> float:
    """The exploration rate of the vector step taken at `num_timesteps`: 1 below learning_starts (SB3 samples uniformly there), else the schedule."""
    return 1.0 if num_timesteps < learning_starts else linear_epsilon(num_timesteps, total_timesteps, fraction, initial, final)


def plan_iterations(num_timesteps: int, n_calls: int, n_iters: int, n_envs: int, train_freq: int, gradient_steps: int, learning_starts: int,
                    target_update_interval: int) -> dict:
    """What `n_iters` iterations of tma_dqn_iterations_local do, from the counters alone (host arithmetic, no GPU): the counters afterwards, the
    optimizer steps and the target updates issued."""
    every = max(target_update_interval // n_envs, 1)
    per = train_freq if gradient_steps < 0 else gradient_steps
    updates = targets = 0
    for _ in range(n_iters):
        for _ in range(train_freq):
            num_timesteps += n_envs
            n_calls += 1
            targets += n_calls % every == 0
        if num_timesteps > learning_starts:
            updates += per
    return {"num_timesteps": num_timesteps, "n_calls": n_calls, "n_updates": updates, "target_updates": targets}


class DQN(OffPolicyAlgorithm):
    """SB3-shaped DQN whose compute is libtma_hip.so.  Constructor / learn / train / predict / save / load keep SB3's names and defaults; learn(),
    the frame of the native loop and the replay-buffer files are OffPolicyAlgorithm's."""

    ALGORITHM = "dqn"

    def __init__(self, policy: str = "MlpPolicy", env=None, learning_rate: float = 1e-4, buffer_size: int = 1_000_000, learning_starts: int = 100,
                 batch_size: int = 32, tau: float = 1.0, gamma: float = 0.99, train_freq=4, gradient_steps: int = 1, optimize_memory_usage: bool = False,
                 n_steps: int = 1, target_update_interval: int = 10_000, exploration_fraction: float = 0.1, exploration_initial_eps: float = 1.0,
                 exploration_final_eps: float = 0.05, max_grad_norm: float = 10, stats_window_size: int = 100, tensorboard_log: str | None = None,
                 policy_kwargs: dict | None = None, verbose: int = 0, seed: int | None = None, device="auto", _init_setup_model: bool = True):
        if not 0.0 < float(exploration_fraction) <= 1.0:
            raise ValueError(f"exploration_fraction must be in (0, 1] (got {exploration_fraction})")
        if not (0.0 <= float(exploration_initial_eps) <= 1.0 and 0.0 <= float(exploration_final_eps) <= 1.0):
            raise ValueError("exploration_initial_eps and exploration_final_eps must be in [0, 1]")
        self.exploration_fraction, self.exploration_initial_eps = float(exploration_fraction), float(exploration_initial_eps)
        self.exploration_final_eps, self.max_grad_norm = float(exploration_final_eps), float(max_grad_norm)
        self.q_net_target: HipActorCriticPolicy | None = None
        super().__init__(policy, env, learning_rate, buffer_size, learning_starts, batch_size, tau, gamma, train_freq, gradient_steps, optimize_memory_usage,
                         n_steps, target_update_interval, stats_window_size, tensorboard_log, policy_kwargs, verbose, seed, _init_setup_model)

    # ------------------------------------------------------------------------------------
    def _setup_model(self) -> None:
        from .vec_normalize import VecNormalize

        env = self.env
        if not isinstance(env, HipVecEnv):
            raise ValueError("env must be a three_mlagents_amd HipVecEnv (use training.make_vector_env)")
        if isinstance(env, VecNormalize):
            raise ValueError("DQN with a VecNormalize env is not supported: its native iteration loop has no normalised form")
        if self.world_size > 1:
            raise ValueError("data-parallel DQN is not supported (world_size > 1)")
        eng = env.engine
        if eng.num_actions == 0:
            raise ValueError("DQN needs a Discrete action space (the task has a Box one)")
        pk = self.policy_kwargs
        arch = list(pk.get("net_arch") or [64, 64])
        if len(arch) != 2 or arch[0] != arch[1]:
            raise ValueError(f"three-mlagents_amd DQN supports net_arch with two equal hidden layers, got {pk.get('net_arch')}")
        from .ppo import policy_dims

        D, A, H = eng.obs_dim, eng.num_actions, int(arch[0])
        act = pk.get("activation_fn", "relu")  # SB3's DQNPolicy: nn.ReLU
        # the shapes csrc/tma_dqn.hip takes, asked of the library before anything touches the device
        dims = policy_dims(D, H, A, False, pk.get("mfma_dtype", "f32"), -1, act)
        ws_bytes = int(_lib.lib().tma_dqn_workspace_bytes(C.byref(dims), self.batch_size))
        if ws_bytes <= 0:
            raise ValueError(f"unsupported DQN shape: {_lib.last_error()}")
        self.device, self.n_envs = eng.device, env.num_envs
        self.observation_space, self.action_space = env.observation_space, env.action_space
        N, dev = self.n_envs, self.device
        # torch's default Linear initialisation (SB3's QNetwork is not re-initialised); equal seeds: the target starts equal to the online net
        self.policy, self.q_net_target = (HipActorCriticPolicy(D, A, False, H, dev, seed=self.seed, mfma_dtype=pk.get("mfma_dtype", "f32"), activation=act,
                                                               ortho_init=False) for _ in range(2))
        dims = self.policy.dims
        if not getattr(self, "_keep_env_state", False):
            env.seed(self.seed)
        self.replay_buffer = ReplayBuffer(self.buffer_size, D, self.action_space, dev, n_envs=N, n_steps=self.n_steps, gamma=self.gamma, seed=self.seed)
        f32, B, P = torch.float32, self.batch_size, self.policy.n_trainable
        z = lambda shape, dtype=f32: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
        self.buf = dict(actions=z((N,), torch.int32), step_obs=z((N, D)), rewards=z((N,)), term=z((N,), torch.uint8), trunc=z((N,), torch.uint8),
                        term_obs=z((N, D)), s_obs=z((B, D)), s_actions=z((B,), torch.int32), s_next_obs=z((B, D)), s_dones=z((B,)), s_rewards=z((B,)),
                        s_discounts=z((B,)), stats=z((3,), torch.float64), td_ws=z((ws_bytes,), torch.uint8))
        self.grad, self.exp_avg, self.exp_avg_sq = z((P,)), z((P,)), z((P,))
        self.workspace = z((int(_lib.lib().tma_ppo_workspace_bytes(C.byref(dims))),), torch.uint8)
        b, rb = self.buf, self.replay_buffer
        self._buffers = _lib.DQNBuffers(*(_lib.ptr(t) for t in (rb.last_obs, b["actions"], b["step_obs"], b["rewards"], b["term"], b["trunc"], b["term_obs"],
                                                                b["s_obs"], b["s_actions"], b["s_next_obs"], b["s_dones"], b["s_rewards"], b["s_discounts"],
                                                                self.grad, self.exp_avg, self.exp_avg_sq, b["stats"], b["td_ws"])), ws_bytes,
                                        _lib.ptr(self.workspace))

    # -- counters and hyper-parameters as the native loop takes them ------------------------------
    @property
    def exploration_rate(self) -> float:
        """SB3's `exploration_rate`: the schedule at the current num_timesteps (the uniform warm-up below learning_starts is applied where an
        action is drawn, as in SB3's _sample_action)."""
        return linear_epsilon(self.num_timesteps, self._total_timesteps, self.exploration_fraction, self.exploration_initial_eps, self.exploration_final_eps)

    def _hparams(self) -> "_lib.DQNHParams":
        eng = self.env.engine
        return _lib.DQNHParams(self._total_timesteps, self.learning_starts, self.batch_size, self.target_update_interval, self.train_freq, self.gradient_steps,
                               self.n_steps, self.tau, self.gamma, self.exploration_fraction, self.exploration_initial_eps, self.exploration_final_eps,
                               self.learning_rate, self.max_grad_norm, self.seed & 0xFFFFFFFF, self.replay_buffer.seed, eng.env_offset & 0xFFFFFFFF)

    def _counters(self) -> "_lib.DQNCounters":
        rb = self.replay_buffer
        return _lib.DQNCounters(self.num_timesteps, self._n_calls, rb.pos, 1 if rb.full else 0, rb._draw & 0xFFFFFFFF, rb._collect_step & 0xFFFFFFFF,
                                self._adam_step, self._n_updates)

    def _run_iterations(self, n_iters: int) -> None:
        self.policy._sync_if_stepped()
        super()._run_iterations(n_iters)

    def _native_iterations(self, hp, c, n_iters: int) -> int:
        pol = self.policy
        return _lib.lib().tma_dqn_iterations_local(self.env.engine._h, _lib.ptr(pol.params), _lib.ptr(self.q_net_target.params), C.byref(pol.dims),
                                                   C.byref(self.replay_buffer._view), C.byref(self._buffers), C.byref(hp), C.byref(c), n_iters, self._stream())

    # -- update ---------------------------------------------------------------------------
    def train(self, gradient_steps: int = 1, batch_size: int | None = None) -> None:
        """SB3 DQN.train: `gradient_steps` times sample -> TD gradient -> clip_grad_norm_ + Adam, on the current stream."""
        L, pol, rb, b, st = _lib.lib(), self.policy, self.replay_buffer, self.buf, self._stream()
        B = self.batch_size if batch_size is None else int(batch_size)
        if int(gradient_steps) < 1 or B < 1:
            raise ValueError(f"train: gradient_steps and batch_size must be at least 1 (got {gradient_steps}, {B})")
        pol._sync_if_stepped()
        ws, need = b["td_ws"], int(L.tma_dqn_workspace_bytes(C.byref(pol.dims), B))
        if ws.numel() < need:
            ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        for _ in range(int(gradient_steps)):
            s = rb.sample(B)
            with torch.cuda.device(self.device):
                _lib.check(L.tma_dqn_td_grad(_lib.ptr(pol.params), _lib.ptr(self.q_net_target.params), C.byref(pol.dims), _lib.ptr(s.observations),
                                             _lib.ptr(s.actions), _lib.ptr(s.next_observations), _lib.ptr(s.dones), _lib.ptr(s.rewards), _lib.ptr(s.discounts), B,
                                             _lib.ptr(self.grad), _lib.ptr(b["stats"]), None, _lib.ptr(ws), ws.numel(), st))
                _lib.check(L.tma_ppo_adam_step_local(_lib.ptr(pol.params), _lib.ptr(self.grad), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                                                     C.byref(pol.dims), self._adam_step + 1, self.learning_rate, 0.9, 0.999, ADAM_EPS, self.max_grad_norm,
                                                     _lib.ptr(self.workspace), st, 0))
            self._adam_step += 1
            self._n_updates += 1
        self._mark_update_done()

    def pop_train_stats(self) -> dict[str, float]:
        """train/loss of the last optimizer step (SB3 logs the mean over one train() call; with gradient_steps = 1 the two coincide)."""
        s = self.buf["stats"].cpu().tolist()
        return {"train/loss": s[0] / s[2] if s[2] else float("nan"), "train/q_taken_mean": s[1] / s[2] if s[2] else float("nan")}

    def _log_row(self, common: dict) -> dict:
        """SB3's DQN row: the exploration rate in front, and of the last optimizer step train/loss alone."""
        return {"rollout/exploration_rate": self.exploration_rate, **common,
                **({"train/loss": self.pop_train_stats()["train/loss"]} if self._n_updates > 0 else {})}

    # -- inference ------------------------------------------------------------------------
    def predict(self, observation, state=None, episode_start=None, deterministic: bool = False):
        """SB3 DQN.predict: greedy through the Q-network; with deterministic=False epsilon-greedy at the current exploration_rate (one coin per
        row).  One tma_dqn_act launch."""
        obs = torch.as_tensor(np.asarray(observation, dtype=np.float32) if not torch.is_tensor(observation) else observation)
        single = obs.dim() == 1
        if single:
            obs = obs.unsqueeze(0)
        pol = self.policy
        if obs.dim() != 2 or obs.shape[1] != pol.obs_dim:
            raise ValueError(f"observation must have shape [{pol.obs_dim}] or [n, {pol.obs_dim}], got {tuple(np.shape(observation))}")
        pol._sync_if_stepped()
        obs = pol._rows(obs)
        n = obs.shape[0]
        self._predict_counter = getattr(self, "_predict_counter", 0) + 1
        actions = torch.empty((n,), dtype=torch.int32, device=pol.device)
        eps = 0.0 if deterministic else min(max(self.exploration_rate, 0.0), 1.0)
        with torch.cuda.device(pol.device):
            _lib.check(_lib.lib().tma_dqn_act(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), n, eps, (self.seed ^ 0x5EED) & 0xFFFFFFFF,
                                              self._predict_counter & 0xFFFFFFFF, 0, _lib.ptr(actions), None, _lib.stream_ptr(pol.device)))
        a = actions.cpu().numpy().astype(np.int64)
        return (a[0] if single else a), None

    # -- artefacts: SB3's DQN zip (policy.pth: q_net.q_net.* and q_net_target.q_net.*; the optimizer over q_net's six tensors) ------------
    def _q_state(self, pol: HipActorCriticPolicy, prefix: str, flat: torch.Tensor | None = None) -> dict[str, torch.Tensor]:
        named = pol.named_from_flat(pol.params[: pol.n_trainable] if flat is None else flat)
        return {f"{prefix}.{q}": named[p] for q, p in zip(Q_KEYS, PI_KEYS)}

    def _data(self) -> dict:
        from . import sb3_format

        pol, rb = self.policy, self.replay_buffer
        data = {
            "policy_kwargs": sb3_format.policy_kwargs_data(pol.hidden, pol.activation, 0.0, True), "num_timesteps": self.num_timesteps,
            "_total_timesteps": self._total_timesteps, "_num_timesteps_at_start": 0, "seed": self.seed, "action_noise": None, "start_time": time.time_ns(),
            "learning_rate": self.learning_rate, "tensorboard_log": self.tensorboard_log, "_last_obs": None, "_last_episode_starts": None,
            "_last_original_obs": None, "_episode_num": 0, "use_sde": False, "sde_sample_freq": -1, "_current_progress_remaining": 0.0,
            "_stats_window_size": self.stats_window_size, "ep_info_buffer": None, "ep_success_buffer": None, "_n_updates": self._n_updates,
            "n_envs": getattr(self, "n_envs", 1), "buffer_size": self.buffer_size, "batch_size": self.batch_size, "learning_starts": self.learning_starts,
            "tau": self.tau, "gamma": self.gamma, "gradient_steps": self.gradient_steps, "optimize_memory_usage": False, "replay_buffer_class": None,
            "replay_buffer_kwargs": {}, "n_steps": self.n_steps, "train_freq": self.train_freq, "use_sde_at_warmup": False,
            "exploration_initial_eps": self.exploration_initial_eps, "exploration_final_eps": self.exploration_final_eps,
            "exploration_fraction": self.exploration_fraction, "target_update_interval": self.target_update_interval, "_n_calls": self._n_calls,
            "max_grad_norm": self.max_grad_norm, "exploration_rate": self.exploration_rate, "verbose": self.verbose, "_custom_logger": False,
            "tma": {"engine": "three-mlagents_amd", "algorithm": "dqn", "task_id": getattr(self.env, "task_id", None), "mfma_dtype": "f32",
                    "activation": pol.activation, "adam_step": self._adam_step, "obs_dim": pol.obs_dim, "act_dim": pol.act_dim, "continuous": False,
                    "hidden": pol.hidden, "n_calls": self._n_calls, "replay_pos": rb.pos if rb else 0, "replay_full": bool(rb.full) if rb else False,
                    "replay_draw": rb._draw if rb else 0, "collect_step": rb._collect_step if rb else 0},
        }
        data.update(sb3_format.data_members(pol_space(self, "observation_space"), pol_space(self, "action_space"),
                                            policy_class=("stable_baselines3.dqn.policies", "DQNPolicy")))
        return data

    def save(self, path, exclude=None, include=None, _frozen: dict | None = None) -> None:
        """SB3's DQN zip.  The replay buffer is not part of it (SB3: save_replay_buffer); the engine's counters sit under data["tma"]."""
        from . import sb3_format

        path = str(path)
        if not os.path.splitext(path)[1]:
            path += ".zip"
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

        def _pth(obj) -> bytes:
            bio = io.BytesIO()
            torch.save(obj, bio)
            return bio.getvalue()

        sd = {**self._q_state(self.policy, "q_net"), **self._q_state(self.q_net_target, "q_net_target")}
        order = [f"q_net.{q}" for q in Q_KEYS]
        m, v = (self._q_state(self.policy, "q_net", t) for t in (self.exp_avg, self.exp_avg_sq))
        opt = sb3_format.adam_state_dict(order, m, v, self._adam_step, self.learning_rate, eps=ADAM_EPS)
        with zipfile.ZipFile(path, "w") as z:
            z.writestr("data", json.dumps(self._data(), indent=2, default=str))
            z.writestr("policy.pth", _pth(sd))
            z.writestr("policy.optimizer.pth", _pth(opt))
            z.writestr("pytorch_variables.pth", _pth({}))
            z.writestr("_stable_baselines3_version", "2.9.0+three-mlagents_amd")

    def _load_q(self, pol: HipActorCriticPolicy, sd: dict, prefix: str, into: torch.Tensor | None = None) -> None:
        """The six tensors `prefix`.* into the pi segment of `pol` (into: of a moment vector instead); the vf segment keeps what it has."""
        named = pol.named_from_flat(pol.params[: pol.n_trainable] if into is None else into)
        named.update({p: sd[f"{prefix}.{q}"] for q, p in zip(Q_KEYS, PI_KEYS)})
        flat = pol.flat_from_named(named).to(pol.device)
        with torch.no_grad():
            (pol.params[: pol.n_trainable] if into is None else into).copy_(flat)
        if into is None:
            pol.sync()

    @classmethod
    def load(cls, path, env=None, device="auto", **kwargs) -> "DQN":
        """DQN.load(path, env): the zips this class writes.  Without an env the model predicts; with one it trains on.  The replay buffer starts
        empty, as after SB3's load: load_replay_buffer(path) puts back what save_replay_buffer(path) wrote."""
        from . import sb3_format

        path = str(path)
        if not os.path.exists(path) and os.path.exists(path + ".zip"):
            path += ".zip"
        if not os.path.exists(path):
            raise FileNotFoundError(f"Model not found: {path}")
        with zipfile.ZipFile(path) as z:
            data = json.loads(z.read("data").decode())
            sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
            try:
                opt = torch.load(io.BytesIO(z.read("policy.optimizer.pth")), map_location="cpu", weights_only=True)
            except Exception:  # noqa: BLE001
                opt = {}
        tma = data.get("tma") if isinstance(data.get("tma"), dict) else {}
        if str(tma.get("algorithm", "dqn")) != "dqn" or "q_net.q_net.0.weight" not in sd:
            raise ValueError(f"{path} does not hold a DQN model")
        w1, w3 = sd["q_net.q_net.0.weight"], sd["q_net.q_net.4.weight"]
        H, D, A = int(w1.shape[0]), int(w1.shape[1]), int(w3.shape[0])
        num = lambda key, default: default if isinstance(data.get(key, default), dict) or data.get(key) is None else data[key]  # noqa: E731
        pk = data.get("policy_kwargs") if isinstance(data.get("policy_kwargs"), dict) else {}
        # (a zip without either member is SB3's default DQNPolicy: ReLU)
        act = sb3_format.policy_kwargs_from_data(data)["activation_fn"] if (tma.get("activation") or pk.get("activation_fn")) else "relu"
        model = cls("MlpPolicy", None, learning_rate=num("learning_rate", 1e-4), buffer_size=num("buffer_size", 1_000_000),
                    learning_starts=num("learning_starts", 100), batch_size=num("batch_size", 32), tau=num("tau", 1.0), gamma=num("gamma", 0.99),
                    train_freq=num("train_freq", 4), gradient_steps=num("gradient_steps", 1), n_steps=num("n_steps", 1),
                    target_update_interval=num("target_update_interval", 10_000), exploration_fraction=num("exploration_fraction", 0.1),
                    exploration_initial_eps=num("exploration_initial_eps", 1.0), exploration_final_eps=num("exploration_final_eps", 0.05),
                    max_grad_norm=num("max_grad_norm", 10), stats_window_size=num("_stats_window_size", 100),
                    policy_kwargs={"net_arch": [H, H], "activation_fn": act}, seed=num("seed", 0), _init_setup_model=False)
        model.num_timesteps, model._n_updates = int(data.get("num_timesteps", 0)), int(data.get("_n_updates", 0))
        model._total_timesteps = int(data.get("_total_timesteps", 0))
        model._adam_step, model._n_calls = int(tma.get("adam_step", 0)), int(tma.get("n_calls", data.get("_n_calls", 0)))
        if env is not None:
            model.env = env
            model._keep_env_state = not kwargs.get("force_reset", True)
            model._setup_model()
            rb = model.replay_buffer
            rb._draw, rb._collect_step = int(tma.get("replay_draw", 0)), int(tma.get("collect_step", 0))  # (counters are never reused across a save / load)
            state = opt.get("state") or {} if isinstance(opt, dict) else {}
            if len(state) == len(Q_KEYS):
                for moment, vec in (("exp_avg", model.exp_avg), ("exp_avg_sq", model.exp_avg_sq)):
                    model._load_q(model.policy, {f"q_net.{q}": state[i][moment] for i, q in enumerate(Q_KEYS)}, "q_net", into=vec)
        else:
            from .vec_env import _require_gpu

            dev = _require_gpu(None if device == "auto" else device)
            model.device = dev
            model.policy, model.q_net_target = (HipActorCriticPolicy(D, A, False, H, dev, seed=model.seed, activation=act, ortho_init=False) for _ in range(2))
        model._load_q(model.policy, sd, "q_net")
        model._load_q(model.q_net_target, sd, "q_net_target")
        return model
