"""A2C with the Stable-Baselines3 `A2C` surface: what `ALGORITHMS["a2c"](policy, env, seed=seed, **kwargs)` builds when the reference's
`train_task` is asked for `--algorithm a2c` (algorithm table: backend/mlagents/training.py:31-37; `_default_model_kwargs` hands A2C
only `tensorboard_log` and `verbose`, so every hyper-parameter is SB3's default).

The rollout, the returns, the policy and the loss gradient are the PPO engine's (tma_rollout_collect, tma_gae_flags at gae_lambda = 1, the same
ActorCriticPolicy, the PPO gradient kernels at a clip range that never clips: at ratio = 1 their gradient is A2C's).  New are the optimizer --
SB3's RMSpropTFLike behind clip_grad_norm_, tma_rmsprop_step -- and the schedule: one optimizer step per n_steps = 5 vector steps, 40 samples at
the reference's 8 envs, so whole iterations are issued natively (tma_a2c_iterations_local) wherever no callback has to run between them.
Semantics follow SB3 2.9.0; DESIGN.md section 11 lists where the numerics differ (counter-based sampling as PPO, f32 IEEE step, fixed-order norm).
"""
from __future__ import annotations

import ctypes as C
import json
import time

import torch

from . import _lib
from .ppo import PPO

RMSPROP_ALPHA = 0.99  # SB3 A2C: RMSpropTFLike(alpha=0.99, eps=rms_prop_eps, weight_decay=0)
ADAM_EPS = 1e-5       # use_rms_prop=False: the policy's default Adam(eps=1e-5), as PPO


class A2C(PPO):
    """SB3-shaped A2C whose compute is libtma_hip.so.  Constructor / learn / predict / save / load keep SB3's names and defaults."""

    ALGORITHM = "a2c"

    def __init__(self, policy: str = "MlpPolicy", env=None, learning_rate: float = 7e-4, n_steps: int = 5, gamma: float = 0.99, gae_lambda: float = 1.0,
                 ent_coef: float = 0.0, vf_coef: float = 0.5, max_grad_norm: float = 0.5, rms_prop_eps: float = 1e-5, use_rms_prop: bool = True,
                 use_sde: bool = False, sde_sample_freq: int = -1, normalize_advantage: bool = False, stats_window_size: int | None = None,
                 tensorboard_log: str | None = None, policy_kwargs: dict | None = None, verbose: int = 0, seed: int | None = None, device="auto",
                 _init_setup_model: bool = True, **unused):
        if use_sde:
            raise ValueError("use_sde=True (gSDE) is not supported")
        if callable(learning_rate):
            raise ValueError("schedules are not supported: pass a constant learning_rate (the reference does)")
        self.rms_prop_eps, self.use_rms_prop = float(rms_prop_eps), bool(use_rms_prop)
        self.square_avg = None
        # (batch_size / n_epochs / clip_range: PPO's members, unused here -- one update over the whole rollout)
        super().__init__(policy, env, learning_rate=learning_rate, n_steps=n_steps, batch_size=max(1, int(n_steps)), n_epochs=1, gamma=gamma,
                         gae_lambda=gae_lambda, normalize_advantage=normalize_advantage, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                         policy_kwargs=policy_kwargs, tensorboard_log=tensorboard_log, verbose=verbose, seed=seed, device=device,
                         _init_setup_model=_init_setup_model, stats_window_size=stats_window_size)

    def _setup_model(self) -> None:
        if self.world_size > 1:
            raise ValueError("data-parallel A2C is not supported (world_size > 1)")
        super()._setup_model()
        self.square_avg = torch.ones_like(self.grad)  # RMSpropTFLike: the state starts at ones, not zeros
        self._a2c_hp = _lib.A2CHParams(self.ent_coef, self.vf_coef, 1 if self.normalize_advantage else 0)

    # -- update ---------------------------------------------------------------------------
    def train(self) -> None:
        """SB3 A2C.train: one gradient over the whole rollout, clip_grad_norm_, one optimizer step."""
        L, pol, ws, st = _lib.lib(), self.policy, _lib.ptr(self.workspace), self._stream()
        pol._sync_if_stepped()
        _lib.check(L.tma_ppo_stats_clear(ws, st))  # SB3 logs the last update's losses, not a mean over the log interval
        if self.use_rms_prop:
            _lib.check(L.tma_a2c_update_local(_lib.ptr(pol.params), C.byref(pol.dims), C.byref(self._rollout_view), C.byref(self._a2c_hp), _lib.ptr(self.grad),
                                              _lib.ptr(self.square_avg), self.learning_rate, RMSPROP_ALPHA, self.rms_prop_eps, self.max_grad_norm, ws, st))
        else:
            _lib.check(L.tma_a2c_grad(_lib.ptr(pol.params), C.byref(pol.dims), C.byref(self._rollout_view), C.byref(self._a2c_hp), _lib.ptr(self.grad), ws, st))
            _lib.check(L.tma_ppo_adam_step_local(_lib.ptr(pol.params), _lib.ptr(self.grad), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), C.byref(pol.dims),
                                                 self._adam_step + 1, self.learning_rate, 0.9, 0.999, ADAM_EPS, self.max_grad_norm, ws, st,
                                                 self.n_steps * self.n_envs))
            self._adam_step += 1
        self._n_updates += 1
        self._mark_update_done()

    def _a2c_stats(self, out) -> dict[str, float]:
        n = max(out[5], 1.0)
        return {"train/policy_loss": out[0] / n, "train/value_loss": out[1] / n, "train/entropy_loss": -out[2] / n, "train/grad_norm": out[6],
                "train/n_samples": out[5]}

    def _fold_train_stats(self, staging: torch.Tensor) -> dict[str, float]:
        out = (C.c_double * 8)()
        _lib.check(_lib.lib().tma_a2c_stats_fold(_lib.ptr(staging), out))
        return self._a2c_stats(out)

    def pop_train_stats(self) -> dict[str, float]:
        staging = self._stats_staging(0)
        _lib.check(_lib.lib().tma_ppo_stats_enqueue(_lib.ptr(self.workspace), _lib.ptr(staging), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()
        return self._fold_train_stats(staging)

    def _read_extra_stats(self, host: torch.Tensor) -> dict[str, float]:
        out = super()._read_extra_stats(host)
        out.pop("train/clip_range", None)  # (SB3's A2C logs neither clip_range nor clip_fraction / approx_kl)
        return out

    # -- learn ----------------------------------------------------------------------------
    def learn(self, total_timesteps: int, callback=None, log_interval: int = 100, tb_log_name: str = "A2C", reset_num_timesteps: bool = True,
              progress_bar: bool = False):
        """SB3's learn (log_interval counts iterations, default 100).  With a callback: PPO.learn's loop, one iteration per call, so that the
        callback sees the parameters of the step it fires at.  Without one: the iterations between two log dumps are ONE native call."""
        if callback is not None or not self.use_rms_prop:
            return super().learn(total_timesteps, callback=callback, log_interval=log_interval, tb_log_name=tb_log_name,
                                 reset_num_timesteps=reset_num_timesteps, progress_bar=progress_bar)
        if reset_num_timesteps:
            self.num_timesteps = 0
        else:
            total_timesteps = int(total_timesteps) + self.num_timesteps
        self._total_timesteps = int(total_timesteps)
        L, eng, pol, b = _lib.lib(), self.env.engine, self.policy, self.buf
        pol._sync_if_stepped()
        T, N = self.n_steps, self.n_envs
        per_iter = T * N
        t0 = time.time()
        if getattr(self.env, "monitor_dir", None) and getattr(eng, "_log_cap", 0) == 0:
            eng.episode_log(self.monitor_log_capacity)
        try:  # (a learn() that unwound between a detach and its pop left a detached set behind: drop it)
            eng.pop_detached_episode_log()
        except ValueError:
            pass
        ev0 = torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(self.device))
        iteration, n_logged, t_prev, pending = 0, 0, 0.0, None

        def finish(p):
            p["ev_train"].synchronize()
            stats = self._fold_train_stats(p["staging"])
            stats.update(self._read_extra_stats(p["extra"]))
            elapsed = max(ev0.elapsed_time(p["ev_train"]) * 1e-3, 1e-9)
            stats.update({"time/fps": p["num_timesteps"] / elapsed, "time/iterations": p["iteration"], "time/total_timesteps": p["num_timesteps"],
                          "rollout/ep_rew_mean": p["window"][0], "rollout/ep_len_mean": p["window"][1], "rollout/episodes": p["ep"][2],
                          "train/n_updates": p["n_updates"]})
            self.logger_values = stats
            self._write_progress(stats, p["num_timesteps"])
            if self.verbose >= 1:
                print(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in stats.items()}), flush=True)

        try:
            while self.num_timesteps < total_timesteps:
                remaining = -(-(total_timesteps - self.num_timesteps) // per_iter)
                n = min(remaining, (log_interval - iteration % log_interval) if log_interval else remaining)
                if not self._last_obs_valid:
                    eng.reset(b["obs"][0])
                    self._last_obs_valid = True
                    carry = 0
                else:
                    carry = 1
                _lib.check(L.tma_a2c_iterations_local(eng._h, _lib.ptr(pol.params), C.byref(pol.dims), C.byref(self._rb), _lib.ptr(b["advantages"]),
                                                      _lib.ptr(b["returns"]), _lib.ptr(self._packed) if self._packed is not None else None, T,
                                                      self.seed & 0xFFFFFFFF, self._rollout_counter & 0xFFFFFFFF, eng.env_offset & 0xFFFFFFFF, self.gamma,
                                                      self.gae_lambda, carry, int(n), C.byref(self._a2c_hp), _lib.ptr(self.grad), _lib.ptr(self.square_avg),
                                                      self.learning_rate, RMSPROP_ALPHA, self.rms_prop_eps, self.max_grad_norm, _lib.ptr(self.workspace),
                                                      self._stream()))
                iteration += n
                self._rollout_counter += n
                self._n_updates += n
                self.num_timesteps += n * per_iter
                self._mark_update_done()
                if not (log_interval and iteration % log_interval == 0):
                    continue
                # the row of this log point is finished at the next one (or at the end), when its update is long over: nothing here waits for the
                # call just queued except the read-back of the episode log (PPO.learn's pipelined logging)
                self._enqueue_explained_variance()  # (the last rollout's values / returns planes: the update does not touch them)
                eng.detach_episode_log()
                ev_roll = torch.cuda.Event()
                ev_roll.record(torch.cuda.current_stream(self.device))
                side = self.side_stream()
                side.wait_event(ev_roll)
                ep, lr_, ll_, le_, seen = eng.pop_detached_episode_log(C.c_void_p(side.cuda_stream))
                staging = self._stats_staging(n_logged & 1)
                _lib.check(L.tma_ppo_stats_enqueue(_lib.ptr(self.workspace), _lib.ptr(staging), self._stream()))
                extra = self._enqueue_extra_stats(n_logged & 1)
                n_logged += 1
                ev_train = torch.cuda.Event(enable_timing=True)
                ev_train.record(torch.cuda.current_stream(self.device))
                now = time.time() - t0
                self._write_monitor(ep[0], ep[1], ep[2], t_prev, now, t0, log=(lr_, ll_, le_, seen))
                t_prev = now
                if pending is not None:
                    finish(pending)
                pending = dict(ev_train=ev_train, staging=staging, extra=extra, ep=ep, iteration=iteration, num_timesteps=self.num_timesteps,
                               n_updates=self._n_updates, window=self._episode_window(lr_, ll_, ep[0], ep[1], ep[2]))
            if pending is not None:
                finish(pending)
        except BaseException:
            self._join_monitor_writer(reraise=False)
            raise
        self._join_monitor_writer()
        return self

    # -- artefacts ------------------------------------------------------------------------
    def _data(self) -> dict:
        data = super()._data()
        for key in ("batch_size", "n_epochs", "clip_range", "clip_range_vf", "target_kl"):  # PPO's members: not in an SB3 A2C zip
            data.pop(key, None)
        data.update({"rms_prop_eps": self.rms_prop_eps, "use_rms_prop": self.use_rms_prop})
        data["tma"].update(algorithm="a2c", rollout_counter=self._rollout_counter)  # (sampling counters are never reused, also across a save / load)
        # SB3 keeps `_last_obs` in the zip (load(force_reset=False) goes on from it): the final observations of the last rollout, while they are few
        buf = getattr(self, "buf", None)
        if buf is not None and self._last_obs_valid and buf["obs"][self.n_steps].numel() <= 1 << 16:
            data["tma"]["last_obs"] = buf["obs"][self.n_steps].cpu().tolist()
        return data

    def freeze_for_save(self) -> dict:
        fz = super().freeze_for_save()
        fz["square_avg"] = self.square_avg.clone() if self.square_avg is not None else None
        fz["n_updates"] = self._n_updates
        return fz

    def _optimizer_state_dict(self, order, fz):
        """`policy.optimizer.pth`: RMSpropTFLike's state_dict (Adam's with use_rms_prop=False, as PPO)."""
        if not self.use_rms_prop:
            return super()._optimizer_state_dict(order, fz)
        from . import sb3_format

        sq = self.square_avg if fz is None else fz.get("square_avg")
        steps = self._n_updates if fz is None else fz.get("n_updates", 0)
        return sb3_format.rmsprop_state_dict(order, self.policy.named_from_flat(sq) if sq is not None else {}, steps if sq is not None else 0,
                                             self.learning_rate, RMSPROP_ALPHA, self.rms_prop_eps)

    @classmethod
    def _from_data(cls, data: dict, num, hidden: int, mfma: str, extra_policy_kwargs: dict | None = None):
        return cls(data.get("policy_class", "MlpPolicy") if isinstance(data.get("policy_class"), str) else "MlpPolicy", None,
                   learning_rate=num("learning_rate", 7e-4), n_steps=num("n_steps", 5), gamma=num("gamma", 0.99), gae_lambda=num("gae_lambda", 1.0),
                   ent_coef=num("ent_coef", 0.0), vf_coef=num("vf_coef", 0.5), max_grad_norm=num("max_grad_norm", 0.5),
                   rms_prop_eps=num("rms_prop_eps", 1e-5), use_rms_prop=num("use_rms_prop", True), normalize_advantage=num("normalize_advantage", False),
                   policy_kwargs={"net_arch": [hidden, hidden], "mfma_dtype": mfma, **(extra_policy_kwargs or {})}, seed=num("seed", 0),
                   _init_setup_model=False)

    def _restore_extra(self, tma_extra: dict) -> None:
        self._rollout_counter = int(tma_extra.get("rollout_counter", 0))
        last = tma_extra.get("last_obs")
        if getattr(self, "_keep_env_state", False) and last is not None and getattr(self, "buf", None) is not None:
            self.buf["obs"][self.n_steps].copy_(torch.tensor(last, dtype=torch.float32).reshape(self.buf["obs"][self.n_steps].shape))
            self._last_obs_valid = True

    def _load_optimizer_state(self, state: dict, order) -> None:
        if not self.use_rms_prop:
            return super()._load_optimizer_state(state, order)
        if len(state) == len(order) and all("square_avg" in state[i] for i in range(len(order))):
            self.square_avg.copy_(self.policy.flat_from_named({k: state[i]["square_avg"] for i, k in enumerate(order)}).to(self.device))
