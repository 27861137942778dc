"""SB3's `VecNormalize` on the device: running mean / variance of the observations and of the per-env discounted returns, kept and applied by
HIP kernels (csrc/tma_vecnorm.hip, include/tma.h `tma_vecnorm_*`), never on the host.

    venv = VecNormalize(make_vector_env("ant", n_envs=8, seed=1))
    model = PPO("MlpPolicy", venv, ...)          # collect_rollouts runs tma_rollout_collect_norm: the buffer holds normalised values
    model.learn(...)
    venv.save("vecnormalize.npz")
    action, _ = model.predict(venv.normalize_obs(raw_obs))   # predict does not normalise, as in SB3

Constructor names and defaults are SB3's.  A `VecNormalize` is a `HipVecEnv` (same engine, same spaces), so it is accepted wherever one is; a
plain `HipVecEnv` takes exactly the code path it took before this class existed.

What stays RAW: Monitor rows, `rollout/ep_rew_mean`, `ep_len_mean` and the returns `evaluate_policy` reports.  They come from the engine's episode
log, which the env kernel fills below this wrapper -- as SB3's Monitor sits inside VecNormalize.

One deviation from SB3: a batch's mean and variance are formed in float64 in a fixed order (SB3: np.mean / np.var of the
float32 array); the two agree to float32 rounding of the batch moments, and the ones here are reproducible bit for bit.

File format: `save(path)` writes an `.npz` with the six statistics and the hyper-parameters -- not SB3's pickle, which pickles an instance of an
SB3 class.  INTEGRATION.md shows how to move the arrays into an SB3 VecNormalize.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .vec_env import HipVecEnv

ONE_LAUNCH_MAX = _lib.VECNORM_ONE_LAUNCH_MAX  # up to this many envs a training step is one kernel launch (include/tma.h)
_FILE_KEYS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "clip_obs", "clip_reward", "gamma", "epsilon", "norm_obs",
              "norm_reward")


class _RunningMeanStdView:
    """`.mean`, `.var`, `.count` of one of the two running statistics as numpy float64, read from the device on every access."""

    def __init__(self, owner: "VecNormalize", which: str):
        self._owner, self._which = owner, which

    def _get(self, key: str):
        return self._owner.get_stats()[f"{self._which}_{key}"]

    mean = property(lambda self: self._get("mean"))
    var = property(lambda self: self._get("var"))
    count = property(lambda self: self._get("count"))


class VecNormalize(HipVecEnv):
    """SB3 `VecNormalize` around a `HipVecEnv`; all statistics are float64 in device memory."""

    def __init__(self, venv: HipVecEnv, training: bool = True, norm_obs: bool = True, norm_reward: bool = True, clip_obs: float = 10.0,
                 clip_reward: float = 10.0, gamma: float = 0.99, epsilon: float = 1e-8):
        if not isinstance(venv, HipVecEnv) or isinstance(venv, VecNormalize):
            raise ValueError("VecNormalize wraps a three_mlagents_amd HipVecEnv (use make_vector_env), and only once")
        self.venv = venv
        self.engine = venv.engine
        # HipVecEnv.__init__ is NOT called (it would build a second engine): the wrapper shares the wrapped vector's engine and copies the
        # attributes that __init__ sets.  An attribute added to HipVecEnv.__init__ must be added to this list too --
        # tests/test_vecnorm_gpu.py::test_wrapper_carries_every_attribute_of_the_vector compares the two attribute sets.
        for name in ("task_id", "num_envs", "observation_space", "action_space", "device", "render_mode", "_t_start", "reset_infos"):
            setattr(self, name, getattr(venv, name))
        self.monitor_dir = getattr(venv, "monitor_dir", None)
        self._actions = None
        self.training = bool(training)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = float(clip_obs), float(clip_reward), float(gamma), float(epsilon)
        self._norm_obs, self._norm_reward = bool(norm_obs), bool(norm_reward)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().tma_vecnorm_create(self.engine.obs_dim, self.num_envs, int(self._norm_obs), int(self._norm_reward), self.clip_obs,
                                                 self.clip_reward, self.gamma, self.epsilon, self.device.index, C.byref(self._h)))
        self.obs_rms, self.ret_rms = _RunningMeanStdView(self, "obs"), _RunningMeanStdView(self, "ret")

    # -- flags (settable after construction, as in SB3) ------------------------------------
    def _set_flags(self, norm_obs: bool, norm_reward: bool) -> None:
        _lib.check(_lib.lib().tma_vecnorm_set_flags(self._h, int(norm_obs), int(norm_reward)))
        self._norm_obs, self._norm_reward = bool(norm_obs), bool(norm_reward)

    norm_obs = property(lambda self: self._norm_obs, lambda self, v: self._set_flags(bool(v), self._norm_reward))
    norm_reward = property(lambda self: self._norm_reward, lambda self, v: self._set_flags(self._norm_obs, bool(v)))

    def _stream(self):
        return _lib.stream_ptr(self.device)

    # -- device API ------------------------------------------------------------------------
    def reset_device(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """Engine reset, then VecNormalize.reset() in place: returns zeroed, statistics updated (training and norm_obs), observations normalised."""
        obs = self.engine.reset(out)
        _lib.check(_lib.lib().tma_vecnorm_reset(self._h, _lib.ptr(obs), self.num_envs, int(self.training), self._stream()))
        return obs

    def step_device(self, actions: torch.Tensor, **kw) -> dict[str, torch.Tensor]:
        """One engine step, then VecNormalize.step_wait() on its outputs in place (obs, rew and the terminal observations of finished envs)."""
        if int(kw.get("n_steps", 1)) != 1:
            raise ValueError("VecNormalize steps one vector step at a time (the statistics change between steps)")
        out = self.engine.step(actions, **kw)
        tobs = out.get("term_obs") if kw.get("want_terminal_obs", True) else None
        _lib.check(_lib.lib().tma_vecnorm_step(self._h, _lib.ptr(out["obs"]), _lib.ptr(out["rew"]), _lib.ptr(tobs), _lib.ptr(out["term"]),
                                               _lib.ptr(out["trunc"]), self.num_envs, int(self.training), self._stream()))
        return out

    def collect(self, params, dims, rb, t_begin: int, t_end: int, T: int, rng_seed: int, rng_step0: int, gamma: float, compute_last_values: bool,
                deterministic: bool) -> None:
        """tma_rollout_collect_norm on this env and its statistics (PPO.collect_rollouts and evaluation.py call it)."""
        eng = self.engine
        _lib.check(_lib.lib().tma_rollout_collect_norm(eng._h, self._h, _lib.ptr(params), C.byref(dims), C.byref(rb), t_begin, t_end, T, rng_seed & 0xFFFFFFFF,
                                                       rng_step0 & 0xFFFFFFFF, eng.env_offset & 0xFFFFFFFF, gamma, int(compute_last_values),
                                                       int(deterministic), int(self.training), self._stream()))

    # -- normalisation with the current statistics ------------------------------------------
    def _map(self, fn_name: str, x, width: int):
        is_tensor = torch.is_tensor(x)
        t = x if is_tensor else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        shape = t.shape
        src = t.to(self.device, torch.float32).reshape(-1, width).contiguous() if width > 1 else t.to(self.device, torch.float32).reshape(-1).contiguous()
        out = torch.empty_like(src)
        _lib.check(getattr(_lib.lib(), fn_name)(self._h, _lib.ptr(src), _lib.ptr(out), src.shape[0], self._stream()))
        out = out.reshape(shape)
        return out if is_tensor else out.cpu().numpy()

    def normalize_obs(self, obs):
        """float32(clip((obs - mean) / sqrt(var + epsilon), +-clip_obs)) computed in float64; numpy in, numpy out; tensor in, tensor out."""
        return self._map("tma_vecnorm_normalize_obs", obs, self.engine.obs_dim)

    def unnormalize_obs(self, obs):
        return self._map("tma_vecnorm_unnormalize_obs", obs, self.engine.obs_dim)

    def normalize_reward(self, reward):
        return self._map("tma_vecnorm_normalize_reward", reward, 1)

    def unnormalize_reward(self, reward):
        return self._map("tma_vecnorm_unnormalize_reward", reward, 1)

    def get_original_obs(self) -> np.ndarray:
        """The raw observations of the last reset / step, bit for bit."""
        out = torch.empty((self.num_envs, self.engine.obs_dim), dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().tma_vecnorm_get_original(self._h, _lib.ptr(out), None, self._stream()))
        return out.cpu().numpy()

    def get_original_reward(self) -> np.ndarray:
        out = torch.empty((self.num_envs,), dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().tma_vecnorm_get_original(self._h, None, _lib.ptr(out), self._stream()))
        return out.cpu().numpy()

    # -- statistics --------------------------------------------------------------------------
    def get_stats(self) -> dict:
        D = self.engine.obs_dim
        mean, var, sc = np.empty(D, np.float64), np.empty(D, np.float64), np.empty(4, np.float64)
        _lib.check(_lib.lib().tma_vecnorm_get_stats(self._h, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(sc), self._stream()))
        return dict(obs_mean=mean, obs_var=var, obs_count=np.float64(sc[0]), ret_mean=np.float64(sc[1]), ret_var=np.float64(sc[2]), ret_count=np.float64(sc[3]))

    def set_stats(self, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count) -> None:
        D = self.engine.obs_dim
        mean, var = (np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1)) for a in (obs_mean, obs_var))
        if mean.size != D or var.size != D:
            raise ValueError(f"observation statistics have {mean.size} / {var.size} elements, the env has {D} observations")
        sc = np.array([float(obs_count), float(ret_mean), float(ret_var), float(ret_count)], np.float64)
        _lib.check(_lib.lib().tma_vecnorm_set_stats(self._h, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(sc), self._stream()))

    def get_returns(self) -> np.ndarray:
        """The per-env discounted returns (float64)."""
        out = np.empty(self.num_envs, np.float64)
        _lib.check(_lib.lib().tma_vecnorm_get_returns(self._h, _lib.ptr(out), self._stream()))
        return out

    # -- persistence -------------------------------------------------------------------------
    def save(self, path) -> None:
        """The six statistics and the hyper-parameters as an .npz (numpy appends the suffix when `path` has none)."""
        s = self.get_stats()
        np.savez(path, **s, clip_obs=np.float64(self.clip_obs), clip_reward=np.float64(self.clip_reward), gamma=np.float64(self.gamma),
                 epsilon=np.float64(self.epsilon), norm_obs=np.bool_(self._norm_obs), norm_reward=np.bool_(self._norm_reward))

    @classmethod
    def load(cls, path, venv: HipVecEnv) -> "VecNormalize":
        """SB3's VecNormalize.load(load_path, venv): a wrapper around `venv` with the saved statistics and hyper-parameters (training = True)."""
        import os

        p = os.fspath(path)
        with np.load(p if os.path.exists(p) else p + ".npz") as z:
            d = {k: z[k] for k in _FILE_KEYS}
        self = cls(venv, training=True, norm_obs=bool(d["norm_obs"]), norm_reward=bool(d["norm_reward"]), clip_obs=float(d["clip_obs"]),
                   clip_reward=float(d["clip_reward"]), gamma=float(d["gamma"]), epsilon=float(d["epsilon"]))
        self.set_stats(d["obs_mean"], d["obs_var"], d["obs_count"], d["ret_mean"], d["ret_var"], d["ret_count"])
        return self

    # -- lifetime ----------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            _lib.lib().tma_vecnorm_destroy(self._h)
            self._h = None
        self.venv.close()

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h:
                _lib.lib().tma_vecnorm_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001
            pass

    def env_is_wrapped(self, wrapper_class, indices=None):
        n = self.num_envs if indices is None else len(list(np.atleast_1d(indices)))
        return [getattr(wrapper_class, "__name__", "") in ("Monitor", "VecNormalize")] * n


def sync_envs_normalization(src, dst) -> None:
    """SB3's sync_envs_normalization(env, eval_env): dst's statistics become src's, device to device on the current stream.  A no-op unless both
    are VecNormalize (SB3 walks both wrapper chains in step and copies where both sides are a VecNormalize)."""
    if isinstance(src, VecNormalize) and isinstance(dst, VecNormalize):
        _lib.check(_lib.lib().tma_vecnorm_copy_stats(dst._h, src._h, _lib.stream_ptr(dst.device)))
