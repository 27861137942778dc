"""Float64 numpy restatement of SB3's RunningMeanStd and VecNormalize (the published algorithm; SB3 is not a dependency): the yardstick of
tests/test_vecnorm_cpu.py and tests/test_vecnorm_gpu.py.

One deviation from SB3, shared with the engine: the batch mean and variance are formed in float64 (SB3: np.mean / np.var of
the float32 array).  Everything else is SB3's operation order.
"""
import numpy as np


def batch_moments(x):
    """Mean and population variance over axis 0 in float64, two passes (never E[x^2] - E[x]^2)."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.sum(axis=0) / x.shape[0]
    var = np.square(x - mean).sum(axis=0) / x.shape[0]
    return mean, var, x.shape[0]


def merge(mean, var, count, bm, bv, n):
    """RunningMeanStd.update_from_moments, SB3's operation sequence."""
    delta = bm - mean
    tot = count + n
    new_mean = mean + delta * n / tot
    m_a = var * count
    m_b = bv * n
    m_2 = m_a + m_b + np.square(delta) * count * n / tot
    new_var = m_2 / tot
    return new_mean, new_var, tot


class RunningMeanStd:
    def __init__(self, epsilon: float = 1e-4, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = float(epsilon)

    def update(self, x) -> None:
        bm, bv, n = batch_moments(x)
        self.mean, self.var, self.count = merge(self.mean, self.var, self.count, bm, bv, n)


def normalize_obs_with(obs, mean, var, epsilon, clip_obs):
    return np.clip((np.asarray(obs, np.float64) - mean) / np.sqrt(var + epsilon), -clip_obs, clip_obs).astype(np.float32)


def normalize_reward_with(rew, var, epsilon, clip_reward):
    return np.clip(np.asarray(rew, np.float64) / np.sqrt(var + epsilon), -clip_reward, clip_reward).astype(np.float32)


class VecNormalizeRef:
    """VecNormalize over arrays: reset(obs) and step(obs, rewards, dones, terminal_obs) take what the wrapped vector env returned."""

    def __init__(self, num_envs: int, obs_dim: int, training: bool = True, norm_obs: bool = True, norm_reward: bool = True, clip_obs: float = 10.0,
                 clip_reward: float = 10.0, gamma: float = 0.99, epsilon: float = 1e-8):
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.obs_rms, self.ret_rms = RunningMeanStd(shape=(obs_dim,)), RunningMeanStd(shape=())
        self.returns = np.zeros(num_envs, np.float64)
        self.old_obs = self.old_reward = None

    def normalize_obs(self, obs):
        if not self.norm_obs:
            return np.asarray(obs, np.float32)
        return normalize_obs_with(obs, self.obs_rms.mean, self.obs_rms.var, self.epsilon, self.clip_obs)

    def normalize_reward(self, rew):
        if not self.norm_reward:
            return np.asarray(rew, np.float32)
        return normalize_reward_with(rew, self.ret_rms.var, self.epsilon, self.clip_reward)

    def unnormalize_obs(self, obs):
        if not self.norm_obs:
            return np.asarray(obs, np.float32)
        return (np.asarray(obs, np.float64) * np.sqrt(self.obs_rms.var + self.epsilon) + self.obs_rms.mean).astype(np.float32)

    def unnormalize_reward(self, rew):
        if not self.norm_reward:
            return np.asarray(rew, np.float32)
        return (np.asarray(rew, np.float64) * np.sqrt(self.ret_rms.var + self.epsilon)).astype(np.float32)

    def reset(self, obs):
        self.old_obs = np.array(obs, np.float32)
        self.returns = np.zeros_like(self.returns)
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        return self.normalize_obs(obs)

    def step(self, obs, rewards, dones, terminal_obs=None):
        """-> (normalised obs, normalised rewards, terminal_obs with the rows of finished envs normalised)."""
        dones = np.asarray(dones, bool)
        self.old_obs, self.old_reward = np.array(obs, np.float32), np.array(rewards, np.float32)
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        out_obs = self.normalize_obs(obs)
        if self.training:
            self.returns = self.returns * self.gamma + np.asarray(rewards, np.float64)
            self.ret_rms.update(self.returns)
        out_rew = self.normalize_reward(rewards)
        out_tobs = None
        if terminal_obs is not None:
            out_tobs = np.array(terminal_obs, np.float32)
            if dones.any():
                out_tobs[dones] = self.normalize_obs(out_tobs[dones])
        self.returns[dones] = 0.0
        return out_obs, out_rew, out_tobs

    def get_original_obs(self):
        return self.old_obs.copy()

    def get_original_reward(self):
        return self.old_reward.copy()
