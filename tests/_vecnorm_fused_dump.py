"""Helper of tests/test_vecnorm_fused_gpu.py: ONE configuration of a rollout under VecNormalize in a fresh process (TMA_NO_NORM_FUSED is read
once per process, hence a subprocess per arm) -> one .npy per array in a directory.  A 256 x 256 f32 policy collects two consecutive
rollouts through tma_rollout_collect_norm; after each (r = 0, 1) it writes every plane of the rollout buffer, last_values, the terminal
observation slots, the observation and return statistics, returns[N] and the raw observations / rewards of the last step; at the end the
plan value the library reports for its last launch (tma_debug_last_rollout_norm_path).

The configuration is one JSON object on the command line:
  task, n_envs, n_steps, seed      the env vector (ring_depth 16) and the rollout length
  slots                            terminal_obs_slots forced to this many (0: the model's own)
  norm_obs, norm_reward            the wrapper's flags
  frozen                           1: ONE training rollout first (statistics away from their initial values), then the two dumped rollouts with
                                   training = False and deterministic = 1, as evaluation runs them; stats_before.npy holds the statistics in
                                   front of them
  age, age_word                    tasks whose untrained policy does not end an episode within the rollout (Ball3D, Glider): behind the first reset the
                                   step counter -- word age_word of the flat state (include/tma.h tma_env_set_state) -- of envs 1, 3, 5, ... is set
                                   to age - 1, age - 8, age - 15, ..., so with age = the task's step limit those envs reach it at steps 0, 7, 14, ...
                                   of the first rollout; nothing else of the state changes
  poison                           1: tma_debug_poison_lds(0) in front of every rollout -- NaNs in every LDS word a kernel does not write itself
  train                            1: behind the dumps PPO.train() and one whole learn() iteration; params_finite.npy
usage: _vecnorm_fused_dump.py '<json>' out_dir"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.ppo import PPO  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402
from three_mlagents_amd.vec_normalize import VecNormalize  # noqa: E402

cfg, out = json.loads(sys.argv[1]), sys.argv[2]
task, N, T, seed = cfg["task"], int(cfg["n_envs"]), int(cfg["n_steps"]), int(cfg.get("seed", 3))
os.makedirs(out, exist_ok=True)
L = _lib.lib()
env = VecNormalize(HipVecEnv(task, N, seed=seed, ring_depth=16), norm_obs=bool(cfg.get("norm_obs", 1)), norm_reward=bool(cfg.get("norm_reward", 1)))
m = PPO("MlpPolicy", env, n_steps=T, batch_size=64, n_epochs=1, seed=seed, policy_kwargs={"net_arch": [256, 256]})
if cfg.get("slots"):
    m._rb.terminal_obs_slots = int(cfg["slots"])
assert m._rb.terminal_obs_slots <= m.buf["terminal_obs"].shape[0]
if cfg.get("age"):
    env.reset_device(m.buf["obs"][0])  # (what the first collect_rollouts() would do)
    m._last_obs_valid = True
    st = env.engine.get_state()
    idx = torch.arange(1, N, 2, device=st.device)
    st[idx, int(cfg["age_word"])] = (int(cfg["age"]) - 1 - 7 * (idx // 2)).to(st.dtype)
    env.engine.set_state(st)


def stats_array():
    s = env.get_stats()
    return np.concatenate([s["obs_mean"], s["obs_var"], [s["obs_count"], s["ret_mean"], s["ret_var"], s["ret_count"]]]).astype(np.float64)


def collect():
    if cfg.get("poison"):
        _lib.check(L.tma_debug_poison_lds(0, _lib.stream_ptr()))
    if not cfg.get("frozen"):
        assert m.collect_rollouts()
        return
    # what evaluation asks of the driver: frozen statistics, the mode of the distribution; the rollout goes on from the last observation
    m.buf["obs"][0].copy_(m.buf["obs"][T])
    env.collect(m.policy.params, m.policy.dims, m._rb, 0, T, T, m.seed, m._rollout_counter * T, m.gamma, True, True)
    m._rollout_counter += 1


if cfg.get("frozen"):
    assert m.collect_rollouts()  # training: N > 8 here, the per-step composition in either arm
    env.training = False
    torch.cuda.synchronize()
    np.save(os.path.join(out, "stats_before.npy"), stats_array())
for r in range(2):
    collect()
    torch.cuda.synchronize()
    for key in ("obs", "actions", "log_probs", "values", "rewards", "terminated", "truncated", "last_values", "terminal_obs"):
        np.save(os.path.join(out, f"r{r}_{key}.npy"), m.buf[key].cpu().numpy())
    np.save(os.path.join(out, f"r{r}_stats.npy"), stats_array())
    np.save(os.path.join(out, f"r{r}_vn_returns.npy"), env.get_returns())
    np.save(os.path.join(out, f"r{r}_original_obs.npy"), env.get_original_obs())
    np.save(os.path.join(out, f"r{r}_original_reward.npy"), env.get_original_reward())
np.save(os.path.join(out, "path.npy"), np.array(L.tma_debug_last_rollout_norm_path()))
last_plan = (C.c_int32 * 3)()
_lib.check(L.tma_debug_last_rollout_plan(last_plan))
np.save(os.path.join(out, "plan.npy"), np.array(list(last_plan)))  # family, waves, rows (TMA_ROLLOUT_FAMILY_*)
np.save(os.path.join(out, "slots.npy"), np.array(m._rb.terminal_obs_slots))
if cfg.get("train"):
    m.train()
    ok = bool(torch.isfinite(m.policy.params).all())
    m.learn(N * T, reset_num_timesteps=False)  # one whole iteration: rollout through the same driver, GAE, update
    ok = ok and bool(torch.isfinite(m.policy.params).all()) and L.tma_debug_last_rollout_norm_path() == int(np.load(os.path.join(out, "path.npy")))
    np.save(os.path.join(out, "params_finite.npy"), np.array(ok))
env.close()
