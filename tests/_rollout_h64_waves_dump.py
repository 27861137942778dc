"""Helper of tests/test_rollout_h64_waves_gpu.py: two consecutive rollouts of a 64 x 64 f32 policy through the fused chunk kernel this
process dispatches to (TMA_ROLL4 / TMA_ROLL2 are read once per process, hence a subprocess per kernel) -> one .npy per array in a directory:
every plane of the rollout buffer after each rollout, last_values, advantages / returns, and behind the second rollout the env state, the
episode index, the per-episode Monitor records (ordered by env; per env in the order the episodes ended), the Monitor aggregate and the
number of waves per tile the library reports for its last chunk launch.
`age` > 0 (tasks whose untrained policy never survives to the step limit: Bicycle falls within some forty steps of its 2000): behind the
first reset the step counter of every fourth env -- the last word of the flat state (include/tma.h tma_env_set_state) -- is set to
age - 1 - k, k = 0..31, so those envs reach the limit within 32 steps unless they terminate first; nothing else of the state changes.
usage: _rollout_h64_waves_dump.py task n_envs n_steps deterministic out_dir [age]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.harness import make_vector_env  # noqa: E402
from three_mlagents_amd.ppo import PPO  # noqa: E402

task, N, T, det, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
age = int(sys.argv[6]) if len(sys.argv) > 6 else 0
os.makedirs(out, exist_ok=True)
env = make_vector_env(task, n_envs=N, seed=5)
m = PPO("MlpPolicy", env, n_steps=T, batch_size=max(256, N * T // 4), n_epochs=1, seed=11, policy_kwargs={"net_arch": [64, 64]})
eng = env.engine
eng.episode_log(2 * N * T)  # (one record per env-step of the two rollouts at most: never overflows)
L = _lib.lib()
if age > 0:
    eng.reset(m.buf["obs"][0])  # (what the first collect_rollouts() would do)
    m._last_obs_valid = True
    st = eng.get_state()
    idx = torch.arange(1, N, 4, device=st.device)
    st[idx, -1] = (age - 1 - (idx // 4) % 32).to(st.dtype)
    eng.set_state(st)


def collect():
    if not det:
        assert m.collect_rollouts()
        return
    # PPO.collect_rollouts with the mode of the distribution instead of a sample (what evaluation asks of tma_rollout_collect)
    if not m._last_obs_valid:
        eng.reset(m.buf["obs"][0])
        m._last_obs_valid = True
    else:
        m.buf["obs"][0].copy_(m.buf["obs"][T])
    _lib.check(L.tma_rollout_collect(eng._h, _lib.ptr(m.policy.params), C.byref(m.policy.dims), C.byref(m._rb), 0, T, T, m.seed & 0xFFFFFFFF,
                                     (m._rollout_counter * T) & 0xFFFFFFFF, eng.env_offset & 0xFFFFFFFF, m.gamma, 1, 1, m._stream()))
    m._rollout_counter += 1
    b = m.buf
    _lib.check(L.tma_gae_flags(_lib.ptr(b["rewards"]), _lib.ptr(b["values"]), _lib.ptr(b["terminated"]), _lib.ptr(b["truncated"]), _lib.ptr(b["last_values"]),
                               m.gamma, m.gae_lambda, T, N, _lib.ptr(b["advantages"]), _lib.ptr(b["returns"]), m._stream()))


for r in range(2):
    collect()
    torch.cuda.synchronize()
    for key in ("obs", "actions", "rewards", "values", "log_probs", "terminated", "truncated", "last_values", "advantages", "returns"):
        np.save(os.path.join(out, f"r{r}_{key}.npy"), m.buf[key].cpu().numpy())
np.save(os.path.join(out, "waves.npy"), np.array(L.tma_debug_last_rollout_waves()))
np.save(os.path.join(out, "env_state.npy"), eng.get_state().cpu().numpy())
np.save(os.path.join(out, "episode_index.npy"), eng.episode_index().cpu().numpy())
s_ret, s_len, cnt = eng.pop_episode_stats()
np.save(os.path.join(out, "monitor_sums.npy"), np.array([s_ret, s_len, cnt], np.float64))
rets, lens, envs, seen = eng.pop_episode_log()
assert seen == len(rets), (seen, len(rets))
order = np.argsort(envs, kind="stable")
np.save(os.path.join(out, "episode_returns.npy"), rets[order])
np.save(os.path.join(out, "episode_lengths.npy"), lens[order])
np.save(os.path.join(out, "episode_envs.npy"), envs[order])
env.close()
