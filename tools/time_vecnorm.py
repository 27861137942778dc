#!/usr/bin/env python3
"""What VecNormalize costs per vector step (HIP events; median and min / max of `reps` timed calls after a warm-up).  Per shape, in us per
vector step: the normalised driver (tma_rollout_collect_norm over T steps / T), the un-normalised tma_rollout_collect at the same shape (what the
wrapper is measured against: it may run a fused chunk kernel, the normalised driver always runs launch by launch), and the vecnorm step alone
(tma_vecnorm_step on the planes of one vector step).  Results: profiles/vecnorm_timing.json.
Usage: python tools/time_vecnorm.py [reps=15] [out=profiles/vecnorm_timing.json]"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.ppo import PPO  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402
from three_mlagents_amd.vec_normalize import VecNormalize  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "vecnorm_timing.json")
SHAPES = [("ball3d", 8, 256, 128), ("ant", 8, 64, 128), ("gridworld", 4096, 64, 64)]  # task, envs, hidden width, steps per timed rollout


def timed(fn, per):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / per)
    us.sort()
    return dict(median=round(us[len(us) // 2], 3), min=round(us[0], 3), max=round(us[-1], 3))


rows = []
for task, N, H, T in SHAPES:
    kw = dict(n_steps=T, batch_size=256, seed=1, policy_kwargs={"net_arch": [H, H]})
    plain = PPO("MlpPolicy", HipVecEnv(task, N, seed=1), **kw)
    wrapped = PPO("MlpPolicy", VecNormalize(HipVecEnv(task, N, seed=1)), **kw)
    venv = wrapped.env
    D = venv.engine.obs_dim
    obs = torch.randn(N, D, device=venv.device)
    rew, tobs = torch.randn(N, device=venv.device), torch.randn(N, D, device=venv.device)
    term = (torch.rand(N, device=venv.device) < 0.1).to(torch.uint8)
    trunc = torch.zeros(N, dtype=torch.uint8, device=venv.device)
    inner = 32  # vecnorm steps per timed call: one step is a few microseconds, below what an event pair resolves

    def step_alone():
        for _ in range(inner):
            _lib.check(_lib.lib().tma_vecnorm_step(venv._h, _lib.ptr(obs), _lib.ptr(rew), _lib.ptr(tobs), _lib.ptr(term), _lib.ptr(trunc), N, 1, _lib.stream_ptr()))

    row = dict(task=task, n_envs=N, hidden=H, obs_dim=D, steps_per_rollout=T, launches_per_vecnorm_step=1 if N <= _lib.VECNORM_ONE_LAUNCH_MAX else 2,
               us_per_vector_step=dict(normalised_driver=timed(wrapped.collect_rollouts, T), plain_driver=timed(plain.collect_rollouts, T),
                                       vecnorm_step_alone=timed(step_alone, inner)))
    print(json.dumps(row), flush=True)
    rows.append(row)
    plain.env.close()
    venv.close()

result = dict(device=torch.cuda.get_device_name(0), reps=reps, one_launch_max=_lib.VECNORM_ONE_LAUNCH_MAX,
              note="us per vector step; collect_rollouts includes the GAE (and record packing) launch at the end of a rollout on both sides", shapes=rows)
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w", encoding="utf-8") as fh:
    json.dump(result, fh, indent=2)
print(f"wrote {out_path}")
