#!/usr/bin/env python3
"""What VecNormalize costs per vector step (HIP events; median and min / max of `reps` timed calls after a warm-up).  Per shape, in us per
vector step: the normalised driver (tma_rollout_collect_norm over T steps / T), the un-normalised tma_rollout_collect at the same shape (what the
wrapper is measured against: it may run a fused chunk kernel; the normalised driver runs one where tma_rollout_norm_plan fuses, else launch by
launch), and the vecnorm step alone (tma_vecnorm_step on the planes of one vector step).  Results: profiles/vecnorm_timing.json.
Usage: python tools/time_vecnorm.py [reps=15] [out=profiles/vecnorm_timing.json]

--fused: the shapes tma_rollout_norm_plan fuses (256 x 256 f32), each in two fresh child processes -- the switch is read once -- the normalised
driver on its fused chunk kernel and with TMA_NO_NORM_FUSED=1 (the per-step composition), and beside them the un-normalised driver, which is the
floor.  `stays_fused`: the fused median is below the per-step arm's minimum of the `reps` calls, the only noise estimate there is.  Results:
profiles/vecnorm_fused_timing.json.
Usage: python tools/time_vecnorm.py --fused [reps=15] [out=profiles/vecnorm_fused_timing.json]"""
import json
import os
import sys

FUSED_SHAPES = [("ball3d", 8, 0), ("brickbreak", 8, 0), ("ant", 8, 0), ("ball3d", 64, 1)]  # task, envs, frozen deterministic evaluation vector

if sys.argv[1:2] == ["--fused"]:  # the parent: starts the children, touches no GPU itself
    import subprocess

    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "vecnorm_fused_timing.json")
    rows, device = [], None
    for task, N, frozen in FUSED_SHAPES:
        arms = {}
        for arm in ("fused", "per_step"):
            e = {k: v for k, v in os.environ.items() if k != "TMA_NO_NORM_FUSED"}
            if arm == "per_step":
                e["TMA_NO_NORM_FUSED"] = "1"
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--fused-child", task, str(N), str(frozen), str(reps)], env=e, check=True,
                                  capture_output=True, text=True, timeout=600)
            arms[arm] = json.loads(done.stdout.strip().splitlines()[-1])
        device = arms["fused"]["device"]
        fused, per_step = arms["fused"]["normalised_driver"], arms["per_step"]["normalised_driver"]
        row = dict(task=task, n_envs=N, hidden=256, frozen_deterministic=bool(frozen), steps_per_rollout=arms["fused"]["steps_per_rollout"],
                   paths=dict(fused=arms["fused"]["path"], per_step=arms["per_step"]["path"]),
                   us_per_vector_step=dict(normalised_fused=fused, normalised_per_step=per_step, plain_driver=arms["fused"]["plain_driver"],
                                           plain_driver_in_per_step_process=arms["per_step"]["plain_driver"]),
                   stays_fused=bool(arms["fused"]["path"] != 0 and fused["median"] < per_step["min"]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    result = dict(device=device, reps=reps, note="us per vector step; a training rollout includes the GAE (and record packing) launch at its end on "
                  "every side; stays_fused: fused median < per-step minimum", shapes=rows)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w", encoding="utf-8") as fh:
        json.dump(result, fh, indent=2)
    print(f"wrote {out_path}")
    sys.exit(0)

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.ppo import PPO  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402
from three_mlagents_amd.vec_normalize import VecNormalize  # noqa: E402

child = sys.argv[1:2] == ["--fused-child"]
reps = int(sys.argv[5]) if child else (int(sys.argv[1]) if len(sys.argv) > 1 else 15)
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


if child:  # one shape in this process: the normalised driver on whatever path the process's switches give it, and the un-normalised one
    import ctypes as C

    task, N, frozen, T = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), 128
    kw = dict(n_steps=T, batch_size=256, seed=1, policy_kwargs={"net_arch": [256, 256]})
    plain = PPO("MlpPolicy", HipVecEnv(task, N, seed=1), **kw)
    wrapped = PPO("MlpPolicy", VecNormalize(HipVecEnv(task, N, seed=1)), **kw)
    venv, L = wrapped.env, _lib.lib()
    if frozen:  # what evaluation runs: frozen statistics (moved by one training rollout first), the mode of the distribution, no last values
        wrapped.collect_rollouts()
        plain.collect_rollouts()
        venv.training = False
        step = [0]

        def run_norm():
            wrapped.buf["obs"][0].copy_(wrapped.buf["obs"][T])
            venv.collect(wrapped.policy.params, wrapped.policy.dims, wrapped._rb, 0, T, T, 1, step[0], 0.99, False, True)
            step[0] += T

        def run_plain():
            eng = plain.env.engine
            plain.buf["obs"][0].copy_(plain.buf["obs"][T])
            _lib.check(L.tma_rollout_collect(eng._h, _lib.ptr(plain.policy.params), C.byref(plain.policy.dims), C.byref(plain._rb), 0, T, T, 1, step[0] & 0xFFFFFFFF,
                                             eng.env_offset & 0xFFFFFFFF, 0.99, 0, 1, _lib.stream_ptr(eng.device)))
            step[0] += T
    else:
        run_norm, run_plain = wrapped.collect_rollouts, plain.collect_rollouts
    res = dict(device=torch.cuda.get_device_name(0), steps_per_rollout=T, normalised_driver=timed(run_norm, T), path=L.tma_debug_last_rollout_norm_path(),
               plain_driver=timed(run_plain, T))
    print(json.dumps(res), flush=True)
    plain.env.close()
    venv.close()
    sys.exit(0)

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
