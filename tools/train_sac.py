#!/usr/bin/env python3
"""Train SAC natively (three_mlagents_amd.SAC, csrc/tma_sac.hip) on `ant` -- the one Box task of this build whose shape the kernels take -- with the
reference's SAC table (backend/mlagents/training.py:392-403) at one env, three seeds, and record the evaluation curve: every --eval-every steps
a deterministic evaluation of --episodes episodes on a vector of its own.  Reports final / best mean reward per seed as measured; the engine's
ant runs the build's own articulated-chain dynamics, so there is no reference threshold to hold the numbers against, and nothing asserts them.
Prints one JSON object; `python tools/train_sac.py OUT.json [--timesteps N]` also writes it."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from three_mlagents_amd import harness, tasks  # noqa: E402
from three_mlagents_amd.evaluation import evaluate_policy  # noqa: E402
from three_mlagents_amd.sac import SAC  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402


def run_seed(seed: int, budget: int, eval_every: int, episodes: int) -> dict:
    task = tasks.resolve("ant")
    table = harness.model_defaults("sac", task, 1, budget)
    env, eval_env = HipVecEnv("ant", 1, seed=seed), HipVecEnv("ant", episodes, seed=seed + 10_000)
    model = SAC("MlpPolicy", env, seed=seed, **table)
    curve = []
    t0 = time.time()
    mean, std = evaluate_policy(model, eval_env, episodes)
    curve.append({"timesteps": 0, "mean_reward": mean, "std_reward": std})
    while model.num_timesteps < budget:
        model.learn(min(eval_every, budget - model.num_timesteps), reset_num_timesteps=False)
        mean, std = evaluate_policy(model, eval_env, episodes)
        curve.append({"timesteps": model.num_timesteps, "mean_reward": mean, "std_reward": std, "seconds": time.time() - t0, **model.pop_train_stats()})
    torch.cuda.synchronize()
    took = time.time() - t0
    env.close()
    eval_env.close()
    rewards = [c["mean_reward"] for c in curve]
    return {"seed": seed, "table": table, "curve": curve, "initial_mean_reward": rewards[0], "final_mean_reward": rewards[-1],
            "best_mean_reward": float(np.max(rewards)), "n_updates": model._n_updates, "seconds_with_evaluations": took}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--timesteps", type=int, default=60_000)
    ap.add_argument("--eval-every", type=int, default=10_000)
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    a = ap.parse_args()
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("TMA_COMMIT", "unknown")
    res = {"what": "SAC on ant at one env with the reference's table; deterministic evaluation of `episodes` episodes every `eval_every` steps; as measured",
           "device": torch.cuda.get_device_name(0), "commit": commit, "timesteps": a.timesteps, "eval_every": a.eval_every, "episodes": a.episodes,
           "runs": [run_seed(s, a.timesteps, a.eval_every, a.episodes) for s in a.seeds]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
