#!/usr/bin/env python3
"""Train TD3 natively (three_mlagents_amd.TD3, csrc/tma_td3.hip) on `ant` -- the one Box task of this build whose shape the kernels take -- with the
reference's table (it gives TD3 the values it gives SAC, backend/mlagents/training.py:392-403) at one env, three seeds, with and without
NormalActionNoise(0, 0.1), and record the evaluation curve: every --eval-every steps an evaluation of --episodes episodes on a vector of its own.
Reports final / best mean reward per run as measured, beside SAC's figures where profiles/sac_native.json is present; the engine's ant runs the
build's own articulated-chain dynamics, so there is no reference threshold to hold the numbers against, and nothing asserts them.
Prints one JSON object; `python tools/train_td3.py OUT.json [--timesteps N]` also writes it."""
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
from three_mlagents_amd.td3 import TD3, NormalActionNoise  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402


def run_seed(seed: int, budget: int, eval_every: int, episodes: int, sigma: float | None) -> dict:
    task = tasks.resolve("ant")
    table = harness.model_defaults("sac", task, 1, budget)  # the reference's off-policy table: the same for td3
    env, eval_env = HipVecEnv("ant", 1, seed=seed), HipVecEnv("ant", episodes, seed=seed + 10_000)
    noise = None if sigma is None else NormalActionNoise(np.zeros(8), sigma * np.ones(8))
    model = TD3("MlpPolicy", env, seed=seed, action_noise=noise, **table)
    curve = []
    t0 = time.time()
    mean, std = evaluate_policy(model, eval_env, episodes)
    curve.append({"timesteps": 0, "mean_reward": mean, "std_reward": std})
    while model.num_timesteps < budget:
        model.learn(min(eval_every, budget - model.num_timesteps), reset_num_timesteps=False)
        mean, std = evaluate_policy(model, eval_env, episodes)
        curve.append({"timesteps": model.num_timesteps, "mean_reward": mean, "std_reward": std, "seconds": time.time() - t0, **model.pop_train_stats()})
        print(f"seed {seed} sigma {sigma}: {model.num_timesteps} steps, mean reward {mean:.2f}", file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    took = time.time() - t0
    env.close()
    eval_env.close()
    rewards = [c["mean_reward"] for c in curve]
    return {"seed": seed, "action_noise_sigma": sigma, "table": table, "curve": curve, "initial_mean_reward": rewards[0], "final_mean_reward": rewards[-1],
            "best_mean_reward": float(np.max(rewards)), "n_updates": model._n_updates, "actor_updates": model._actor_adam_step,
            "seconds_with_evaluations": took}


def sac_summary():
    """SAC's figures from profiles/sac_native.json, as recorded there (None where the file is absent)."""
    try:
        with open(os.path.join(ROOT, "profiles", "sac_native.json"), encoding="utf-8") as fh:
            sac = json.load(fh)
    except OSError:
        return None
    return [{k: r[k] for k in ("seed", "initial_mean_reward", "final_mean_reward", "best_mean_reward")} for r in sac.get("runs", [])]


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
    res = {"what": "TD3 on ant at one env with the reference's table, without action noise and with NormalActionNoise(0, 0.1); evaluation of `episodes` "
                   "episodes every `eval_every` steps; as measured",
           "device": torch.cuda.get_device_name(0), "commit": commit, "timesteps": a.timesteps, "eval_every": a.eval_every, "episodes": a.episodes,
           "runs": [run_seed(s, a.timesteps, a.eval_every, a.episodes, sigma) for sigma in (None, 0.1) for s in a.seeds],
           "sac_on_the_same_task": sac_summary()}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
