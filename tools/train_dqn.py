#!/usr/bin/env python3
"""Train the native `DQN` class (three_mlagents_amd/dqn.py, csrc/tma_dqn.hip) with the reference's hyper-parameter table
(backend/mlagents/training.py:343-360: [128, 128] ReLU nets, lr 3e-4, batch 64, train_freq 4, target copy every 1 000 steps, epsilon
1.0 -> 0.03 over 25 % of the run, buffer and learning_starts from total_timesteps) and report the evaluation tools/dqn_example.py uses: the mean
return of the FIRST episode each of 128 greedy envs finishes, ten times over the run.  Basic, and GridWorld with n_steps 1 and 3, three seeds each.
The curves are reported as measured; nothing here asserts a reward (one-env DQN on GridWorld swings around its threshold).
Usage: python tools/train_dqn.py [OUT.json] [--timesteps N] [--seeds 1,2,3]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from three_mlagents_amd import ENGINE_TASKS  # noqa: E402
from three_mlagents_amd.callbacks import BaseCallback  # noqa: E402
from three_mlagents_amd.dqn import DQN  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402

RUNS = [("basic", 1), ("gridworld", 1), ("gridworld", 3)]  # (task, n_steps)


def table(total: int) -> dict:
    return dict(learning_rate=3e-4, buffer_size=max(25_000, min(500_000, total)), learning_starts=min(2_000, max(100, total // 20)), batch_size=64, gamma=0.99,
                train_freq=4, gradient_steps=1, target_update_interval=1_000, exploration_fraction=0.25, exploration_final_eps=0.03,
                policy_kwargs={"net_arch": [128, 128]})


def evaluate(model, eval_env):
    """tools/dqn_example.py evaluate(): greedy, the first episode of each of the 128 envs"""
    obs = eval_env.reset_device()
    eval_env.engine.clear_episode_log()
    with torch.no_grad():
        for _ in range(eval_env.engine.max_episode_steps):
            obs = eval_env.step_device(model.policy.head(obs)[0].argmax(dim=1).to(torch.int32))["obs"][0]
    returns, _, envs, _ = eval_env.engine.pop_episode_log()
    first = {}
    for r, i in zip(returns.tolist(), envs.tolist()):
        first.setdefault(i, r)
    return sum(first.values()) / len(first), len(first)


class EvalEvery(BaseCallback):
    def __init__(self, eval_env, every: int, total: int):
        super().__init__()
        self.eval_env, self.every, self.total, self.next_eval, self.curve = eval_env, every, total, every, []

    def _on_step(self) -> bool:
        t = self.model.num_timesteps
        if t >= self.next_eval or t >= self.total:
            if not self.curve or self.curve[-1]["timesteps"] != t:
                self.next_eval += self.every
                mean_reward, episodes = evaluate(self.model, self.eval_env)
                self.curve.append({"timesteps": t, "epsilon": round(self.model.exploration_rate, 4), "mean_eval_reward": mean_reward, "eval_episodes": episodes,
                                   "n_updates": self.model._n_updates})
        return True


def run(task_name: str, n_steps: int, seed: int, total: int) -> dict:
    task = ENGINE_TASKS[task_name]
    env, eval_env = HipVecEnv(task_name, 1, seed=seed), HipVecEnv(task_name, 128, seed=seed + 1000)
    eval_env.engine.episode_log(128 * eval_env.engine.max_episode_steps)
    model = DQN("MlpPolicy", env, n_steps=n_steps, seed=seed, **table(total))
    cb = EvalEvery(eval_env, max(total // 10, 1), total)
    t0 = time.time()
    model.learn(total, callback=cb)
    torch.cuda.synchronize()
    wall = time.time() - t0
    if not cb.curve or cb.curve[-1]["timesteps"] != model.num_timesteps:
        mean_reward, episodes = evaluate(model, eval_env)
        cb.curve.append({"timesteps": model.num_timesteps, "epsilon": round(model.exploration_rate, 4), "mean_eval_reward": mean_reward, "eval_episodes": episodes,
                         "n_updates": model._n_updates})
    out = {"task": task_name, "n_steps": n_steps, "seed": seed, "timesteps": model.num_timesteps, "reward_threshold": task.reward_threshold,
           "final_mean_eval_reward": cb.curve[-1]["mean_eval_reward"], "best_mean_eval_reward": max(p["mean_eval_reward"] for p in cb.curve),
           "n_updates": model._n_updates, "wall_seconds_with_evaluations": round(wall, 2), "train_loss_last": model.logger_values.get("train/loss"), "curve": cb.curve}
    env.close()
    eval_env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="")
    ap.add_argument("--timesteps", type=int, default=0, help="default: each task's total_timesteps")
    ap.add_argument("--seeds", default="1,2,3")
    args = ap.parse_args()
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("TMA_COMMIT", "unknown")
    res = {"what": "DQN.learn (one env, the reference's DQN table, one native iteration per call under the evaluation callback); evaluation: mean return of the "
                   "first episode of each of 128 greedy envs, ten times over the run; reported as measured, nothing asserted",
           "device": torch.cuda.get_device_name(0), "commit": commit, "runs": []}
    for task_name, n_steps in RUNS:
        total = args.timesteps or ENGINE_TASKS[task_name].total_timesteps
        for seed in (int(s) for s in args.seeds.split(",")):
            r = run(task_name, n_steps, seed, total)
            res["runs"].append(r)
            print(json.dumps({k: v for k, v in r.items() if k != "curve"}), flush=True)
    res["summary"] = {f"{t}_n{n}": {"final": [r["final_mean_eval_reward"] for r in res["runs"] if (r["task"], r["n_steps"]) == (t, n)],
                                    "best": [r["best_mean_eval_reward"] for r in res["runs"] if (r["task"], r["n_steps"]) == (t, n)],
                                    "reward_threshold": ENGINE_TASKS[t].reward_threshold} for t, n in RUNS}
    print(json.dumps(res["summary"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
