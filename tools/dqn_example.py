#!/usr/bin/env python3
"""SB3's DQN loop written over the device pieces, with the reference's hyper-parameter table (backend/mlagents/training.py:343-360): [128, 128]
nets, lr 3e-4, batch 64, train_freq 4, target copy every 1 000 steps, epsilon 1.0 -> 0.03 over 25 % of the run, Huber loss, gradient clip 10.
The data half is `ReplayBuffer` (csrc/tma_replay.hip: collect = Q head -> tma_egreedy_actions -> step_device -> tma_replay_add, no host round
trip; sample = one tma_replay_sample launch, n-step returns included); Q is `policy.head(obs)[0]` of a Discrete HipActorCriticPolicy (the value
net rides along unused), the target net a second policy refreshed from the first; the loss arithmetic and Adam are torch on device tensors.
Prints the mean evaluation reward (greedy, the first episode of each of 128 envs) over time.  The harness still refuses algorithm="dqn": this is an example.
Usage: python tools/dqn_example.py [--task gridworld] [--n-envs 1] [--n-step 1] [--timesteps N] [--seed 1] [--evals 10] [--out curve.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from three_mlagents_amd import ENGINE_TASKS, ReplayBuffer  # noqa: E402
from three_mlagents_amd.ppo import HipActorCriticPolicy  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--task", default="gridworld")
ap.add_argument("--n-envs", type=int, default=1)
ap.add_argument("--n-step", type=int, default=1)
ap.add_argument("--timesteps", type=int, default=0, help="default: the task's total_timesteps")
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--evals", type=int, default=10)
ap.add_argument("--out", default="")
args = ap.parse_args()

task, N = ENGINE_TASKS[args.task], args.n_envs
total = args.timesteps or task.total_timesteps
lr, batch_size, gamma, train_freq, target_interval, eps_fraction, eps_final, max_grad_norm = 3e-4, 64, 0.99, 4, 1000, 0.25, 0.03, 10.0
learning_starts = min(2000, max(100, total // 20))

env, eval_env = HipVecEnv(args.task, N, seed=args.seed), HipVecEnv(args.task, 128, seed=args.seed + 1000)
eval_env.engine.episode_log(128 * eval_env.engine.max_episode_steps)
dev, D, A = env.device, env.observation_space.shape[0], env.action_space.n
# SB3's QNetwork: ReLU layers, torch's default initialisation (both nets start equal, as SB3's target does)
q_net, target_net = (HipActorCriticPolicy(D, A, False, 128, dev, seed=args.seed, activation="relu", ortho_init=False) for _ in range(2))
params = q_net.parameters()                                      # one leaf that aliases the live weights
opt = torch.optim.Adam(params, lr=lr)
rb = ReplayBuffer(max(25_000, min(500_000, total)), D, env.action_space, dev, n_envs=N, n_steps=args.n_step, gamma=gamma, seed=args.seed)


def q_values(obs):
    return q_net.head(obs)[0]


def evaluate():
    """mean return of the FIRST episode each of the 128 greedy envs finishes (every env finishes one within the horizon; counting all the
    episodes of a fixed number of steps would count the short ones more often)"""
    obs = eval_env.reset_device()
    eval_env.engine.clear_episode_log()
    with torch.no_grad():
        for _ in range(eval_env.engine.max_episode_steps):
            obs = eval_env.step_device(q_values(obs).argmax(dim=1).to(torch.int32))["obs"][0]
    returns, _, envs, _ = eval_env.engine.pop_episode_log()      # in the order the episodes finished
    first = {}
    for r, i in zip(returns.tolist(), envs.tolist()):
        first.setdefault(i, r)
    return sum(first.values()) / len(first), len(first)


curve, steps, next_target, next_eval = [], 0, target_interval, total // args.evals
rb.start(env.reset_device())
while steps < total:
    eps = max(eps_final, 1.0 - (1.0 - eps_final) * steps / (eps_fraction * total))
    rb.collect(env, q_values, train_freq, eps)                   # train_freq vector steps, nothing copied to the host
    steps += train_freq * N
    if steps >= learning_starts:
        data = rb.sample(batch_size)
        with torch.no_grad():                                     # y = R_n + (1 - done) * gamma^L * max_a Q_target(s', a)
            y = data.rewards + (1.0 - data.dones) * data.discounts * target_net.head(data.next_observations)[0].max(dim=1).values
        q_taken = q_values(data.observations).gather(1, data.actions.long()[:, None]).squeeze(1)
        loss = F.smooth_l1_loss(q_taken, y)
        opt.zero_grad()
        loss.backward()                                           # one tma_policy_head_vjp call
        torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
        opt.step()
    if steps >= next_target:
        next_target += target_interval
        with torch.no_grad():
            target_net.params[: target_net.n_trainable].copy_(q_net.params[: q_net.n_trainable])
        target_net.sync()
    if steps >= next_eval or steps >= total:
        next_eval += total // args.evals
        mean_reward, episodes = evaluate()
        curve.append({"timesteps": steps, "epsilon": round(eps, 4), "mean_eval_reward": mean_reward, "eval_episodes": episodes})
        print(f"timesteps {steps:>8}  epsilon {eps:.3f}  mean eval reward {mean_reward:+.4f} over {episodes} episodes", flush=True)
result = {"task": args.task, "n_envs": N, "n_step": args.n_step, "timesteps": total, "seed": args.seed, "reward_threshold": task.reward_threshold,
          "final_mean_eval_reward": curve[-1]["mean_eval_reward"], "curve": curve}
print(json.dumps({k: v for k, v in result.items() if k != "curve"}))
if args.out:
    with open(args.out, "w", encoding="utf-8") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
env.close()
eval_env.close()
