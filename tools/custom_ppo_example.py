#!/usr/bin/env python3
"""SB3's PPO.train loop, written in torch on the device, with the three options the native train() refuses: clip_range_vf, the target_kl early
stop and a linear learning-rate schedule.  The rollout is the engine's (collect_rollouts); the minibatches are the engine's own
(`model.rollout_buffer.get`, one tma_rollout_gather launch each); the forward and backward of the nets are the HIP kernels behind the
differentiable `policy.evaluate_actions`; the loss arithmetic and Adam are torch on device tensors.  The PPO constructor still refuses the three
arguments: they live in this loop.  Usage: python tools/custom_ppo_example.py [iterations=6] [target_kl=0.01] [lr=1e-3]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from three_mlagents_amd.ppo import PPO  # noqa: E402
from three_mlagents_amd.vec_env import HipVecEnv  # noqa: E402

iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 6
target_kl = float(sys.argv[2]) if len(sys.argv) > 2 else 0.01
lr0 = float(sys.argv[3]) if len(sys.argv) > 3 else 1e-3
clip_range, clip_range_vf, n_epochs, batch_size = 0.2, 0.2, 10, 256

env = HipVecEnv("gridworld", 64, seed=1)
model = PPO("MlpPolicy", env, n_steps=128, batch_size=batch_size, n_epochs=n_epochs, seed=1, policy_kwargs={"net_arch": [64, 64]})
policy = model.policy
opt = torch.optim.Adam(policy.parameters(), lr=lr0, eps=1e-5)   # parameters(): one leaf that aliases the live weights

for it in range(iterations):
    model.collect_rollouts()                                     # the native rollout driver + GAE, reading the weights the loop below stepped
    ret_sum, _, episodes = env.engine.pop_episode_stats()
    for group in opt.param_groups:                               # learning_rate = lambda progress_remaining: progress_remaining * lr0
        group["lr"] = lr0 * (1.0 - it / iterations)
    stopped_at, approx_kl = None, 0.0
    for epoch in range(n_epochs):
        for data in model.rollout_buffer.get(batch_size):        # the minibatches (and their order) the native train() would have used
            values, log_prob, entropy = policy.evaluate_actions(data.observations, data.actions)
            adv = (data.advantages - data.advantages.mean()) / (data.advantages.std() + 1e-8)
            ratio = torch.exp(log_prob - data.old_log_prob)
            policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
            values_pred = data.old_values + torch.clamp(values - data.old_values, -clip_range_vf, clip_range_vf)   # clip_range_vf
            loss = policy_loss + model.ent_coef * -entropy.mean() + model.vf_coef * F.mse_loss(data.returns, values_pred)
            with torch.no_grad():
                log_ratio = log_prob - data.old_log_prob
                approx_kl = float(((torch.exp(log_ratio) - 1) - log_ratio).mean())
            if approx_kl > 1.5 * target_kl:                      # target_kl: stop BEFORE the step, as SB3 does
                stopped_at = epoch
                break
            opt.zero_grad()
            loss.backward()                                      # one tma_policy_evaluate_actions_backward call
            torch.nn.utils.clip_grad_norm_(policy.parameters(), model.max_grad_norm)
            opt.step()
        if stopped_at is not None:
            break
    where = f"early stop by target_kl in epoch {stopped_at}" if stopped_at is not None else f"ran all {n_epochs} epochs"
    print(f"iteration {it}  lr {opt.param_groups[0]['lr']:.2e}  approx_kl {approx_kl:.4f}  {where}  "
          f"ep_rew_mean {ret_sum / max(episodes, 1):+.3f} over {episodes} episodes")
env.close()
