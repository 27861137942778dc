#!/usr/bin/env python3
"""Policy distillation on the device: a 256-wide teacher into a 64-wide student on GridWorld observations, minimising the full
KL(teacher || student) -- a loss on `policy.get_distribution(obs)`, as one writes it against an SB3 policy.  The nets run in the HIP kernels
(`head`, one tma_policy_head call; its backward, one tma_policy_head_backward call), the distribution arithmetic is torch on device tensors:
nothing leaves the device.  Usage: python tools/distill_example.py [steps=300]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
from torch.distributions import kl_divergence  # noqa: E402

from three_mlagents_amd.ppo import HipActorCriticPolicy  # noqa: E402
from three_mlagents_amd.vec_env import HipEnvEngine  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
dev = torch.device("cuda", 0)

env = HipEnvEngine("gridworld", 4096, seed=1)                    # observations: a reset and a few random-action steps of 4096 envs
frames = [env.reset().clone()]
for t in range(0, 16, 4):
    frames.append(env.step(None, n_steps=4, tape_seed=7, tape_t0=t)["obs"].flatten(0, 1).clone())
obs = torch.cat(frames)
D, A = env.obs_dim, env.num_actions
env.close()

teacher = HipActorCriticPolicy(D, A, False, 256, dev, seed=11)   # stands in for a trained 256 x 256 checkpoint
student = HipActorCriticPolicy(D, A, False, 64, dev, seed=5)
sd = teacher.state_dict()
sd["action_net.weight"] = sd["action_net.weight"] * 40           # (an untrained head is almost uniform: give the teacher opinions)
teacher.load_state_dict(sd)

opt = torch.optim.Adam(student.parameters(), lr=1e-3)            # parameters(): one leaf that aliases the live weights
for step in range(steps):
    batch = obs[torch.randint(0, obs.shape[0], (256,), device=dev)]
    with torch.no_grad():
        target = teacher.get_distribution(batch).distribution    # Categorical(logits = the teacher's head)
    loss = kl_divergence(target, student.get_distribution(batch).distribution).mean()
    opt.zero_grad()
    loss.backward()                                              # one tma_policy_head_backward call
    opt.step()                                                   # writes the flat buffer; the next kernel call re-derives its weight copies
    if step % 50 == 0 or step == steps - 1:
        print(f"step {step:4d}  KL {loss.item():.3e}")
with torch.no_grad():
    kl = kl_divergence(teacher.get_distribution(obs).distribution, student.get_distribution(obs).distribution).mean().item()
    agree = (teacher.get_distribution(obs).mode() == student.get_distribution(obs).mode()).float().mean().item()
print(f"KL over all {obs.shape[0]} observations: {kl:.3e}; greedy actions agree on {agree:.3f}")
