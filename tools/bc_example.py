#!/usr/bin/env python3
"""Behaviour cloning on the device policy: the student's evaluate_actions is a node of a torch autograd graph, so the loop is the one
`imitation`'s BC runs on an SB3 policy -- evaluate_actions -> loss.backward() -> optimizer.step().  Usage: python tools/bc_example.py [steps=200]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from three_mlagents_amd.ppo import HipActorCriticPolicy  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda", 0)
teacher = HipActorCriticPolicy(4, 5, False, 64, dev, seed=11)   # stands in for an expert checkpoint
student = HipActorCriticPolicy(4, 5, False, 64, dev, seed=5)
sd = teacher.state_dict()
sd["action_net.weight"] = sd["action_net.weight"] * 40          # (an untrained head is almost uniform: give the expert opinions)
teacher.load_state_dict(sd)

obs = torch.randn(4096, 4, device=dev)                          # recorded observations ...
expert_actions, _, _ = teacher.act(obs, deterministic=True)     # ... and what the expert did there

opt = torch.optim.Adam(student.parameters(), lr=1e-3)           # parameters(): one leaf that aliases the live weights
for step in range(steps):
    idx = torch.randint(0, obs.shape[0], (256,), device=dev)
    _, log_prob, entropy = student.evaluate_actions(obs[idx], expert_actions[idx])
    loss = -log_prob.mean() - 1e-3 * entropy.mean()             # imitation's BC loss: negative log-likelihood + entropy bonus
    opt.zero_grad()
    loss.backward()                                             # one tma_policy_evaluate_actions_backward call
    opt.step()                                                  # writes the flat buffer; the next kernel call re-derives its weight copies
    if step % 50 == 0 or step == steps - 1:
        print(f"step {step:4d}  loss {loss.item():.4f}")
with torch.no_grad():
    picked, _, _ = student.act(obs, deterministic=True)
print(f"agreement with the expert: {(picked == expert_actions).float().mean().item():.3f}")
