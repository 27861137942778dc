#!/usr/bin/env python3
"""A torch module in front of the device policy, trained end to end: a 256-wide teacher on raw GridWorld observations is distilled into a student
made of a small torch encoder (observations -> 16 features, an nn.Sequential) and a 64-wide device policy with obs_dim = 16, minimising
KL(teacher || student).  One torch optimizer steps the encoder's parameters and the policy's flat leaf together: the loss reaches the policy's
weights through phase (b) of tma_policy_head_vjp and the encoder through its observation gradient (phase (c)), both from one call per backward.
At the end: the largest |dKL/dobs| of the FROZEN teacher on a batch -- a policy on which parameters() was never called, differentiated with respect
to its input.  Usage: python tools/encoder_example.py [steps=300]"""
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
D, A, F = env.obs_dim, env.num_actions, 16
env.close()

teacher = HipActorCriticPolicy(D, A, False, 256, dev, seed=11)   # stands in for a trained 256 x 256 checkpoint; stays frozen
sd = teacher.state_dict()
sd["action_net.weight"] = sd["action_net.weight"] * 40           # (an untrained head is almost uniform: give the teacher opinions)
teacher.load_state_dict(sd)
torch.manual_seed(0)
encoder = torch.nn.Sequential(torch.nn.Linear(D, 32), torch.nn.Tanh(), torch.nn.Linear(32, F)).to(dev)
student = HipActorCriticPolicy(F, A, False, 64, dev, seed=5)     # sees the encoder's features, not the observations
student.enable_obs_grad()                                        # its input is an edge of the autograd graph: the encoder's cotangent

opt = torch.optim.Adam(list(encoder.parameters()) + student.parameters(), lr=1e-3)
for step in range(steps):
    batch = obs[torch.randint(0, obs.shape[0], (256,), device=dev)]
    with torch.no_grad():
        target = teacher.get_distribution(batch).distribution
    loss = kl_divergence(target, student.get_distribution(encoder(batch)).distribution).mean()
    opt.zero_grad()
    loss.backward()                                              # one tma_policy_head_vjp call: leaf.grad and the encoder's cotangent
    opt.step()
    if step % 50 == 0 or step == steps - 1:
        print(f"step {step:4d}  KL {loss.item():.3e}")

# the frozen-policy path: saliency of the teacher's disagreement with the trained student, with respect to the raw observations
teacher.enable_obs_grad()
x = obs[:256].clone().requires_grad_(True)
with torch.no_grad():
    s_dist = student.get_distribution(encoder(x)).distribution
kl_divergence(teacher.get_distribution(x).distribution, s_dist).sum().backward()
assert teacher._leaf is None                                     # parameters() never called: no leaf was made
print(f"frozen teacher: max |dKL/dobs| over {x.shape[0]} observations {x.grad.abs().max().item():.3e}")
