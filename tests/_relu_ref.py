"""float64-capable CPU restatement of SB3's ActorCriticPolicy(MlpPolicy) with the hidden activation as an ARGUMENT -- TEST INFRASTRUCTURE ONLY.

oracle/sb3_ref.py is tanh-only and frozen; this holds the same functions (forward, evaluate_actions, ppo_loss) with `activation` in
("tanh", "relu"), plus what a comparison of an f32 ReLU kernel with a float64 reference needs: the hidden pre-activations, so that a test can
assert FIRST that no row sits on the kink (a mask bit that differs between the two precisions is a real, large difference, not rounding), and the
CPU twin of tests/test_policy_vjp_gpu.py::_policy's weights.
"""
from __future__ import annotations

import torch

from oracle.sb3_ref import KEYS

KINK_MARGIN = 5e-5  # an f32 dot product of <= 256 terms of order 1 is off by about 1e-5 at worst


def _act(name):
    return {"tanh": torch.tanh, "relu": torch.relu}[name]


def preactivations(sd, obs):
    """[z1_pi, z2_pi, z1_vf, z2_vf] of a ReLU policy: the hidden pre-activations of both layers of both nets, every row."""
    lin, out = torch.nn.functional.linear, []
    for base in (0, 6):
        z1 = lin(obs, sd[KEYS[base]], sd[KEYS[base + 1]])
        z2 = lin(torch.relu(z1), sd[KEYS[base + 2]], sd[KEYS[base + 3]])
        out += [z1, z2]
    return out


def kink_margin(sd, obs) -> float:
    """min |z| over every hidden pre-activation, in float64"""
    sd64 = {k: v.double() for k, v in sd.items()}
    return min(float(z.abs().min()) for z in preactivations(sd64, obs.double()))


def forward(sd, obs, activation="relu"):
    """latent_pi / latent_vf -> (logits or mean, values[B]): sb3_ref.forward with the activation chosen."""
    lin, f = torch.nn.functional.linear, _act(activation)
    hp = f(lin(f(lin(obs, sd[KEYS[0]], sd[KEYS[1]])), sd[KEYS[2]], sd[KEYS[3]]))
    hv = f(lin(f(lin(obs, sd[KEYS[6]], sd[KEYS[7]])), sd[KEYS[8]], sd[KEYS[9]]))
    return lin(hp, sd[KEYS[4]], sd[KEYS[5]]), lin(hv, sd[KEYS[10]], sd[KEYS[11]]).flatten()


def evaluate_actions(sd, obs, actions, activation="relu"):
    """ActorCriticPolicy.evaluate_actions -> values, log_prob, entropy."""
    out, values = forward(sd, obs, activation)
    if "log_std" in sd:
        dist = torch.distributions.Normal(out, torch.ones_like(out) * sd["log_std"].exp())
        return values, dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)
    dist = torch.distributions.Categorical(logits=out)
    return values, dist.log_prob(actions.long().flatten()), dist.entropy()


def ppo_loss(sd, obs, actions, old_log_prob, advantages, returns, *, activation="relu", clip_range=0.2, ent_coef=0.01, vf_coef=0.5,
             normalize_advantage=True):
    """sb3_ref.ppo_loss (PPO.train's loop body, clip_range_vf = target_kl = None) through evaluate_actions above."""
    values, log_prob, entropy = evaluate_actions(sd, obs, actions, activation)
    adv = advantages
    if normalize_advantage and len(adv) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(log_prob - old_log_prob)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    value_loss = torch.nn.functional.mse_loss(returns, values)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        log_ratio = log_prob - old_log_prob
        stats = dict(policy_loss=float(policy_loss), value_loss=float(value_loss), entropy_loss=float(entropy_loss),
                     approx_kl=float(torch.mean((torch.exp(log_ratio) - 1) - log_ratio)),
                     clip_fraction=float(torch.mean((torch.abs(ratio - 1) > clip_range).float())), loss=float(loss))
    return loss, stats


def policy_sd(D, H, A, cont, seed=5):
    """The weights tests/test_policy_vjp_gpu.py::_policy loads, built on the CPU: the engine's own initialisation, heads made non-trivial (the
    gain-0.01 init gives almost uniform logits), non-zero biases and log_std."""
    from three_mlagents_amd.ppo import orthogonal_init

    sd = orthogonal_init(D, H, A, cont, seed)
    if cont:
        sd["log_std"] = torch.linspace(-0.7, 0.3, A)
    g = torch.Generator().manual_seed(seed)
    sd["action_net.weight"] = sd["action_net.weight"] * 40 + 0.05 * torch.randn(sd["action_net.weight"].shape, generator=g)
    sd["action_net.bias"] = 0.1 * torch.randn(sd["action_net.bias"].shape, generator=g)
    for k in list(sd):
        if k.endswith("bias") and k != "action_net.bias":
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    return sd


def clear_obs(sd, D, n, seed):
    """n rows of randn(., D) from the seeded CPU generator, in draw order, SKIPPING every row with a hidden pre-activation (float64) closer than
    KINK_MARGIN to zero.  (Whole batches that are clear by luck exist only at small n: among 256 seeds there is none for 33 rows at (4, 320), for
    48 rows at (6, 256) or for 272 rows at any of the tested shapes, so the rows are screened one by one -- the condition is per row anyway.)"""
    g, sd64, rows, have = torch.Generator().manual_seed(seed), {k: v.double() for k, v in sd.items()}, [], 0
    while have < n:
        cand = torch.randn(2 * n + 16, D, generator=g)
        margin = torch.stack([z.abs().min(dim=1).values for z in preactivations(sd64, cand.double())]).min(dim=0).values
        rows.append(cand[margin >= KINK_MARGIN])
        have += rows[-1].shape[0]
    return torch.cat(rows)[:n].contiguous()
