"""CPU references for tests/test_policy_head_gpu.py, all through oracle/sb3_ref.py forward (logits or mean, values): float64 autograd of a linear
functional of the head, the head cotangent that evaluate_actions' three cotangents imply, and the KL / distillation restatements."""
import torch

from oracle import sb3_ref


def double(sd, grad=False):
    return {k: v.double().clone().requires_grad_(grad) for k, v in sd.items()}


def forward64(sd, obs):
    with torch.no_grad():
        return sb3_ref.forward(double(sd), obs.double())


def grads(sd64):
    return {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in sd64.items()}


def head_grad(sd, obs, g_head, g_values):
    """SB3-named float64 gradients of  sum g_head . head + sum g_values . V  (a cotangent may be None)"""
    sd64 = double(sd, grad=True)
    head, values = sb3_ref.forward(sd64, obs.double())
    loss = 0.0
    if g_head is not None:
        loss = loss + (g_head.double() * head).sum()
    if g_values is not None:
        loss = loss + (g_values.double() * values).sum()
    loss.backward()
    return grads(sd64)


def implied_head_cotangent(sd, obs, actions, g_logp, g_entropy):
    """d(sum g_logp logp + g_entropy H) / d head, formed by hand in float64.
    Categorical: g_logp (onehot - p) + g_entropy dH/dlogits, dH/dlogits_j = -p_j (log p_j + H).  Gaussian: g_logp (a - mu) / sigma^2 (the entropy
    does not depend on the mean)."""
    head, _ = forward64(sd, obs)
    if "log_std" in sd:
        return (g_logp.double()[:, None] * (actions.double() - head) / (2.0 * sd["log_std"].double()).exp()).float()
    logp = torch.log_softmax(head, dim=1)
    p = logp.exp()
    ent = -(p * logp).sum(dim=1, keepdim=True)
    onehot = torch.nn.functional.one_hot(actions.long(), head.shape[1]).double()
    return (g_logp.double()[:, None] * (onehot - p) - g_entropy.double()[:, None] * p * (logp + ent)).float()


def distribution(sd, obs):
    """torch distribution of sb3_ref.forward's head at the dtype of sd / obs"""
    head, _ = sb3_ref.forward(sd, obs)
    if "log_std" in sd:
        return torch.distributions.Normal(head, torch.ones_like(head) * sd["log_std"].exp())
    return torch.distributions.Categorical(logits=head)


def kl_grad(teacher_sd, student_sd, obs):
    """float64 autograd of  kl_divergence(teacher, student).mean()  with respect to the student: (loss, SB3-named gradients)"""
    s64 = double(student_sd, grad=True)
    with torch.no_grad():
        t = distribution(double(teacher_sd), obs.double())
    loss = torch.distributions.kl_divergence(t, distribution(s64, obs.double())).mean()
    loss.backward()
    return loss.item(), grads(s64)


def distill(teacher_sd, student_sd, obs, dtype, steps, lr=1e-3):
    """`steps` Adam steps on the full KL from a fixed teacher, on the CPU at `dtype`: (first loss, last loss)"""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in student_sd.items()}
    with torch.no_grad():
        t = distribution({k: v.to(dtype) for k, v in teacher_sd.items()}, obs.to(dtype))
    opt = torch.optim.Adam(list(sd.values()), lr=lr)
    kl = lambda: torch.distributions.kl_divergence(t, distribution(sd, obs.to(dtype))).mean()  # noqa: E731
    first = kl().item()
    for _ in range(steps):
        opt.zero_grad()
        kl().backward()
        opt.step()
    with torch.no_grad():
        return first, kl().item()
