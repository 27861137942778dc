"""Emulation of the three-term bf16 split gradient (mfma_dtype = 2, csrc/tma_split3.h) with plain torch on the CPU: the reference (float64) and
the calibration (float32) of the bf16x3 rows of tests/test_policy_dispatch_gpu.py.  Importable without a GPU.

What is modelled -- read from grad_split3_body, not from the header's prose:
  * split3(x): x (an f32) = hi + mid + lo, each term the bf16 round-to-nearest-even of what the previous terms left (split1 / split_quad: the
    __bf16 conversion of gfx950 rounds to nearest even).
  * The forward / backward CHAIN (layer outputs, tanh, the loss, dz3 -> dz2 -> dz1) keeps all six products of order <= 2: it is emulated as plain
    `dtype` arithmetic.  The three dropped products are <= 2^-24 of a product.
  * Every weight-matrix gradient keeps only the three products of order <= 1 (S3_WG0 = 3: the loop `for t = S3_WG0; t < NT`):
        dW = (a_hi + a_mid)^T d_hi + a_hi^T d_mid,
    a = the layer's input (observations / h1 / h2), d = its pre-activation gradient (dz1 / dz2 / dz3: 1/B, the entropy term and vf_coef
    included), both rounded to f32 -- what the kernel holds before it splits -- and split.  The observation tile is stored in three planes
    like the activations (P0 splits px into Xa and Xt), so dW1 loses the same three products: a_lo . d_hi is dropped for observations too.
  * Bias gradients are plain sums of the f32 deltas (sB1 / sB2 / ab3): no split involved.
Where the header and the code differ, the code is emulated.  Two such places: the header's "x = hi + mid + lo ... the split of an f32 is
exact" holds only while the lo term is a normal bf16 (see split3); and its "a product is good to ~2^-16 of its size" describes the weight
gradients alone -- the chain the header's first paragraph describes is the six-product one.
Statistics are sb3_ref.ppo_loss's (the chain is not truncated, so neither are they)."""
import torch

from oracle import sb3_ref

NETS = (("policy_net", "action_net"), ("value_net", "value_net"))


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def split3(x):
    """(hi, mid, lo) of a float32 tensor, as float32 tensors holding bf16 values.  Both residuals are exact in float32 (they have at most 16,
    then 8 significant bits); hi + mid + lo == x unless the third term falls below bf16's normal range (|x| < ~2^-110: bf16 shares float32's
    exponent range, so the residual of a small x is subnormal in bf16 too and loses bits, or is flushed by hardware that flushes denormals)."""
    assert x.dtype == torch.float32
    hi = _bf(x)
    r = x - hi
    mid = _bf(r)
    return hi, mid, _bf(r - mid)


def _wgrad(a, d, dtype, products):
    """d^T a ([out][in], SB3's layout) from the split terms of the f32-rounded operands; products = "kernel" (the three of order <= 1) or "all"
    (every product, and what the rounding to f32 left of a `dtype` operand as a fourth term: the sum is then the plain product, which is what
    the CPU test holds to autograd -- it checks the manual backward and that the terms add up, not the truncation)."""
    ah, am, al = (t.to(dtype) for t in split3(a.float()))
    dh, dm, dl = (t.to(dtype) for t in split3(d.float()))
    if products == "all":
        a, d = a.to(dtype), d.to(dtype)
        return ((dh + dm + dl) + (d - d.float().to(dtype))).t() @ ((ah + am + al) + (a - a.float().to(dtype)))
    return dh.t() @ (ah + am) + dm.t() @ ah


def emulated_grads(sd, rows, idx, dtype, hp, products="kernel"):
    """(grads in SB3 naming, stats) of the PPO loss over rows[idx], manual backward in `dtype` with the split kernel's weight-gradient products
    (float64: the reference; float32: the calibration).  Same contract as _grads / _emulated_grads of test_policy_dispatch_gpu.py.
    Discrete heads only (the kernel has no Box head)."""
    assert "log_std" not in sd
    p = {k: v.detach().to(dtype) for k, v in sd.items()}
    if len(idx) == 0:
        return {k: torch.zeros_like(v) for k, v in p.items()}, None
    x = {k: v[idx] for k, v in rows.items()}
    X32 = x["obs"].float()
    X, old_lp, adv, ret = X32.to(dtype), x["old_lp"].to(dtype), x["adv"].to(dtype), x["ret"].to(dtype)
    acts = x["actions"].long().flatten()
    B = X.shape[0]
    with torch.no_grad():
        _, stats = sb3_ref.ppo_loss(p, X, x["actions"], old_lp, adv, ret, **hp)
        fwd = {}
        for prefix, head in NETS:
            h1 = torch.tanh(X @ p[f"mlp_extractor.{prefix}.0.weight"].t() + p[f"mlp_extractor.{prefix}.0.bias"])
            h2 = torch.tanh(h1 @ p[f"mlp_extractor.{prefix}.2.weight"].t() + p[f"mlp_extractor.{prefix}.2.bias"])
            fwd[prefix] = (h1, h2, h2 @ p[f"{head}.weight"].t() + p[f"{head}.bias"])
        # ---- loss gradient with respect to the head outputs
        logits, values = fwd["policy_net"][2], fwd["value_net"][2].squeeze(-1)
        lp_all = torch.log_softmax(logits, dim=1)
        prob = lp_all.exp()
        logp = lp_all.gather(1, acts.view(-1, 1)).squeeze(1)
        ent = -(prob * lp_all).sum(dim=1)
        a = adv
        if hp["normalize_advantage"] and B > 1:
            a = (a - a.mean()) / (a.std() + 1e-8)
        ratio = torch.exp(logp - old_lp)
        c = hp["clip_range"]
        unclipped = a * ratio <= a * torch.clamp(ratio, 1 - c, 1 + c)  # min() takes the first term (inside the range both are the same number)
        g_lp = torch.where(unclipped, -(a * ratio) / B, torch.zeros_like(a))
        onehot = torch.zeros_like(prob).scatter_(1, acts.view(-1, 1), 1.0)
        dz3_pi = g_lp.unsqueeze(1) * (onehot - prob) + (hp["ent_coef"] / B) * prob * (lp_all + ent.unsqueeze(1))
        dz3_vf = ((hp["vf_coef"] * 2.0 / B) * (values - ret)).unsqueeze(1)
        grads = {}
        for (prefix, head), dz3 in zip(NETS, (dz3_pi, dz3_vf)):
            h1, h2, _ = fwd[prefix]
            grads[f"{head}.weight"], grads[f"{head}.bias"] = _wgrad(h2, dz3, dtype, products), dz3.sum(0)
            dz2 = (dz3 @ p[f"{head}.weight"]) * (1 - h2 * h2)
            grads[f"mlp_extractor.{prefix}.2.weight"], grads[f"mlp_extractor.{prefix}.2.bias"] = _wgrad(h1, dz2, dtype, products), dz2.sum(0)
            dz1 = (dz2 @ p[f"mlp_extractor.{prefix}.2.weight"]) * (1 - h1 * h1)
            grads[f"mlp_extractor.{prefix}.0.weight"], grads[f"mlp_extractor.{prefix}.0.bias"] = _wgrad(X32, dz1, dtype, products), dz1.sum(0)
    return grads, stats
