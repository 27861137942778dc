#!/usr/bin/env python3
"""Time the observation gradient (phase (c) of csrc/tma_vjp.hip) with HIP events: for tma_policy_evaluate_actions and tma_policy_head, the
..._backward call as it is (parameters only), the ..._vjp call with both outputs and the ..._vjp call with grad_obs only (a frozen policy: no
weight-gradient launch).  Shapes of profiles/vjp_timing.json -- (4, 64, 5) and (6, 256, 5) at 256 and 131072 rows -- and, as the case where
obs_dim is not small beside the hidden width, the Box shape (172, 256, 20).  Every entry point is called through the C ABI on preallocated buffers;
the calls of a shape are interleaved so all see the same clocks.  Prints one JSON object; `python tools/time_input_grad.py OUT.json` also writes it
(profiles/input_grad_timing.json)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.ppo import HipActorCriticPolicy  # noqa: E402

DEV = torch.device("cuda", 0)
L = _lib.lib()
SHAPES = [(4, 64, 5, False), (6, 256, 5, False), (172, 256, 20, True)]
ROWS = [256, 131072]


def chain_us(fn, reps, warm=10, rounds=5):
    """median over `rounds` of (HIP-event time of `reps` back-to-back calls) / reps"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    out.sort()
    return out[len(out) // 2]


def shape_timing(D, H, A, cont, n):
    pol = HipActorCriticPolicy(D, A, cont, H, DEV, seed=1)
    g = torch.Generator().manual_seed(n)
    obs = torch.randn(n, D, generator=g).to(DEV)
    actions = (torch.randn(n, A, generator=g) if cont else torch.randint(0, A, (n,), generator=g, dtype=torch.int32)).to(DEV)
    g_head = torch.randn(n, A, generator=g).to(DEV)
    g_v, g_lp, g_ent = (torch.randn(n, generator=g).to(DEV) for _ in range(3))
    grad, grad_obs = torch.empty(pol.n_trainable, device=DEV), torch.empty(n, D, device=DEV)
    need = int(L.tma_policy_vjp_workspace_bytes(C.byref(pol.dims), n))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    P, d, st, p = _lib.ptr(pol.params), C.byref(pol.dims), _lib.stream_ptr(), _lib.ptr

    def ea(gp, go):
        return lambda: _lib.check(L.tma_policy_evaluate_actions_vjp(P, d, p(obs), p(actions), n, p(g_v), p(g_lp), p(g_ent), p(gp), p(go), p(ws), need, st))

    def hd(gp, go):
        return lambda: _lib.check(L.tma_policy_head_vjp(P, d, p(obs), n, p(g_head), p(g_v), p(gp), p(go), p(ws), need, st))

    calls = {
        "evaluate_actions_backward": lambda: _lib.check(L.tma_policy_evaluate_actions_backward(P, d, p(obs), p(actions), n, p(g_v), p(g_lp), p(g_ent), p(grad),
                                                                                                   p(ws), need, st)),
        "evaluate_actions_vjp_both": ea(grad, grad_obs),
        "evaluate_actions_vjp_obs_only": ea(None, grad_obs),
        "head_backward": lambda: _lib.check(L.tma_policy_head_backward(P, d, p(obs), n, p(g_head), p(g_v), p(grad), p(ws), need, st)),
        "head_vjp_both": hd(grad, grad_obs),
        "head_vjp_obs_only": hd(None, grad_obs),
    }
    reps = 400 if n <= 4096 else 40
    us = {}
    for _ in range(2):  # A / B / ... / A / B: the smaller of two interleaved passes
        for name, fn in calls.items():
            t = chain_us(fn, reps)
            us[name] = min(us.get(name, t), t)
    return {"us_per_call": us,
            "evaluate_actions_both_over_backward": us["evaluate_actions_vjp_both"] / us["evaluate_actions_backward"],
            "evaluate_actions_obs_only_over_backward": us["evaluate_actions_vjp_obs_only"] / us["evaluate_actions_backward"],
            "head_both_over_backward": us["head_vjp_both"] / us["head_backward"],
            "head_obs_only_over_backward": us["head_vjp_obs_only"] / us["head_backward"],
            "grad_obs_bytes": n * D * 4, "vjp_workspace_bytes": need, "calls_per_timed_window": reps}


def main():
    res = {"what": "HIP-event time per C ABI call, median of 5 windows, the smaller of two interleaved passes; whole entry points (launches included)",
           "device": torch.cuda.get_device_name(0), "abi": int(L.tma_version()),
           "shapes": {f"{D}x{H}x{A}{'box' if cont else ''}": {str(n): shape_timing(D, H, A, cont, n) for n in ROWS} for D, H, A, cont in SHAPES}}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
