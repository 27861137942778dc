#!/usr/bin/env python3
"""Time tma_policy_head next to the kernels it shares, and tma_policy_head_backward next to tma_policy_evaluate_actions_backward, with HIP events:
(4, 64, 5) -- the H = 64 weight-image family -- and (6, 256, 5) -- the f32 column-parallel family -- at 256 and 131072 rows.  Every entry point is
called through the C ABI on preallocated buffers (no torch allocation inside a timed window); A / B pairs are interleaved so both see the same
clocks.  Prints one JSON object; `python tools/time_policy_head.py OUT.json` also writes it there."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.ppo import HipActorCriticPolicy  # noqa: E402

DEV = torch.device("cuda", 0)
L = _lib.lib()
SHAPES = [(4, 64, 5), (6, 256, 5)]
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


def shape_timing(D, H, A, n):
    pol = HipActorCriticPolicy(D, A, False, H, DEV, seed=1)
    g = torch.Generator().manual_seed(n)
    obs = torch.randn(n, D, generator=g).to(DEV)
    actions = torch.randint(0, A, (n,), generator=g, dtype=torch.int32).to(DEV)
    head, g_head = torch.empty(n, A, device=DEV), torch.randn(n, A, generator=g).to(DEV)
    v, lp, ent, a_out = torch.empty(n, device=DEV), torch.empty(n, device=DEV), torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    g_v, g_lp, g_ent = (torch.randn(n, generator=g).to(DEV) for _ in range(3))
    grad = torch.empty(pol.n_trainable, device=DEV)
    need = int(L.tma_policy_vjp_workspace_bytes(C.byref(pol.dims), n))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    P, d, st, p = _lib.ptr(pol.params), C.byref(pol.dims), _lib.stream_ptr(), _lib.ptr

    calls = {
        "head": lambda: _lib.check(L.tma_policy_head(P, d, p(obs), n, p(head), p(v), st)),
        "evaluate_actions": lambda: _lib.check(L.tma_policy_evaluate_actions(P, d, p(obs), p(actions), n, p(v), p(lp), p(ent), st)),
        "act": lambda: _lib.check(L.tma_policy_act(P, d, p(obs), n, 1, 2, 0, 0, p(a_out), p(v), p(lp), st)),
        "head_backward": lambda: _lib.check(L.tma_policy_head_backward(P, d, p(obs), n, p(g_head), p(g_v), p(grad), p(ws), need, st)),
        "evaluate_actions_backward": lambda: _lib.check(L.tma_policy_evaluate_actions_backward(P, d, p(obs), p(actions), n, p(g_v), p(g_lp), p(g_ent), p(grad),
                                                                                                   p(ws), need, st)),
    }
    reps = 400 if n <= 4096 else 40
    us = {}
    for _ in range(2):  # A / B / ... / A / B: the smaller of two interleaved passes
        for name, fn in calls.items():
            t = chain_us(fn, reps)
            us[name] = min(us.get(name, t), t)
    store_bytes = n * A * 4
    return {"us_per_call": us, "head_over_evaluate_actions": us["head"] / us["evaluate_actions"], "head_over_act": us["head"] / us["act"],
            "head_backward_over_evaluate_actions_backward": us["head_backward"] / us["evaluate_actions_backward"], "head_store_bytes": store_bytes,
            "vjp_workspace_bytes": need, "calls_per_timed_window": reps}


def main():
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("TMA_COMMIT", "unknown")
    res = {"what": "HIP-event time per C ABI call, median of 5 windows, the smaller of two interleaved passes; whole entry points (launches included)",
           "device": torch.cuda.get_device_name(0), "commit": commit, "abi": int(L.tma_version()),
           "shapes": {f"{D}x{H}x{A}": {str(n): shape_timing(D, H, A, n) for n in ROWS} for D, H, A in SHAPES}}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
