#!/usr/bin/env python3
"""Time a ReLU policy beside the tanh policy of the same shape with HIP events: tma_policy_act, tma_ppo_minibatch_grad and a rollout
(tma_rollout_collect: the ReLU policy runs the per-step composition, tma_policy_act_bootstrap + env step, the tanh policy whatever its shape
runs -- the fused chunk kernels on the three task shapes here).

Shapes (D, H, A): (4, 64, 5), (6, 256, 5), (105, 256, 8 Box) -- tanh runs its tuned family there (H = 64 LDS images, column-parallel), ReLU the
generic one-wave-per-tile kernels: the ratio is the price of the generic path -- and (4, 512, 3), generic for both, where the expectation is
relu <= 1.05 tanh (5 % for event noise; the project's A/B tables scatter by 2-3 %).  n = 256 and 131072 rows / samples.  Every entry point is
called through the C ABI on preallocated buffers; tanh and ReLU are interleaved so both see the same clocks; median of 5 windows, the smaller
of two passes.  Prints one JSON object; `python tools/time_activation.py OUT.json` also writes it there."""
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
SHAPES = [(4, 64, 5, False), (6, 256, 5, False), (105, 256, 8, True), (4, 512, 3, False)]
ROWS = [256, 131072]
ROLLOUT = {(4, 64, 5, False): "gridworld", (6, 256, 5, False): "ball3d", (105, 256, 8, True): "ant"}  # the shapes that are a task's: a rollout needs an env
ROLLOUT_ENVS, ROLLOUT_STEPS = 256, 32
NAMES = None  # TMA_DISPATCH_ value -> name, parsed from include/tma.h on first use


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


def last_dispatch():
    global NAMES
    if NAMES is None:
        import re

        text = open(os.path.join(ROOT, "include", "tma.h")).read()
        NAMES = {int(m.group(2)): m.group(1) for m in re.finditer(r"\bTMA_DISPATCH_([A-Z0-9_]+)\s*=\s*(\d+)", text) if m.group(1) != "GRID_CAPPED"}
    f, g = C.c_int32(-1), C.c_int32(-1)
    _lib.check(L.tma_debug_last_dispatch(C.byref(f), C.byref(g), None))
    return NAMES.get(f.value & 0xFF, "?"), NAMES.get(g.value & 0xFF, "?")


def interleaved(calls, reps):
    us = {}
    for _ in range(2):  # tanh / relu / tanh / relu: the smaller of two interleaved passes
        for name, fn in calls.items():
            t = chain_us(fn, reps)
            us[name] = min(us.get(name, t), t)
    return us


def shape_timing(D, H, A, cont, n):
    p, st = _lib.ptr, _lib.stream_ptr()
    g = torch.Generator().manual_seed(n)
    T, N = 16, n // 16
    obs = torch.randn(T, N, D, generator=g).to(DEV)
    if cont:
        actions, a_out = (0.7 * torch.randn(T, N, A, generator=g)).to(DEV), torch.empty(n, A, device=DEV)
    else:
        actions, a_out = torch.randint(0, A, (T, N), generator=g, dtype=torch.int32).to(DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    old_lp, adv, ret = ((s * torch.randn(T, N, generator=g) + m).to(DEV) for s, m in ((0.1, -1.5), (1.0, 0.0), (1.0, 0.0)))
    v, lp = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    rv = _lib.Rollout(p(obs), p(actions), p(old_lp), p(adv), p(ret), T, N)
    mb = _lib.Minibatch(None, 7, 0, 0, n)
    hp = _lib.PPOHParams(0.2, 0.01, 0.5, 1)
    act_calls, grad_calls, kernels, keep = {}, {}, {}, []
    for name in ("tanh", "relu"):
        pol = HipActorCriticPolicy(D, A, cont, H, DEV, seed=1, activation=name)
        grad = torch.zeros(pol.n_trainable, device=DEV)
        ws = torch.zeros(int(L.tma_ppo_workspace_bytes(C.byref(pol.dims))), dtype=torch.uint8, device=DEV)
        keep.append((pol, grad, ws))
        act_calls[name] = lambda pol=pol: _lib.check(L.tma_policy_act(p(pol.params), C.byref(pol.dims), p(obs), n, 1, 2, 0, 0, p(a_out), p(v), p(lp), st))
        grad_calls[name] = lambda pol=pol, grad=grad, ws=ws: _lib.check(L.tma_ppo_minibatch_grad(p(pol.params), C.byref(pol.dims), C.byref(rv), C.byref(mb),
                                                                                                  C.byref(hp), p(grad), p(ws), st))
        act_calls[name]()
        grad_calls[name]()
        kernels[name] = dict(zip(("act", "grad"), last_dispatch()))
    reps = 400 if n <= 4096 else 40
    us_act, us_grad = interleaved(act_calls, reps), interleaved(grad_calls, reps)
    return {"us_per_call": {"tma_policy_act": us_act, "tma_ppo_minibatch_grad": us_grad}, "kernels": kernels,
            "relu_over_tanh": {"tma_policy_act": us_act["relu"] / us_act["tanh"], "tma_ppo_minibatch_grad": us_grad["relu"] / us_grad["tanh"]},
            "calls_per_timed_window": reps}


def rollout_timing(D, H, A, cont, task):
    """collect_rollouts (tma_rollout_collect + GAE) over ROLLOUT_STEPS steps of ROLLOUT_ENVS envs, each policy on the path its plan gives it: ReLU
    the per-step composition, tanh the task's fused chunk kernel where it has one"""
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv

    calls, envs = {}, []
    for name in ("tanh", "relu"):
        env = HipVecEnv(task, ROLLOUT_ENVS, seed=1)
        envs.append(env)
        m = PPO("MlpPolicy", env, n_steps=ROLLOUT_STEPS, batch_size=256, n_epochs=1, seed=1, policy_kwargs={"net_arch": [H, H], "activation_fn": name})
        assert (m.policy.obs_dim, m.policy.act_dim, m.policy.continuous) == (D, A, cont)
        m.collect_rollouts()
        calls[name] = m.collect_rollouts
    us = interleaved(calls, 10)
    for env in envs:
        env.close()
    return {"us_per_rollout": us, "relu_over_tanh": us["relu"] / us["tanh"], "envs": ROLLOUT_ENVS, "steps": ROLLOUT_STEPS, "task": task,
            "paths": {"relu": "per-step composition", "tanh": "as dispatched (fused chunk kernel where the shape has one)"}}


def main():
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("TMA_COMMIT", "unknown")
    shapes = {}
    for D, H, A, cont in SHAPES:
        entry = {str(n): shape_timing(D, H, A, cont, n) for n in ROWS}
        if (D, H, A, cont) in ROLLOUT:
            entry["per_step_rollout"] = rollout_timing(D, H, A, cont, ROLLOUT[(D, H, A, cont)])
        shapes[f"{D}x{H}x{A}{' box' if cont else ''}"] = entry
    both_generic = shapes["4x512x3"]
    res = {"what": "HIP-event time per C ABI call (whole entry points, launches included), median of 5 windows, the smaller of two interleaved passes; "
                   "relu_over_tanh on the first three shapes is the generic kernel family against the tuned tanh one, on 4x512x3 both are generic",
           "device": torch.cuda.get_device_name(0), "commit": commit, "abi": int(L.tma_version()), "shapes": shapes,
           "generic_for_both_relu_within_5_percent_of_tanh": all(r <= 1.05 for n in ROWS for r in both_generic[str(n)]["relu_over_tanh"].values())}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
