#!/usr/bin/env python3
"""Time `ReplayBuffer.add_step` (tma_replay_add) and `ReplayBuffer.sample` (tma_replay_sample, ABI 224) against the torch compositions they
replace, with HIP events, at the shapes of DESIGN.md section 16: D 4 / Discrete / B 64 (one env), D 21 / Discrete / B 256 (8 envs), D 105 with
8 Box actions / B 256 and B 65 536 (2048 envs), each sampled at n_step 1 and 3.
  * add:     `add_call` the C ABI call, `add_step` the Python method, `torch_add` eight torch ops (two row copies, a where, three scalar row
             copies, the action row copy, the last_obs copy).
  * sample:  `sample_call` the C ABI call on preallocated outputs, `sample` the Python method (six torch.empty + the call), `torch_sample` the
             n_step = 1 composition: two torch.randint draws and five advanced-indexing gathers (obs, actions, next_obs, terminated -> float,
             rewards).  torch has no one-call n-step window, so the n_step = 3 kernel is set against the same n_step = 1 composition: the ratio
             there is a lower bound of what a torch n-step would cost.
A timed window is `reps` back-to-back calls between two events (tens of milliseconds); the figure is the window over reps, median of 5 windows,
the smaller of two interleaved rounds.  Prints one JSON object; `python tools/time_replay.py OUT.json` also writes it."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.replay_buffer import ReplayBuffer  # noqa: E402

DEV = torch.device("cuda", 0)
L = _lib.lib()
# (rows, n_envs, D, A, Box actions, batch sizes)
SHAPES = [(100_000, 1, 4, 5, False, (64,)), (16_384, 8, 21, 3, False, (256,)), (512, 2048, 105, 8, True, (256, 65_536))]


def window_us(fn, reps, warm=2, rounds=5):
    """median over `rounds` of (HIP-event time of `reps` back-to-back fn()) / reps"""
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


def best_of_two(variants, reps):
    us = {}
    for _ in range(2):  # A / B / C / A / B / C: the smaller of two interleaved rounds
        for name, fn in variants:
            t = window_us(fn, reps)
            us[name] = min(us.get(name, t), t)
    return us


def fill(rb, g):
    """every plane random, the ring full: what is timed does not depend on how the rows got there"""
    rb.observations.normal_(generator=g), rb.next_observations.normal_(generator=g), rb.rewards.normal_(generator=g)
    rb.actions.normal_(generator=g) if rb.continuous else rb.actions.random_(0, rb.act_dim, generator=g)
    rb.terminated.copy_(torch.rand(rb.terminated.shape, generator=g, device=DEV) < 0.02)
    rb.truncated.copy_(torch.rand(rb.truncated.shape, generator=g, device=DEV) < 0.01)
    rb.pos, rb.full = rb.buffer_size // 3, True


def shape_timing(R, N, D, A, cont, batches):
    g = torch.Generator(device=DEV).manual_seed(R + N)
    rb = ReplayBuffer(R * N, D, (A, cont), DEV, n_envs=N, seed=1)
    fill(rb, g)
    st, view = _lib.stream_ptr(DEV), C.byref(rb._view)
    # ---- add ----
    out = dict(obs=torch.randn((1, N, D), generator=g, device=DEV), rew=torch.randn((1, N), generator=g, device=DEV),
               term=(torch.rand((1, N), generator=g, device=DEV) < 0.02).to(torch.uint8), trunc=torch.zeros((1, N), dtype=torch.uint8, device=DEV),
               term_obs=torch.randn((1, N, D), generator=g, device=DEV))
    actions = torch.randn((N, A), generator=g, device=DEV) if cont else torch.randint(0, A, (N,), generator=g, device=DEV, dtype=torch.int32)
    add_ptrs = [_lib.ptr(t) for t in (rb.last_obs, actions, out["obs"], out["rew"], out["term"], out["trunc"], out["term_obs"])]
    state = {"pos": 0}

    def next_pos():
        state["pos"] = (state["pos"] + 1) % R
        return state["pos"]

    def add_call():
        _lib.check(L.tma_replay_add(view, next_pos(), *add_ptrs, st))

    def torch_add():
        p = next_pos()
        ended = (out["term"][0] | out["trunc"][0]).bool()[:, None]
        rb.observations[p].copy_(rb.last_obs)
        rb.next_observations[p].copy_(torch.where(ended, out["term_obs"][0], out["obs"][0]))
        rb.actions[p].copy_(actions), rb.rewards[p].copy_(out["rew"][0]), rb.terminated[p].copy_(out["term"][0]), rb.truncated[p].copy_(out["trunc"][0])
        rb.last_obs.copy_(out["obs"][0])

    add_us = best_of_two((("add_call", add_call), ("add_step", lambda: rb.add_step(actions, out)), ("torch_add", torch_add)), 4096)
    fill(rb, g)
    res = {"rows": R, "n_envs": N, "D": D, "A": A, "box_actions": cont, "add_us": add_us, "torch_add_over_add_call": add_us["torch_add"] / add_us["add_call"],
           "torch_add_over_add_step": add_us["torch_add"] / add_us["add_step"], "add_bytes_read_plus_written": N * (5 * D * 4 + 2 * (A * 4 if cont else 4) + 2 * 6), "sample": {}}
    # ---- sample ----
    flat = [rb.observations, rb.actions, rb.next_observations, rb.terminated, rb.rewards]

    def torch_sample(B):
        t, i = torch.randint(0, R, (B,), device=DEV), torch.randint(0, N, (B,), device=DEV)
        return flat[0][t, i], flat[1][t, i], flat[2][t, i], flat[3][t, i].float(), flat[4][t, i]

    for B in batches:
        outs = (torch.empty((B, D), device=DEV), torch.empty((B, A), device=DEV) if cont else torch.empty((B,), dtype=torch.int32, device=DEV),
                torch.empty((B, D), device=DEV), *(torch.empty((B,), device=DEV) for _ in range(3)))
        ptrs = [_lib.ptr(t) for t in outs]
        reps = 8192 if B <= 4096 else 1024
        rb.n_steps = 1  # the kernel and the composition must agree on the kernel's own indices before either is timed
        got, t, i = rb.sample(B, return_indices=True)
        for x, plane in zip(got[:3] + (got.rewards,), (flat[0], flat[1], flat[2], flat[4])):
            assert torch.equal(x, plane[t.long(), i.long()])
        assert torch.equal(got.dones, flat[3][t.long(), i.long()].float())
        for n_step in (1, 3):
            rb.n_steps, draw = n_step, {"k": 0}

            def sample_call():
                draw["k"] += 1
                _lib.check(L.tma_replay_sample(view, R, rb.pos - 1, n_step, 0.99, 1, draw["k"], B, *ptrs, None, None, st))

            us = best_of_two((("sample_call", sample_call), ("sample", lambda: rb.sample(B)), ("torch_sample", lambda: torch_sample(B))), reps)
            moved = 2 * B * (2 * D * 4 + (A * 4 if cont else 4)) + B * (3 * 4 + n_step * 6)
            res["sample"][f"B{B}_n{n_step}"] = {"us": us, "torch_sample_over_sample_call": us["torch_sample"] / us["sample_call"],
                                               "torch_sample_over_sample": us["torch_sample"] / us["sample"], "bytes_read_plus_written": moved,
                                               "sample_call_bytes_per_s": moved / (us["sample_call"] * 1e-6)}
    return res


def main():
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("TMA_COMMIT", "unknown")
    res = {"what": "HIP-event time per call in microseconds, median of 5 windows of back-to-back calls, the smaller of two interleaved rounds; whole calls "
                   "(launches and, for `sample` and the torch compositions, the allocation of their results included)",
           "device": torch.cuda.get_device_name(0), "commit": commit, "abi": int(L.tma_version()),
           "shapes": {f"{R}x{N}_D{D}": shape_timing(R, N, D, A, cont, batches) for R, N, D, A, cont, batches in SHAPES}}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
