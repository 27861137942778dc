#!/usr/bin/env python3
"""Time one minibatch of `rollout_buffer.get` (tma_rollout_gather, ABI 221) against the torch composition it replaces -- an index tensor from
tma_ppo_permutation uploaded once, then six index_select calls -- with HIP events, at the three shapes of DESIGN.md section 15:
1024 x 8 at D = 21, B = 256;  1024 x 4096 at D = 6, B = 131 072;  2048 x 2048 at D = 105 with 8 Box actions, B = 65 536.
A timed window is whole passes over the rollout, minibatch after minibatch (each call touches other rows, as in a real pass); the figure is the
window over its number of minibatches, median of 5 windows, the smaller of two interleaved A / B rounds.  Three variants: `gather_call`, the C ABI
call on preallocated outputs; `get`, the generator as a user drives it (six torch.empty per minibatch + the call); `index_select`, the
composition (which allocates its six results too).  Bytes = what a minibatch reads plus what it writes; rates are against the 8.0 TB/s HBM3E
specification and the 6.29 TB/s a float4 copy reaches.  Prints one JSON object; `python tools/time_rollout_gather.py OUT.json` also writes it."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.rollout_buffer import RolloutBuffer, perm_seed  # noqa: E402

DEV = torch.device("cuda", 0)
L = _lib.lib()
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
# (T, N, D, A, Box head, B)
SHAPES = [(1024, 8, 21, 3, False, 256), (1024, 4096, 6, 5, False, 131072), (2048, 2048, 105, 8, True, 65536)]


def window_us(fn, calls_per_fn, target_calls, warm=2, rounds=5):
    """median over `rounds` of (HIP-event time of `reps` back-to-back fn()) / (reps * calls_per_fn)"""
    reps = max(1, target_calls // calls_per_fn)
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
        out.append(a.elapsed_time(b) * 1e3 / (reps * calls_per_fn))
    out.sort()
    return out[len(out) // 2], reps


def shape_timing(T, N, D, A, cont, B):
    total, seed = T * N, 1
    n_mb = -(-total // B)
    g = torch.Generator(device=DEV).manual_seed(total)
    buf = dict(obs=torch.randn((T + 1, N, D), generator=g, device=DEV),
               actions=torch.randn((T, N, A), generator=g, device=DEV) if cont else torch.randint(0, A, (T, N), generator=g, device=DEV, dtype=torch.int32),
               **{k: torch.randn((T, N), generator=g, device=DEV) for k in ("values", "log_probs", "advantages", "returns")})
    dims = _lib.PolicyDims(D, 64, A, 1 if cont else 0, 0, 0)
    view = _lib.Rollout(_lib.ptr(buf["obs"]), _lib.ptr(buf["actions"]), _lib.ptr(buf["log_probs"]), _lib.ptr(buf["advantages"]), _lib.ptr(buf["returns"]), T, N, None)
    # RolloutBuffer reads these members of a model and nothing else
    model = types.SimpleNamespace(n_steps=T, n_envs=N, buf=buf, policy=types.SimpleNamespace(dims=dims), device=DEV, seed=seed, _epoch_counter=0,
                                  _rollout_view=view, _stream=lambda: _lib.stream_ptr(DEV))
    rb = RolloutBuffer(model)
    rb.full = True

    outs = (torch.empty((B, D), device=DEV), torch.empty((B, A), device=DEV) if cont else torch.empty((B,), dtype=torch.int32, device=DEV),
            *(torch.empty((B,), device=DEV) for _ in range(4)))
    out_ptrs = [_lib.ptr(t) for t in outs]
    st, d_ref, v_ref, val_ptr = _lib.stream_ptr(DEV), C.byref(dims), C.byref(view), _lib.ptr(buf["values"])
    batches = [_lib.Minibatch(None, perm_seed(seed), 0, s, min(B, total - s), 0, 0) for s in range(0, total, B)]

    def gather_pass():
        for mb in batches:
            _lib.check(L.tma_rollout_gather(v_ref, val_ptr, d_ref, C.byref(mb), *out_ptrs, st))

    def get_pass():
        for _ in rb.get(B, perm_epoch=0):
            pass

    # the composition: the permutation from the host function, uploaded once as plane rows t*N + i of the env-major flat indices f = i*T + t
    idx = np.zeros(total, dtype=np.int64)
    _lib.check(L.tma_ppo_permutation(perm_seed(seed), 0, total, idx.ctypes.data_as(C.c_void_p)))
    f = torch.from_numpy(idx).to(DEV)
    rows = (f % T) * N + f // T
    slices = [rows[s:s + B] for s in range(0, total, B)]
    flat = [buf["obs"][:T].reshape(total, D), buf["actions"].reshape(total, A) if cont else buf["actions"].reshape(total),
            *(buf[k].reshape(total) for k in ("values", "log_probs", "advantages", "returns"))]

    def index_select_pass():
        for sl in slices:
            for plane in flat:
                torch.index_select(plane, 0, sl)

    # the two must agree before either is timed
    got = next(iter(rb.get(B, perm_epoch=0)))
    for x, plane in zip(got, flat):
        assert torch.equal(x, torch.index_select(plane, 0, slices[0]))
    target = 16384 if B <= 4096 else 2048  # minibatches per timed window: tens of milliseconds and more at every shape
    us, reps = {}, {}
    for _ in range(2):  # A / B / C / A / B / C: the smaller of two interleaved rounds
        for name, fn in (("gather_call", gather_pass), ("get", get_pass), ("index_select", index_select_pass)):
            t, r = window_us(fn, n_mb, target)
            us[name] = min(us.get(name, t), t)
            reps[name] = r * n_mb
    moved = 2 * B * (D * 4 + (A * 4 if cont else 4) + 4 * 4)
    rate = {k: moved / (v * 1e-6) for k, v in us.items()}
    return {"T": T, "N": N, "D": D, "A": A, "box_actions": cont, "batch_size": B, "minibatches_per_pass": n_mb, "us_per_minibatch": us,
            "bytes_read_plus_written_per_minibatch": moved, "bytes_per_s": rate,
            "share_of_hbm_spec_8.0TBs": {k: v / HBM_SPEC for k, v in rate.items()}, "share_of_float4_copy_6.29TBs": {k: v / HBM_COPY for k, v in rate.items()},
            "index_select_over_gather_call": us["index_select"] / us["gather_call"], "index_select_over_get": us["index_select"] / us["get"],
            "minibatches_per_timed_window": reps}


def main():
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("TMA_COMMIT", "unknown")
    res = {"what": "HIP-event time per minibatch over whole passes, median of 5 windows, the smaller of two interleaved rounds; whole calls (launches and, for "
                   "`get` and `index_select`, the allocation of the six results included)",
           "device": torch.cuda.get_device_name(0), "commit": commit, "abi": int(L.tma_version()),
           "shapes": {f"{T}x{N}_D{D}_B{B}": shape_timing(T, N, D, A, cont, B) for T, N, D, A, cont, B in SHAPES}}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
