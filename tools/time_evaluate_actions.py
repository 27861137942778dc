#!/usr/bin/env python3
"""tma_policy_act against tma_policy_evaluate_actions (HIP events, one launch group per sample): the evaluate mode runs the GEMMs of `act` minus
the sampling, so the two columns should sit within each other's run-to-run spread.  Per shape: median and min / max of `reps` timed calls after
a warm-up, at n rows.  Usage: python tools/time_evaluate_actions.py [n=131072] [reps=30]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.ppo import HipActorCriticPolicy  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
SHAPES = [(4, 64, 5, False, "f32"), (6, 256, 5, False, "f32"), (6, 256, 5, False, "bf16"), (105, 256, 8, True, "f32")]
dev = torch.device("cuda", 0)
L = _lib.lib()


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    us.sort()
    return us[len(us) // 2], us[0], us[-1]


print(f"n = {n}, {reps} timed calls each (us: median [min .. max])")
for D, H, A, cont, mfma in SHAPES:
    pol = HipActorCriticPolicy(D, A, cont, H, dev, seed=1, mfma_dtype=mfma)
    obs = torch.randn(n, D, device=dev)
    actions = torch.empty((n, A), dtype=torch.float32, device=dev) if cont else torch.empty((n,), dtype=torch.int32, device=dev)
    values, logp, ent = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
    st = _lib.stream_ptr(dev)
    act = lambda: _lib.check(L.tma_policy_act(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), n, 1, 2, 0, 0, _lib.ptr(actions), _lib.ptr(values),  # noqa: E731
                                              _lib.ptr(logp), st))
    ev = lambda: _lib.check(L.tma_policy_evaluate_actions(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), _lib.ptr(actions), n, _lib.ptr(values),  # noqa: E731
                                                          _lib.ptr(logp), _lib.ptr(ent), st))
    a, e = timed(act), timed(ev)  # (act first: it fills `actions`)
    a2 = timed(act)
    print(f"({D}, {H}, {A}{', Box' if cont else ''}) {mfma}: act {a[0]:.1f} [{a[1]:.1f} .. {a[2]:.1f}]  evaluate_actions {e[0]:.1f} [{e[1]:.1f} .. {e[2]:.1f}]"
          f"  act again {a2[0]:.1f} [{a2[1]:.1f} .. {a2[2]:.1f}]")
