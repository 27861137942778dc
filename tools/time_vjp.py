#!/usr/bin/env python3
"""tma_policy_evaluate_actions_backward beside tma_ppo_minibatch_grad on the same rows (HIP events around one call each, interleaved rounds in one
process): the PPO gradient launch is the yardstick -- the same forward / backward GEMMs with the loss compiled in, on kernels tuned per shape,
where the VJP is one deterministic two-phase path for every shape.  Shapes (4, 64, 5) and (6, 256, 5) at n = 256 and 131 072.  Writes
profiles/vjp_timing.json.  Usage: python tools/time_vjp.py [reps=20] [out=profiles/vjp_timing.json]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from three_mlagents_amd import _lib  # noqa: E402
from three_mlagents_amd.ppo import HipActorCriticPolicy  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "vjp_timing.json")
dev = torch.device("cuda", 0)
L = _lib.lib()
st = _lib.stream_ptr(dev)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


rows = []
for D, H, A in ((4, 64, 5), (6, 256, 5)):
    for n in (256, 131072):
        pol = HipActorCriticPolicy(D, A, False, H, dev, seed=1)
        g = torch.Generator().manual_seed(0)
        T, N = 1, n  # the rollout planes are the minibatch: rows 0 .. n - 1 in order
        obs = torch.randn(n, D, generator=g).to(dev)
        actions = torch.randint(0, A, (n,), generator=g, dtype=torch.int32).to(dev)
        cots = [torch.randn(n, generator=g).to(dev) for _ in range(3)]
        old_lp, adv, ret = (torch.randn(n, generator=g).to(dev) for _ in range(3))
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        rv = _lib.Rollout(_lib.ptr(obs), _lib.ptr(actions), _lib.ptr(old_lp), _lib.ptr(adv), _lib.ptr(ret), T, N)
        mb = _lib.Minibatch(_lib.ptr(idx), 0, 0, 0, n)
        hp = _lib.PPOHParams(0.2, 0.01, 0.5, 1)
        grad = torch.zeros(pol.n_trainable, device=dev)
        ws = torch.zeros(int(L.tma_ppo_workspace_bytes(C.byref(pol.dims))), dtype=torch.uint8, device=dev)
        need = int(L.tma_policy_vjp_workspace_bytes(C.byref(pol.dims), n))
        vws = torch.empty(need, dtype=torch.uint8, device=dev)
        vgrad = torch.empty(pol.n_trainable, device=dev)
        ppo = lambda: _lib.check(L.tma_ppo_minibatch_grad(_lib.ptr(pol.params), C.byref(pol.dims), C.byref(rv), C.byref(mb), C.byref(hp), _lib.ptr(grad),  # noqa: E731
                                                          _lib.ptr(ws), st))
        vjp = lambda: _lib.check(L.tma_policy_evaluate_actions_backward(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), _lib.ptr(actions), n,  # noqa: E731
                                                                        _lib.ptr(cots[0]), _lib.ptr(cots[1]), _lib.ptr(cots[2]), _lib.ptr(vgrad), _lib.ptr(vws),
                                                                        need, st))
        for _ in range(3):
            ppo(), vjp()
        torch.cuda.synchronize()
        t_ppo, t_vjp = [], []
        for _ in range(reps):  # interleaved rounds
            t_ppo.append(once(ppo))
            t_vjp.append(once(vjp))
        t_ppo.sort(), t_vjp.sort()
        row = dict(obs_dim=D, hidden=H, n_actions=A, n=n, reps=reps, workspace_bytes=need,
                   ppo_minibatch_grad_us=dict(median=t_ppo[reps // 2], min=t_ppo[0], max=t_ppo[-1]),
                   vjp_us=dict(median=t_vjp[reps // 2], min=t_vjp[0], max=t_vjp[-1]), ratio_of_medians=t_vjp[reps // 2] / t_ppo[reps // 2])
        rows.append(row)
        print(f"({D}, {H}, {A}) n = {n}: tma_ppo_minibatch_grad {t_ppo[reps // 2]:.1f} [{t_ppo[0]:.1f} .. {t_ppo[-1]:.1f}] us   "
              f"evaluate_actions_backward {t_vjp[reps // 2]:.1f} [{t_vjp[0]:.1f} .. {t_vjp[-1]:.1f}] us   ratio {row['ratio_of_medians']:.2f}", flush=True)
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(dict(tool="tools/time_vjp.py", device=torch.cuda.get_device_name(0), unit="us, HIP events around one call, host launch overhead included",
                   rows=rows), fh, indent=1)
    fh.write("\n")
