"""Helper of tests/test_h64_head_width_gpu.py: for a GridWorld-shaped policy (4 observations, 64 x 64, 5 actions) and a fixed synthetic
rollout, one minibatch gradient of B samples and two update epochs of batch size B through tma_ppo_train_epoch_local -> .npz (run in a
subprocess: TMA_H64_RUNTIME_A is read once per process)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from test_ppo_gpu import HP, _hip_grad, _policy, _rollout  # noqa: E402
from three_mlagents_amd import _lib  # noqa: E402

B, out = int(sys.argv[1]), sys.argv[2]
D, H, A, T, start = 4, 64, 5, 16, 3
N = (start + 2 * B + T - 1) // T + 1  # two full minibatches of B samples and a short one per epoch
L = _lib.lib()
dev = torch.device("cuda", 0)
pol, sd = _policy(D, H, A, False)
obs, actions, old_lp, adv, ret = _rollout(pol, sd, D, A, False, T, N, seed=B % 7919)
bufs = dict(obs=obs, actions=actions, old_lp=old_lp, adv=adv, ret=ret)
# ---- one minibatch gradient over explicit indices: B samples starting at a row that is not a multiple of the tile
perm = torch.randperm(T * N, generator=torch.Generator().manual_seed(B))
grad, stats, _ = _hip_grad(pol, bufs, T, N, perm, start, B, HP)
f, g, o = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
_lib.check(L.tma_debug_last_dispatch(C.byref(f), C.byref(g), C.byref(o)))
res = dict(grad=grad.cpu().numpy(), grad_stats=np.array(stats), grad_dispatch=np.array(g.value))
# ---- two epochs: every minibatch's clip + Adam step, the on-device permutation, the optimizer step folded into the next gradient launch
d = {k: v.to(dev).contiguous() for k, v in bufs.items()}
rv = _lib.Rollout(_lib.ptr(d["obs"]), _lib.ptr(d["actions"]), _lib.ptr(d["old_lp"]), _lib.ptr(d["adv"]), _lib.ptr(d["ret"]), T, N)
hpar = _lib.PPOHParams(HP["clip_range"], HP["ent_coef"], HP["vf_coef"], 1)
gbuf = torch.zeros(pol.n_trainable, device=dev)
m, v = torch.zeros(pol.n_trainable, device=dev), torch.zeros(pol.n_trainable, device=dev)
ws = torch.zeros(int(L.tma_ppo_workspace_bytes(C.byref(pol.dims))), dtype=torch.uint8, device=dev)
n_mb, step = -(-(T * N) // B), 1
for epoch in range(2):
    _lib.check(L.tma_ppo_train_epoch_local(_lib.ptr(pol.params), C.byref(pol.dims), C.byref(rv), 77, epoch, B, C.byref(hpar), _lib.ptr(gbuf),
                                           _lib.ptr(m), _lib.ptr(v), step, 3e-4, 0.9, 0.999, 1e-5, 0.5, _lib.ptr(ws), _lib.stream_ptr()))
    step += n_mb
st = (C.c_double * 8)()
_lib.check(L.tma_ppo_pop_stats(_lib.ptr(ws), st, _lib.stream_ptr()))
torch.cuda.synchronize()
res.update(params=pol.params.cpu().numpy(), exp_avg=m.cpu().numpy(), exp_avg_sq=v.cpu().numpy(), epoch_stats=np.array(list(st)),
           n_steps=np.array(step - 1))
np.savez(out, **res)
