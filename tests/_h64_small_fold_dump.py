"""Helper of tests/test_h64_small_fold_gpu.py: for a D x 64 x 64 x A Discrete policy and the synthetic rollout of
tests/test_policy_dispatch_gpu.py, one minibatch gradient of B samples and two update epochs of batch size B through
tma_ppo_train_epoch_local -> .npz (run in a subprocess: TMA_H64_SMALL_SERIAL is read once per process).  The state dict and the gradient
in SB3 naming go along, so that the test can hold the gradient to the float64 reference without a GPU of its own."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from test_policy_dispatch_gpu import HP, _policy, _rollout  # noqa: E402
from test_ppo_gpu import _hip_grad  # noqa: E402
from three_mlagents_amd import _lib  # noqa: E402

D, A, B, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
H, T, start = 64, 16, 3
# three minibatches per epoch.  B = 256: 768 rows, a whole number of minibatches, so that the epochs run the persistent epoch kernel
# (tma_h64p.hip takes an epoch only then); larger B: two full minibatches and a short one through the per-minibatch launches
N = 48 if B == 256 else (start + 2 * B + T - 1) // T + 1
L = _lib.lib()
dev = torch.device("cuda", 0)
pol, sd = _policy(D, H, A, False)
bufs, _ = _rollout(sd, D, A, False, T, N, seed=B % 7919)
# ---- one minibatch gradient over explicit indices: B samples starting at a row that is not a multiple of the tile
perm = torch.randperm(T * N, generator=torch.Generator().manual_seed(B))
grad, stats, _ = _hip_grad(pol, bufs, T, N, perm, start, B, HP)
f, g, o = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
_lib.check(L.tma_debug_last_dispatch(C.byref(f), C.byref(g), C.byref(o)))
res = dict(grad=grad.cpu().numpy(), grad_stats=np.array(stats), grad_dispatch=np.array(g.value))
res.update({"named_" + k: v.cpu().numpy() for k, v in pol.named_from_flat(grad).items()})
res.update({"sd_" + k: v.detach().cpu().numpy() for k, v in sd.items()})
# ---- two epochs: every minibatch's clip + Adam step; B = 256 runs the persistent epoch kernel, larger B the per-minibatch launches with
# the optimizer step folded into the next one
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
# ---- did those epochs run the persistent kernel?  Its fall-backs are counted: none so far; then one more epoch (results above are saved)
# with the launch told to find its abort word set (TMA_PERSIST_FORCE_FAIL, read per launch).  The count goes to 1 exactly where the epoch
# is handed to the persistent kernel, which the same shape a moment ago therefore was as well; elsewhere no such launch exists and it stays 0.
cnt = C.c_int64(-1)
_lib.check(L.tma_ppo_persist_fallbacks(_lib.ptr(ws), C.byref(cnt), _lib.stream_ptr()))
before = cnt.value
os.environ["TMA_PERSIST_FORCE_FAIL"] = "1"
_lib.check(L.tma_ppo_train_epoch_local(_lib.ptr(pol.params), C.byref(pol.dims), C.byref(rv), 77, 2, B, C.byref(hpar), _lib.ptr(gbuf),
                                       _lib.ptr(m), _lib.ptr(v), step, 3e-4, 0.9, 0.999, 1e-5, 0.5, _lib.ptr(ws), _lib.stream_ptr()))
_lib.check(L.tma_ppo_persist_fallbacks(_lib.ptr(ws), C.byref(cnt), _lib.stream_ptr()))
torch.cuda.synchronize()
res.update(persist_fallbacks=np.array([before, cnt.value]))
np.savez(out, **res)
