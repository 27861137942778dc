"""Helper of tests/test_h64_pair_balance_gpu.py, modelled on tests/_h64_small_fold_dump.py: for a D x 64 x 64 x A Discrete policy and the
synthetic rollout of tests/test_policy_dispatch_gpu.py, one minibatch gradient of B samples and two update epochs of batch size B through
tma_ppo_train_epoch_local, once as the library launches them and once under TMA_H64_NO_PAIR_BALANCE=1.  The switch is read per call, so
both arms run in the calling process, from the same policy, rollout and permutation; the environment is put back afterwards."""
import ctypes as C
import os

import numpy as np
import torch

from test_policy_dispatch_gpu import HP, _policy, _rollout
from test_ppo_gpu import _hip_grad
from three_mlagents_amd import _lib

H, T, START = 64, 16, 3
SWITCH = "TMA_H64_NO_PAIR_BALANCE"


def _arm(D, A, B, sd0, bufs, N):
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    pol, _ = _policy(D, H, A, False)
    pol.load_state_dict(sd0)
    # ---- one minibatch gradient over explicit indices: B samples starting at a row that is not a multiple of the tile
    perm = torch.randperm(T * N, generator=torch.Generator().manual_seed(B))
    grad, stats, _ = _hip_grad(pol, bufs, T, N, perm, START, B, HP)
    f, g, o = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    _lib.check(L.tma_debug_last_dispatch(C.byref(f), C.byref(g), C.byref(o)))
    res = dict(grad=grad.cpu().numpy(), grad_stats=np.array(stats), grad_dispatch=np.array(g.value))
    # ---- two epochs of two full minibatches and a short one: every minibatch's clip + Adam step, folded into the next launch
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
    return res


def both_arms(D, A, B):
    """(default, TMA_H64_NO_PAIR_BALANCE=1): two dicts of arrays."""
    N = (START + 2 * B + T - 1) // T + 1
    _, sd = _policy(D, H, A, False)
    bufs, _ = _rollout(sd, D, A, False, T, N, seed=B % 7919)
    saved = os.environ.pop(SWITCH, None)
    try:
        on = _arm(D, A, B, sd, bufs, N)
        os.environ[SWITCH] = "1"
        off = _arm(D, A, B, sd, bufs, N)
    finally:
        os.environ.pop(SWITCH, None)
        if saved is not None:
            os.environ[SWITCH] = saved
    return on, off
