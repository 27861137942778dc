"""Helper of tests/test_h64_fold_prologue_gpu.py: a synthetic rollout of any (D, A) the H = 64 gradient kernels take, pushed through
tma_ppo_train_epochs_local twice from the same starting state -- as built (the optimizer step of minibatch k in the prologue of gradient
launch k + 1) and under TMA_NO_ADAM_FOLD=1 (read per call: one optimizer launch per minibatch).  Imported by the test; run as a script
(python _h64_fold_prologue_dump.py out.npz D A total batch normalize max_grad_norm) for the case that needs a switch the library reads
once per process (TMA_H64_RUNTIME_A)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

N_ENVS = 256
N_EPOCHS = 2
SWITCHES = ("TMA_NO_ADAM_FOLD", "TMA_NO_PERSIST")


def run_case(D, A, total, batch, normalize=True, max_grad_norm=0.5, seed=7):
    """-> dict of numpy arrays: params / exp_avg / exp_avg_sq / stats (the eight doubles of tma_ppo_pop_stats: six sums, the last gradient
    norm, the last clip coefficient) and the pre-pass counts (tma_debug_last_prep_fold) of the folded run and the reference run, whether the
    two left different workspaces, and the parameters both started from"""
    from three_mlagents_amd import _lib
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    L = _lib.lib()
    assert total % N_ENVS == 0
    T, N = total // N_ENVS, N_ENVS
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    pol = HipActorCriticPolicy(D, A, False, 64, dev, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    obs = torch.randn((T + 1, N, D), generator=gen).to(dev)
    actions = torch.randint(0, A, (T, N), generator=gen, dtype=torch.int32).to(dev)
    log_probs = (-float(np.log(A)) + 0.1 * torch.randn((T, N), generator=gen)).to(dev)
    advantages = (1.0 + 2.0 * torch.randn((T, N), generator=gen)).to(dev)
    returns = torch.randn((T, N), generator=gen).to(dev)
    stream = _lib.stream_ptr(dev)
    n_packed = L.tma_ppo_packed_floats(C.byref(pol.dims), T, N)
    packed = torch.empty(n_packed, dtype=torch.float32, device=dev) if n_packed > 0 else None
    view = _lib.Rollout(_lib.ptr(obs), _lib.ptr(actions), _lib.ptr(log_probs), _lib.ptr(advantages), _lib.ptr(returns), T, N, _lib.ptr(packed))
    if packed is not None:
        _lib.check(L.tma_ppo_pack_samples(C.byref(view), C.byref(pol.dims), _lib.ptr(packed), stream))
    hp = _lib.PPOHParams(0.2, 0.01, 0.5, 1 if normalize else 0)
    P = pol.n_trainable
    tensors = {"params": pol.params, "exp_avg": torch.zeros(P, device=dev), "exp_avg_sq": torch.zeros(P, device=dev), "grad": torch.zeros(P, device=dev),
               "workspace": torch.zeros(int(L.tma_ppo_workspace_bytes(C.byref(pol.dims))), dtype=torch.uint8, device=dev)}
    torch.cuda.synchronize()
    snap = {k: v.clone() for k, v in tensors.items()}
    res = {"start_params": snap["params"].cpu().numpy(), "n_trainable": np.array(P)}
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    ws = {}
    try:
        os.environ["TMA_NO_PERSIST"] = "1"  # (batch 256: the per-minibatch launches, not the persistent epoch kernel)
        for name, switch in (("fold", None), ("ref", "1")):
            for k, v in tensors.items():
                v.copy_(snap[k])
            os.environ.pop("TMA_NO_ADAM_FOLD", None)
            if switch is not None:
                os.environ["TMA_NO_ADAM_FOLD"] = switch
            _lib.check(L.tma_ppo_train_epochs_local(_lib.ptr(tensors["params"]), C.byref(pol.dims), C.byref(view), 12345, 0, N_EPOCHS, batch, C.byref(hp),
                                                    _lib.ptr(tensors["grad"]), _lib.ptr(tensors["exp_avg"]), _lib.ptr(tensors["exp_avg_sq"]), 1, 3e-4, 0.9,
                                                    0.999, 1e-5, float(max_grad_norm), _lib.ptr(tensors["workspace"]), stream))
            out = (C.c_double * 8)()
            _lib.check(L.tma_ppo_pop_stats(_lib.ptr(tensors["workspace"]), out, stream))
            for k in ("params", "exp_avg", "exp_avg_sq"):
                res[name + "_" + k] = tensors[k].cpu().numpy()
            res[name + "_stats"] = np.array(list(out), dtype=np.float64)
            folded, alone = C.c_int(-1), C.c_int(-1)
            _lib.check(L.tma_debug_last_prep_fold(C.byref(folded), C.byref(alone)))
            res[name + "_counts"] = np.array([folded.value, alone.value])  # advantage pre-passes carried by a gradient launch / launched alone
            ws[name] = tensors["workspace"].clone()
        # the folded chain keeps the other half of the state double buffer in the workspace; the reference sequence never writes it
        res["workspace_differs"] = np.array(not torch.equal(ws["fold"], ws["ref"]))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return res


if __name__ == "__main__":
    out = sys.argv[1]
    D, A, total, batch, normalize = (int(a) for a in sys.argv[2:7])
    np.savez(out, **run_case(D, A, total, batch, bool(normalize), float(sys.argv[7])))
