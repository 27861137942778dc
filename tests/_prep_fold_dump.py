"""Helper of tests/test_prep_fold_gpu.py: one rollout, then train() twice from the same state -- as built, and under TMA_NO_PREP_FOLD=1 (read
per call) -- with the pre-pass counts of each run (tma_debug_last_prep_fold).  Imported by the test; run as a script
(python _prep_fold_dump.py out.npz task n_envs n_steps batch n_epochs normalize) for the cases that need a switch the library reads once
per process (TMA_H64_RUNTIME_A)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

STAT_KEYS = ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/approx_kl", "train/clip_fraction", "train/grad_norm",
             "train/n_samples")


def expected_counts(total, batch, n_epochs):
    """(folded, stand-alone) pre-passes of one chained call: a hand-over is folded when both sides run on the eight-wave kernel, which takes
    minibatches of more than 128 tiles of 16 rows; every other minibatch (the call's first one included) gets a launch of its own."""
    epoch = [min(batch, total - s) for s in range(0, total, batch)]
    seq = epoch * n_epochs
    folded = sum(1 for a, b in zip(seq, seq[1:]) if a > 2048 and b > 2048)
    return folded, len(seq) - folded


def run_case(task, n_envs, n_steps, batch, n_epochs, normalize=True, seed=5):
    """-> dict of numpy arrays: params / exp_avg / exp_avg_sq / stats / (folded, standalone) of the two runs, and the state they started from"""
    from three_mlagents_amd import _lib
    from three_mlagents_amd.harness import make_vector_env
    from three_mlagents_amd.ppo import PPO

    L = _lib.lib()
    env = make_vector_env(task, n_envs=n_envs, seed=seed)
    m = PPO("MlpPolicy", env, n_steps=n_steps, batch_size=batch, n_epochs=n_epochs, seed=seed, normalize_advantage=normalize,
            policy_kwargs={"net_arch": [64, 64]})
    m.collect_rollouts()
    torch.cuda.synchronize()
    tensors = {"params": m.policy.params, "exp_avg": m.exp_avg, "exp_avg_sq": m.exp_avg_sq, "grad": m.grad, "workspace": m.workspace}
    snap = {k: v.clone() for k, v in tensors.items()}
    counters = (m._adam_step, m._epoch_counter, m._n_updates)
    res = {"start_params": snap["params"].cpu().numpy(), "n_trainable": np.array(m.policy.n_trainable)}
    saved = os.environ.pop("TMA_NO_PREP_FOLD", None)
    try:
        for name, switch in (("fold", None), ("ref", "1")):
            for k, v in tensors.items():
                v.copy_(snap[k])
            m._adam_step, m._epoch_counter, m._n_updates = counters
            if switch is None:
                os.environ.pop("TMA_NO_PREP_FOLD", None)
            else:
                os.environ["TMA_NO_PREP_FOLD"] = switch
            m.train()
            folded, alone = C.c_int(-1), C.c_int(-1)
            _lib.check(L.tma_debug_last_prep_fold(C.byref(folded), C.byref(alone)))
            st = m.pop_train_stats()
            res[name + "_params"] = m.policy.params.cpu().numpy()
            res[name + "_exp_avg"] = m.exp_avg.cpu().numpy()
            res[name + "_exp_avg_sq"] = m.exp_avg_sq.cpu().numpy()
            res[name + "_stats"] = np.array([st[k] for k in STAT_KEYS], dtype=np.float64)
            res[name + "_counts"] = np.array([folded.value, alone.value])
            res[name + "_adam_step"] = np.array(m._adam_step)
    finally:
        os.environ.pop("TMA_NO_PREP_FOLD", None)
        if saved is not None:
            os.environ["TMA_NO_PREP_FOLD"] = saved
        env.close()
    return res


if __name__ == "__main__":
    out, task = sys.argv[1], sys.argv[2]
    n_envs, n_steps, batch, n_epochs, normalize = (int(a) for a in sys.argv[3:8])
    np.savez(out, **run_case(task, n_envs, n_steps, batch, n_epochs, bool(normalize)))
