"""The H = 64 gradient tile runs its two small weight gradients (dW1 with the b1 sums, dW3 with the b3 sum; the 4x4x1 MFMA form) under the
two big MFMA streams of the same tile -- dW1 on dW2's 64 MFMAs, dW3 on the dh1 chain -- and dz2 has an LDS slot of its own (slot C) so that
h2 survives until dW3 has read it.  TMA_H64_SMALL_SERIAL=1 selects the order of rounds 3-10 (each in a phase of its own) on the same slot
layout.  Every accumulator sees the same operands in the same order, so the two must agree to the last bit: the gradient and statistics
of one minibatch, and parameters and both Adam moments after two epochs of tma_ppo_train_epoch_local.

Shapes (D, A): (4, 5) the compile-time-width kernel, both dW3 halves; (4, 3) one dW3 half; (6, 3) two observation blocks in dW1;
(16, 16) both 16x16x4 fallbacks on the new slot layout.  Minibatches: 256 the four-wave kernel and, in the epochs (768 rows: a whole number
of minibatches), the persistent epoch kernel's use of the tile -- asserted through its fall-back count, see the helper; 2 049 the eight-wave kernel, 15 invalid rows in the last tile; 4 112 the eight-wave kernel on 33 blocks a net
with 7 idle waves in the last; 16 385 = 1 025 tiles over the 1 024 waves of a net's 128 blocks, so one wave runs a second tile and reuses
slot C (4 112 is 257 tiles over 264 waves: one tile each).  In the default order the gradient is
also held to the float64 reference with the comparator and constants of tests/test_policy_dispatch_gpu.py.

TMA_H64_SMALL_SERIAL=A / =B run one fold alone in the compile-time-width kernel (the measuring arms; every other kernel runs the serial order
under them): the second test holds them to the default at (4, 5), bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
H, T, START = 64, 16, 3


def _n_envs(batch):
    return 48 if batch == 256 else (START + 2 * batch + T - 1) // T + 1  # (the helper's N)


def _dump(tmp_path, name, D, A, batch, **env):
    out = str(tmp_path / f"{name}.npz")
    e = {k: v for k, v in os.environ.items() if k not in ("TMA_H64_SMALL_SERIAL", "TMA_PERSIST_FORCE_FAIL", "TMA_NO_PERSIST")}
    e.update(env)
    subprocess.run([sys.executable, os.path.join(HERE, "_h64_small_fold_dump.py"), str(D), str(A), str(batch), out], check=True, env=e, timeout=600)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("batch", [256, 2049, 4112, 16385])
@pytest.mark.parametrize("D,A", [(4, 5), (4, 3), (6, 3), (16, 16)])
def test_folded_small_weight_gradients_equal_the_serial_order_bit_for_bit(tmp_path, D, A, batch):
    from test_policy_dispatch_gpu import HP, F, K, _grads, _rollout, _segment_errors, expected_value

    fold = _dump(tmp_path, "folded", D, A, batch)
    ser = _dump(tmp_path, "serial", D, A, batch, TMA_H64_SMALL_SERIAL="1")
    ident = "GRAD_H64_SMALL" if batch <= 2048 else "GRAD_H64"
    for r in (fold, ser):
        assert int(r["grad_dispatch"]) == expected_value(ident)
        assert np.isfinite(r["grad"]).all() and float(np.abs(r["grad"]).max()) > 0
        assert r["grad_stats"][5] == batch
        assert np.isfinite(r["params"]).all() and int(r["n_steps"]) == 2 * 3  # (three minibatches per epoch)
        # the epochs of 256-sample minibatches ran the persistent epoch kernel without a fall-back, the others have no such launch
        assert list(r["persist_fallbacks"]) == ([0, 1] if batch == 256 else [0, 0])
    for key in ("grad", "grad_stats", "params", "exp_avg", "exp_avg_sq", "epoch_stats"):
        assert np.array_equal(fold[key], ser[key]), (key, float(np.abs(fold[key] - ser[key]).max()))
    assert float(np.abs(fold["exp_avg"]).max()) > 0 and float(np.abs(fold["exp_avg_sq"]).max()) > 0
    # ---- the default order against float64 autograd: test_gradient_branch_against_float64's comparator on the helper's data
    sd = {k[3:]: torch.from_numpy(v) for k, v in fold.items() if k.startswith("sd_")}
    g = {k[6:]: torch.from_numpy(v) for k, v in fold.items() if k.startswith("named_")}
    N = _n_envs(batch)
    _, rows = _rollout(sd, D, A, False, T, N, seed=batch % 7919)
    idx = torch.randperm(T * N, generator=torch.Generator().manual_seed(batch))[START:START + batch]
    g64, s64 = _grads(sd, rows, idx, torch.float64, HP)
    g32, _ = _grads(sd, rows, idx, torch.float32, HP)
    assert set(g) == set(g64)
    errs = _segment_errors(g, g64, g32)
    print("budget use", max(e / (K * e32 + F * m) for e, e32, m in errs.values()))
    bad = {key: v for key, v in errs.items() if v[0] > K * v[1] + F * v[2]}
    assert not bad, bad
    st = fold["grad_stats"]
    assert st[4] == round(s64["clip_fraction"] * batch), (st[4], s64["clip_fraction"] * batch)
    for got_v, ref_v, what in ((st[0] / batch, s64["policy_loss"], "policy_loss"), (st[1] / batch, s64["value_loss"], "value_loss"),
                               (-st[2] / batch, s64["entropy_loss"], "entropy_loss"), (st[3] / batch, s64["approx_kl"], "approx_kl")):
        assert abs(got_v - ref_v) <= 2e-6 * max(1.0, abs(ref_v)), (what, got_v, ref_v)


@pytest.mark.parametrize("batch", [2049, 16385])
def test_each_fold_alone_equals_both_bit_for_bit(tmp_path, batch):
    from test_policy_dispatch_gpu import expected_value

    both = _dump(tmp_path, "both", 4, 5, batch)
    for arm in ("A", "B"):
        one = _dump(tmp_path, arm, 4, 5, batch, TMA_H64_SMALL_SERIAL=arm)
        assert int(one["grad_dispatch"]) == expected_value("GRAD_H64") and one["grad_stats"][5] == batch
        for key in ("grad", "grad_stats", "params", "exp_avg", "exp_avg_sq", "epoch_stats"):
            assert np.array_equal(both[key], one[key]), (arm, key, float(np.abs(both[key] - one[key]).max()))
