"""The eight-wave H = 64 gradient kernel of the headline shape sets each wave's issue priority at every tile top from how many tiles it and
the wave that shares its SIMD (wave ^ 4) have completed, read from an LDS word that nobody waits on.  Priority decides WHEN a wave's
instructions issue, never which or in what order: every accumulator sees the same operands in the same order, so the launch must agree
with TMA_H64_NO_PAIR_BALANCE=1 (the kernel without the counter) to the last bit -- the gradient and statistics of one minibatch, and
parameters and both Adam moments after two epochs of tma_ppo_train_epoch_local.

Shapes (D, A): (4, 5) the headline instantiation, the one that carries the balance; (6, 3) a runtime-width instantiation (these launch
without it under either setting: with the counter they spill more registers).  Minibatches, the smallest that reach each way the counter
can go wrong: 2 049 the eight-wave kernel, 15 invalid rows in the last tile; 4 112 = 257 tiles over 264 waves: some waves run no tile, so a
partner's word stays 0 for the whole launch; 16 385 = 1 025 tiles over 1 024 waves: one wave runs a second tile after its partner has left;
32 784 = 2 049 tiles: a pair whose waves own 3 and 2 tiles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEYS = ("grad", "grad_stats", "params", "exp_avg", "exp_avg_sq", "epoch_stats")


@pytest.mark.parametrize("batch", [2049, 4112, 16385, 32784])
@pytest.mark.parametrize("D,A", [(4, 5), (6, 3)])
def test_pair_balance_changes_no_bit(D, A, batch):
    from _h64_pair_balance import both_arms
    from test_policy_dispatch_gpu import expected_value

    on, off = both_arms(D, A, batch)
    for r in (on, off):
        assert int(r["grad_dispatch"]) == expected_value("GRAD_H64")  # the eight-wave kernel
        assert np.isfinite(r["grad"]).all() and float(np.abs(r["grad"]).max()) > 0
        assert r["grad_stats"][5] == batch
        assert np.isfinite(r["params"]).all() and int(r["n_steps"]) == 2 * 3  # (three minibatches per epoch)
        assert float(np.abs(r["exp_avg"]).max()) > 0 and float(np.abs(r["exp_avg_sq"]).max()) > 0
    for key in KEYS:
        assert np.array_equal(on[key], off[key]), (key, float(np.abs(on[key] - off[key]).max()))
