"""The optimizer step folded into the prologue of the next H = 64 gradient launch (AdamImageFold, csrc/tma_h64.hip) at the shapes where its
ownership and its image slots can go wrong: the eight-wave kernel's 4 x 2 layer-2 blocks and round-robin parameters on 512 threads (the
headline instantiation with compile-time widths, and every runtime-width one up to the ownership bound D = 16, A = 16), the 256-thread
workgroups of the small kernel, and the hand-over between the two.  Every case runs two epochs of three minibatches (both halves of the
state double buffer) through tma_ppo_train_epochs_local on a synthetic rollout, once as built and once under TMA_NO_ADAM_FOLD=1 (one
optimizer launch per minibatch), from the same starting state; parameters (the whole buffer: derived copies and weight images included),
both Adam moments and the statistics must be equal bit for bit, and the update must have moved the parameters."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _h64_fold_prologue_dump import N_EPOCHS, run_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MB = 2304  # 144 tiles of 16 rows: the eight-wave kernel (more than 128 tiles), 18 block pairs, most waves without a tile


def _expected_counts(total, batch):
    """(carried, alone) advantage pre-passes of the folded chain: a hand-over is carried when both sides run on the eight-wave kernel (more
    than 2 048 rows); without any such minibatch size the chain prepares once per epoch, as the reference sequence does"""
    if batch <= 2048:
        return 0, N_EPOCHS
    seq = [min(batch, total - s) for s in range(0, total, batch)] * N_EPOCHS
    carried = sum(1 for a, b in zip(seq, seq[1:]) if a > 2048 and b > 2048)
    return carried, len(seq) - carried


def _check(r, total, max_grad_norm=0.5, batch=MB):
    nt = int(r["n_trainable"])
    # the first run really was the folded chain (h64_fold_epochs) and the second was not: only the chain hands pre-passes from launch to launch,
    # and only it keeps a half of the optimizer state in the workspace -- otherwise both runs are one sequence and everything below is trivial
    assert tuple(r["fold_counts"]) == _expected_counts(total, batch), (tuple(r["fold_counts"]), _expected_counts(total, batch))
    assert tuple(r["ref_counts"]) == (0, N_EPOCHS), tuple(r["ref_counts"])
    assert bool(r["workspace_differs"])
    for key in ("params", "exp_avg", "exp_avg_sq"):
        a, b = r["fold_" + key], r["ref_" + key]
        assert np.isfinite(b).all(), key
        assert np.array_equal(a, b), (key, float(np.abs(a - b).max()), int((a != b).sum()))
    assert np.array_equal(r["fold_stats"], r["ref_stats"]), (r["fold_stats"], r["ref_stats"])
    # not on nothing: the update moved the parameters, both moments are populated, every row of every epoch was counted
    assert not np.array_equal(r["ref_params"][:nt], r["start_params"][:nt])
    assert float(np.abs(r["ref_exp_avg"]).max()) > 0 and float(np.abs(r["ref_exp_avg_sq"]).max()) > 0
    assert r["ref_stats"][5] == N_EPOCHS * total
    norm, coef = r["fold_stats"][6], r["fold_stats"][7]
    assert norm > 0
    if max_grad_norm <= 0:
        assert coef == 1.0
    elif max_grad_norm < 0.1:
        # the clip bites (the pair read back is the one of the call's last step, an ordinary optimizer launch; the prologue forms its coefficient
        # from the same kind of partials, and a wrong one there would show in the parameters compared above)
        assert coef < 1.0 and norm > max_grad_norm, (norm, coef)


@pytest.mark.parametrize("normalize,max_grad_norm", [(True, 0.5), (False, 0.5), (True, 0.01), (True, 0.0)])
def test_headline_instantiation_on_the_eight_wave_kernel(normalize, max_grad_norm):
    """D = 4, A = 5: ppo_grad_h64_kernel<4, 2, 5>, three minibatches of 2 304 rows"""
    _check(run_case(4, 5, 3 * MB, MB, normalize, max_grad_norm), 3 * MB, max_grad_norm)


def test_hand_over_into_and_out_of_the_small_kernel():
    """2 304 + 2 304 + 512 rows: the 512-row tail runs ppo_grad_h64_small_kernel (256 threads) with a fold in front of it and behind it"""
    _check(run_case(4, 5, 2 * MB + 512, MB), 2 * MB + 512)


@pytest.mark.parametrize("D,A", [(6, 5), (4, 3), (16, 16), (9, 8), (9, 9)])
def test_runtime_width_instantiations(D, A):
    """<6, 2>; <4, 2> with a runtime head; all 2 192 non-W2 parameters (the ownership bound); both sides of the w3_blocks switch"""
    _check(run_case(D, A, 3 * MB, MB), 3 * MB)


def test_headline_shape_on_the_runtime_head_width_kernel(tmp_path):
    """D = 4, A = 5 under TMA_H64_RUNTIME_A=1 (read once per process, hence the child): the <4, 2> instantiation"""
    out = str(tmp_path / "runtime_a.npz")
    env = dict(os.environ, TMA_H64_RUNTIME_A="1")
    subprocess.run([sys.executable, os.path.join(HERE, "_h64_fold_prologue_dump.py"), out, "4", "5", str(3 * MB), str(MB), "1", "0.5"], check=True, env=env,
                   timeout=600)
    with np.load(out) as z:
        r = {k: z[k] for k in z.files}
    _check(r, 3 * MB)


@pytest.mark.parametrize("D,A", [(4, 5), (16, 16)])
def test_256_row_minibatch_chain_on_the_small_kernel(D, A):
    """three minibatches of 256 rows: 4 + 4 workgroups of 256 threads, every launch but the call's first with a folded step"""
    _check(run_case(D, A, 3 * 256, 256), 3 * 256, batch=256)
