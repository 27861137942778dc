"""H = 64 fast path of tma_ppo_train_epochs_local at minibatches the eight-wave gradient kernel takes: the per-epoch advantage pre-pass
(sample offsets + (sum, sum of squares) partials, tma_ppo_epoch_prepare's launch) is gone -- the value blocks of gradient launch k run the
pre-pass of minibatch k + 1 in their idle tail, across epoch boundaries too.  The shared body (adv_partial_block) keeps every operand and
every order of adv_partial_kernel, so the update must equal the per-epoch sequence (TMA_NO_PREP_FOLD=1) bit for bit: every case runs
collect_rollouts() once, then train() twice from the same state, and compares parameters, both Adam moments and the popped statistics
exactly -- and asks the library how many pre-passes rode on a gradient launch (tma_debug_last_prep_fold), so that a case cannot pass on
the old sequence."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _prep_fold_dump import expected_counts, run_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _check(r, total, batch, n_epochs):
    nt = int(r["n_trainable"])
    folded, alone = expected_counts(total, batch, n_epochs)
    assert folded > 0 and tuple(r["fold_counts"]) == (folded, alone), (tuple(r["fold_counts"]), folded, alone)
    assert tuple(r["ref_counts"]) == (0, n_epochs)  # the switch: one prepare launch per epoch
    n_mb = -(-total // batch)
    assert int(r["fold_adam_step"]) == int(r["ref_adam_step"]) == n_epochs * n_mb
    for key in ("params", "exp_avg", "exp_avg_sq"):
        a, b = r["fold_" + key], r["ref_" + key]
        assert np.isfinite(b).all()
        assert np.array_equal(a[:nt], b[:nt]), (key, float(np.abs(a[:nt] - b[:nt]).max()))
        assert np.array_equal(a, b), key  # (parameters: the derived copies and weight images behind the trainable part as well)
    assert np.array_equal(r["fold_stats"], r["ref_stats"]), (r["fold_stats"], r["ref_stats"])
    # not on nothing: the update moved the parameters, both moments are populated, every sample of every epoch was counted
    assert not np.array_equal(r["ref_params"][:nt], r["start_params"][:nt])
    assert float(np.abs(r["ref_exp_avg"]).max()) > 0 and float(np.abs(r["ref_exp_avg_sq"]).max()) > 0
    assert r["ref_stats"][6] == n_epochs * total


def test_launch_counts_follow_the_hand_over_rule():
    """(no GPU work) what the cases below expect of tma_debug_last_prep_fold"""
    assert expected_counts(8192, 4096, 2) == (3, 1)
    assert expected_counts(8192, 2560, 2) == (4, 4)  # 2560 / 2560 / 2560 / 512: the 512 runs on the small kernel, so does not carry and is not carried
    assert expected_counts(262144, 131072, 2) == (3, 1)
    assert expected_counts(8192, 4096, 1) == (1, 1)


@pytest.mark.parametrize("task,n_envs,n_steps,batch,n_epochs,normalize", [
    ("gridworld", 64, 128, 4096, 2, True),       # 1: the <4, 2, 5> kernel, 4 partial blocks of the next minibatch against 32 block pairs, one epoch boundary
    ("gridworld", 64, 128, 2560, 2, True),       # 2: into and out of the small kernel on the 512-row tail; an epoch boundary behind a small-kernel launch
    ("gridworld", 256, 1024, 131072, 2, True),   # 3: the headline launch geometry: 128 pairs, 128 partial blocks of 1 024 rows
    ("gridworld", 64, 128, 4096, 2, False),      # 4: advantages not normalised: offsets only
    ("ball3d", 64, 128, 4096, 2, True),          # 5b: 6 observations: the <6, 2> instantiation
    ("bicycle", 64, 128, 4096, 2, True),         # 5c: 7 observations, 3 actions: the runtime-width <0, 2> instantiation
    ("gridworld", 64, 128, 4096, 1, True),       # 6: one epoch: nothing carried past the call, exactly one stand-alone pre-pass
])
def test_folded_pre_pass_equals_the_per_epoch_prepare_bit_for_bit(task, n_envs, n_steps, batch, n_epochs, normalize):
    r = run_case(task, n_envs, n_steps, batch, n_epochs, normalize)
    _check(r, n_envs * n_steps, batch, n_epochs)


def test_folded_pre_pass_on_the_runtime_head_width_kernel(tmp_path):
    """5a: shape 1 under TMA_H64_RUNTIME_A=1 (read once per process, hence the child): GridWorld on the <4, 2> instantiation"""
    out = str(tmp_path / "runtime_a.npz")
    env = dict(os.environ, TMA_H64_RUNTIME_A="1")
    subprocess.run([sys.executable, os.path.join(HERE, "_prep_fold_dump.py"), out, "gridworld", "64", "128", "4096", "2", "1"], check=True, env=env, timeout=600)
    with np.load(out) as z:
        r = {k: z[k] for k in z.files}
    _check(r, 64 * 128, 4096, 2)
