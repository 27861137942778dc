"""CPU side of A2C: the new C-ABI symbols and their refusals, the harness lookup, the constructor's SB3 surface, and the float64 yardstick the
GPU tests (tests/test_a2c_gpu.py) measure the RMSprop kernels with.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _a2c_ref as R  # noqa: E402

NEW_SYMBOLS = ["tma_rmsprop_step", "tma_rmsprop_step_local", "tma_a2c_update_local", "tma_a2c_iterations_local"]


def test_new_symbols_are_exported_and_bound():
    from three_mlagents_amd import _lib

    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert [f[0] for f in _lib.A2CHParams._fields_] == ["ent_coef", "vf_coef", "normalize_advantage"]  # tma_a2c_hparams
    assert L.tma_version() >= 214


def test_harness_lookup_and_exports():
    import three_mlagents_amd
    from three_mlagents_amd import harness, tasks
    from three_mlagents_amd.a2c import A2C

    assert three_mlagents_amd.A2C is A2C and "A2C" in three_mlagents_amd.__all__
    assert "a2c" in harness.ALGORITHMS and harness.ALGORITHMS["a2c"] is A2C
    assert harness._algorithm_for("a2c", tasks.resolve("ball3d")) == ("a2c", None)
    assert harness._algorithm_for(None, tasks.resolve("basic"))[0] == "ppo"  # PPO still stands in for the DQN defaults
    with pytest.raises(ValueError, match="without an MI355X implementation"):
        harness._algorithm_for("dqn", tasks.resolve("basic"))
    assert harness.model_defaults("a2c", tasks.resolve("ball3d"), 8) == {}  # the reference hands A2C only tensorboard_log and verbose


def test_constructor_defaults_are_sb3s():
    from three_mlagents_amd.a2c import A2C

    want = dict(learning_rate=7e-4, n_steps=5, gamma=0.99, gae_lambda=1.0, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, rms_prop_eps=1e-5,
                use_rms_prop=True, use_sde=False, normalize_advantage=False, tensorboard_log=None, policy_kwargs=None, verbose=0, seed=None, device="auto")
    sig = inspect.signature(A2C.__init__).parameters
    for key, value in want.items():
        assert key in sig and sig[key].default == value, key
    assert "stats_window_size" in sig
    assert inspect.signature(A2C.learn).parameters["log_interval"].default == 100
    m = A2C("MlpPolicy", None)
    assert (m.learning_rate, m.n_steps, m.gae_lambda, m.rms_prop_eps, m.use_rms_prop, m.normalize_advantage) == (7e-4, 5, 1.0, 1e-5, True, False)


def test_constructor_refusals():
    from three_mlagents_amd.a2c import A2C

    with pytest.raises(ValueError, match="use_sde"):
        A2C("MlpPolicy", None, use_sde=True)
    with pytest.raises(ValueError, match="schedules"):
        A2C("MlpPolicy", None, learning_rate=lambda progress: 7e-4 * progress)


def test_float64_restatement_equals_the_literal_torch_sequence():
    """_a2c_ref.rmsprop_tflike (numpy float64) against clip_grad_norm_ + the literal RMSpropTFLike.step() sequence on torch float64 tensors: equal
    to 1e-15 relative.  Inputs span what the GPU test uses: gradient magnitudes 1e-8 .. 10 with exact zeros, state in {0, 1e-12, 1, 1e4}, the clip
    active and not."""
    rng = np.random.default_rng(0)
    n = 4097
    g = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 1, n)
    g[rng.integers(0, n, 200)] = 0.0
    sq = rng.choice([0.0, 1e-12, 1.0, 1e4], n)
    p = rng.standard_normal(n)
    norm = float(np.sqrt(np.sum(g * g)))
    for max_norm in (0.3 * norm, 2.0 * norm):
        for scale in (1.0, 0.5):
            p_ref, sq_ref, norm_ref = R.rmsprop_tflike(p, g, sq, max_norm=max_norm, grad_scale=scale)
            # the clip: norm and coefficient as torch.nn.utils.clip_grad_norm_ reports and applies them
            tp = torch.tensor(p, dtype=torch.float64).requires_grad_(True)
            tp.grad = torch.tensor(g * scale, dtype=torch.float64)
            tnorm = float(torch.nn.utils.clip_grad_norm_([tp], max_norm))
            norm_np, coef = R.clip_coef(g * scale, max_norm)
            assert norm_np == norm_ref and abs(tnorm - norm_ref) <= 1e-15 * norm_ref
            assert torch.allclose(tp.grad, torch.tensor(g * scale * coef), rtol=1e-15, atol=0)
            assert (coef < 1.0) == (max_norm < norm * scale)  # (both sides of the clip are in the sweep)
            # the step: the literal sequence on the clipped gradient
            tg, tsq = torch.tensor(g * scale * coef, dtype=torch.float64), torch.tensor(sq, dtype=torch.float64)
            with torch.no_grad():
                R.torch_rmsprop_tflike_(tp, tg, tsq)
            assert np.all(np.abs(tsq.numpy() - sq_ref) <= 1e-15 * np.abs(sq_ref))
            assert np.all(np.abs(tp.detach().numpy() - p_ref) <= 1e-15 * np.abs(p_ref))
    # eps inside the root, and a state of ones: the two things "TF-like" means
    p1, sq1, _ = R.rmsprop_tflike([0.0], [1.0], [0.0], lr=1.0, alpha=0.0, eps=3.0, max_norm=10.0)
    assert sq1[0] == 1.0 and p1[0] == -0.5  # 1 / sqrt(1 + 3), not 1 / (1 + 3)


def test_null_buffers_are_refused_before_any_hip_call():
    from three_mlagents_amd import _lib

    L = _lib.lib()
    d = _lib.PolicyDims(4, 64, 5, 0, 0, -1)
    assert L.tma_rmsprop_step(None, None, None, C.byref(d), 7e-4, 0.99, 1e-5, 0.5, 1.0, None, None) == _lib.TMA_ERR_INVALID
    assert "null" in _lib.last_error()
    assert L.tma_rmsprop_step_local(None, None, None, C.byref(d), 7e-4, 0.99, 1e-5, 0.5, None, None, 40) == _lib.TMA_ERR_INVALID
    assert "null" in _lib.last_error()
    hp = _lib.A2CHParams(0.0, 0.5, 0)
    rb = _lib.Rollout(None, None, None, None, None, 5, 8, None)
    assert L.tma_a2c_update_local(None, C.byref(d), C.byref(rb), C.byref(hp), None, None, 7e-4, 0.99, 1e-5, 0.5, None, None) == _lib.TMA_ERR_INVALID
    assert "null" in _lib.last_error()
    buf = (C.c_float * 16)()  # non-null host memory stands in for the buffers: the rollout view's null planes are refused next
    assert L.tma_a2c_update_local(buf, C.byref(d), C.byref(rb), C.byref(hp), buf, buf, 7e-4, 0.99, 1e-5, 0.5, buf, None) == _lib.TMA_ERR_INVALID
    assert "null" in _lib.last_error()
    assert L.tma_rmsprop_step(buf, buf, buf, C.byref(d), 7e-4, 1.5, 1e-5, 0.5, 1.0, buf, None) == _lib.TMA_ERR_INVALID  # alpha outside [0, 1)
    assert "alpha" in _lib.last_error()
    bad = _lib.PolicyDims(4, 65, 5, 0, 0, -1)
    assert L.tma_rmsprop_step(buf, buf, buf, C.byref(bad), 7e-4, 0.99, 1e-5, 0.5, 1.0, buf, None) == _lib.TMA_ERR_INVALID


def test_rmsprop_dispatch_ids_sit_beside_the_adam_ids():
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tma.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"(TMA_DISPATCH_OPT_[A-Z0-9_]+)(?: =)? (\d+)", header)}
    pairs = [("SCATTER_H64", "RMSPROP_SCATTER_H64"), ("SCATTER_WIDE", "RMSPROP_SCATTER_WIDE"), ("SMALL", "RMSPROP_SMALL"), ("ADAM", "RMSPROP_STEP"),
             ("LOCAL_SCATTER_H64", "RMSPROP_LOCAL_SCATTER_H64"), ("LOCAL_SCATTER_WIDE", "RMSPROP_LOCAL_SCATTER_WIDE")]
    for adam, rms in pairs:
        assert ids["TMA_DISPATCH_OPT_" + rms] == ids["TMA_DISPATCH_OPT_" + adam] + 8
    assert (ids["TMA_DISPATCH_OPT_SCATTER_H64"], ids["TMA_DISPATCH_OPT_LOCAL_SCATTER_WIDE"]) == (64, 69)  # the existing ids are unchanged
