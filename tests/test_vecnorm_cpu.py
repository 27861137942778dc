"""VecNormalize without a GPU: the float64 restatement (tests/_vecnorm_ref.py) against exact rational arithmetic and against a literal
transcription of SB3's six steps; the C ABI's symbols and host-side refusals; the Python surface (constructor defaults, TrainConfig, parser).

Bounds (eps = 2^-53, n rows per batch), derived from rounding, not measured:
  * a float64 sum of n terms carries at most (n - 1) roundings of relative size eps each, the division one more: the batch mean is within
    n eps max|x| of the exact one; 4 n eps max|x| leaves margin for any summation order;
  * the centred squares (x - mean)^2 carry the mean's error twice plus three roundings each, their sum n more: 16 n eps max|x - mean|^2;
  * a merge is a dozen float64 operations on top of the batch moments, with no cancellation in M2 (a sum of non-negative terms), so k merges
    stay within 8 k n eps -- of the variance itself for the variance, of max|x| for the mean (whose terms are of that size).
"""
import ctypes as C
import dataclasses
import inspect
import os
from fractions import Fraction

import numpy as np
import pytest

import _vecnorm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53

NEW_SYMBOLS = ["tma_vecnorm_create", "tma_vecnorm_destroy", "tma_vecnorm_set_flags", "tma_vecnorm_reset", "tma_vecnorm_step", "tma_vecnorm_normalize_obs",
               "tma_vecnorm_unnormalize_obs", "tma_vecnorm_normalize_reward", "tma_vecnorm_unnormalize_reward", "tma_vecnorm_get_stats",
               "tma_vecnorm_set_stats", "tma_vecnorm_copy_stats", "tma_vecnorm_get_returns", "tma_vecnorm_get_original", "tma_rollout_collect_norm"]


def _cases():
    rng = np.random.default_rng(7)
    plain = (rng.uniform(-1000.0, 1000.0, size=(4, 33, 3))).astype(np.float32)
    offset = (1e5 + rng.integers(0, 64, size=(4, 33, 3)) / 64.0).astype(np.float32)  # spread ~ 1 on top of 1e5: every value is float32-exact
    assert np.array_equal(offset.astype(np.float64), 1e5 + np.round((offset.astype(np.float64) - 1e5) * 64) / 64)
    single = rng.uniform(-1000.0, 1000.0, size=(3, 1, 2)).astype(np.float32)
    return {"plain": plain, "offset": offset, "single_row": single}


def _exact_moments(batch):
    n, d = batch.shape
    cols = [[Fraction(float(v)) for v in batch[:, j]] for j in range(d)]
    mean = [sum(c) / n for c in cols]
    var = [sum((v - m) ** 2 for v in c) / n for c, m in zip(cols, mean)]
    return mean, var


@pytest.mark.parametrize("name", ["plain", "offset", "single_row"])
def test_reference_moments_and_merges_against_exact_arithmetic(name):
    batches = _cases()[name]
    k_total, n, d = batches.shape
    rms = ref.RunningMeanStd(shape=(d,))
    ex_mean, ex_var, ex_count = [Fraction(0)] * d, [Fraction(1)] * d, Fraction(1e-4)
    for k, batch in enumerate(batches, start=1):
        bm, bv, rows = ref.batch_moments(batch)
        em, ev = _exact_moments(batch)
        amax = float(np.abs(batch.astype(np.float64)).max())
        for j in range(d):
            dev = max(abs(Fraction(float(v)) - em[j]) for v in batch[:, j])
            assert abs(Fraction(float(bm[j])) - em[j]) <= 4 * n * EPS * amax, (name, k, j)
            assert abs(Fraction(float(bv[j])) - ev[j]) <= 16 * n * EPS * float(dev) ** 2, (name, k, j)
        if n == 1:
            assert np.array_equal(bv, np.zeros(d)) and np.array_equal(bm, batch[0].astype(np.float64))
        rms.update(batch)
        tot = ex_count + rows
        for j in range(d):
            delta = em[j] - ex_mean[j]
            m2 = ex_var[j] * ex_count + ev[j] * rows + delta * delta * ex_count * rows / tot
            ex_mean[j], ex_var[j] = ex_mean[j] + delta * rows / tot, m2 / tot
        ex_count = tot
        seen = float(np.abs(batches[:k].astype(np.float64)).max())
        for j in range(d):
            assert abs(Fraction(float(rms.mean[j])) - ex_mean[j]) <= 8 * k * n * EPS * seen, (name, k, j)
            assert abs(Fraction(float(rms.var[j])) - ex_var[j]) <= 8 * k * n * EPS * ex_var[j], (name, k, j)
        assert abs(Fraction(rms.count) - ex_count) <= 8 * k * EPS * ex_count


def test_naive_variance_is_wrong_on_the_offset_case():
    """Why the kernels must use centred sums: E[x^2] - E[x]^2 in float64 loses the sixth digit of the variance at 1e5 + k / 64."""
    batch = _cases()["offset"][0]
    x = batch.astype(np.float64)
    naive = (x * x).mean(axis=0) - x.mean(axis=0) ** 2
    _, exact = _exact_moments(batch)
    _, two_pass, _ = ref.batch_moments(batch)
    rel_naive = max(abs(Fraction(float(a)) - e) / e for a, e in zip(naive, exact))
    rel_two = max(abs(Fraction(float(a)) - e) / e for a, e in zip(two_pass, exact))
    assert rel_naive > 1e-7 and rel_two < 1e-13, (float(rel_naive), float(rel_two))


def _literal_run(obs_seq, rew_seq, done_seq, tobs_seq, reset_obs, *, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0,
                 gamma=0.99, epsilon=1e-8, freeze_after=None):
    """SB3's reset() and the six steps of step_wait(), written out line by line on plain arrays (no shared code with the restatement)."""
    n, d = reset_obs.shape
    o_mean, o_var, o_count = np.zeros(d), np.ones(d), 1e-4
    r_mean, r_var, r_count = 0.0, 1.0, 1e-4
    returns = np.zeros(n)

    def upd(mean, var, count, x):
        x = np.asarray(x, np.float64)
        bm = x.sum(axis=0) / x.shape[0]
        bv = ((x - bm) ** 2).sum(axis=0) / x.shape[0]
        delta, tot = bm - mean, count + x.shape[0]
        return mean + delta * x.shape[0] / tot, (var * count + bv * x.shape[0] + delta ** 2 * count * x.shape[0] / tot) / tot, tot

    def nobs(o):
        return np.clip((o.astype(np.float64) - o_mean) / np.sqrt(o_var + epsilon), -clip_obs, clip_obs).astype(np.float32) if norm_obs else o

    if training and norm_obs:
        o_mean, o_var, o_count = upd(o_mean, o_var, o_count, reset_obs)
    log = [dict(obs=nobs(reset_obs))]
    for t, (obs, rew, done, tobs) in enumerate(zip(obs_seq, rew_seq, done_seq, tobs_seq)):
        if freeze_after is not None and t >= freeze_after:
            training = False
        if training and norm_obs:                                   # 1
            o_mean, o_var, o_count = upd(o_mean, o_var, o_count, obs)
        out_obs = nobs(obs)                                         # 2
        if training:                                                # 3
            returns = returns * gamma + rew.astype(np.float64)
            r_mean, r_var, r_count = upd(r_mean, r_var, r_count, returns)
        out_rew = np.clip(rew.astype(np.float64) / np.sqrt(r_var + epsilon), -clip_reward, clip_reward).astype(np.float32) if norm_reward else rew  # 4
        out_tobs = tobs.copy()                                      # 5
        for i in np.nonzero(done)[0]:
            out_tobs[i] = nobs(tobs[i])
        returns_before_zeroing = returns.copy()
        returns = returns.copy()
        returns[done] = 0.0                                         # 6
        log.append(dict(obs=out_obs, rew=out_rew, tobs=out_tobs, returns=returns.copy(), returns_before=returns_before_zeroing, o_mean=o_mean.copy(),
                        o_var=o_var.copy(), o_count=o_count, r_mean=r_mean, r_var=r_var, r_count=r_count))
    return log


def _script(seed=3, n=5, d=4, steps=9):
    rng = np.random.default_rng(seed)
    reset_obs = rng.normal(3.0, 2.0, size=(n, d)).astype(np.float32)
    obs = rng.normal(3.0, 2.0, size=(steps, n, d)).astype(np.float32)
    rew = rng.normal(1.0, 5.0, size=(steps, n)).astype(np.float32)
    done = rng.random((steps, n)) < 0.3
    done[2] = False
    done[4, 1] = True
    tobs = rng.normal(40.0, 2.0, size=(steps, n, d)).astype(np.float32)  # far from the observations: they would move the statistics if they entered
    return reset_obs, obs, rew, done, tobs


@pytest.mark.parametrize("kw", [{}, {"norm_reward": False}, {"norm_obs": False}, {"clip_obs": 0.5, "clip_reward": 0.25, "gamma": 0.9, "epsilon": 1e-4}])
def test_restated_wrapper_matches_the_literal_six_steps(kw):
    reset_obs, obs, rew, done, tobs = _script()
    log = _literal_run(obs, rew, done, tobs, reset_obs, **kw)
    w = ref.VecNormalizeRef(reset_obs.shape[0], reset_obs.shape[1], **kw)
    assert np.array_equal(w.reset(reset_obs), log[0]["obs"])
    for t in range(len(obs)):
        o, r, tb = w.step(obs[t], rew[t], done[t], tobs[t])
        e = log[t + 1]
        assert np.array_equal(o, e["obs"]) and np.array_equal(r, e["rew"]) and np.array_equal(tb, e["tobs"]), t
        assert np.array_equal(w.returns, e["returns"]) and np.array_equal(w.obs_rms.mean, e["o_mean"]) and np.array_equal(w.obs_rms.var, e["o_var"])
        assert (w.obs_rms.count, float(w.ret_rms.mean), float(w.ret_rms.var), w.ret_rms.count) == (e["o_count"], e["r_mean"], e["r_var"], e["r_count"])
        # returns are zeroed AFTER they entered the statistics and the reward was normalised, exactly where done
        assert np.array_equal(w.returns == 0.0, done[t] | (e["returns_before"] == 0.0))
        assert np.array_equal(w.get_original_obs(), obs[t]) and np.array_equal(w.get_original_reward(), rew[t])
        # terminal observations use the statistics of THIS step and never enter them: the rows of unfinished envs are untouched
        assert np.array_equal(tb[~done[t]], tobs[t][~done[t]])
        if kw.get("norm_obs", True) and done[t].any():
            assert np.array_equal(tb[done[t]], ref.normalize_obs_with(tobs[t][done[t]], w.obs_rms.mean, w.obs_rms.var, w.epsilon, w.clip_obs))
    if kw.get("norm_reward", True) is False:  # ret_rms moves although rewards pass through
        assert w.ret_rms.count == 1e-4 + len(obs) * reset_obs.shape[0] and float(w.ret_rms.var) != 1.0
    if kw.get("norm_obs", True) is False:
        assert w.obs_rms.count == 1e-4 and np.array_equal(w.obs_rms.var, np.ones(4))
    else:  # had the terminal observations (around 40) entered, the mean would sit far above the observations' 3
        assert np.all(np.abs(w.obs_rms.mean - 3.0) < 1.5)


def test_training_false_freezes_the_statistics():
    reset_obs, obs, rew, done, tobs = _script(seed=5)
    log = _literal_run(obs, rew, done, tobs, reset_obs, freeze_after=4)
    w = ref.VecNormalizeRef(reset_obs.shape[0], reset_obs.shape[1])
    w.reset(reset_obs)
    for t in range(len(obs)):
        if t == 4:
            w.training = False
            frozen = (w.obs_rms.mean.copy(), w.obs_rms.var.copy(), w.obs_rms.count, float(w.ret_rms.mean), float(w.ret_rms.var), w.ret_rms.count, w.returns.copy())
        o, r, tb = w.step(obs[t], rew[t], done[t], tobs[t])
        e = log[t + 1]
        assert np.array_equal(o, e["obs"]) and np.array_equal(r, e["rew"]) and np.array_equal(tb, e["tobs"]) and np.array_equal(w.returns, e["returns"])
        if t >= 4:
            assert np.array_equal(w.obs_rms.mean, frozen[0]) and np.array_equal(w.obs_rms.var, frozen[1]) and w.obs_rms.count == frozen[2]
            assert (float(w.ret_rms.mean), float(w.ret_rms.var), w.ret_rms.count) == frozen[3:6]
    assert w.obs_rms.count == 1e-4 + 5 * reset_obs.shape[0]  # the reset and four steps


def test_unnormalize_inverts_normalize_inside_the_clip():
    reset_obs, obs, rew, done, tobs = _script(seed=9)
    w = ref.VecNormalizeRef(reset_obs.shape[0], reset_obs.shape[1], clip_obs=100.0, clip_reward=100.0)
    w.reset(reset_obs)
    w.step(obs[0], rew[0], done[0], tobs[0])
    assert np.allclose(w.unnormalize_obs(w.normalize_obs(obs[1])), obs[1], rtol=1e-5, atol=1e-5)
    assert np.allclose(w.unnormalize_reward(w.normalize_reward(rew[1])), rew[1], rtol=1e-5, atol=1e-5)


# ---- the C ABI on the host: symbols and refusals (no HIP call is reached) ----

def _lib():
    from three_mlagents_amd import _lib

    return _lib


def test_library_exports_every_new_symbol():
    lib = _lib()
    L = lib.lib()
    header = open(os.path.join(ROOT, "include", "tma.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in lib.SIGNATURES and f"{name}(" in header, name
    assert L.tma_version() >= 217
    assert lib.VECNORM_ONE_LAUNCH_MAX == int(__import__("re").search(r"#define TMA_VECNORM_ONE_LAUNCH_MAX (\d+)", header).group(1)) >= 64


def _refused(status):
    lib = _lib()
    assert status == lib.TMA_ERR_INVALID, status
    assert lib.last_error(), "a refusal carries a message"


GOOD = dict(D=6, N=8, norm_obs=1, norm_reward=1, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8, device=0)


def _create(**over):
    lib = _lib()
    a = {**GOOD, **over}
    h = C.c_void_p()
    rc = lib.lib().tma_vecnorm_create(a["D"], a["N"], a["norm_obs"], a["norm_reward"], a["clip_obs"], a["clip_reward"], a["gamma"], a["epsilon"], a["device"], C.byref(h))
    return rc, h


@pytest.mark.parametrize("over", [{"D": 0}, {"D": -3}, {"D": 100000}, {"N": 0}, {"N": -1}, {"clip_obs": 0.0}, {"clip_obs": -1.0}, {"clip_reward": 0.0},
                                  {"clip_reward": float("nan")}, {"epsilon": 0.0}, {"epsilon": -1e-8}, {"gamma": -0.01}, {"gamma": 1.01}, {"gamma": float("nan")}])
def test_create_refuses_bad_arguments(over):
    rc, h = _create(**over)
    _refused(rc)
    assert not h.value


def test_create_refuses_null_output_and_accepts_the_edges():
    lib = _lib()
    _refused(lib.lib().tma_vecnorm_create(6, 8, 1, 1, 10.0, 10.0, 0.99, 1e-8, 0, None))
    for over in ({"gamma": 0.0}, {"gamma": 1.0}, {"D": 1, "N": 1}):
        rc, h = _create(**over)
        assert rc == lib.TMA_OK and h.value
        assert lib.lib().tma_vecnorm_destroy(h) == lib.TMA_OK


def test_null_handles_are_refused():
    L = _lib().lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for status in (L.tma_vecnorm_destroy(None), L.tma_vecnorm_set_flags(None, 1, 1), L.tma_vecnorm_reset(None, p, 8, 1, None),
                   L.tma_vecnorm_step(None, p, p, p, p, p, 8, 1, None), L.tma_vecnorm_normalize_obs(None, p, p, 1, None),
                   L.tma_vecnorm_unnormalize_obs(None, p, p, 1, None), L.tma_vecnorm_normalize_reward(None, p, p, 1, None),
                   L.tma_vecnorm_unnormalize_reward(None, p, p, 1, None), L.tma_vecnorm_get_stats(None, p, p, p, None),
                   L.tma_vecnorm_set_stats(None, p, p, p, None), L.tma_vecnorm_copy_stats(None, None, None), L.tma_vecnorm_get_returns(None, p, None),
                   L.tma_vecnorm_get_original(None, p, p, None)):
        _refused(status)
    dims = _lib().PolicyDims(6, 64, 5, 0, 0, 0)
    rb = _lib().RolloutBuffers(p, p, p, p, p, p, p, p, p, 8, 1)
    _refused(L.tma_rollout_collect_norm(None, None, p, C.byref(dims), C.byref(rb), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))


def test_null_planes_and_wrong_row_counts_are_refused_before_any_hip_call():
    """A handle allocates its device memory on first use, so these calls are answered on a machine without a GPU."""
    lib = _lib()
    L = lib.lib()
    rc, h = _create()
    assert rc == lib.TMA_OK
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    try:
        _refused(L.tma_vecnorm_reset(h, None, 8, 1, None))
        _refused(L.tma_vecnorm_reset(h, p, 7, 1, None))  # N differs from the handle's
        _refused(L.tma_vecnorm_step(h, None, p, p, p, p, 8, 1, None))
        _refused(L.tma_vecnorm_step(h, p, None, p, p, p, 8, 1, None))
        _refused(L.tma_vecnorm_step(h, p, p, p, None, p, 8, 1, None))
        _refused(L.tma_vecnorm_step(h, p, p, p, p, None, 8, 1, None))
        _refused(L.tma_vecnorm_step(h, p, p, p, p, p, 9, 1, None))  # N differs from the handle's
        _refused(L.tma_vecnorm_normalize_obs(h, None, p, 4, None))
        _refused(L.tma_vecnorm_normalize_obs(h, p, p, 0, None))
        _refused(L.tma_vecnorm_unnormalize_reward(h, p, None, 4, None))
        _refused(L.tma_vecnorm_get_stats(h, None, p, p, None))
        _refused(L.tma_vecnorm_set_stats(h, p, None, p, None))
        _refused(L.tma_vecnorm_get_returns(h, None, None))
        _refused(L.tma_vecnorm_get_original(h, None, None, None))
        rc2, other = _create(D=7)
        assert rc2 == lib.TMA_OK
        _refused(L.tma_vecnorm_copy_stats(h, other, None))  # observation widths differ
        assert L.tma_vecnorm_destroy(other) == lib.TMA_OK
        # the rollout driver: null env / null plane / buffers whose N differs from the handle's, all before the env handle is looked at
        dims = lib.PolicyDims(6, 64, 5, 0, 0, 0)
        fake_env = p  # never dereferenced: the checks below fail first
        rb = lib.RolloutBuffers(p, p, p, p, p, p, p, p, p, 9, 1)
        _refused(L.tma_rollout_collect_norm(fake_env, h, p, C.byref(dims), C.byref(rb), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
        rb_null = lib.RolloutBuffers(p, None, p, p, p, p, p, p, p, 8, 1)
        _refused(L.tma_rollout_collect_norm(fake_env, h, p, C.byref(dims), C.byref(rb_null), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
        dims7 = lib.PolicyDims(7, 64, 5, 0, 0, 0)
        rb8 = lib.RolloutBuffers(p, p, p, p, p, p, p, p, p, 8, 1)
        _refused(L.tma_rollout_collect_norm(fake_env, h, p, C.byref(dims7), C.byref(rb8), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
        _refused(L.tma_rollout_collect_norm(fake_env, h, p, C.byref(dims), C.byref(rb8), 2, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))  # bad step range
        assert L.tma_vecnorm_set_flags(h, 0, 1) == lib.TMA_OK
    finally:
        assert L.tma_vecnorm_destroy(h) == lib.TMA_OK


# ---- the Python surface ----

def test_constructor_defaults_are_sb3s():
    from three_mlagents_amd.vec_env import HipVecEnv
    from three_mlagents_amd.vec_normalize import VecNormalize, sync_envs_normalization

    params = inspect.signature(VecNormalize.__init__).parameters
    assert list(params) == ["self", "venv", "training", "norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma", "epsilon"]
    assert {k: p.default for k, p in params.items() if p.default is not inspect.Parameter.empty} == dict(
        training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)
    assert issubclass(VecNormalize, HipVecEnv) and callable(sync_envs_normalization)
    for name in ("reset", "step_async", "step_wait", "step", "reset_device", "step_device", "normalize_obs", "normalize_reward", "unnormalize_obs",
                 "unnormalize_reward", "get_original_obs", "get_original_reward", "save", "load", "norm_obs", "norm_reward", "close"):
        assert hasattr(VecNormalize, name), name
    with pytest.raises(ValueError):
        VecNormalize(object())


def test_train_config_and_parser():
    from three_mlagents_amd import harness
    from three_mlagents_amd.__main__ import parser

    assert harness.TrainConfig("basic").normalize is False
    assert [f.name for f in dataclasses.fields(harness.TrainConfig)][-1] == "normalize"
    assert harness.TrainConfig("basic", normalize=True).normalize is True
    assert parser().parse_args(["train", "ball3d", "--normalize"]).normalize is True
    assert parser().parse_args(["train", "ball3d"]).normalize is False
