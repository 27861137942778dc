"""tma_explained_variance (SB3's `train/explained_variance`) and the `train/` keys PPO.learn logs with it: explained_variance, learning_rate,
clip_range, std (Box heads) -- in logger_values, progress.csv and both logging modes.

The device result is held to 2e-9 * max(1, |1 - ev|) against numpy in float64: each of the two variances is a sum of at most 2^22 + 3 float64
terms, and n * 2^-53 ~ 4.7e-10 bounds the relative error of such a fixed-order sum in the worst case.  tests/test_explained_variance_cpu.py
shows that numpy's float64 value itself is within a few 1e-15 of the exact one for these inputs."""
import csv
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1000, 131072, 2 ** 22 + 3)
NOISE = (0.3, 3.0)


def synthetic(n, noise, seed=0):
    """returns = 100 + N(0, 1), values = returns + noise * N(0, 1), float32."""
    rng = np.random.default_rng(seed + n)
    returns = (100.0 + rng.standard_normal(n)).astype(np.float32)
    values = (returns.astype(np.float64) + noise * rng.standard_normal(n)).astype(np.float32)
    return values, returns


def bound(ev):
    return 2e-9 * max(1.0, abs(1.0 - ev))


def numpy_ev(values, returns):
    y, p = np.asarray(returns, np.float32).astype(np.float64).ravel(), np.asarray(values, np.float32).astype(np.float64).ravel()
    var_y = np.var(y)
    return float("nan") if var_y == 0 else float(1.0 - np.var(y - p) / var_y)


def device_ev(values, returns):
    from three_mlagents_amd import _lib

    v, r = torch.from_numpy(values).cuda(), torch.from_numpy(returns).cuda()
    scratch = torch.full((_lib.EV_SCRATCH_DOUBLES,), float("nan"), dtype=torch.float64, device="cuda")  # (a partial the kernels did not write would poison the result)
    out = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().tma_explained_variance(_lib.ptr(v), _lib.ptr(r), v.numel(), _lib.ptr(scratch), _lib.ptr(out), _lib.stream_ptr()))
    return float(out.cpu()[0])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("noise", NOISE)
def test_matches_numpy_float64_and_is_bit_identical_from_run_to_run(n, noise):
    values, returns = synthetic(n, noise)
    ref = numpy_ev(values, returns)
    a, b = device_ev(values, returns), device_ev(values, returns)
    print(f"n = {n}, noise {noise}: numpy f64 {ref!r}, device {a!r}, |diff| {abs(a - ref):.3g}, bound {bound(ref):.3g}")
    assert abs(a - ref) <= bound(ref), (a, ref)
    assert np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.mark.parametrize("n", (1, 7, 1000, 300001))
def test_constant_returns_give_nan(n):
    returns = np.full(n, 100.25, np.float32)
    values = (returns + np.random.default_rng(1).standard_normal(n)).astype(np.float32)
    assert np.isnan(numpy_ev(values, returns)) and np.isnan(device_ev(values, returns))


def test_small_and_odd_sizes():
    for n in (2, 3, 63, 64, 65, 255, 257, 1023, 1025, 262145):
        values, returns = synthetic(n, 1.0, seed=11)
        ref, dev = numpy_ev(values, returns), device_ev(values, returns)
        assert abs(dev - ref) <= bound(ref), (n, dev, ref)


def _learn_once(tmp_path, monkeypatch, name, sync, task="gridworld", n_envs=256, hidden=64):
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv

    if sync:
        monkeypatch.setenv("TMA_SYNC_LOGGING", "1")
    else:
        monkeypatch.delenv("TMA_SYNC_LOGGING", raising=False)
    env = HipVecEnv(task, n_envs, seed=3)
    try:
        model = PPO("MlpPolicy", env, n_steps=64, batch_size=2048, n_epochs=2, seed=5, learning_rate=2.5e-4, clip_range=0.15,
                    policy_kwargs={"net_arch": [hidden, hidden]}, tensorboard_log=str(tmp_path / name))
        model.learn(n_envs * 64)  # one iteration
        torch.cuda.synchronize()
        with open(tmp_path / name / "progress.csv") as f:
            rows = list(csv.DictReader(f))
        ref = numpy_ev(model.buf["values"].cpu().numpy(), model.buf["returns"].cpu().numpy())
        log_std = model.policy.state_dict().get("log_std")
        return dict(model.logger_values), rows, ref, log_std
    finally:
        env.close()


def test_learn_logs_the_new_train_keys_in_both_logging_modes(tmp_path, monkeypatch):
    lv_p, rows_p, ref_p, _ = _learn_once(tmp_path, monkeypatch, "pipelined", False)
    lv_s, rows_s, ref_s, _ = _learn_once(tmp_path, monkeypatch, "sync", True)
    assert ref_p == ref_s and np.isfinite(ref_p)  # (the two modes train the same model)
    for lv, rows, ref in ((lv_p, rows_p, ref_p), (lv_s, rows_s, ref_s)):
        assert len(rows) == 1
        for key in ("train/explained_variance", "train/learning_rate", "train/clip_range"):
            assert key in lv and key in rows[0], key
            assert float(rows[0][key]) == lv[key]
        assert "train/std" not in lv and "train/std" not in rows[0]  # (Box heads only)
        print(f"train/explained_variance {lv['train/explained_variance']!r}, numpy f64 over the buffer {ref!r}")
        assert abs(lv["train/explained_variance"] - ref) <= bound(ref)
        assert lv["train/learning_rate"] == 2.5e-4 and lv["train/clip_range"] == 0.15
    assert np.float64(lv_p["train/explained_variance"]).tobytes() == np.float64(lv_s["train/explained_variance"]).tobytes()
    # the keys that were there before are still there, with the values of the other mode
    for key in ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/approx_kl", "train/clip_fraction", "train/n_updates"):
        assert key in lv_p and abs(lv_p[key] - lv_s[key]) <= 1e-12 * max(1.0, abs(lv_s[key])), key  # (tests/test_dropin_gpu.py's comparison of the two modes)


@pytest.mark.parametrize("sync", (False, True), ids=("pipelined", "sync"))
def test_a_box_head_also_logs_train_std(tmp_path, monkeypatch, sync):
    lv, rows, ref, log_std = _learn_once(tmp_path, monkeypatch, "ant", sync, task="ant", n_envs=64, hidden=256)
    assert log_std is not None and bool((log_std != 0).any())  # (the update moved it: the logged value is the one AFTER the update, as SB3's)
    want = float(torch.exp(log_std.to(torch.float32)).mean())
    assert lv["train/std"] == want and float(rows[0]["train/std"]) == want
    assert abs(lv["train/explained_variance"] - ref) <= bound(ref)
