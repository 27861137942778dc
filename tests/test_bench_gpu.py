"""`python bench.py` without --full: the headline figure of the timed iterations and nothing else, and --dump-outputs writes what the
last timed iteration computed (the updated policy parameters, a seeded sample of its rollout buffer) as float32 / float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")
DUMPED = ("policy_params", "sample_index", "last_values", "obs", "actions", "log_probs", "values", "rewards", "terminated", "truncated", "advantages",
          "returns")


@pytest.mark.timeout(300)
def test_plain_run_prints_the_headline_and_dumps_the_last_iteration(tmp_path):
    N, T, steps = 512, 64, 3
    dump = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--n-envs", str(N), "--n-steps", str(T),
           "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in CONTRACT:
        assert k in d, k
    assert d["metric"] == "env_steps_per_sec" and d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == steps and d["warmup"] == 1 and d["config"]["envs_per_gpu"] == N
    assert d["value"] == pytest.approx(N * T / (d["ms_per_step"] * 1e-3), rel=1e-6)
    assert not any(k in d for k in ("roofline", "cpu_baseline", "extra_configs", "other_rooflines", "literal_batch_256")) and d["extras_path"] is None

    got = {os.path.splitext(f)[0]: np.load(dump / f) for f in os.listdir(dump)}
    assert sorted(got) == sorted(DUMPED)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["policy_params"].shape == (9350,) and np.isfinite(got["policy_params"]).all()  # GridWorld, MLP pi/vf 64x64
    idx = got["sample_index"]
    assert idx.shape == (N * T,) and np.array_equal(idx, np.arange(N * T))  # a rollout this small is dumped whole
    assert got["obs"].shape == (N * T, 4) and got["last_values"].shape == (N,)
    for k in ("actions", "log_probs", "values", "rewards", "terminated", "truncated", "advantages", "returns"):
        assert got[k].shape == (N * T,) and np.isfinite(got[k]).all(), k
    assert np.isin(got["actions"], np.arange(5)).all() and np.isin(got["terminated"], (0.0, 1.0)).all()
    assert np.allclose(got["returns"], got["advantages"] + got["values"], rtol=1e-6, atol=1e-6)  # SB3: returns = advantages + values
