"""The H = 64 gradient kernel has an instantiation with the head width as a compile-time constant for the headline shape (GridWorld: 4
observations, 5 actions); every other shape, and every shape under TMA_H64_RUNTIME_A=1, runs the runtime-width kernel.  Folding the width
removes branches, dead MFMA paths and the loss work of head rows that can never hold an action -- no operation on a live value changes and
no sum changes its order, so the two kernels must agree to the last bit: the gradient of one minibatch, and parameters and both Adam moments
after two update epochs through tma_ppo_train_epoch_local.  Sizes: those at which tests/test_policy_dispatch_gpu.py reaches GRAD_H64 (2 049
and 16 385 end in a partial tile; 131 072 is the headline minibatch).  Both paths are held to a float64 reference there: (4, 64, 5) takes
the specialised kernel, (16, 64, 16) the runtime one."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _dump(tmp_path, name, batch, **env):
    out = str(tmp_path / f"{name}.npz")
    e = {k: v for k, v in os.environ.items() if k != "TMA_H64_RUNTIME_A"}
    e.update(env)
    subprocess.run([sys.executable, os.path.join(HERE, "_h64_head_width_dump.py"), str(batch), out], check=True, env=e, timeout=600)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("batch", [2049, 16385, 131072])
def test_compile_time_head_width_kernel_equals_the_runtime_width_kernel_bit_for_bit(tmp_path, batch):
    from test_policy_dispatch_gpu import expected_value

    spec = _dump(tmp_path, "specialised", batch)
    runt = _dump(tmp_path, "runtime", batch, TMA_H64_RUNTIME_A="1")
    for r in (spec, runt):
        assert int(r["grad_dispatch"]) == expected_value("GRAD_H64")
        assert np.isfinite(r["grad"]).all() and float(np.abs(r["grad"]).max()) > 0
        assert r["grad_stats"][5] == batch
        assert np.isfinite(r["params"]).all() and int(r["n_steps"]) == 2 * 3  # (two full minibatches and a short one per epoch)
    for key in ("grad", "grad_stats", "params", "exp_avg", "exp_avg_sq", "epoch_stats"):
        assert np.array_equal(spec[key], runt[key]), (key, float(np.abs(spec[key] - runt[key]).max()))
    assert float(np.abs(spec["exp_avg"]).max()) > 0 and float(np.abs(spec["exp_avg_sq"]).max()) > 0
