"""The 64-wide fused rollout chunk runs on eight waves per 16-env tile (rollout_chunk8_h64_kernel: a wave holds one 16-unit tile of a net,
the activations of a layer are formed once and exchanged through LDS) wherever it ran on four (rollout_chunk4_h64_kernel, now behind
TMA_ROLL4=1).  Per accumulator the operations and their order are those of h64t_forward in both, so the two kernels must agree to the last
bit: two consecutive rollouts, every plane of the buffer after each, last_values, advantages and returns, the env state and the episode
index behind the second, every episode's Monitor record (return, length, env).

The Monitor AGGREGATE is three float64 sums a 256-env slot collects with one atomic add per tile and launch, in whatever order the 16
workgroups of the slot arrive -- the same for both kernels.  Episode count and summed length are integers (exact in any order) and are
compared exactly; the summed return is compared exactly where a slot has ONE tile (16 envs), and elsewhere to the rounding of a float64 sum
taken in another order (n terms: n * 2^-53 * sum |r|) -- the per-episode returns that go into it are compared bit for bit.

So that a case cannot pass on nothing: the two runs must report different kernels (tma_debug_last_rollout_waves), and the compared buffers
must hold at least one terminated and one truncated row -- n_steps is chosen from the task's step limit (two rollouts reach past it).
Bicycle and Glider never reach their limits of 2000 / 4000 steps under an untrained policy (196 074 Bicycle episodes in 2 x 1001 steps at
4096 envs, none truncated), so for these two the helper sets the step counter of every fourth env to within 32 steps of the limit behind the
first reset (state injection, tma_env_set_state) and the rollouts are 129 steps.
Glider stays on four waves by a compile-time property of the task (its env step does not fit the 256 registers a wave of eight has): for it
the test pins that both runs report four waves, and the results still have to agree."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PLANES = ("obs", "actions", "rewards", "values", "log_probs", "terminated", "truncated", "last_values", "advantages", "returns")
AFTER = ("env_state", "episode_index", "episode_returns", "episode_lengths", "episode_envs")
MAXSTEPS = {"gridworld": 100, "push": 120, "walljump": 150, "ball3d": 200, "bicycle": 2000, "glider": 4000}  # tests/test_abi_cpu.py pins these
FOUR_WAVE_TASKS = ("glider",)


AGED_TASKS = ("bicycle", "glider")


def _dump(tmp_path, name, task, n_envs, n_steps, det, **env):
    out = str(tmp_path / name)
    e = {k: v for k, v in os.environ.items() if k not in ("TMA_ROLL4", "TMA_ROLL2")}
    e.update(env)
    subprocess.run([sys.executable, os.path.join(HERE, "_rollout_h64_waves_dump.py"), task, str(n_envs), str(n_steps), str(det), out,
                    str(MAXSTEPS[task] if task in AGED_TASKS else 0)], check=True, env=e, timeout=900)
    return out


def _load(d, key):
    return np.load(os.path.join(d, key + ".npy"), mmap_mode="r")


def _n_steps(task):  # two rollouts of this many steps reach one step past the limit; odd
    return 129 if task in AGED_TASKS else (MAXSTEPS[task] // 2 + 1) | 1


CASES = [(task, 4096, _n_steps(task), 0) for task in MAXSTEPS] + [
    ("gridworld", 16, 237, 0),     # one tile
    ("gridworld", 100, 53, 0),     # a partial tile (rows 100..111 of the last one stand for no env)
    ("gridworld", 4096, 37, 0),    # an odd n_steps below the step limit (no timeout yet: exempt from the truncated-row condition)
    ("gridworld", 100, 237, 0),    # timeouts inside a rollout: the bootstrap pass inside the step loop, several times per env
    ("gridworld", 4096, 53, 1),    # deterministic actions
]


@pytest.mark.parametrize("task,n_envs,n_steps,det", CASES)
def test_eight_wave_rollout_equals_the_four_wave_rollout_bit_for_bit(tmp_path, task, n_envs, n_steps, det):
    new = _dump(tmp_path, "default", task, n_envs, n_steps, det)
    old = _dump(tmp_path, "roll4", task, n_envs, n_steps, det, TMA_ROLL4="1")
    # the two runs took different kernels
    assert int(_load(old, "waves")) == 4
    assert int(_load(new, "waves")) == (4 if task in FOUR_WAVE_TASKS else 8)
    # the four-wave run alone exercises both ways an episode ends
    n_term = sum(int(np.count_nonzero(_load(old, f"r{r}_terminated"))) for r in range(2))
    n_trunc = sum(int(np.count_nonzero(_load(old, f"r{r}_truncated"))) for r in range(2))
    print(f"{task} N={n_envs} T={n_steps} det={det}: terminated rows {n_term}, truncated rows {n_trunc}, episodes {len(_load(old, 'episode_returns'))}")
    assert n_term > 0
    if 2 * n_steps > MAXSTEPS[task] or task in AGED_TASKS:
        assert n_trunc > 0
    for r in range(2):
        for key in PLANES:
            a, b = _load(new, f"r{r}_{key}"), _load(old, f"r{r}_{key}")
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.array_equal(a, b), (r, key, int(np.count_nonzero(np.asarray(a) != np.asarray(b))))
        for key in ("values", "log_probs", "rewards", "advantages", "returns", "last_values", "obs"):
            assert np.isfinite(_load(old, f"r{r}_{key}")).all(), (r, key)
    assert float(np.abs(_load(old, "r1_values")).max()) > 0 and float(np.abs(_load(old, "r1_log_probs")).max()) > 0
    for key in AFTER:
        a, b = _load(new, key), _load(old, key)
        assert a.shape == b.shape and np.array_equal(a, b), key
    # Monitor aggregate (see the module docstring)
    sa, sb = np.asarray(_load(new, "monitor_sums")), np.asarray(_load(old, "monitor_sums"))
    rets = np.asarray(_load(old, "episode_returns"))
    assert np.array_equal(sa[1:], sb[1:]) and int(sb[2]) == len(rets) == n_term + n_trunc
    if n_envs <= 16:
        assert np.array_equal(sa, sb)
    else:
        assert abs(sa[0] - sb[0]) <= len(rets) * 2.0 ** -53 * float(np.abs(rets).sum()), (sa[0], sb[0])
