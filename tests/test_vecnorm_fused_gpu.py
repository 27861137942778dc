"""The VecNormalize step inside the 8-env-tile f32 fused rollout chunks (csrc/tma_rollout.hip, the NORM forms; include/tma.h ABI 219) against
the per-step composition it replaces, bit for bit.

Each case runs tests/_vecnorm_fused_dump.py twice in fresh processes -- plain, and with TMA_NO_NORM_FUSED=1 (the switch is read once) -- and
demands that the plain run reports the fused plan value, the other one PER_STEP, and that every array either run left is the same bytes:
the rollout buffers (obs in all T + 1 slots, actions, log_probs, values, rewards after the bootstrap, flags, last_values), the observation
and return statistics, returns[N], the raw copies of the last step, after the first rollout and again after a second one on the same model
(statistics and env state handed from chunk to chunk and from call to call).  There is no tolerance anywhere: both arms run the same device
functions (csrc/tma_vecnorm.h) in the same order.  terminal_obs is defined at truncated rows only, and which slot a step's row lands in
depends on where an arm's chunks begin: the rows are compared directly where both arms open the same windows (case B, see _terminal_rows);
in every case they are compared through the rewards, to which the bootstrap adds gamma * V(normalised terminal observation).

An untrained policy ends no Ball3D or Glider episode within a few dozen steps (checked with the per-step arm on seeds 1 .. 7), so cases A and
C age some envs to their step limit behind the first reset (the helper's `age`): their episode ends are time limits, with resets from the ring.

Shapes: the smallest at which the kernels can go wrong (the table of CASES says what each one catches); all 256 x 256 f32."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PER_STEP, FUSED_DISC, FUSED_CONT = 0, 1, 2
FAMILY_PER_STEP, FAMILY_F32_DISC, FAMILY_F32_BOX = 0, 5, 6  # include/tma.h TMA_ROLLOUT_FAMILY_*
KEYS = ("obs", "actions", "log_probs", "values", "rewards", "terminated", "truncated", "last_values", "stats", "vn_returns", "original_obs", "original_reward")

# name -> (configuration, plan value of the plain run).  Seed 3 was checked once with the per-step arm: B truncates (4 rows), E terminates (5).
CASES = {
    "A": (dict(task="ball3d", n_envs=8, n_steps=24, seed=3, age=200, age_word=6), FUSED_DISC),  # full tile, MT-ring resets; ring_depth 16: chunks split at refills
    "B": (dict(task="basic", n_envs=8, n_steps=60, seed=3, slots=4), FUSED_DISC),  # truncations at 50 steps; 4 slots: many chunks per rollout
    "C": (dict(task="glider", n_envs=5, n_steps=12, seed=3, age=4000, age_word=13), FUSED_DISC),  # partial tile: pow2ceil(5) = 8, three absent rows in the shuffle tree
    "D": (dict(task="gridworld", n_envs=1, n_steps=12, seed=3), FUSED_DISC),    # one row: batch variance exactly 0, R = 1
    "E": (dict(task="brickbreak", n_envs=8, n_steps=12, seed=3), FUSED_DISC),   # D = 45: the column loop of the moments takes two rounds
    "F": (dict(task="ant", n_envs=8, n_steps=8, seed=3), FUSED_CONT),           # Box kernel, D = 105
    "G": (dict(task="ant", n_envs=3, n_steps=8, seed=3), FUSED_CONT),           # Box kernel on a partial tile
    "H-no-obs": (dict(task="basic", n_envs=8, n_steps=20, seed=3, norm_obs=0), FUSED_DISC),     # the return statistics still update
    "H-no-rew": (dict(task="basic", n_envs=8, n_steps=20, seed=3, norm_reward=0), FUSED_DISC),
    "I": (dict(task="ball3d", n_envs=64, n_steps=12, seed=3, frozen=1), FUSED_DISC),  # frozen, deterministic: eight workgroups
    "J": (dict(task="ant", n_envs=24, n_steps=8, seed=3, frozen=1), FUSED_CONT),      # frozen, Box kernel: three workgroups
}

_DUMPS = {}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """dump(name, fused, tag='', **extra): the directory one run of the helper wrote; each (configuration, arm, tag) runs once per module."""
    root = tmp_path_factory.mktemp("vecnorm_fused")

    def run(name, fused, tag="", **extra):
        key = (name, fused, tag)
        if key not in _DUMPS:
            cfg = {**CASES[name][0], **extra}
            out = str(root / f"{name}_{'fused' if fused else 'stepped'}{tag}")
            e = {k: v for k, v in os.environ.items() if k not in ("TMA_NO_NORM_FUSED", "TMA_NO_WIDE_FUSED", "TMA_WIDE_F32_ROWS", "TMA_NO_CONT_F32_FUSED")}
            if not fused:
                e["TMA_NO_NORM_FUSED"] = "1"
            subprocess.run([sys.executable, os.path.join(HERE, "_vecnorm_fused_dump.py"), json.dumps(cfg), out], check=True, env=e, timeout=600)
            _DUMPS[key] = out
        return _DUMPS[key]

    return run


def _load(d, key):
    return np.load(os.path.join(d, key + ".npy"))


def _terminal_rows(d, r):
    """The chunk's terminal-observation slots where they are defined: rows of truncated envs.  Both arms open a window of `slots` steps at
    every multiple of `slots` where no reset-ring refill splits a chunk (Basic draws its resets inline); step t then owns slot t % slots, and
    what is left at the end is, per (slot, env), the row of the LAST truncated step of that slot."""
    trunc, tobs, slots = _load(d, f"r{r}_truncated"), _load(d, f"r{r}_terminal_obs"), int(_load(d, "slots"))
    rows = {}
    for t, i in zip(*np.nonzero(trunc)):
        rows[(int(t) % slots, int(i))] = tobs[int(t) % slots, int(i)]
    return rows


def _assert_same_bits(a, b, what):
    for r in range(2):
        for key in KEYS:
            x, y = _load(a, f"r{r}_{key}"), _load(b, f"r{r}_{key}")
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, r, key, int(np.sum(x != y)))


@pytest.mark.parametrize("name", list(CASES))
def test_fused_chunk_equals_the_per_step_composition(name, dump):
    cfg, plan = CASES[name]
    fused, stepped = dump(name, True), dump(name, False)
    assert int(_load(fused, "path")) == plan and int(_load(stepped, "path")) == PER_STEP
    # ... and the plan the driver recorded (csrc/tma_rollout_plan.h): one of the two f32 policy-only families on 8-env tiles, against the per-step composition
    assert tuple(_load(fused, "plan")) == ({FUSED_DISC: FAMILY_F32_DISC, FUSED_CONT: FAMILY_F32_BOX}[plan], 0, 8)
    assert tuple(_load(stepped, "plan")) == (FAMILY_PER_STEP, 0, 0)
    _assert_same_bits(fused, stepped, name)
    for r in range(2):
        for key in ("obs", "log_probs", "values", "rewards", "last_values", "stats", "vn_returns"):
            assert np.isfinite(_load(fused, f"r{r}_{key}")).all(), (name, r, key)
    n, D = cfg["n_envs"], _load(fused, "r0_obs").shape[-1]
    st0, st1 = _load(stepped, "r0_stats"), _load(stepped, "r1_stats")
    if cfg.get("frozen"):  # the statistics are bit-unchanged by the calls, in either arm
        before = _load(fused, "stats_before")
        assert before.tobytes() == _load(stepped, "stats_before").tobytes()
        for d in (fused, stepped):
            assert _load(d, "r0_stats").tobytes() == before.tobytes() and _load(d, "r1_stats").tobytes() == before.tobytes(), name
        assert before[2 * D] > 1.0  # (they had moved away from the initial ones)
    else:  # every step merged n rows: the counts are sums of exact integers on top of 1e-4
        T = cfg["n_steps"]
        obs_rows = n * (1 + 2 * T) if cfg.get("norm_obs", 1) else 0
        assert abs(st1[2 * D] - (1e-4 + obs_rows)) < 1e-6 and abs(st1[2 * D + 3] - (1e-4 + 2 * n * T)) < 1e-6, name
        assert not np.array_equal(st0, st1)
    # terminal observations: defined at truncated rows only
    trunc = np.concatenate([_load(stepped, "r0_truncated"), _load(stepped, "r1_truncated")])
    done = trunc | np.concatenate([_load(stepped, "r0_terminated"), _load(stepped, "r1_terminated")])
    if name == "B":
        assert int(trunc.sum()) > 0, "case B must contain a truncation"
        for r in range(2):
            ra, rb = _terminal_rows(fused, r), _terminal_rows(stepped, r)
            assert ra.keys() == rb.keys()
            for k in ra:
                assert ra[k].tobytes() == rb[k].tobytes() and np.isfinite(ra[k]).all() and np.abs(ra[k]).max() <= 10.0, (r, k)
    if name in ("A", "C", "E"):
        assert int(done.sum()) > 0, f"case {name} must contain an episode end"
    if name in ("A", "C"):  # the aged envs ran into their step limit: the bootstrap read normalised terminal observations
        assert int(trunc.sum()) == cfg["n_envs"] // 2, name
    if name == "H-no-obs":  # observations pass through: the buffer holds the raw ones
        assert _load(fused, "r1_obs")[-1].tobytes() == _load(fused, "r1_original_obs").tobytes()
        assert np.array_equal(st1[:D], np.zeros(D)) and np.array_equal(st1[D:2 * D], np.ones(D)) and st1[2 * D + 2] != 1.0
    if name == "H-no-rew":
        assert st1[2 * D + 2] != 1.0  # the return statistics moved although rewards pass through


def test_two_runs_give_identical_bits(dump):
    _assert_same_bits(dump("A", True), dump("A", True, tag="_again"), "A twice")


@pytest.mark.parametrize("name", ["A", "F"])
def test_behind_poisoned_lds(name, dump):
    """A read of an LDS word the kernel never wrote shows as NaN (every GPU test starts behind one poisoning: tests/conftest.py; here every rollout
    of the helper's process does)."""
    poisoned = dump(name, True, tag="_poison", poison=1)
    assert int(_load(poisoned, "path")) == CASES[name][1]
    _assert_same_bits(dump(name, True), poisoned, name + " poisoned")
    for r in range(2):
        for key in ("obs", "actions", "log_probs", "values", "rewards", "last_values", "stats", "vn_returns", "original_obs", "original_reward"):
            assert np.isfinite(_load(poisoned, f"r{r}_{key}").astype(np.float64)).all(), (name, r, key)


def test_update_and_learn_behind_the_fused_rollout(dump):
    d = dump("A", True, tag="_train", train=1)
    assert int(_load(d, "path")) == FUSED_DISC and bool(_load(d, "params_finite"))
    _assert_same_bits(dump("A", True), d, "A before the update")
