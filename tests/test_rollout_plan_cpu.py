"""Which kernel family tma_rollout_collect / tma_rollout_collect_norm run for a shape, without a GPU: the host-only query
tma_debug_plan_rollout -- the pure plan function of csrc/tma_rollout_plan.h behind both drivers -- against a table written from the
conditions of the driver as it stood before the plan existed.  tests/test_ppo_gpu.py holds the driver to the same query on
hardware (tma_debug_last_rollout_plan), so a row meant for a fused kernel cannot pass on the per-step composition."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

NONE, TRAINING, FROZEN = 0, 1, 2
PER_STEP = ("PER_STEP", 0, 0)


def _lib():
    from three_mlagents_amd import _lib

    return _lib


def _tasks():
    from three_mlagents_amd import ENGINE_TASKS

    L = _lib().lib()
    out = {}
    for name, task in ENGINE_TASKS.items():
        tid = _lib().task_id(task.kernel)
        n_act = L.tma_task_num_actions(tid)
        out[name] = dict(id=tid, obs=L.tma_task_obs_dim(tid), act=n_act if n_act > 0 else L.tma_task_act_dim(tid), cont=int(n_act == 0))
    return out


def planned(task, hidden, mfma, n, norm=NONE, is_reset=1, slots=1, activation=0, **over):
    """(status, (family name, waves, rows), (grid, block, lds)) of tma_debug_plan_rollout for a policy of the task's own widths (or `over`)"""
    lib = _lib()
    t = _tasks()[task]
    dims = lib.PolicyDims(over.get("obs", t["obs"]), hidden, over.get("act", t["act"]), over.get("cont", t["cont"]), {"f32": 0, "bf16": 1}[mfma], 0, activation)
    out = (C.c_int32 * 6)(*([-1] * 6))
    rc = lib.lib().tma_debug_plan_rollout(t["id"], C.byref(dims), n, is_reset, slots, norm, out)
    return rc, (lib.ROLLOUT_FAMILIES[out[0]] if rc == 0 else None, out[1], out[2]), tuple(out[3:])


# (task, hidden, mfma_dtype, N, norm) -> (family, waves per 16-env tile, envs per tile or group); the reason beside each row
H64_8, H64_4, H64_1 = ("H64", 8, 16), ("H64", 4, 16), ("H64", 1, 16)
TABLE = [
    # ---- every row of tests/test_ppo_gpu.py::test_native_rollout_equals_stepwise_composition, in its order
    ("gridworld", 64, "f32", 200, NONE, H64_8),  # 13 tiles < 1024: one tile per workgroup, on eight waves
    ("push", 64, "f32", 200, NONE, H64_8),
    ("ball3d", 64, "f32", 200, NONE, H64_8),
    ("walljump", 64, "f32", 200, NONE, H64_8),
    ("basic", 64, "f32", 200, NONE, PER_STEP),  # 21 observations: no LDS weight images (img_pi < 0), and Basic resets inline (no ring: no H64 kernel)
    ("gridworld", 128, "f32", 200, NONE, PER_STEP),  # 128 wide: neither the 64-wide images nor a 256-wide family
    ("gridworld", 64, "f32", 16400, NONE, H64_1),  # 1025 tiles >= 1024: four tiles a workgroup, one wave each
    ("ball3d", 256, "bf16", 200, NONE, ("BF16_DISC", 0, 16)),  # <= 4096 envs: 16 envs per block
    ("gridworld", 256, "bf16", 200, NONE, ("BF16_DISC", 0, 16)),
    ("push", 256, "bf16", 96, NONE, ("BF16_DISC", 0, 16)),
    ("basic", 256, "bf16", 40, NONE, ("BF16_DISC", 0, 16)),  # 21 observations <= 32
    ("walljump", 256, "bf16", 64, NONE, ("BF16_DISC", 0, 16)),
    ("ball3d", 256, "f32", 200, NONE, ("F32_DISC", 0, 8)),  # <= 2048 envs: tiles of eight
    ("basic", 256, "f32", 8, NONE, ("F32_DISC", 0, 8)),
    ("basic", 256, "f32", 40, NONE, ("F32_DISC", 0, 8)),
    ("basic", 256, "f32", 5, NONE, ("F32_DISC", 0, 8)),
    ("gridworld", 256, "f32", 200, NONE, ("F32_DISC", 0, 8)),
    ("gridworld", 256, "f32", 2100, NONE, ("F32_DISC", 0, 16)),  # beyond 2048 envs: tiles of 16
    ("push", 256, "f32", 72, NONE, ("F32_DISC", 0, 8)),
    ("walljump", 256, "f32", 64, NONE, ("F32_DISC", 0, 8)),
    ("bicycle", 256, "f32", 40, NONE, ("F32_DISC", 0, 8)),
    ("glider", 256, "f32", 40, NONE, ("F32_DISC", 0, 8)),
    ("crawler", 256, "bf16", 72, NONE, ("BF16_BOX_PI", 0, 16)),  # Box bf16 without TMA_CONT_TWO_NET: the policy-only chunk, <= 4096 envs: 16 per block
    ("crawler", 256, "f32", 40, NONE, ("F32_BOX", 0, 8)),  # Box f32 up to 4096 envs
    ("ant", 256, "bf16", 72, NONE, ("BF16_BOX_PI", 0, 16)),
    ("ant", 256, "f32", 40, NONE, ("F32_BOX", 0, 8)),
    ("crawler", 256, "f32", 12, NONE, ("F32_BOX", 0, 8)),
    ("bicycle", 64, "f32", 200, NONE, H64_8),
    ("glider", 64, "f32", 200, NONE, H64_4),  # Glider on four waves: its env step needs a four-wave workgroup's registers (ROLL8 = false)
    ("bicycle", 256, "bf16", 72, NONE, ("BF16_DISC", 0, 16)),
    ("glider", 256, "bf16", 72, NONE, ("BF16_DISC", 0, 16)),
    ("brickbreak", 64, "f32", 100, NONE, PER_STEP),  # 45 observations: no LDS weight images, no H64 kernel
    ("brickbreak", 256, "f32", 8, NONE, ("F32_DISC", 0, 8)),  # the BrickBreak exception: 45 observations on the 8-env tiles, up to 2048 envs
    ("brickbreak", 256, "f32", 44, NONE, ("F32_DISC", 0, 8)),
    ("brickbreak", 256, "f32", 2100, NONE, PER_STEP),  # ... and beyond them no 16-env form
    # ---- the edges of every threshold
    ("gridworld", 256, "f32", 2048, NONE, ("F32_DISC", 0, 8)),  # N <= 2048: tiles of eight
    ("gridworld", 256, "f32", 2049, NONE, ("F32_DISC", 0, 16)),
    ("brickbreak", 256, "f32", 2048, NONE, ("F32_DISC", 0, 8)),
    ("brickbreak", 256, "f32", 2049, NONE, PER_STEP),
    ("gridworld", 256, "bf16", 4096, NONE, ("BF16_DISC", 0, 16)),  # N <= 4096: 16 envs per block, else 32
    ("gridworld", 256, "bf16", 4097, NONE, ("BF16_DISC", 0, 32)),
    ("crawler", 256, "bf16", 4096, NONE, ("BF16_BOX_PI", 0, 16)),
    ("crawler", 256, "bf16", 4097, NONE, ("BF16_BOX_PI", 0, 32)),
    ("ant", 256, "f32", 4096, NONE, ("F32_BOX", 0, 8)),  # N <= 4096: the f32 Box chunk, else step by step
    ("ant", 256, "f32", 4097, NONE, PER_STEP),
    ("gridworld", 64, "f32", 16368, NONE, H64_8),  # 1023 tiles
    ("gridworld", 64, "f32", 16369, NONE, H64_1),  # 1024 tiles
    ("glider", 64, "f32", 16368, NONE, H64_4),
    ("glider", 64, "f32", 16369, NONE, H64_1),
    # ---- under VecNormalize: the two f32 policy-only families with the step inside the chunk, or the per-step composition
    ("ball3d", 256, "f32", 8, TRAINING, ("F32_DISC", 0, 8)),  # moving statistics: one tile is the whole vector
    ("ball3d", 256, "f32", 9, TRAINING, PER_STEP),
    ("ball3d", 256, "f32", 2048, FROZEN, ("F32_DISC", 0, 8)),  # frozen statistics: the 8-env tiles' own cap
    ("ball3d", 256, "f32", 2049, FROZEN, PER_STEP),  # (16-env tiles have no normalised form)
    ("brickbreak", 256, "f32", 8, TRAINING, ("F32_DISC", 0, 8)),
    ("ant", 256, "f32", 8, TRAINING, ("F32_BOX", 0, 8)),
    ("ant", 256, "f32", 9, TRAINING, PER_STEP),
    ("crawler", 256, "f32", 4096, FROZEN, ("F32_BOX", 0, 8)),
    ("crawler", 256, "f32", 4097, FROZEN, PER_STEP),
    ("gridworld", 64, "f32", 200, TRAINING, PER_STEP),  # no other family has a normalised form: H64 ...
    ("gridworld", 256, "bf16", 8, TRAINING, PER_STEP),  # ... the bf16 ones
    ("crawler", 256, "bf16", 8, FROZEN, PER_STEP),
]


def test_plan_query_gives_every_row_its_family():
    import torch

    import test_ppo_gpu

    gpu_rows = [(t, h, m, n) for t, h, n, m in test_ppo_gpu.test_native_rollout_equals_stepwise_composition.pytestmark[0].args[1]]
    head = TABLE[: len(gpu_rows)]
    assert [r[:4] for r in head] == gpu_rows and all(r[4] == NONE for r in head), "a rollout row without a table row"
    # tests/test_ppo_gpu.py FUSED_ROLLOUT_ROWS: exactly the rows this table gives a fused family
    assert {r[:4] for r in head if r[5] != PER_STEP} == {(t, h, m, n) for t, h, n, m in test_ppo_gpu.FUSED_ROLLOUT_ROWS}
    assert len(set(r[:5] for r in TABLE)) == len(TABLE)
    for task, hidden, mfma, n, norm, want in TABLE:
        rc, got, (grid, block, lds) = planned(task, hidden, mfma, n, norm)
        assert rc == 0 and got == want, (task, hidden, mfma, n, norm, got)
        assert grid >= 1 and block % 64 == 0 and 0 <= lds <= 160 * 1024, (task, hidden, mfma, n, grid, block, lds)
        if want != PER_STEP:  # one workgroup per tile or group (H64 on one wave: four tiles a workgroup of four waves)
            family, waves, rows = want
            assert grid == -(-n // (64 if waves == 1 else rows)), (task, n, grid)
            assert block == (64 * waves if waves > 1 else 256 if family in ("H64", "F32_DISC", "F32_BOX") else 512), (task, n, block)
    assert {r[5][0] for r in TABLE} | {"BF16_BOX_TWO_NET"} == set(_lib().ROLLOUT_FAMILIES)  # (the two-net Box chunk: only under its switch, below)
    assert not torch.cuda.is_initialized()


def test_shapes_no_fused_kernel_takes_are_per_step():
    t = _tasks()
    for task, hidden, mfma in (("gridworld", 64, "f32"), ("gridworld", 256, "bf16"), ("gridworld", 256, "f32"), ("crawler", 256, "bf16"), ("ant", 256, "f32")):
        assert planned(task, hidden, mfma, 200)[1] != PER_STEP
        assert planned(task, hidden, mfma, 200, is_reset=0)[1] == PER_STEP, task  # a chunk kernel starts from a reset env handle
        if mfma == "f32":  # ReLU (f32 operands only: bf16 dims with it are refused): every chunk kernel is tanh code
            assert planned(task, hidden, mfma, 200, activation=1)[1] == PER_STEP, task
        else:
            assert planned(task, hidden, mfma, 200, activation=1)[0] == _lib().TMA_ERR_INVALID
        assert planned(task, hidden, mfma, 200, obs=t[task]["obs"] + 1)[1] == PER_STEP, task  # not the task's observation width
        assert planned(task, hidden, mfma, 200, act=t[task]["act"] + 1)[1] == PER_STEP, task  # ... or action width
    assert planned("gridworld", 256, "f32", 200, cont=1)[1] == PER_STEP  # a Box policy on a Discrete task
    assert planned("ant", 256, "f32", 200, cont=0)[1] == PER_STEP  # ... and a Discrete one on a Box task
    # the side stream of the Box families needs two terminal-observation slots; the selection does not depend on them
    assert planned("ant", 256, "f32", 200, slots=1)[1:] == planned("ant", 256, "f32", 200, slots=8)[1:]


def test_norm_plan_is_a_view_of_the_plan():
    """every (task, dims, N, training) tests/test_vecnorm_fused_cpu.py probes: tma_rollout_norm_plan answers with a fused value exactly where
    tma_debug_plan_rollout gives F32_DISC or F32_BOX for the same arguments under that norm"""
    import test_vecnorm_fused_cpu as v

    t = _tasks()
    probes = [(name, n, tr, {}) for name, task in t.items() for tr in (True, False) for n in (1, 3, 5, 8, 9, 16, 24, 64, 2048, 2049, 4096, 4097)]
    for tr in (True, False):
        probes += [(name, 8, tr, dict(hidden=hidden)) for name in ("ball3d", "basic", "brickbreak", "ant") for hidden in (64, 128)]
        probes += [(name, 8, tr, dict(mfma_dtype=1)) for name in ("ball3d", "gridworld", "ant", "crawler")]
        probes += [("ball3d", 8, tr, dict(obs=t["ball3d"]["obs"] + 1)), ("ball3d", 8, tr, dict(act=t["ball3d"]["act"] - 1)), ("ball3d", 8, tr, dict(cont=1))]
        probes += [("ant", 8, tr, dict(obs=t["ant"]["obs"] - 1)), ("ant", 8, tr, dict(act=t["ant"]["act"] + 1)), ("ant", 8, tr, dict(cont=0, act=8))]
        probes += [("crawler", 8, tr, dict(cont=0, act=16))]
    view = {"F32_DISC": v.FUSED_DISC, "F32_BOX": v.FUSED_CONT, "PER_STEP": v.PER_STEP}
    fused = 0
    for name, n, tr, over in probes:
        over = dict(over)
        hidden, mfma = over.pop("hidden", 256), "bf16" if over.pop("mfma_dtype", 0) else "f32"
        rc, got, _ = planned(name, hidden, mfma, n, TRAINING if tr else FROZEN, **over)
        assert rc == 0 and view[got[0]] == v._plan(name, n, tr, hidden=hidden, mfma_dtype=int(mfma == "bf16"), **over), (name, n, tr, over, got)
        fused += got[0] != "PER_STEP"
    assert fused >= 40


def test_plan_query_refuses_what_the_real_calls_refuse():
    lib = _lib()
    L = lib.lib()
    dims = lib.PolicyDims(6, 256, 5, 0, 0, 0, 0)
    out = (C.c_int32 * 6)()
    assert L.tma_debug_plan_rollout(2, None, 8, 1, 1, 0, out) == lib.TMA_ERR_INVALID and lib.last_error()
    assert L.tma_debug_plan_rollout(2, C.byref(dims), 8, 1, 1, 0, None) == lib.TMA_ERR_INVALID and lib.last_error()
    assert L.tma_debug_plan_rollout(99, C.byref(dims), 8, 1, 1, 0, out) == lib.TMA_ERR_UNKNOWN_TASK and lib.last_error()
    assert L.tma_debug_plan_rollout(-1, C.byref(dims), 8, 1, 1, 0, out) == lib.TMA_ERR_UNKNOWN_TASK
    assert L.tma_debug_plan_rollout(2, C.byref(dims), 0, 1, 1, 0, out) == lib.TMA_ERR_INVALID
    assert L.tma_debug_plan_rollout(2, C.byref(dims), 8, 1, 1, 3, out) == lib.TMA_ERR_INVALID  # norm is none of the three
    bad = lib.PolicyDims(6, 100, 5, 0, 0, 0, 0)  # hidden is no multiple of 64
    assert L.tma_debug_plan_rollout(2, C.byref(bad), 8, 1, 1, 0, out) == lib.TMA_ERR_INVALID
    assert L.tma_debug_last_rollout_plan(None) == lib.TMA_ERR_INVALID
    out3 = (C.c_int32 * 3)(-1, -1, -1)
    assert L.tma_debug_last_rollout_plan(out3) == lib.TMA_OK and tuple(out3) == (0, 0, 0)  # nothing ran on this thread


def test_library_exports_the_plan_queries():
    import re

    lib = _lib()
    header = open(os.path.join(ROOT, "include", "tma.h")).read()
    for name in ("tma_debug_plan_rollout", "tma_debug_last_rollout_plan"):
        assert hasattr(lib.lib(), name) and name in lib.SIGNATURES and f"{name}(" in header, name
    assert lib.lib().tma_version() >= 223
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"TMA_ROLLOUT_FAMILY_([A-Z0-9_]+) = (\d+)", header)}
    assert ids == {name: i for i, name in enumerate(lib.ROLLOUT_FAMILIES)}
    assert "TMA_ROLLOUT_PLAN_NORM_NONE = 0, TMA_ROLLOUT_PLAN_NORM_TRAINING = 1, TMA_ROLLOUT_PLAN_NORM_FROZEN = 2" in header
    assert (lib.ROLLOUT_PLAN_NORM_NONE, lib.ROLLOUT_PLAN_NORM_TRAINING, lib.ROLLOUT_PLAN_NORM_FROZEN) == (NONE, TRAINING, FROZEN)


# One row per switch: what it forces.  The switches are read once per process, so each row runs in a child process with its switch set.
SWITCH_ROWS = {
    "TMA_NO_WIDE_FUSED=1": [(("gridworld", 256, "bf16", 200), PER_STEP), (("gridworld", 256, "f32", 200), PER_STEP), (("ant", 256, "f32", 40), PER_STEP),
                            (("ant", 256, "bf16", 40), PER_STEP), (("gridworld", 64, "f32", 200), H64_8)],  # every 256-wide shape step by step; H64 stays
    "TMA_NO_CONT_F32_FUSED=1": [(("ant", 256, "f32", 40), PER_STEP), (("ant", 256, "bf16", 40), ("BF16_BOX_PI", 0, 16)), (("ant", 256, "f32", 8, TRAINING), PER_STEP)],
    "TMA_CONT_TWO_NET=1": [(("crawler", 256, "bf16", 72), ("BF16_BOX_TWO_NET", 0, 32)), (("ant", 256, "bf16", 72), ("BF16_BOX_TWO_NET", 0, 32)),
                           (("ant", 256, "f32", 40), ("F32_BOX", 0, 8))],
    "TMA_CONT_SERIAL=1": [(("ant", 256, "f32", 40), ("F32_BOX", 0, 8)), (("ant", 256, "bf16", 72), ("BF16_BOX_PI", 0, 16))],  # one stream: the same kernels
    "TMA_WIDE_F32_ROWS=16": [(("gridworld", 256, "f32", 200), ("F32_DISC", 0, 16)), (("brickbreak", 256, "f32", 44), PER_STEP),  # BrickBreak has no 16-env form
                             (("gridworld", 256, "f32", 8, TRAINING), PER_STEP)],  # ... and neither has the normalised chunk
    "TMA_WIDE_F32_ROWS=8": [(("gridworld", 256, "f32", 2100), ("F32_DISC", 0, 8)), (("brickbreak", 256, "f32", 2100), PER_STEP),  # (its cap is not the switch's to lift)
                            (("brickbreak", 256, "f32", 44), ("F32_DISC", 0, 8))],
    "TMA_WIDE_ROWS=32": [(("gridworld", 256, "bf16", 200), ("BF16_DISC", 0, 32))],
    "TMA_WIDE_ROWS=16": [(("gridworld", 256, "bf16", 4097), ("BF16_DISC", 0, 16))],
    "TMA_CONT_ROWS=32": [(("crawler", 256, "bf16", 72), ("BF16_BOX_PI", 0, 32))],
    "TMA_CONT_ROWS=16": [(("crawler", 256, "bf16", 4097), ("BF16_BOX_PI", 0, 16))],
    "TMA_ROLL2=1": [(("gridworld", 64, "f32", 200), ("H64", 2, 16)), (("glider", 64, "f32", 200), ("H64", 2, 16)), (("gridworld", 64, "f32", 16400), H64_1)],
    "TMA_ROLL4=1": [(("gridworld", 64, "f32", 200), H64_4), (("gridworld", 64, "f32", 16400), H64_1)],
    "TMA_NO_NORM_FUSED=1": [(("ball3d", 256, "f32", 8, TRAINING), PER_STEP), (("ant", 256, "f32", 8, FROZEN), PER_STEP), (("ball3d", 256, "f32", 8), ("F32_DISC", 0, 8))],
}


def check_switch_rows(switch):
    import torch

    for args, want in SWITCH_ROWS[switch]:
        rc, got, (grid, block, lds) = planned(*args)
        assert rc == 0 and got == want, (switch, args, got)
        assert grid >= 1 and block % 64 == 0 and 0 <= lds <= 160 * 1024, (switch, args, grid, block, lds)
    # tma_rollout_norm_plan reads no switch: its answers are those of a process without any
    import test_vecnorm_fused_cpu as v

    assert v._plan("ball3d", 8, True) == v.FUSED_DISC and v._plan("ant", 8, False) == v.FUSED_CONT
    assert not torch.cuda.is_initialized()


@pytest.mark.parametrize("switch", sorted(SWITCH_ROWS))
def test_each_switch_forces_its_family_or_rows_in_a_child_process(switch):
    import subprocess

    rollout_switches = ("TMA_NO_WIDE_FUSED", "TMA_NO_CONT_F32_FUSED", "TMA_CONT_TWO_NET", "TMA_CONT_SERIAL", "TMA_WIDE_F32_ROWS", "TMA_WIDE_ROWS", "TMA_CONT_ROWS",
                        "TMA_ROLL2", "TMA_ROLL4", "TMA_NO_NORM_FUSED")
    assert {s.split("=")[0] for s in SWITCH_ROWS} == set(rollout_switches)
    name, value = switch.split("=")
    env = {k: v for k, v in os.environ.items() if k not in rollout_switches}
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import test_rollout_plan_cpu as m; m.check_switch_rows({switch!r})"
    r = subprocess.run([sys.executable, "-c", code], env=dict(env, **{name: value}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
