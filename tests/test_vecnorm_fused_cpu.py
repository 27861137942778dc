"""The fused VecNormalize rollout chunks without a GPU (include/tma.h, ABI 219): the two new symbols, the table of tma_rollout_norm_plan -- a pure
host function: which shapes tma_rollout_collect_norm runs inside the 8-env-tile f32 chunk kernels -- and the driver's refusals, which still come
back before any HIP call."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PER_STEP, FUSED_DISC, FUSED_CONT = 0, 1, 2


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


def _plan(task, n, training, hidden=256, mfma_dtype=0, **over):
    lib = _lib()
    t = _tasks()[task]
    dims = lib.PolicyDims(over.get("obs", t["obs"]), hidden, over.get("act", t["act"]), over.get("cont", t["cont"]), mfma_dtype, 0)
    return lib.lib().tma_rollout_norm_plan(t["id"], C.byref(dims), n, int(training))


def test_library_exports_the_new_symbols():
    lib = _lib()
    L = lib.lib()
    header = open(os.path.join(ROOT, "include", "tma.h")).read()
    for name in ("tma_rollout_norm_plan", "tma_debug_last_rollout_norm_path"):
        assert hasattr(L, name) and name in lib.SIGNATURES and f"{name}(" in header, name
    assert L.tma_version() >= 219
    assert (lib.ROLLOUT_NORM_PER_STEP, lib.ROLLOUT_NORM_FUSED_DISC_F32, lib.ROLLOUT_NORM_FUSED_CONT_F32) == (PER_STEP, FUSED_DISC, FUSED_CONT)
    assert "TMA_ROLLOUT_NORM_PER_STEP = 0, TMA_ROLLOUT_NORM_FUSED_DISC_F32 = 1, TMA_ROLLOUT_NORM_FUSED_CONT_F32 = 2" in header
    assert "The fused chunk kernels are not used" not in header
    assert L.tma_debug_last_rollout_norm_path() == PER_STEP  # nothing was launched on this thread


def test_every_task_is_in_the_table():
    tasks = _tasks()
    assert {"ant", "crawler"} <= {k for k, t in tasks.items() if t["cont"]}
    assert {"basic", "gridworld", "ball3d", "push", "walljump", "bicycle", "brickbreak", "glider"} <= {k for k, t in tasks.items() if not t["cont"]}


def test_plan_table_discrete_tasks():
    for name, t in _tasks().items():
        if t["cont"]:
            continue
        for n in (1, 5, 8):
            assert _plan(name, n, True) == FUSED_DISC, (name, n)
        for n in (9, 16):
            assert _plan(name, n, True) == PER_STEP, (name, n)
        for n in (64, 2048):
            assert _plan(name, n, False) == FUSED_DISC, (name, n)
        assert _plan(name, 2049, False) == PER_STEP, name


def test_plan_table_box_tasks():
    for name in ("ant", "crawler"):
        for n in (1, 3, 8):
            assert _plan(name, n, True) == FUSED_CONT, (name, n)
        for n in (9, 16, 4096):
            assert _plan(name, n, True) == PER_STEP, (name, n)
        for n in (1, 24, 2049, 4096):
            assert _plan(name, n, False) == FUSED_CONT, (name, n)
        assert _plan(name, 4097, False) == PER_STEP, name


@pytest.mark.parametrize("training", [True, False])
def test_plan_is_per_step_off_the_256_wide_f32_shape(training):
    for name in ("ball3d", "basic", "brickbreak", "ant"):
        for hidden in (64, 128):
            assert _plan(name, 8, training, hidden=hidden) == PER_STEP, (name, hidden)
    for name in ("ball3d", "gridworld", "ant", "crawler"):
        assert _plan(name, 8, training, mfma_dtype=1) == PER_STEP, name  # bf16 operands
    t = _tasks()
    assert _plan("ball3d", 8, training, obs=t["ball3d"]["obs"] + 1) == PER_STEP
    assert _plan("ball3d", 8, training, act=t["ball3d"]["act"] - 1) == PER_STEP
    assert _plan("ant", 8, training, obs=t["ant"]["obs"] - 1) == PER_STEP
    assert _plan("ant", 8, training, act=t["ant"]["act"] + 1) == PER_STEP
    assert _plan("ant", 8, training, cont=0, act=8) == PER_STEP  # a Discrete policy on a Box task
    assert _plan("crawler", 8, training, cont=0, act=16) == PER_STEP
    assert _plan("ball3d", 8, training, cont=1) == PER_STEP  # ... and a Box policy on a Discrete task


def test_plan_refuses_bad_arguments_with_a_negative_status():
    lib = _lib()
    L = lib.lib()
    dims = lib.PolicyDims(6, 256, 5, 0, 0, 0)
    assert L.tma_rollout_norm_plan(2, None, 8, 1) == -lib.TMA_ERR_INVALID and lib.last_error()
    assert L.tma_rollout_norm_plan(99, C.byref(dims), 8, 1) == -lib.TMA_ERR_UNKNOWN_TASK and lib.last_error()
    assert L.tma_rollout_norm_plan(-1, C.byref(dims), 8, 1) == -lib.TMA_ERR_UNKNOWN_TASK
    assert L.tma_rollout_norm_plan(2, C.byref(dims), 0, 1) == -lib.TMA_ERR_INVALID
    bad = lib.PolicyDims(6, 100, 5, 0, 0, 0)  # hidden is no multiple of 64
    assert L.tma_rollout_norm_plan(2, C.byref(bad), 8, 1) == -lib.TMA_ERR_INVALID


def _refused(status):
    lib = _lib()
    assert status == lib.TMA_ERR_INVALID, status
    assert lib.last_error(), "a refusal carries a message"


def test_driver_refusals_come_back_before_any_hip_call():
    """The calls of tests/test_vecnorm_cpu.py, on the shape the plan now fuses as well: NULL or mismatched handles are answered on a machine
    without a GPU, and the fake env handle is never dereferenced."""
    lib = _lib()
    L = lib.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for dims in (lib.PolicyDims(6, 64, 5, 0, 0, 0), lib.PolicyDims(6, 256, 5, 0, 0, 0)):
        rb = lib.RolloutBuffers(p, p, p, p, p, p, p, p, p, 8, 1)
        _refused(L.tma_rollout_collect_norm(None, None, p, C.byref(dims), C.byref(rb), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
        h = C.c_void_p()
        assert L.tma_vecnorm_create(6, 8, 1, 1, 10.0, 10.0, 0.99, 1e-8, 0, C.byref(h)) == lib.TMA_OK
        try:
            fake_env = p  # never dereferenced: the checks below fail first
            _refused(L.tma_rollout_collect_norm(None, h, p, C.byref(dims), C.byref(rb), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
            _refused(L.tma_rollout_collect_norm(fake_env, h, None, C.byref(dims), C.byref(rb), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
            _refused(L.tma_rollout_collect_norm(fake_env, h, p, None, C.byref(rb), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
            rb9 = lib.RolloutBuffers(p, p, p, p, p, p, p, p, p, 9, 1)  # buffers whose N differs from the handle's
            _refused(L.tma_rollout_collect_norm(fake_env, h, p, C.byref(dims), C.byref(rb9), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
            rb_null = lib.RolloutBuffers(p, None, p, p, p, p, p, p, p, 8, 1)
            _refused(L.tma_rollout_collect_norm(fake_env, h, p, C.byref(dims), C.byref(rb_null), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
            dims7 = lib.PolicyDims(7, dims.hidden, 5, 0, 0, 0)  # an observation width that is not the handle's
            _refused(L.tma_rollout_collect_norm(fake_env, h, p, C.byref(dims7), C.byref(rb), 0, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
            _refused(L.tma_rollout_collect_norm(fake_env, h, p, C.byref(dims), C.byref(rb), 2, 1, 1, 0, 0, 0, 0.99, 1, 0, 1, None))  # bad step range
            _refused(L.tma_rollout_collect_norm(fake_env, h, p, C.byref(dims), C.byref(rb), 0, 2, 1, 0, 0, 0, 0.99, 1, 0, 1, None))
        finally:
            assert L.tma_vecnorm_destroy(h) == lib.TMA_OK
    assert L.tma_debug_last_rollout_norm_path() == PER_STEP
