"""tma_replay_add / tma_replay_sample / tma_egreedy_actions (include/tma.h, ABI 224) and three-mlagents_amd/replay_buffer.py without a GPU:
the symbols are exported and bound, every documented refusal comes back as TMA_ERR_INVALID with its message before any HIP call (host memory
stands in for the buffers), the package exports the buffer and its sample tuple, the constructor refuses what is not built -- and the numpy
reference the GPU tests compare against (tests/_replay_ref.py) is held to hand-worked windows and to the uniformity of its draws."""
import ctypes as C
import re

import numpy as np
import pytest

import _replay_ref as ref
from _sampling_stats import chi2_counts
from three_mlagents_amd import _lib

_BUF = (C.c_float * 64)()


def _p(on=True, offset=0):
    return C.c_void_p(C.addressof(_BUF) + offset) if on else None


def _view(*, planes=(True,) * 6, R=5, N=3, D=4, A=5, cont=0):
    return _lib.Replay(*(_p(on) for on in planes), R, N, D, A, cont)


def _add(*, rb=True, pos=0, args=(True,) * 6, term_obs=True, last_offset=0, step_offset=48, **view):
    """args: last_obs_inout, actions, step_obs, rewards, term, trunc.  The offsets (bytes) place last_obs_inout and step_obs, N * D = 12 floats
    each: by default step_obs starts exactly where last_obs_inout ends, which is no overlap."""
    v = _view(**view)
    last, actions, step, rew, term, trunc = args
    return _lib.lib().tma_replay_add(C.byref(v) if rb else None, pos, _p(last, last_offset), _p(actions), _p(step, step_offset), _p(rew), _p(term),
                                     _p(trunc), _p(term_obs), None)


def _sample(*, rb=True, size=4, newest=3, n_step=1, count=8, outs=(True,) * 8, **view):
    """outs: obs, actions, next_obs, dones, rewards, discounts, rows, envs"""
    v = _view(**view)
    return _lib.lib().tma_replay_sample(C.byref(v) if rb else None, size, newest, n_step, 0.99, 1, 0, count, *(_p(on) for on in outs), None)


def _egreedy(*, q=True, out=True, n=3, A=5, eps=0.1):
    return _lib.lib().tma_egreedy_actions(_p(q), n, A, eps, 1, 0, 0, _p(out), None)


def _only(i, n):
    return tuple(k == i for k in range(n))


def _without(i, n):
    return tuple(k != i for k in range(n))


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    assert L.tma_version() >= 224
    for name, n_args in (("tma_replay_add", 10), ("tma_replay_sample", 17), ("tma_egreedy_actions", 9)):
        assert name in _lib.SIGNATURES and hasattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    assert _lib.SIGNATURES["tma_replay_add"][1][0] == C.POINTER(_lib.Replay) == _lib.SIGNATURES["tma_replay_sample"][1][0]
    assert [f[0] for f in _lib.Replay._fields_] == ["obs", "next_obs", "actions", "rewards", "terminated", "truncated", "capacity", "n_envs", "obs_dim",
                                                    "act_dim", "continuous"]


@pytest.mark.parametrize("case,call,kw,word", [
    ("add: rb NULL", _add, dict(rb=False), "null argument"),
    *((f"add: plane {k} NULL", _add, dict(planes=_without(k, 6)), "plane of the replay view is null") for k in range(6)),
    *((f"add: argument {k} NULL", _add, dict(args=_without(k, 6)), "null argument") for k in range(6)),
    ("add: pos < 0", _add, dict(pos=-1), "outside [0, 5)"),
    ("add: pos = R", _add, dict(pos=5), "outside [0, 5)"),
    ("add: last_obs_inout is step_obs", _add, dict(step_offset=0), "overlaps"),
    ("add: step_obs starts in last_obs's last float", _add, dict(step_offset=44), "overlaps"),
    ("add: last_obs starts in step_obs's last float", _add, dict(last_offset=44, step_offset=0), "overlaps"),
    ("add: capacity 0", _add, dict(R=0), "capacity >= 1"),
    ("add: n_envs 0", _add, dict(N=0), "n_envs >= 1"),
    ("add: obs_dim 0", _add, dict(D=0), "obs_dim"),
    ("sample: rb NULL", _sample, dict(rb=False), "null argument"),
    ("sample: size 0", _sample, dict(size=0, newest=0), "size 0"),
    ("sample: size > R", _sample, dict(size=6, newest=0), "size 6"),
    ("sample: newest = size", _sample, dict(size=4, newest=4), "newest 4"),
    ("sample: newest < 0", _sample, dict(newest=-1), "newest -1"),
    ("sample: count 0", _sample, dict(count=0), "count"),
    ("sample: count < 0", _sample, dict(count=-3), "count"),
    ("sample: n_step 0", _sample, dict(n_step=0), "n_step 0"),
    ("sample: n_step 65", _sample, dict(n_step=65), "n_step 65"),
    ("sample: R * N = 2^31", _sample, dict(R=1 << 15, N=1 << 16), "below 2^31"),
    ("sample: N = 2^31", _sample, dict(R=1, N=1 << 31, size=1, newest=0), "below 2^31"),
    ("sample: every output NULL", _sample, dict(outs=(False,) * 8), "every output is null"),
    ("sample: obs plane NULL, obs_out given", _sample, dict(planes=_without(0, 6)), "source plane is null"),
    ("sample: next_obs plane NULL, next_obs_out given", _sample, dict(planes=_without(1, 6)), "source plane is null"),
    ("sample: actions plane NULL, actions_out given", _sample, dict(planes=_without(2, 6)), "source plane is null"),
    ("sample: rewards plane NULL", _sample, dict(planes=_without(3, 6), outs=_only(6, 8)), "source plane is null"),
    ("sample: terminated plane NULL", _sample, dict(planes=_without(4, 6), outs=_only(6, 8)), "source plane is null"),
    ("sample: truncated plane NULL", _sample, dict(planes=_without(5, 6), outs=_only(6, 8)), "source plane is null"),
    ("egreedy: q NULL", _egreedy, dict(q=False), "null argument"),
    ("egreedy: actions_out NULL", _egreedy, dict(out=False), "null argument"),
    ("egreedy: n 0", _egreedy, dict(n=0), "n must be"),
    ("egreedy: A 1", _egreedy, dict(A=1), "A 1"),
    ("egreedy: A 17", _egreedy, dict(A=17), "A 17"),
    ("egreedy: eps < 0", _egreedy, dict(eps=-1e-9), "eps"),
    ("egreedy: eps > 1", _egreedy, dict(eps=1.0 + 1e-9), "eps"),
    ("egreedy: eps NaN", _egreedy, dict(eps=float("nan")), "eps"),
])
def test_refusals_come_back_before_any_hip_call(case, call, kw, word):
    _lib.lib().tma_policy_param_count(None, None, None)  # leaves ANOTHER message behind: the one asserted below is this call's
    assert call(**kw) == _lib.TMA_ERR_INVALID, case
    msg = _lib.last_error()
    entry = {"add": "tma_replay_add", "sample": "tma_replay_sample", "egreedy": "tma_egreedy_actions"}[case.split(":")[0]]
    assert msg.startswith(entry) and word in msg, (case, msg)
    with pytest.raises(ValueError):
        _lib.check(call(**kw))


def test_the_package_exports_the_buffer_and_its_sample_tuple():
    import three_mlagents_amd as pkg
    from three_mlagents_amd.replay_buffer import ReplayBuffer, ReplayBufferSamples

    assert ReplayBufferSamples._fields == ("observations", "actions", "next_observations", "dones", "rewards", "discounts")
    assert pkg.ReplayBuffer is ReplayBuffer and pkg.ReplayBufferSamples is ReplayBufferSamples
    assert "ReplayBuffer" in pkg.__all__ and "ReplayBufferSamples" in pkg.__all__
    for name in ("size", "reset", "start", "add_step", "add", "sample", "collect"):
        assert callable(getattr(ReplayBuffer, name)), name


@pytest.mark.parametrize("kw,word", [
    (dict(handle_timeout_termination=False), "not built"),
    (dict(optimize_memory_usage=True), "not built"),
    (dict(buffer_size=0), "at least 1"),
    (dict(obs_dim=0), "at least 1"),
    (dict(n_envs=0), "at least 1"),
    (dict(n_steps=0), "n_steps"),
    (dict(n_steps=65), "n_steps"),
    (dict(action_space=0), "at least one action"),
    (dict(action_space="five"), "action_space"),
    (dict(buffer_size=1 << 31), "below 2^31"),
])
def test_the_constructor_refuses_before_it_allocates(kw, word):
    from three_mlagents_amd.replay_buffer import ReplayBuffer

    args = dict(buffer_size=100, obs_dim=4, action_space=5, device="cuda:0")
    args.update(kw)
    with pytest.raises(ValueError, match=re.escape(word)):
        ReplayBuffer(**args)


def test_action_geometry_of_spaces_ints_and_pairs():
    from three_mlagents_amd.replay_buffer import _action_geometry
    from three_mlagents_amd.spaces import task_spaces

    assert _action_geometry(task_spaces("gridworld")[1]) == (5, False) and _action_geometry(task_spaces("ant")[1]) == (8, True)
    assert _action_geometry(3) == (3, False) and _action_geometry((8, True)) == (8, True) and _action_geometry((4, False)) == (4, False)


# ---- the reference against hand-worked windows ----------------------------------------------------------------------------------------
# one env, six rows; rewards 1, 2, 4, 8, 16, 32 so that every sum names the rows it took
_R = np.array([[1.0], [2.0], [4.0], [8.0], [16.0], [32.0]], np.float32)


def _flags(term=(), trunc=()):
    t, u = np.zeros((6, 1), np.uint8), np.zeros((6, 1), np.uint8)
    t[list(term)], u[list(trunc)] = 1, 1
    return t, u


def _w(t, newest, n, gamma, term=(), trunc=()):
    row, rew, done, disc, steps, why = ref.window(_R, *_flags(term, trunc), t, 0, newest, n, gamma)
    return row, float(rew), float(done), float(disc), steps, why


def test_reference_windows_by_hand():
    g = 0.5  # exact in binary: the sums below are exact
    assert _w(0, 5, 3, g) == (2, 1 + 0.5 * 2 + 0.25 * 4, 0.0, 0.125, 3, "n")                       # the full window
    assert _w(0, 5, 3, g, term=[1]) == (1, 1 + 0.5 * 2, 1.0, 0.25, 2, "done")                     # cut by a done
    assert _w(0, 5, 3, g, trunc=[1]) == (1, 1 + 0.5 * 2, 0.0, 0.25, 2, "timeout")                 # cut by a time-out: not a done
    assert _w(0, 5, 3, g, term=[0]) == (0, 1.0, 1.0, 0.5, 1, "done")                              # a done on the first step
    assert _w(3, 4, 3, g) == (4, 8 + 0.5 * 16, 0.0, 0.25, 2, "head")                              # cut by the write head
    assert _w(4, 4, 5, g) == (4, 16.0, 0.0, 0.5, 1, "head")                                       # the newest row alone
    assert _w(4, 1, 4, g) == (1, 16 + 0.5 * 32 + 0.25 * 1 + 0.125 * 2, 0.0, 0.0625, 4, "head")    # across the ring seam, up to the head
    assert _w(5, 3, 3, g) == (1, 32 + 0.5 * 1 + 0.25 * 2, 0.0, 0.125, 3, "n")                     # across the seam, full
    assert _w(1, 5, 4, 1.0) == (4, 2.0 + 4 + 8 + 16, 0.0, 1.0, 4, "n")                            # gamma = 1
    assert _w(2, 5, 1, 0.99) == (2, 4.0, 0.0, float(np.float32(0.99)), 1, "n")                    # n_step = 1: the stored reward, gamma
    assert _w(2, 5, 1, 0.99, term=[2]) == (2, 4.0, 1.0, float(np.float32(0.99)), 1, "done")
    assert _w(2, 5, 1, 0.99, trunc=[2]) == (2, 4.0, 0.0, float(np.float32(0.99)), 1, "timeout")
    # float64 accumulation, one rounding: 0.99 and 0.99 ** 2 by repeated multiplication
    row, rew, _, disc, _, _ = ref.window(_R, *_flags(), 0, 0, 5, 3, 0.99)
    assert rew == np.float32(1.0 + 0.99 * 2.0 + (0.99 * 0.99) * 4.0) and disc == np.float32(0.99 * 0.99 * 0.99) and row == 2


def test_reference_sample_gathers_the_rows_the_windows_name():
    rng = np.random.default_rng(5)
    R, N, D = 6, 2, 3
    planes = dict(obs=rng.normal(size=(R, N, D)).astype(np.float32), next_obs=rng.normal(size=(R, N, D)).astype(np.float32),
                  actions=rng.integers(0, 5, (R, N)).astype(np.int32), rewards=rng.normal(size=(R, N)).astype(np.float32),
                  terminated=(rng.random((R, N)) < 0.2).astype(np.uint8), truncated=(rng.random((R, N)) < 0.2).astype(np.uint8))
    out = ref.sample(planes, R, 3, 3, 0.9, 7, 2, 50)
    t, i = ref.draw_indices(7, 2, 50, R, N)
    assert np.array_equal(out["rows"], t) and np.array_equal(out["envs"], i) and t.min() >= 0 and t.max() < R and i.max() < N
    for b in range(50):
        row, rew, done, disc, _, why = ref.window(planes["rewards"], planes["terminated"], planes["truncated"], t[b], i[b], 3, 3, 0.9)
        assert np.array_equal(out["obs"][b], planes["obs"][t[b], i[b]]) and out["actions"][b] == planes["actions"][t[b], i[b]]
        assert np.array_equal(out["next_obs"][b], planes["next_obs"][row, i[b]])
        assert (out["rewards"][b], out["dones"][b], out["discounts"][b], out["why"][b]) == (rew, done, disc, why)


# ---- uniformity of the draws: fixed seeds and counters, a deterministic run -- a fixed condition, not a flaky one -------------------------
@pytest.mark.parametrize("seed,draw", [(0, 0), (1, 5), (12345, 77)])
def test_reference_draw_is_uniform_over_rows_and_envs(seed, draw):
    size, N, n = 7, 3, 42000
    t, i = ref.draw_indices(seed, draw, n, size, N)
    assert chi2_counts(t.astype(np.int64) * N + i, np.full(size * N, 1.0 / (size * N))) > 0.01


@pytest.mark.parametrize("seed,step,A", [(0, 0, 5), (1, 5, 2), (12345, 77, 16)])
def test_reference_egreedy_random_branch_is_uniform(seed, step, A):
    n = 42000
    q = np.zeros((n, A), np.float32)
    q[:, 0] = 1.0  # the greedy action would be 0 everywhere
    assert chi2_counts(ref.egreedy(q, 1.0, seed, step), np.full(A, 1.0 / A)) > 0.01
    assert (ref.egreedy(q, 0.0, seed, step) == 0).all()
    share = float((ref.egreedy(q, 0.3, seed, step) != 0).mean())  # random with probability 0.3, then not column 0 with (A - 1) / A
    assert abs(share - 0.3 * (A - 1) / A) < 0.01


def test_reference_egreedy_ties_and_nans():
    nan = np.nan
    q = np.array([[1, 3, 3, 2], [nan, 1, 2, 2], [nan, nan, nan, nan], [5, nan, 5, 1], [-np.inf, -np.inf, nan, -np.inf], [0.0, -0.0, 0.0, -1]], np.float32)
    assert ref.egreedy(q, 0.0, 1, 0).tolist() == [1, 2, 0, 0, 0, 0]
