"""tma_rollout_gather (include/tma.h, ABI 221; csrc/tma_gather.hip) and `model.rollout_buffer` (three-mlagents_amd/rollout_buffer.py) on the
device: the kernel against numpy bit for bit on planes whose every element names its own (t, i, column); the buffer of a real rollout -- views,
the `full` flag, the order and the counter of `get`; and SB3's PPO.train loop written in torch over `get` against the native train()."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64  # floats of sentinel in front of and behind every output (256 bytes: the outputs keep their 16-byte alignment)
SENTINEL = -7.0e37
NAMES = ("obs", "actions", "values", "log_probs", "advantages", "returns")


def _planes(T, N, D, A, cont):
    """Host planes in the engine's [T][N] layout; with r = t*N + i every element is exact in f32 and names (r, column): r * D + c for the
    observations, r * A + k + 0.5 for Box actions (r for Discrete ones: the kernel copies the int, it never indexes with it), r + 0.25,
    -r - 0.5, r + 0.75 and -r for the four scalar planes (r < 2^22 keeps two fraction bits exact)."""
    r = np.arange(T * N, dtype=np.int64)
    assert T * N * max(D, A) < 1 << 23 and T * N < 1 << 22
    obs = (r[:, None] * D + np.arange(D)[None, :]).astype(np.float32).reshape(T, N, D)
    if cont:
        actions = (r[:, None] * A + np.arange(A)[None, :] + 0.5).astype(np.float32).reshape(T, N, A)
    else:
        actions = r.astype(np.int32).reshape(T, N)
    rf = r.astype(np.float64)
    scal = [(rf + 0.25), (-rf - 0.5), (rf + 0.75), (-rf)]
    values, log_probs, advantages, returns = (x.astype(np.float32).reshape(T, N) for x in scal)
    return dict(obs=obs, actions=actions, values=values, log_probs=log_probs, advantages=advantages, returns=returns)


def _env_major(x, T, N):
    """SB3's swap_and_flatten: [T][N][...] -> [N*T][...], flat index f = i*T + t"""
    return np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape((T * N,) + x.shape[2:])


def _permutation(seed, epoch, total):
    from three_mlagents_amd import _lib

    idx = np.zeros(total, dtype=np.int64)
    _lib.check(_lib.lib().tma_ppo_permutation(seed, epoch, total, idx.ctypes.data_as(C.c_void_p)))
    return idx


class _Device:
    """The planes of one case on the device, and the call."""

    def __init__(self, T, N, D, A, cont):
        from three_mlagents_amd import _lib

        self.T, self.N, self.D, self.A, self.cont = T, N, D, A, cont
        self.host = _planes(T, N, D, A, cont)
        self.flat = {k: _env_major(v, T, N) for k, v in self.host.items()}
        self.dev = {k: torch.from_numpy(v).cuda() for k, v in self.host.items()}
        self.dims = _lib.PolicyDims(D, 64, A, 1 if cont else 0, 0, -1)

    def gather(self, start, count, *, seed=77, epoch=0, indices=None, skip=(), no_values_plane=False, misalign=0):
        """One tma_rollout_gather call; returns {name: numpy output or None where skipped}.  Every output sits between two guard bands of
        sentinels, which are checked here.  misalign: floats by which the observation output is shifted off its 16-byte alignment."""
        from three_mlagents_amd import _lib

        d = self.dev
        widths = dict(obs=self.D, actions=self.A if self.cont else 1, values=1, log_probs=1, advantages=1, returns=1)
        skip = set(skip) | ({"values"} if no_values_plane else set())
        bufs, ptrs = {}, {}
        for name in NAMES:
            if name in skip:
                ptrs[name] = None
                continue
            shift = misalign if name == "obs" else 0
            n = count * widths[name]
            if name == "actions" and not self.cont:
                buf = torch.full((2 * GUARD + n,), -12345, dtype=torch.int32, device="cuda")
            else:
                buf = torch.full((2 * GUARD + n + shift,), SENTINEL, dtype=torch.float32, device="cuda")
            bufs[name] = (buf, GUARD + shift, n)
            ptrs[name] = C.c_void_p(buf.data_ptr() + 4 * (GUARD + shift))
        rv = _lib.Rollout(_lib.ptr(d["obs"]), _lib.ptr(d["actions"]), _lib.ptr(d["log_probs"]), _lib.ptr(d["advantages"]), _lib.ptr(d["returns"]), self.T, self.N, None)
        mb = _lib.Minibatch(_lib.ptr(indices) if indices is not None else None, seed, epoch, start, count, 12345, 678)  # (prepared_batch / stats_count: ignored)
        _lib.check(_lib.lib().tma_rollout_gather(C.byref(rv), None if no_values_plane else _lib.ptr(d["values"]), C.byref(self.dims), C.byref(mb),
                                                 *(ptrs[k] for k in NAMES), _lib.stream_ptr()))
        torch.cuda.synchronize()
        out = {}
        for name in NAMES:
            if name not in bufs:
                out[name] = None
                continue
            buf, lo, n = bufs[name]
            h = buf.cpu().numpy()
            guard = h[:lo].tolist() + h[lo + n:].tolist()
            assert all(g == (-12345 if h.dtype == np.int32 else np.float32(SENTINEL)) for g in guard), f"{name}: a guard band was written"
            body = h[lo:lo + n]
            out[name] = body.reshape(count, widths[name]) if name == "obs" or (name == "actions" and self.cont) else body
        return out

    def expect(self, rows):
        return {k: v[rows] for k, v in self.flat.items()}


def _same_bits(got, want, what):
    for name in NAMES:
        if got[name] is None:
            continue
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), (what, name, int((g != w).sum()))


# (T, N, D, A, Box head, batch size): a -- T*N = 15 is no power of two (the cycle-walking loop runs), a short last batch of 3; b -- rows that are
# not 16-byte aligned; c -- float action rows, rows wider than a wave (and 16-row wave blocks); the (5, 7, 16, 2) case: 16-row blocks with a
# ragged last block, the float4 walk
SMALL = [(5, 3, 4, 5, False, 4), (3, 2, 21, 3, False, 4), (2, 3, 105, 8, True, 4), (2, 2, 172, 20, True, 3), (5, 7, 16, 2, True, 35), (13, 11, 6, 5, False, 100)]


@pytest.mark.parametrize("T,N,D,A,cont,B", SMALL)
def test_every_minibatch_of_a_pass_equals_numpy_fancy_indexing(T, N, D, A, cont, B):
    case = _Device(T, N, D, A, cont)
    total = T * N
    for epoch in (0, 3):
        idx = _permutation(77, epoch, total)
        assert sorted(idx.tolist()) == list(range(total))
        for start in range(0, total, B):
            n = min(B, total - start)
            _same_bits(case.gather(start, n, epoch=epoch), case.expect(idx[start:start + n]), (epoch, start, n))
    # count = 1 at every position (start > 0, the last row), and the whole pass as one batch
    idx = _permutation(77, 0, total)
    for start in (0, 1, total // 2, total - 1):
        _same_bits(case.gather(start, 1), case.expect(idx[start:start + 1]), ("one row", start))
    _same_bits(case.gather(0, total), case.expect(idx), "whole")


def test_observation_rows_of_a_multiple_of_four_floats_on_an_unaligned_output():
    """D % 4 == 0 moves float4 only where both bases are 16-byte aligned: an output shifted by one float takes the dword walk."""
    case = _Device(5, 3, 4, 5, False)
    idx = _permutation(77, 0, 15)
    for shift in (1, 2, 3):
        _same_bits(case.gather(2, 11, misalign=shift), case.expect(idx[2:13]), shift)


@pytest.mark.parametrize("T,N,D", [(2, 262147, 3), (2, 65539, 16)])
def test_a_batch_beyond_the_grid_cap_is_walked_in_strides(T, N, D):
    """More row blocks than the capped grid has waves (GATHER_BLOCKS workgroups of four waves, 64-row blocks at D = 3, 16-row blocks at D = 16):
    one pass as one batch, compared whole."""
    from three_mlagents_amd import _lib

    total = T * N
    assert total > _lib.GATHER_BLOCKS * 4 * (16 if D >= 16 else 64) and total - _lib.GATHER_BLOCKS * 4 * (16 if D >= 16 else 64) < 64
    case = _Device(T, N, D, 5, False)
    idx = _permutation(9, 2, total)
    _same_bits(case.gather(0, total, seed=9, epoch=2), case.expect(idx), "capped grid")


def test_explicit_indices_on_device_memory():
    T, N, D, A = 5, 3, 21, 3
    case = _Device(T, N, D, A, False)
    rev = np.arange(T * N - 1, -1, -1, dtype=np.int64)
    dev_idx = torch.from_numpy(rev).cuda()
    _same_bits(case.gather(0, T * N, indices=dev_idx), case.expect(rev), "reversed")
    _same_bits(case.gather(4, 7, indices=dev_idx), case.expect(rev[4:11]), "reversed slice")


@pytest.mark.parametrize("cont", [False, True])
def test_each_output_may_be_null(cont):
    T, N, D, A = 5, 3, 21, 8 if cont else 3
    case = _Device(T, N, D, A, cont)
    idx = _permutation(77, 0, T * N)
    want = case.expect(idx[3:14])
    for name in NAMES:
        got = case.gather(3, 11, skip=(name,))
        assert got[name] is None and sum(v is not None for v in got.values()) == 5
        _same_bits(got, want, f"without {name}")
    got = case.gather(3, 11, no_values_plane=True)  # values == NULL: old_values_out is NULL as well
    assert got["values"] is None
    _same_bits(got, want, "without a values plane")
    got = case.gather(3, 11, skip=("obs", "actions", "values", "log_probs", "advantages"))
    _same_bits(got, want, "returns alone")


# ---- model.rollout_buffer on a real rollout -------------------------------------------------------------------------------------------


def _model(kind="ppo", task="gridworld", n_envs=64, n_steps=24, norm=False, seed=1, **kw):
    from three_mlagents_amd.a2c import A2C
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv
    from three_mlagents_amd.vec_normalize import VecNormalize

    env = HipVecEnv(task, n_envs, seed=seed)
    if norm:
        env = VecNormalize(env)
    if kind == "a2c":
        return A2C("MlpPolicy", env, n_steps=n_steps, seed=seed, policy_kwargs={"net_arch": [64, 64]}, **kw), env
    return PPO("MlpPolicy", env, n_steps=n_steps, batch_size=256, n_epochs=1, seed=seed, policy_kwargs={"net_arch": [64, 64]}, **kw), env


def _flat_planes(model):
    """env-major flattening of the engine's planes (device tensors), in RolloutBufferSamples order"""
    T, N, b = model.n_steps, model.n_envs, model.buf
    planes = (b["obs"][:T], b["actions"], b["values"], b["log_probs"], b["advantages"], b["returns"])
    return [p.transpose(0, 1).reshape((T * N,) + tuple(p.shape[2:])) for p in planes]


def _check_pass(model, batch_size, epoch, **kw):
    from three_mlagents_amd.rollout_buffer import RolloutBufferSamples, perm_seed

    total = model.n_steps * model.n_envs
    idx = torch.from_numpy(_permutation(perm_seed(model.seed), epoch, total)).cuda()
    flat = _flat_planes(model)
    samples = list(model.rollout_buffer.get(batch_size, **kw))
    B = total if batch_size is None else batch_size
    assert len(samples) == -(-total // B)
    for k, s in enumerate(samples):
        assert isinstance(s, RolloutBufferSamples)
        rows = idx[k * B:(k + 1) * B]
        for name, got, plane in zip(s._fields, s, flat):
            assert got.is_cuda and got.dtype == plane.dtype and tuple(got.shape) == (len(rows),) + tuple(plane.shape[1:]), (k, name, got.shape)
            assert torch.equal(got, plane[rows]), (k, name)
    return samples


@pytest.mark.parametrize("kind,task,n_envs,n_steps,norm", [("ppo", "gridworld", 64, 24, False), ("ppo", "ant", 8, 16, False), ("ppo", "ball3d", 8, 16, True),
                                                          ("a2c", "gridworld", 64, 24, False)])
def test_rollout_buffer_views_and_passes(kind, task, n_envs, n_steps, norm):
    model, env = _model(kind, task, n_envs, n_steps, norm)
    rb, b, T, N = model.rollout_buffer, model.buf, n_steps, n_envs
    D = b["obs"].shape[2]
    assert (rb.buffer_size, rb.n_envs, rb.full) == (T, N, False)
    with pytest.raises(ValueError):
        rb.get(256)
    # views, not copies, in SB3's shapes
    assert rb.observations.data_ptr() == b["obs"].data_ptr() and tuple(rb.observations.shape) == (T, N, D)
    for name, key in (("actions", "actions"), ("rewards", "rewards"), ("values", "values"), ("log_probs", "log_probs"), ("advantages", "advantages"),
                      ("returns", "returns"), ("terminated", "terminated"), ("truncated", "truncated")):
        view = getattr(rb, name)
        assert view.data_ptr() == b[key].data_ptr() and tuple(view.shape[:2]) == (T, N), name
    cont = b["actions"].dtype == torch.float32
    assert rb.actions.dtype == (torch.float32 if cont else torch.int32) and rb.actions.dim() == (3 if cont else 2)
    assert model.collect_rollouts() is True and rb.full is True
    if norm:  # the buffer holds what the native update sees: the normalised observations (clipped to VecNormalize's clip_obs = 10)
        assert float(rb.observations.abs().max()) <= 10.0 and torch.equal(rb.observations, model.buf["obs"][:T])
    total, e0 = T * N, model._epoch_counter
    B = 256 if total > 256 else 48  # (the Box / VecNormalize rollouts have 128 samples: 48 leaves a short last batch of 32)
    first = _check_pass(model, B, e0)
    assert model._epoch_counter == e0 + 1
    second = _check_pass(model, B, e0 + 1)
    assert model._epoch_counter == e0 + 2
    assert not torch.equal(first[0].observations, second[0].observations) or not torch.equal(first[0].returns, second[0].returns)
    # over one pass every sample appears exactly once: the pass is the flat planes at the permutation, slice by slice (above), the slices cover
    # [0, T*N) and the permutation is a bijection
    from three_mlagents_amd.rollout_buffer import perm_seed

    assert sorted(_permutation(perm_seed(model.seed), e0, total).tolist()) == list(range(total))
    assert sum(s.returns.shape[0] for s in first) == total
    # an explicit perm_epoch leaves the counter alone, and repeats that pass
    again = _check_pass(model, B, e0, perm_epoch=e0)
    assert model._epoch_counter == e0 + 2 and all(torch.equal(x.observations, y.observations) for x, y in zip(first, again))
    # None: one batch of everything
    (everything,) = _check_pass(model, None, e0 + 2)
    assert everything.observations.shape[0] == total and model._epoch_counter == e0 + 3
    # an abandoned pass does not advance the counter
    next(iter(rb.get(B)))
    assert model._epoch_counter == e0 + 3
    with pytest.raises(ValueError):
        rb.get(0)
    # train() still runs behind all this, on fresh permutations
    model.train()
    assert torch.isfinite(model.policy.params).all() and model._epoch_counter == e0 + 3 + (1 if kind == "ppo" else 0)
    env.close()


def test_full_is_false_after_an_interrupted_rollout():
    from three_mlagents_amd.callbacks import BaseCallback

    class Stop(BaseCallback):
        def _on_step(self) -> bool:
            return self.n_calls < 3

    model, env = _model()
    assert model.collect_rollouts() is True and model.rollout_buffer.full is True
    cb = Stop()
    cb.init_callback(model)
    assert model.collect_rollouts(cb, chunk=1) is False and model.rollout_buffer.full is False
    with pytest.raises(ValueError):
        model.rollout_buffer.get(256)
    assert model.collect_rollouts() is True and model.rollout_buffer.full is True
    env.close()


def test_a_model_that_never_calls_get_trains_to_the_same_bits():
    res = []
    for touch in (False, True):
        model, env = _model()
        for _ in range(2):
            model.collect_rollouts()
            if touch:
                assert model.rollout_buffer.observations.shape[0] == model.n_steps  # reads the attribute, launches nothing
            model.train()
        torch.cuda.synchronize()
        res.append((model.policy.params.clone(), model._epoch_counter))
        env.close()
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]


# ---- the point of the feature: SB3's PPO.train in torch over rollout_buffer.get ---------------------------------------------------------------


def test_sb3_train_loop_in_torch_over_get_equals_the_native_train():
    """Twin PPO models (same seed, GridWorld, T, N, B, H = 24, 64, 256, 64, n_epochs = 1: six optimizer steps, the schedule of
    test_ppo_gpu.py::test_persistent_epoch_kernel_equals_per_minibatch_launches) collect the same rollout.  A runs the native train(); B runs
    SB3's loop in torch over rollout_buffer.get(256): normalize_advantage with the unbiased std + 1e-8, the clipped surrogate, vf_coef 0.5, the
    model's ent_coef, clip_grad_norm_(0.5), Adam(lr 3e-4, eps 1e-5).  Bound: the project holds the native epoch to 2e-5 of the f32 torch
    restatement on this schedule (test_ppo_gpu.py, the atol=2e-5 loop); the VJP path is an f32 evaluation of the same loss; 4e-5 is the two
    bounds end to end.  Measured on an MI355X: see DESIGN.md section 15."""
    a, env_a = _model()
    b, env_b = _model()
    assert a.collect_rollouts() and b.collect_rollouts()
    for key in ("obs", "actions", "log_probs", "advantages", "returns", "values"):
        assert torch.equal(a.buf[key], b.buf[key]), key
    a.train()
    pol = b.policy
    p_init = pol.params[: pol.n_trainable].clone()
    opt = torch.optim.Adam(pol.parameters(), lr=3e-4, eps=1e-5)
    clip, kls = b.clip_range, []
    for data in b.rollout_buffer.get(256):
        values, log_prob, entropy = pol.evaluate_actions(data.observations, data.actions)
        adv = data.advantages
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(log_prob - data.old_log_prob)
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
        value_loss = torch.nn.functional.mse_loss(data.returns, values)
        loss = policy_loss + b.ent_coef * -entropy.mean() + 0.5 * value_loss
        with torch.no_grad():
            log_ratio = log_prob - data.old_log_prob
            kls.append(float(((torch.exp(log_ratio) - 1) - log_ratio).mean()))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(pol.parameters(), 0.5)
        opt.step()
    assert len(kls) == 6 and b._epoch_counter == a._epoch_counter == 1
    n = pol.n_trainable
    pa, pb = a.policy.params[:n].detach(), pol.params[:n].detach()
    worst = float((pa - pb).abs().max())
    print(f"max |params_native - params_torch_loop| = {worst:.3e}; approx_kl per minibatch = {kls}")
    assert torch.isfinite(pa).all() and float((pa - a.policy.params[:n]).abs().max()) == 0.0
    assert worst <= 4e-5, worst
    assert abs(kls[0]) <= 1e-6, kls[0]  # the first minibatch evaluates the rollout's own parameters: as the native path reports
    assert float((pb - p_init).abs().max()) > 1e-4  # (the loop moved the parameters)
    env_a.close()
    env_b.close()
