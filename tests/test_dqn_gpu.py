"""csrc/tma_dqn.hip and three_mlagents_amd/dqn.py on the GPU (include/tma.h ABI 225).

  * tma_dqn_act: Q against the float64 restatement (tests/_dqn_ref.py) at the project's V_TOL; actions bit-equal to the epsilon-greedy
    restatement on the kernel's OWN q_out, so that no tie between precisions decides the test; q_out = NULL; canaries behind both outputs.
  * tma_dqn_td_grad: against float64 autograd at the project's gradient bound, max|err| <= 2e-5 max(max|ref|, 1) + 1e-6
    (tests/test_policy_vjp_gpu.py), on batches whose properties are asserted first from the reference; the loss statistic, exact zeros on vf.*,
    a canary, equal bits on equal inputs, the Q of tma_dqn_act bit for bit, one n above the grid cap.
  * tma_dqn_target_update: tau = 1 a copy; tau < 1 BIT-EQUAL to float32 torch arithmetic.
  * six optimizer steps against the same loop in float64 torch, the bound ten times the float32 - float64 gap of the torch runs.
  * tma_dqn_iterations_local against the same sequence issued one C-ABI call at a time: every buffer and counter bit-equal.
  * the DQN class: learn, counters, schedule, log keys, predict, evaluate_policy, save / load and continued training.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _dqn_ref as ref
from three_mlagents_amd import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
V_TOL = dict(rtol=1e-5, atol=1e-5)  # tests/test_policy_vjp_gpu.py
SHAPES = [(4, 128, 5), (21, 128, 3), (21, 64, 16), (7, 256, 2)]  # (D, H, A)
TANH_SHAPE = (6, 64, 4)
GRID_CAP_ROWS = 64 * 16  # csrc/tma_dqn.hip DQN_GRID_CAP workgroups of one 16-row tile each


def _grad_bound(ref_flat):
    return 2e-5 * max(float(ref_flat.abs().max()), 1.0) + 1e-6


def _policy(D, H, A, seed, act="relu"):
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    pol = HipActorCriticPolicy(D, A, False, H, DEV, seed=seed, activation=act, ortho_init=False)
    return pol, pol.state_dict()


@functools.lru_cache(maxsize=None)
def _nets(D, H, A, act):
    """(online policy, its SB3-named weights, target policy, its weights): different seeds, so the target differs from the online net"""
    return _policy(D, H, A, 5, act) + _policy(D, H, A, 9, act)


def _flat64(pol, named):
    flat = torch.zeros(pol.n_trainable, dtype=torch.float64)
    for key, off, shape in pol._segments():
        gk = named[key].double().reshape(shape)
        gk = gk.t().contiguous() if len(shape) == 2 else gk
        flat[off:off + gk.numel()] = gk.reshape(-1)
    return flat


def _obs(sd, D, n, seed, act):
    return ref.clear_obs(sd, D, n, seed) if act == "relu" else torch.randn(n, D, generator=torch.Generator().manual_seed(seed))


def _run_act(pol, obs_d, eps, seed, step, offset, want_q=True):
    n, A = obs_d.shape[0], pol.act_dim
    actions = torch.full((n + 64,), -7, dtype=torch.int32, device=DEV)
    q = torch.full((n * A + 64,), 12345.0, dtype=torch.float32, device=DEV) if want_q else None
    _lib.check(_lib.lib().tma_dqn_act(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs_d), n, eps, seed, step, offset, _lib.ptr(actions),
                                      _lib.ptr(q), _lib.stream_ptr(DEV)))
    assert bool((actions[n:] == -7).all()) and (q is None or bool((q[n * A:] == 12345.0).all()))  # canaries
    return actions[:n].cpu().numpy(), (q[:n * A].reshape(n, A).cpu() if want_q else None)


ACT_CASES = [(s, n, "relu") for s in SHAPES for n in (1, 16, 17, 67)] + [(TANH_SHAPE, 35, "tanh")]


@pytest.mark.parametrize("shape,n,act", ACT_CASES)
def test_act_q_matches_float64_and_actions_follow_the_egreedy_rule(shape, n, act):
    D, H, A = shape
    pol, sd, _, _ = _nets(D, H, A, act)
    obs = _obs(sd, D, n, 100 + n, act)
    obs_d = obs.to(DEV)
    q_ref = ref.q_values(ref.to_dtype(sd, torch.float64), obs.double(), act)
    q0 = None
    for k, eps in enumerate((0.0, 0.3, 1.0)):
        seed, step, offset = 11 + k, 5 + 3 * k, 1000 * k
        a, q = _run_act(pol, obs_d, eps, seed, step, offset)
        assert torch.allclose(q.double(), q_ref, **V_TOL), float((q.double() - q_ref).abs().max())
        assert q0 is None or torch.equal(q, q0)  # the forward does not depend on the pick
        q0 = q
        want = ref.egreedy(q.numpy(), eps, seed, step, offset)
        assert np.array_equal(a, want), (eps, a, want)
        a_null, _ = _run_act(pol, obs_d, eps, seed, step, offset, want_q=False)
        assert np.array_equal(a_null, a)
    if n >= 16:
        a_rand = _run_act(pol, obs_d, 1.0, 3, 1, 0)[0]
        assert len(set(a_rand.tolist())) > 1 and a_rand.min() >= 0 and a_rand.max() < A


def _to_dev(batch):
    return {k: v.to(DEV).contiguous() for k, v in batch.items()}


def _run_td(pol, tgt, b, n, want_q=False, poison=False):
    """(grad [P] cpu, tail canary ok, stats [3], q or None) of one tma_dqn_td_grad call on the device batch b"""
    L, P, A = _lib.lib(), pol.n_trainable, pol.act_dim
    need = int(L.tma_dqn_workspace_bytes(C.byref(pol.dims), n))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    grad = torch.full((P + 64,), 777.0, dtype=torch.float32, device=DEV)
    stats = torch.full((3,), -1.0, dtype=torch.float64, device=DEV)
    q = torch.empty((n, A), dtype=torch.float32, device=DEV) if want_q else None
    if poison:
        _lib.check(L.tma_debug_poison_lds(0, _lib.stream_ptr(DEV)))
    _lib.check(L.tma_dqn_td_grad(_lib.ptr(pol.params), _lib.ptr(tgt.params), C.byref(pol.dims), _lib.ptr(b["obs"]), _lib.ptr(b["actions"]),
                                 _lib.ptr(b["next_obs"]), _lib.ptr(b["dones"]), _lib.ptr(b["rewards"]), _lib.ptr(b["discounts"]), n, _lib.ptr(grad),
                                 _lib.ptr(stats), _lib.ptr(q), _lib.ptr(ws), need, _lib.stream_ptr(DEV)))
    assert bool((grad[P:] == 777.0).all())  # canary behind grad_out
    return grad[:P].cpu(), stats.cpu(), (q.cpu() if want_q else None)


@functools.lru_cache(maxsize=None)
def _td_case(D, H, A, n, act):
    """The batch of a TD-gradient case and its float64 reference, computed once and shared"""
    pol, sd, tgt, tsd = _nets(D, H, A, act)
    obs = _obs(sd, D, n, 200 + n, act)
    next_obs = torch.randn(n, D, generator=torch.Generator().manual_seed(300 + n))
    batch = ref.make_batch(sd, tsd, obs, next_obs, A, act, seed=n)
    ref.check_batch(sd, tsd, batch, A, act)  # asserted FIRST, from the reference
    grads, loss, q_sum = ref.td_grad(sd, tsd, batch, act)
    return batch, _flat64(pol, grads), loss, q_sum


TD_CASES = [(s, n, "relu") for s in SHAPES for n in (1, 15, 16, 17, 64, 67)] + [(TANH_SHAPE, 35, "tanh"), ((4, 128, 5), GRID_CAP_ROWS + 7, "relu")]


@pytest.mark.parametrize("shape,n,act", TD_CASES)
def test_td_grad_matches_float64_autograd(shape, n, act):
    D, H, A = shape
    pol, sd, tgt, tsd = _nets(D, H, A, act)
    batch, g_ref, loss_ref, q_sum_ref = _td_case(D, H, A, n, act)
    b = _to_dev(batch)
    grad, stats, q = _run_td(pol, tgt, b, n, want_q=True, poison=True)
    err, bound = float((grad.double() - g_ref).abs().max()), _grad_bound(g_ref)
    print(f"td_grad {shape} n={n} {act}: max|err| {err:.3e} (bound {bound:.3e}, max|ref| {float(g_ref.abs().max()):.3e}); loss {stats[0] / stats[2]:.9f} ref {loss_ref:.9f}")
    assert err <= bound, (err, bound)
    # the statistics: (loss sum, sum of Q taken, rows) in float64 of float32 terms
    assert float(stats[2]) == n
    assert float(stats[0]) / n == pytest.approx(loss_ref, rel=1e-5, abs=1e-6) and float(stats[1]) == pytest.approx(q_sum_ref, rel=1e-5, abs=1e-5 * n)
    # the vf segment: exact zeros (and +0, not -0)
    vf0 = pol.offsets[6]
    assert bool((grad[vf0:] == 0).all()) and not bool(torch.signbit(grad[vf0:]).any()) and bool((grad[:vf0] != 0).any())
    # equal inputs give equal bits
    grad2, stats2, _ = _run_td(pol, tgt, b, n)
    assert torch.equal(grad, grad2) and torch.equal(stats, stats2)
    # the Q the loss used has the bits tma_dqn_act gives the same rows
    _, q_act = _run_act(pol, b["obs"], 0.0, 1, 0, 0)
    assert torch.equal(q, q_act)
    # the target net matters: changing ONLY the target changes the gradient (rows that are not done bootstrap from it)
    if n >= 3:
        grad3, _, _ = _run_td(pol, pol, b, n)
        assert not torch.equal(grad, grad3)


def test_td_grad_row_with_an_action_outside_the_head():
    """include/tma.h: such an action is only compared with column indices -- the row adds nothing to the gradient (the mean still divides by n)
    and turns the two sums of the statistics to NaN."""
    D, H, A, n = 4, 128, 5, 17
    pol, sd, tgt, tsd = _nets(D, H, A, "relu")
    batch, _, _, _ = _td_case(D, H, A, n, "relu")
    bad = {k: v.clone() for k, v in batch.items()}
    bad["actions"][3], bad["actions"][11] = A + 2, -1
    grad, stats, _ = _run_td(pol, tgt, _to_dev(bad), n)
    keep = torch.ones(n, dtype=torch.bool)
    keep[3] = keep[11] = False
    sub = {k: v[keep] for k, v in batch.items()}
    grads, _, _ = ref.td_grad(sd, tsd, sub, "relu")
    g_ref = _flat64(pol, grads) * (n - 2) / n
    assert bool(torch.isfinite(grad).all()) and float((grad.double() - g_ref).abs().max()) <= _grad_bound(g_ref)
    assert bool(torch.isnan(stats[0])) and bool(torch.isnan(stats[1])) and float(stats[2]) == n


@pytest.mark.parametrize("shape", [(4, 128, 5), (21, 64, 16)])
def test_target_update(shape):
    """tau = 1: the source's bits.  tau < 1: BIT-EQUAL to float32 torch arithmetic -- the kernel forms two rounded products and one rounded sum
    (the library is built without contraction into FMAs), and so do three separate torch operations; tau and 1 - tau reach both as the same
    float32 values.  The same call rebuilds the target's derived copies: the target policy's own head then agrees with the online one's."""
    D, H, A = shape
    pol, sd = _policy(D, H, A, 5)
    tgt, _ = _policy(D, H, A, 9)
    P, L = pol.n_trainable, _lib.lib()
    obs = torch.randn(33, D, generator=torch.Generator().manual_seed(1)).to(DEV)
    for tau in (0.5, 0.3):
        before = tgt.params[:P].clone()
        _lib.check(L.tma_dqn_target_update(_lib.ptr(pol.params), _lib.ptr(tgt.params), C.byref(pol.dims), tau, _lib.stream_ptr(DEV)))
        t32, omt32 = torch.tensor(tau, dtype=torch.float32, device=DEV), torch.tensor(1.0 - tau, dtype=torch.float32, device=DEV)
        want = t32 * pol.params[:P] + omt32 * before
        assert torch.equal(tgt.params[:P], want) and not torch.equal(tgt.params[:P], before)
        assert torch.allclose(tgt.head(obs)[0].double().cpu(), ref.q_values(ref.to_dtype(tgt.state_dict(), torch.float64), obs.double().cpu()), **V_TOL)
    _lib.check(L.tma_dqn_target_update(_lib.ptr(pol.params), _lib.ptr(tgt.params), C.byref(pol.dims), 1.0, _lib.stream_ptr(DEV)))
    assert torch.equal(tgt.params[:P], pol.params[:P])
    assert torch.equal(tgt.params, pol.params)  # derived copies included
    assert torch.equal(tgt.head(obs)[0], pol.head(obs)[0])


def test_six_optimizer_steps_land_where_float64_torch_lands():
    """sample -> tma_dqn_td_grad -> Adam (clip 10, lr 1e-3, eps 1e-8) six times, the target replaced by the online net after the third step; the
    same loop in torch at float32 and at float64 on the rows tma_replay_sample reported.  Compared: what the loop produces, the pi parameters
    after the sixth step, element by element (max |difference| over the 19 k of them).  Bound: ten times the same maximum between the float32
    and the float64 torch runs, computed here.
    Why the parameters and not a loss: a scalar's float32 - float64 gap can cancel to nothing and is then no yardstick of float32 arithmetic.
    Measured on an MI355X, the TD loss of the last batch at each run's final weights (evaluated in float64): float64 run 0.467636360, float32
    run 0.467636358, device 0.467636071 -- the torch gap, 2.8e-9, is a tenth of one float32 ulp of 0.47 (3.0e-8), while the parameters of the
    same two torch runs differ by 1.97e-7 at the most; the device's differ from the float64 run's by 1.49e-7.  The losses are printed."""
    from three_mlagents_amd.replay_buffer import ReplayBuffer

    D, H, A, R, N, B, steps, lr, clip = 21, 128, 3, 40, 2, 64, 6, 1e-3, 10.0
    pol, sd0 = _policy(D, H, A, 5)
    tgt, tsd0 = _policy(D, H, A, 9)
    g = torch.Generator().manual_seed(7)
    rb = ReplayBuffer(R * N, D, A, DEV, n_envs=N, seed=13)
    for _ in range(R):
        rb.add(torch.randn(N, D, generator=g).to(DEV), torch.randn(N, D, generator=g).to(DEV), torch.randint(0, A, (N,), generator=g, dtype=torch.int32).to(DEV),
               torch.randn(N, generator=g).to(DEV), (torch.rand(N, generator=g) < 0.2).to(torch.uint8).to(DEV), torch.zeros(N, dtype=torch.uint8, device=DEV))
    L, P = _lib.lib(), pol.n_trainable
    grad, m, v = (torch.zeros(P, dtype=torch.float32, device=DEV) for _ in range(3))
    opt_ws = torch.zeros(int(L.tma_ppo_workspace_bytes(C.byref(pol.dims))), dtype=torch.uint8, device=DEV)
    need = int(L.tma_dqn_workspace_bytes(C.byref(pol.dims), B))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    batches = []
    for k in range(steps):
        s, rows, envs = rb.sample(B, return_indices=True)
        assert torch.equal(s.observations, rb.observations[rows.long(), envs.long()]) and torch.equal(s.rewards, rb.rewards[rows.long(), envs.long()])
        batches.append(dict(obs=s.observations.cpu(), actions=s.actions.cpu(), next_obs=s.next_observations.cpu(), dones=s.dones.cpu(),
                            rewards=s.rewards.cpu(), discounts=s.discounts.cpu()))
        _lib.check(L.tma_dqn_td_grad(_lib.ptr(pol.params), _lib.ptr(tgt.params), C.byref(pol.dims), _lib.ptr(s.observations), _lib.ptr(s.actions),
                                     _lib.ptr(s.next_observations), _lib.ptr(s.dones), _lib.ptr(s.rewards), _lib.ptr(s.discounts), B, _lib.ptr(grad), None, None,
                                     _lib.ptr(ws), need, _lib.stream_ptr(DEV)))
        _lib.check(L.tma_ppo_adam_step_local(_lib.ptr(pol.params), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), C.byref(pol.dims), k + 1, lr, 0.9, 0.999, 1e-8,
                                             clip, _lib.ptr(opt_ws), _lib.stream_ptr(DEV), 0))
        if k == 2:
            _lib.check(L.tma_dqn_target_update(_lib.ptr(pol.params), _lib.ptr(tgt.params), C.byref(pol.dims), 1.0, _lib.stream_ptr(DEV)))

    def torch_run(dtype):
        w = {k: t.requires_grad_(k in ref.PI_KEYS) for k, t in ref.to_dtype(sd0, dtype).items()}
        wt = ref.to_dtype(tsd0, dtype)
        leaves = [w[k] for k in ref.PI_KEYS]
        opt = torch.optim.Adam(leaves, lr=lr, eps=1e-8)
        for k, b in enumerate(batches):
            bt = {key: (t.to(dtype) if t.is_floating_point() else t) for key, t in b.items()}
            opt.zero_grad()
            ref.td_loss(w, wt, bt).backward()
            torch.nn.utils.clip_grad_norm_(leaves, clip)
            opt.step()
            if k == 2:
                wt = {key: t.detach().clone() for key, t in w.items()}
        return {k: t.detach() for k, t in w.items()}, wt

    def final_loss(w, wt):
        b64 = {key: (t.double() if t.is_floating_point() else t) for key, t in batches[-1].items()}
        return float(ref.td_loss(ref.to_dtype(w, torch.float64), ref.to_dtype(wt, torch.float64), b64))

    (w32, wt32), (w64, wt64) = torch_run(torch.float32), torch_run(torch.float64)
    l32, l64 = final_loss(w32, wt32), final_loss(w64, wt64)
    l_dev = final_loss(pol.state_dict(), tgt.state_dict())
    l_start = final_loss(sd0, tsd0)
    gap = abs(l32 - l64)
    p_gap = max(float((w32[k].double() - w64[k]).abs().max()) for k in ref.PI_KEYS)
    p_dev = max(float((pol.state_dict()[k].double() - w64[k]).abs().max()) for k in ref.PI_KEYS)
    print(f"six steps: loss start {l_start:.9f}; final device {l_dev:.9f}, torch f32 {l32:.9f}, torch f64 {l64:.9f}; f32-f64 gap {gap:.3e}, device-f64 "
          f"{abs(l_dev - l64):.3e}; parameters: f32-f64 {p_gap:.3e}, device-f64 {p_dev:.3e}")
    assert abs(l_start - l64) > 1e-3  # the six steps moved the loss far beyond the bound
    assert not torch.equal(tgt.params[:P], pol.params[:P])  # three more steps since the copy
    for k in ref.KEYS[6:12]:  # zero gradients leave vf.* untouched, bit for bit
        assert torch.equal(pol.state_dict()[k], sd0[k])
    vf0 = pol.offsets[6]
    assert not bool(m[vf0:].any()) and not bool(v[vf0:].any())
    assert p_dev <= 10.0 * p_gap, (p_dev, p_gap)


# ---- the native loop against the same calls issued one at a time
def _loop_model(n_envs, gradient_steps, n_step):
    from three_mlagents_amd.dqn import DQN
    from three_mlagents_amd.vec_env import HipVecEnv

    env = HipVecEnv("gridworld", n_envs, seed=1)
    m = DQN("MlpPolicy", env, learning_rate=1e-3, learning_starts=16, buffer_size=48 * n_envs, batch_size=32, train_freq=4, gradient_steps=gradient_steps,
            target_update_interval=8, n_steps=n_step, exploration_fraction=0.5, seed=5, policy_kwargs=dict(net_arch=[128, 128]))
    m._total_timesteps = 100 * n_envs
    with torch.no_grad():  # a target that differs from the online net from the start
        m.q_net_target.params[: m.policy.n_trainable].mul_(1.25)
    m.q_net_target.sync()
    return m, env


@pytest.mark.parametrize("n_envs,gradient_steps,n_step", [(1, 1, 1), (3, -1, 3), (1, -1, 3), (3, 1, 1)])
def test_native_loop_equals_the_calls_issued_one_by_one(monkeypatch, n_envs, gradient_steps, n_step):
    """64 vector steps of gridworld through tma_dqn_iterations_local (one call, on a side stream, torch.Tensor.cpu disabled) and through the
    same C-ABI calls issued from Python in the order tests/_dqn_ref.py iteration_events gives.  Ring of 48 rows: it wraps."""
    L, N, ITERS = _lib.lib(), n_envs, 16
    native, env1 = _loop_model(n_envs, gradient_steps, n_step)
    manual, env2 = _loop_model(n_envs, gradient_steps, n_step)
    assert torch.equal(native.policy.params, manual.policy.params) and not torch.equal(native.policy.params, native.q_net_target.params)
    p0 = native.policy.params.clone()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with monkeypatch.context() as mp, torch.cuda.stream(side):
        def no_host_copy(self, *a, **k):
            raise AssertionError("the native loop copied a tensor to the host")

        mp.setattr(torch.Tensor, "cpu", no_host_copy)
        native._run_iterations(ITERS)
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    # the same sequence, call by call
    m, rb, b, pol, tgt, st = manual, manual.replay_buffer, manual.buf, manual.policy, manual.q_net_target, _lib.stream_ptr(DEV)
    eng = env2.engine
    rb.start(env2.reset_device())
    c = ref.new_counters()
    kinds = []
    for ev in ref.iteration_events(c, ITERS, n_envs=N, capacity=48, train_freq=4, gradient_steps=gradient_steps, learning_starts=16, target_update_interval=8,
                                   total_timesteps=100 * N, exploration_fraction=0.5, exploration_initial_eps=1.0, exploration_final_eps=0.05):
        kinds.append(ev[0])
        if ev[0] == "step":
            _, eps, rng_step, pos = ev
            _lib.check(L.tma_dqn_act(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(rb.last_obs), N, eps, 5, rng_step, eng.env_offset, _lib.ptr(b["actions"]),
                                     None, st))
            _lib.check(L.tma_env_step(eng._h, _lib.ptr(b["actions"]), _lib.ACT_I32, 0, 0, 1, _lib.ptr(b["step_obs"]), _lib.ptr(b["rewards"]), _lib.ptr(b["term"]),
                                      _lib.ptr(b["trunc"]), _lib.ptr(b["term_obs"]), None, None, st))
            _lib.check(L.tma_replay_add(C.byref(rb._view), pos, _lib.ptr(rb.last_obs), _lib.ptr(b["actions"]), _lib.ptr(b["step_obs"]), _lib.ptr(b["rewards"]),
                                        _lib.ptr(b["term"]), _lib.ptr(b["trunc"]), _lib.ptr(b["term_obs"]), st))
        elif ev[0] == "target":
            _lib.check(L.tma_dqn_target_update(_lib.ptr(pol.params), _lib.ptr(tgt.params), C.byref(pol.dims), 1.0, st))
        else:
            _, size, newest, draw, adam_step = ev
            _lib.check(L.tma_replay_sample(C.byref(rb._view), size, newest, n_step, 0.99, rb.seed, draw, 32, _lib.ptr(b["s_obs"]), _lib.ptr(b["s_actions"]),
                                           _lib.ptr(b["s_next_obs"]), _lib.ptr(b["s_dones"]), _lib.ptr(b["s_rewards"]), _lib.ptr(b["s_discounts"]), None, None, st))
            _lib.check(L.tma_dqn_td_grad(_lib.ptr(pol.params), _lib.ptr(tgt.params), C.byref(pol.dims), _lib.ptr(b["s_obs"]), _lib.ptr(b["s_actions"]),
                                         _lib.ptr(b["s_next_obs"]), _lib.ptr(b["s_dones"]), _lib.ptr(b["s_rewards"]), _lib.ptr(b["s_discounts"]), 32, _lib.ptr(m.grad),
                                         _lib.ptr(b["stats"]), None, _lib.ptr(b["td_ws"]), b["td_ws"].numel(), st))
            _lib.check(L.tma_ppo_adam_step_local(_lib.ptr(pol.params), _lib.ptr(m.grad), _lib.ptr(m.exp_avg), _lib.ptr(m.exp_avg_sq), C.byref(pol.dims), adam_step,
                                                 1e-3, 0.9, 0.999, 1e-8, 10.0, _lib.ptr(m.workspace), st, 0))
    assert kinds.count("step") == 64 and kinds.count("target") > 0 and kinds.count("train") > 0
    # counters
    nrb = native.replay_buffer
    got = dict(num_timesteps=native.num_timesteps, n_calls=native._n_calls, pos=nrb.pos, full=nrb.full, draw=nrb._draw, collect_step=nrb._collect_step,
               adam_step=native._adam_step, n_updates=native._n_updates)
    assert got == c and c["full"] and c["num_timesteps"] == 64 * N
    # every buffer, bit for bit
    pairs = [("params", native.policy.params, pol.params), ("target", native.q_net_target.params, tgt.params), ("exp_avg", native.exp_avg, m.exp_avg),
             ("exp_avg_sq", native.exp_avg_sq, m.exp_avg_sq), ("last_obs", nrb.last_obs, rb.last_obs), ("stats", native.buf["stats"], b["stats"])]
    pairs += [(name, getattr(nrb, name), getattr(rb, name)) for name in ("observations", "next_observations", "actions", "rewards", "terminated", "truncated")]
    for name, x, y in pairs:
        assert torch.equal(x, y), name
    assert not torch.equal(native.policy.params, p0) and bool(torch.isfinite(native.policy.params).all())
    if n_envs == 1:  # (this run of one env ends episodes inside the last 48 rows: terminal observations were stored)
        assert bool(nrb.terminated.any() | nrb.truncated.any())
    env1.close()
    env2.close()


# ---- the class
def _class_model(env):
    from three_mlagents_amd.dqn import DQN

    return DQN("MlpPolicy", env, learning_starts=50, buffer_size=500, target_update_interval=100, policy_kwargs=dict(net_arch=[128, 128]))


def test_the_class_learns_predicts_saves_and_goes_on(tmp_path):
    from three_mlagents_amd.dqn import DQN, linear_epsilon, plan_iterations
    from three_mlagents_amd.evaluation import evaluate_policy
    from three_mlagents_amd.vec_env import HipVecEnv

    env = HipVecEnv("gridworld", 1)
    model = _class_model(env)
    P = model.policy.n_trainable
    start = model.policy.params.clone()
    assert torch.equal(model.q_net_target.params, model.policy.params) and model.policy.activation == "relu" and model.policy.hidden == 128
    model.learn(400)
    plan = plan_iterations(0, 0, 100, 1, 4, 1, 50, 100)
    assert model.num_timesteps == 400 == plan["num_timesteps"] and model._n_calls == 400
    assert model._n_updates == plan["n_updates"] == 88 and model._adam_step == 88  # iterations 13 .. 100 train (52 > 50)
    assert model.exploration_rate == linear_epsilon(400, 400, 0.1, 1.0, 0.05) == 0.05
    params = model.policy.params
    assert bool(torch.isfinite(params).all()) and not torch.equal(params[:P], start[:P])
    vf0 = model.policy.offsets[6]
    assert torch.equal(params[vf0:P], start[vf0:P])  # the value net rides along untouched
    assert not torch.equal(model.q_net_target.params[:vf0], params[:vf0])  # copied at n_calls 400, then the last optimizer step moved the online net
    rb = model.replay_buffer
    assert (rb.pos, rb.full, rb._draw, rb._collect_step) == (400, False, 88, 400)
    for key in ("rollout/exploration_rate", "rollout/ep_rew_mean", "rollout/ep_len_mean", "train/loss", "train/n_updates", "train/learning_rate",
                "time/fps", "time/total_timesteps", "time/episodes", "time/time_elapsed"):
        assert key in model.logger_values, key
    assert np.isfinite(model.logger_values["train/loss"]) and model.logger_values["train/learning_rate"] == 1e-4
    # predict: greedy = the first maximal column of policy.head; epsilon-greedy at the current rate otherwise
    obs = torch.randn(40, 4, generator=torch.Generator().manual_seed(2))
    a, state = model.predict(obs.numpy(), deterministic=True)
    q = model.policy.head(obs.to(DEV))[0].cpu().numpy()
    assert state is None and a.dtype == np.int64 and np.array_equal(a, ref.egreedy(q, 0.0, 0, 0))
    one, _ = model.predict(obs[0].numpy(), deterministic=True)
    assert int(one) == int(a[0])
    a_eps, _ = model.predict(obs.numpy())
    assert a_eps.shape == (40,) and a_eps.min() >= 0 and a_eps.max() < 5
    eval_env = HipVecEnv("gridworld", 8, seed=77)
    mean_r, std_r = evaluate_policy(model, eval_env, 5)
    assert np.isfinite(mean_r) and np.isfinite(std_r)
    eval_env.close()
    # train() as a public method
    n0 = model._n_updates
    before = model.policy.params.clone()
    model.train(gradient_steps=2, batch_size=16)
    assert model._n_updates == n0 + 2 and not torch.equal(model.policy.params, before) and np.isfinite(model.pop_train_stats()["train/loss"])
    env.close()


def test_save_load_restores_every_bit_and_training_goes_on_equally(tmp_path):
    """Two histories from equal seeds: A learns 400 + 100 steps; B learns 400, is saved (zip + replay buffer), loaded onto its env where it
    stands, and learns the 100.  Parameters, target, moments and counters after the load equal those before it; A and B end bit-equal."""
    from three_mlagents_amd.dqn import DQN
    from three_mlagents_amd.vec_env import HipVecEnv

    env_a, env_b = HipVecEnv("gridworld", 1), HipVecEnv("gridworld", 1)
    a, b = _class_model(env_a), _class_model(env_b)
    a.learn(400)
    b.learn(400)
    assert torch.equal(a.policy.params, b.policy.params)  # the run is reproducible
    b.save(tmp_path / "dqn")
    b.save_replay_buffer(tmp_path / "replay.pt")
    loaded = DQN.load(tmp_path / "dqn", env=env_b, force_reset=False)
    loaded.load_replay_buffer(tmp_path / "replay.pt")
    for name in ("learning_rate", "buffer_size", "learning_starts", "batch_size", "tau", "gamma", "train_freq", "gradient_steps", "n_steps",
                 "target_update_interval", "exploration_fraction", "exploration_initial_eps", "exploration_final_eps", "max_grad_norm", "seed",
                 "num_timesteps", "_n_updates", "_adam_step", "_n_calls", "_total_timesteps"):
        assert getattr(loaded, name) == getattr(b, name), name
    for x, y in ((loaded.policy.params, b.policy.params), (loaded.q_net_target.params, b.q_net_target.params), (loaded.exp_avg, b.exp_avg),
                 (loaded.exp_avg_sq, b.exp_avg_sq), (loaded.replay_buffer.observations, b.replay_buffer.observations),
                 (loaded.replay_buffer.last_obs, b.replay_buffer.last_obs)):
        assert torch.equal(x, y)
    lr, br = loaded.replay_buffer, b.replay_buffer
    assert (lr.pos, lr.full, lr._draw, lr._collect_step) == (br.pos, br.full, br._draw, br._collect_step) and loaded.policy.activation == "relu"
    a.learn(100, reset_num_timesteps=False)
    loaded.learn(100, reset_num_timesteps=False)
    assert a.num_timesteps == loaded.num_timesteps == 500 and a._n_updates == loaded._n_updates == 88 + 25
    assert torch.equal(a.policy.params, loaded.policy.params) and torch.equal(a.q_net_target.params, loaded.q_net_target.params)
    assert torch.equal(a.exp_avg, loaded.exp_avg) and torch.equal(a.exp_avg_sq, loaded.exp_avg_sq)
    assert not torch.equal(a.policy.params, b.policy.params)  # (b itself stayed at 400)
    # without an env the model predicts
    bare = DQN.load(tmp_path / "dqn")
    obs = torch.randn(9, 4, generator=torch.Generator().manual_seed(4)).numpy()
    assert np.array_equal(bare.predict(obs, deterministic=True)[0], b.predict(obs, deterministic=True)[0])
    env_a.close()
    env_b.close()
