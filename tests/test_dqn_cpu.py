"""DQN without a GPU (include/tma.h ABI 225, three_mlagents_amd/dqn.py): the symbols and their refusals, the constructor, the exploration
schedule, the TD-gradient reference against a hand-worked case, and the loop's counters against a plain-loop restatement."""
import ctypes as C
import inspect

import pytest
import torch

import _dqn_ref as ref
from three_mlagents_amd import _lib

NEW_SYMBOLS = ["tma_dqn_act", "tma_dqn_workspace_bytes", "tma_dqn_td_grad", "tma_dqn_target_update", "tma_dqn_epsilon", "tma_dqn_iterations_local"]


def _dims(D=4, H=128, A=5, cont=0, mfma=0, act=1):
    return _lib.PolicyDims(D, H, A, cont, mfma, -1, act)


def _host(n=64):
    return (C.c_float * n)()


def _refused(rc, *words):
    assert rc == _lib.TMA_ERR_INVALID, rc
    msg = _lib.last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    assert L.tma_version() >= 225
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes is not None


# (dims, words of the message): what every entry point refuses on its shape argument
BAD_DIMS = [(_dims(H=192), ("hidden 192",)), (_dims(H=100), ("hidden",)), (_dims(A=17), ("[2, 16]", "17")), (_dims(A=1), ("[2, 16]",)),
            (_dims(H=128, mfma=1, act=0), ("mfma_dtype 1",)), (_dims(cont=1), ("Box",)), (_dims(D=129), ("obs_dim 129", "128"))]


@pytest.mark.parametrize("d,words", BAD_DIMS)
def test_every_entry_refuses_unsupported_shapes_before_any_hip_call(d, words):
    L, p, q, o, a = _lib.lib(), _host(), _host(), _host(), (C.c_int32 * 64)()
    _refused(L.tma_dqn_act(p, C.byref(d), o, 4, 0.1, 1, 0, 0, a, None, None), *words)
    _refused(L.tma_dqn_td_grad(p, q, C.byref(d), o, a, o, o, o, o, 4, p, None, None, p, 1 << 20, None), *words)
    _refused(L.tma_dqn_target_update(p, q, C.byref(d), 1.0, None), *words)
    assert L.tma_dqn_workspace_bytes(C.byref(d), 4) == 0
    for w in words:
        assert w in _lib.last_error()


def test_argument_refusals_on_host_pointers():
    L, d, p, q, o, a = _lib.lib(), _dims(), _host(), _host(), _host(), (C.c_int32 * 64)()
    # tma_dqn_act
    _refused(L.tma_dqn_act(None, C.byref(d), o, 4, 0.1, 1, 0, 0, a, None, None), "tma_dqn_act", "null")
    _refused(L.tma_dqn_act(p, C.byref(d), None, 4, 0.1, 1, 0, 0, a, None, None), "null")
    _refused(L.tma_dqn_act(p, C.byref(d), o, 4, 0.1, 1, 0, 0, None, None, None), "null")
    _refused(L.tma_dqn_act(p, None, o, 4, 0.1, 1, 0, 0, a, None, None), "null")
    _refused(L.tma_dqn_act(p, C.byref(d), o, 0, 0.1, 1, 0, 0, a, None, None), "n must be at least 1")
    for eps in (-0.1, 1.5, float("nan")):
        _refused(L.tma_dqn_act(p, C.byref(d), o, 4, eps, 1, 0, 0, a, None, None), "eps", "[0, 1]")
    # tma_dqn_td_grad: every pointer in turn, n, the workspace
    need = L.tma_dqn_workspace_bytes(C.byref(d), 4)
    P = (4 * 128 + 128 + 128 * 128 + 128 + 128 * 5 + 5)
    assert need == 32 + P * 4  # one tile: one slab of the pi segment behind one (loss, q, rows) record of 24 bytes, padded to a multiple of 16
    assert L.tma_dqn_workspace_bytes(C.byref(d), 64) == 96 + 4 * P * 4 and L.tma_dqn_workspace_bytes(C.byref(d), 10 ** 9) == 64 * 24 + 64 * P * 4
    good = [p, q, C.byref(d), o, a, o, o, o, o, 4, p, None, None, p, need, None]
    for i in (0, 1, 3, 4, 5, 6, 7, 8, 10):
        args = list(good)
        args[i] = None
        _refused(L.tma_dqn_td_grad(*args), "tma_dqn_td_grad", "null")
    _refused(L.tma_dqn_td_grad(*(good[:9] + [0] + good[10:])), "n must be at least 1")
    _refused(L.tma_dqn_td_grad(*(good[:14] + [need - 1, None])), "workspace", str(need))
    _refused(L.tma_dqn_td_grad(*(good[:13] + [None, need, None])), "workspace")
    assert L.tma_dqn_workspace_bytes(C.byref(d), 0) == 0 and "n must be at least 1" in _lib.last_error()
    # tma_dqn_target_update
    for tau in (0.0, -0.5, 1.0001, float("nan")):
        _refused(L.tma_dqn_target_update(p, q, C.byref(d), tau, None), "tau", "(0, 1]")
    _refused(L.tma_dqn_target_update(None, q, C.byref(d), 1.0, None), "null")
    _refused(L.tma_dqn_target_update(p, None, C.byref(d), 1.0, None), "null")
    _refused(L.tma_dqn_target_update(p, p, C.byref(d), 1.0, None), "same buffer")
    # tma_dqn_iterations_local
    hp = _lib.DQNHParams(1000, 16, 32, 8, 4, 1, 1, 1.0, 0.99, 0.1, 1.0, 0.05, 1e-4, 10.0, 1, 1, 0)
    rb = _lib.Replay(*([C.cast(p, C.c_void_p)] * 6), 48, 1, 4, 5, 0)
    bufs = _lib.DQNBuffers(*([C.cast(p, C.c_void_p)] * 18), 1 << 20, C.cast(p, C.c_void_p))
    c = _lib.DQNCounters()
    fake_env = C.cast(p, C.c_void_p)
    call = lambda **kw: L.tma_dqn_iterations_local(kw.get("env", fake_env), p, q, C.byref(kw.get("d", d)), C.byref(kw.get("rb", rb)),  # noqa: E731
                                                   C.byref(kw.get("bufs", bufs)), C.byref(kw.get("hp", hp)), C.byref(kw.get("c", c)), kw.get("n", 1), None)
    _refused(call(env=None), "tma_dqn_iterations_local", "null")
    _refused(call(n=0), "n_iters")
    empty = _lib.DQNBuffers()
    _refused(call(bufs=empty), "buffer")
    for field, value in (("train_freq", 0), ("batch_size", 0), ("target_update_interval", 0), ("gradient_steps", 0), ("gradient_steps", -2)):
        bad = _lib.DQNHParams.from_buffer_copy(hp)
        setattr(bad, field, value)
        _refused(call(hp=bad), "train_freq")
    bad = _lib.DQNHParams.from_buffer_copy(hp)
    bad.exploration_fraction = 0.0
    _refused(call(hp=bad), "exploration_fraction")
    _refused(call(rb=_lib.Replay(*([C.cast(p, C.c_void_p)] * 6), 48, 1, 4, 5, 1)), "replay view")
    _refused(call(rb=_lib.Replay(*([C.cast(p, C.c_void_p)] * 6), 48, 1, 7, 5, 0)), "replay view")
    _refused(call(c=_lib.DQNCounters(0, 0, 48, 0, 0, 0, 0, 0)), "counters")
    _refused(call(d=_dims(H=192)), "hidden 192")


def test_constructor_defaults_and_refusals():
    import three_mlagents_amd
    from three_mlagents_amd.dqn import DQN

    assert three_mlagents_amd.DQN is DQN and "DQN" in three_mlagents_amd.__all__
    sig = inspect.signature(DQN.__init__).parameters
    want = dict(policy="MlpPolicy", learning_rate=1e-4, buffer_size=1_000_000, learning_starts=100, batch_size=32, tau=1.0, gamma=0.99, train_freq=4,
                gradient_steps=1, optimize_memory_usage=False, n_steps=1, target_update_interval=10_000, exploration_fraction=0.1,
                exploration_initial_eps=1.0, exploration_final_eps=0.05, max_grad_norm=10, stats_window_size=100, tensorboard_log=None,
                policy_kwargs=None, verbose=0, seed=None, device="auto")
    assert {k: sig[k].default for k in want} == want
    names = [k for k in sig if k not in ("self", "_init_setup_model")]
    assert names[:2] == ["policy", "env"] and names[2:] == list(want)[1:]
    m = DQN("MlpPolicy", None)
    assert (m.exploration_rate, m.num_timesteps, m._n_updates, m.train_freq, m.gradient_steps) == (1.0, 0, 0, 4, 1)
    assert DQN("MlpPolicy", None, train_freq=(8, "step")).train_freq == 8
    for kw, word in ((dict(train_freq=(1, "episode")), "episode"), (dict(learning_rate=lambda p: 1e-4), "schedules"),
                     (dict(optimize_memory_usage=True), "optimize_memory_usage"), (dict(gradient_steps=0), "gradient_steps"), (dict(tau=0.0), "tau"),
                     (dict(exploration_fraction=0.0), "exploration_fraction"), (dict(policy="CnnPolicy"), "MlpPolicy"), (dict(batch_size=0), "batch_size")):
        with pytest.raises(ValueError, match=word):
            DQN(**{"policy": "MlpPolicy", "env": None, **kw})


def _fake_env(cls, num_actions, obs_dim=4):
    """An env object that reaches DQN._setup_model's refusals without a device: the class, the action count and the observation width."""
    env = cls.__new__(cls)

    class Engine:
        pass

    env.engine = Engine()
    env.engine.num_actions, env.engine.obs_dim, env.engine.act_dim = num_actions, obs_dim, 1
    return env


def test_setup_refusals_come_before_the_device():
    from three_mlagents_amd.dqn import DQN
    from three_mlagents_amd.vec_env import HipVecEnv
    from three_mlagents_amd.vec_normalize import VecNormalize

    def setup(env, world=1, **kw):
        m = DQN("MlpPolicy", None, **kw)
        m.env, m.world_size = env, world
        m._setup_model()

    with pytest.raises(ValueError, match="HipVecEnv"):
        setup(object())
    with pytest.raises(ValueError, match="Box"):
        setup(_fake_env(HipVecEnv, 0))
    with pytest.raises(ValueError, match="VecNormalize"):
        setup(_fake_env(VecNormalize, 5))
    with pytest.raises(ValueError, match="world_size"):
        setup(_fake_env(HipVecEnv, 5), world=2)
    for pk, word in (({"net_arch": [64, 128]}, "net_arch"), ({"net_arch": [64]}, "net_arch"), ({"net_arch": [192, 192]}, "hidden 192"),
                     ({"net_arch": [128, 128], "mfma_dtype": "bf16", "activation_fn": "tanh"}, "mfma_dtype")):
        with pytest.raises(ValueError, match=word):
            setup(_fake_env(HipVecEnv, 5), policy_kwargs=pk)
    with pytest.raises(ValueError, match="got 17"):
        setup(_fake_env(HipVecEnv, 17))
    with pytest.raises(ValueError, match="obs_dim 172"):
        setup(_fake_env(HipVecEnv, 5, obs_dim=172))


def test_epsilon_schedule_against_hand_worked_values():
    """total 1000, fraction 0.1, 1.0 -> 0.05, learning_starts 20: eps(t) = 1 - 0.95 t / 100 on the ramp."""
    from three_mlagents_amd.dqn import epsilon_at, linear_epsilon

    hp = _lib.DQNHParams(1000, 20, 32, 8, 4, 1, 1, 1.0, 0.99, 0.1, 1.0, 0.05, 1e-4, 10.0, 1, 1, 0)
    native = lambda t: _lib.lib().tma_dqn_epsilon(C.byref(hp), t)  # noqa: E731
    cases = [(0, 1.0),          # start (and the warm-up)
             (19, 1.0),         # below learning_starts: uniform
             (20, 0.81),        # the first scheduled step: 1 - 0.95 * 0.2
             (50, 0.525),       # inside the ramp
             (100, 0.05),       # exactly at exploration_fraction
             (101, 0.05), (1000, 0.05), (5000, 0.05)]  # beyond it
    for t, want in cases:
        for got in (native(t), ref.epsilon(t, 1000, 20, 0.1, 1.0, 0.05), epsilon_at(t, 1000, 20, 0.1, 1.0, 0.05)):
            assert got == pytest.approx(want, abs=1e-12), (t, got, want)
        assert native(t) == epsilon_at(t, 1000, 20, 0.1, 1.0, 0.05)  # the same double arithmetic in the same order
    # without a warm-up the schedule starts at its initial value; SB3's exploration_rate attribute has no warm-up either
    assert ref.epsilon(0, 1000, 0, 0.1, 1.0, 0.05) == 1.0 and linear_epsilon(10, 1000, 0.1, 1.0, 0.05) == pytest.approx(0.905, abs=1e-12)
    assert linear_epsilon(0, 400, 0.5, 0.8, 0.2) == 0.8 and linear_epsilon(100, 400, 0.5, 0.8, 0.2) == pytest.approx(0.5, abs=1e-12)


def test_reference_td_gradient_against_a_hand_worked_case():
    """features 1 -> 1 -> 1 -> 2, ReLU, every unit active.  Online Q(x) = [2x + 0.5, -x], target Q'(x) = [x, 3x] for x > 0.
    Row 0: x = 1, a = 0, x' = 0.5, r = 1, discount 0.9, not done: y = 1 + 0.9 * 1.5 = 2.35, Q = 2.5, delta = 0.15 (quadratic: 0.01125, cotangent 0.075).
    Row 1: x = 2, a = 1, x' = 1, r = 3, done: y = 3, Q = -2, delta = -5 (linear: 4.5, cotangent -0.5).
    loss = 2.255625;  dW3 = [0.075 * 1, -0.5 * 2], db3 = [0.075, -0.5];  dz2 = dz1 = [0.075 * 2, -0.5 * -1] = [0.15, 0.5];
    dW2 = dW1 = 0.15 * 1 + 0.5 * 2 = 1.15, db2 = db1 = 0.65."""
    K = ref.PI_KEYS
    t = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    sd = {K[0]: t([1.0]), K[1]: t(0.0), K[2]: t([1.0]), K[3]: t(0.0), K[4]: t([2.0], [-1.0]), K[5]: t(0.5, 0.0)}
    tg = {**sd, K[4]: t([1.0], [3.0]), K[5]: t(0.0, 0.0)}
    batch = dict(obs=t([1.0], [2.0]), next_obs=t([0.5], [1.0]), actions=torch.tensor([0, 1], dtype=torch.int32), dones=t(0.0, 1.0),
                 rewards=t(1.0, 3.0), discounts=t(0.9, 0.9))
    q_taken, y, delta = ref.td_parts(sd, tg, batch)
    assert torch.allclose(q_taken, t(2.5, -2.0)) and torch.allclose(y, t(2.35, 3.0)) and torch.allclose(delta, t(0.15, -5.0))
    grads, loss, q_sum = ref.td_grad(sd, tg, batch)
    assert loss == pytest.approx(2.255625, abs=1e-12) and q_sum == pytest.approx(0.5, abs=1e-12)
    want = {K[0]: t([1.15]), K[1]: t(0.65), K[2]: t([1.15]), K[3]: t(0.65), K[4]: t([0.075], [-1.0]), K[5]: t(0.075, -0.5)}
    for k in K:
        assert torch.allclose(grads[k], want[k], rtol=0, atol=1e-12), (k, grads[k], want[k])
    # tanh runs, and a done row ignores the target net
    g2, _, _ = ref.td_grad(sd, {**tg, K[4]: t([9.0], [9.0])}, {**batch, "dones": t(1.0, 1.0), "rewards": t(2.35, 3.0)})
    assert torch.allclose(g2[K[5]], want[K[5]], atol=1e-12) and float(ref.td_loss(sd, tg, batch, "tanh")) > 0


@pytest.mark.parametrize("n_envs", [1, 3])
@pytest.mark.parametrize("gradient_steps", [1, -1, 3])
def test_the_plan_counts_what_a_plain_loop_counts(n_envs, gradient_steps):
    """learning_starts 16, train_freq 4, target interval 8, 16 iterations: by hand at one env -- 64 steps; training from num_timesteps = 20
    on (iterations 5 .. 16: 12 of them); the target update at n_calls 8, 16, ..., 64 (eight)."""
    from three_mlagents_amd.dqn import plan_iterations

    kw = dict(n_envs=n_envs, train_freq=4, gradient_steps=gradient_steps, learning_starts=16, target_update_interval=8)
    c, n_train, n_target, events = ref.count_events(16, capacity=48, total_timesteps=200, exploration_fraction=0.5, exploration_initial_eps=1.0,
                                                    exploration_final_eps=0.05, **kw)
    plan = plan_iterations(0, 0, 16, **kw)
    assert plan == {"num_timesteps": c["num_timesteps"], "n_calls": c["n_calls"], "n_updates": n_train, "target_updates": n_target}
    per = 4 if gradient_steps < 0 else gradient_steps
    if n_envs == 1:
        assert (plan["num_timesteps"], plan["n_calls"], plan["n_updates"], plan["target_updates"]) == (64, 64, 12 * per, 8)
    else:  # 12 env steps an iteration: training from the second iteration (24 > 16); interval max(8 // 3, 1) = 2 vector steps
        assert (plan["num_timesteps"], plan["n_calls"], plan["n_updates"], plan["target_updates"]) == (192, 64, 15 * per, 32)
    assert (c["pos"], c["full"], c["collect_step"], c["draw"], c["adam_step"]) == (64 - 48, True, 64, n_train, n_train)
    # the ring positions the steps were written to, and what the first and the last training call sample from
    assert [e[3] for e in events if e[0] == "step"] == [k % 48 for k in range(64)]
    trains = [e for e in events if e[0] == "train"]
    first_at = 20 if n_envs == 1 else 8
    assert trains[0][1:3] == (first_at, first_at - 1) and trains[-1][1:3] == (48, 15) and [e[4] for e in trains] == list(range(1, n_train + 1))
    # resumed counters give the same tail: two calls of eight iterations are one of sixteen
    half = plan_iterations(0, 0, 8, **kw)
    rest = plan_iterations(half["num_timesteps"], half["n_calls"], 8, **kw)
    assert (rest["num_timesteps"], rest["n_calls"], half["n_updates"] + rest["n_updates"], half["target_updates"] + rest["target_updates"]) == tuple(plan.values())
