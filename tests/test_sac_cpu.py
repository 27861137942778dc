"""SAC without a GPU (include/tma.h ABI 226, three_mlagents_amd/sac.py): the symbols and their refusals, the constructor, the harness wiring, the
parameter layout against the restatement's tensor shapes, the restatement's gradients against a hand-worked case, and the loop's counters
against a plain-loop restatement."""
import ctypes as C
import inspect
import math

import pytest
import torch

import _sac_ref as ref
from three_mlagents_amd import _lib

NEW_SYMBOLS = ["tma_sac_param_offsets", "tma_sac_act", "tma_sac_workspace_bytes", "tma_sac_critic_grad", "tma_sac_actor_grad", "tma_sac_ent_coef_grad",
               "tma_adam_step_flat", "tma_polyak_update", "tma_sac_iterations_local"]


def _dims(D=6, A=2, H=128, act=1):
    return _lib.SACDims(D, A, H, act, -1)


def _host(n=64):
    return (C.c_float * n)()


def _refused(rc, *words):
    assert rc == _lib.TMA_ERR_INVALID, rc
    msg = _lib.last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    assert L.tma_version() >= 226
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes is not None


def _critic_call(L, d, p, **kw):
    args = dict(actor=p, critic=p, target=p, log=p, obs=p, actions=p, next_obs=p, dones=p, rewards=p, discounts=p, n=4, grad=p, ws=p, ws_bytes=1 << 30)
    args.update(kw)
    return L.tma_sac_critic_grad(args["actor"], args["critic"], args["target"], args["log"], d, args["obs"], args["actions"], args["next_obs"], args["dones"],
                                 args["rewards"], args["discounts"], args["n"], 1, 0, None, args["grad"], None, None, None, None, None, args["ws"],
                                 args["ws_bytes"], None)


def _actor_call(L, d, p, **kw):
    args = dict(actor=p, critic=p, log=p, obs=p, n=4, grad=p, ws=p, ws_bytes=1 << 30)
    args.update(kw)
    return L.tma_sac_actor_grad(args["actor"], args["critic"], args["log"], d, args["obs"], args["n"], 1, 0, None, args["grad"], None, None, None, None, None,
                                args["ws"], args["ws_bytes"], None)


# (dims, words of the message): what every entry point refuses on its shape argument.  Crawler (172 / 20) is the last one.
BAD_DIMS = [(_dims(H=192), ("hidden 192",)), (_dims(H=100), ("hidden",)), (_dims(A=9), ("act_dim 9", "[1, 8]")), (_dims(A=0), ("[1, 8]",)),
            (_dims(D=121, A=8), ("obs_dim 121", "128")), (_dims(D=0), ("obs_dim 0",)), (_dims(act=2), ("activation 2",)), (_dims(D=172, A=20), ("act_dim 20",))]


@pytest.mark.parametrize("d,words", BAD_DIMS)
def test_every_entry_refuses_unsupported_shapes_before_any_hip_call(d, words):
    L, p = _lib.lib(), _host()
    off = _lib.SACOffsets()
    _refused(L.tma_sac_param_offsets(C.byref(d), C.byref(off)), "tma_sac_param_offsets", *words)
    _refused(L.tma_sac_act(p, C.byref(d), p, 4, 0, 1, 0, 0, None, p, None, None, None, None), "tma_sac_act", *words)
    _refused(_critic_call(L, C.byref(d), p), "tma_sac_critic_grad", *words)
    _refused(_actor_call(L, C.byref(d), p), "tma_sac_actor_grad", *words)
    assert L.tma_sac_workspace_bytes(C.byref(d), 4) == 0
    for w in words:
        assert w in _lib.last_error()


def test_argument_refusals_on_host_pointers():
    L, d, p = _lib.lib(), _dims(), _host()
    dd = C.byref(d)
    # tma_sac_param_offsets
    _refused(L.tma_sac_param_offsets(None, C.byref(_lib.SACOffsets())), "null")
    _refused(L.tma_sac_param_offsets(dd, None), "null")
    # tma_sac_act
    act = lambda actor=p, obs=p, n=4, mode=0, noise=None, out=p, logp=None, nout=None, head=None, dims=dd: L.tma_sac_act(  # noqa: E731
        actor, dims, obs, n, mode, 1, 0, 0, noise, out, logp, nout, head, None)
    _refused(act(dims=None), "tma_sac_act", "null")
    _refused(act(actor=None), "null")
    _refused(act(obs=None), "null")
    _refused(act(out=None), "null")
    _refused(act(n=0), "n must be at least 1")
    _refused(act(mode=3), "mode 3")
    _refused(act(mode=_lib.SAC_DETERMINISTIC, noise=p), "deterministic", "noise_in")
    for kw in (dict(noise=p), dict(logp=p), dict(nout=p), dict(head=p)):
        _refused(act(mode=_lib.SAC_UNIFORM, **kw), "uniform", "NULL")
    # the workspace: one slab of the wider buffer behind one record of four doubles per workgroup, at most 64 workgroups
    off = _lib.SACOffsets()
    assert L.tma_sac_param_offsets(dd, C.byref(off)) == 0
    widest = max(off.n_actor, off.n_critic)
    assert L.tma_sac_workspace_bytes(dd, 4) == 32 + widest * 4 and L.tma_sac_workspace_bytes(dd, 64) == 4 * (32 + widest * 4)
    assert L.tma_sac_workspace_bytes(dd, 10 ** 9) == 64 * (32 + widest * 4)
    assert L.tma_sac_workspace_bytes(dd, 0) == 0 and "n must be at least 1" in _lib.last_error()
    need = L.tma_sac_workspace_bytes(dd, 4)
    # tma_sac_critic_grad / tma_sac_actor_grad: every pointer in turn, n, the workspace
    for name in ("actor", "critic", "target", "log", "obs", "actions", "next_obs", "dones", "rewards", "discounts", "grad"):
        _refused(_critic_call(L, dd, p, **{name: None}), "tma_sac_critic_grad", "null")
    _refused(_critic_call(L, None, p), "null")
    _refused(_critic_call(L, dd, p, n=0), "n must be at least 1")
    _refused(_critic_call(L, dd, p, ws_bytes=need - 1), "workspace", str(need))
    _refused(_critic_call(L, dd, p, ws=None), "workspace")
    for name in ("actor", "critic", "log", "obs", "grad"):
        _refused(_actor_call(L, dd, p, **{name: None}), "tma_sac_actor_grad", "null")
    _refused(_actor_call(L, None, p), "null")
    _refused(_actor_call(L, dd, p, n=0), "n must be at least 1")
    _refused(_actor_call(L, dd, p, ws_bytes=need - 1), "workspace", str(need))
    _refused(_actor_call(L, dd, p, ws=None), "workspace")
    # tma_sac_ent_coef_grad
    dbl = (C.c_double * 4)()
    _refused(L.tma_sac_ent_coef_grad(None, -2.0, p, None), "tma_sac_ent_coef_grad", "null")
    _refused(L.tma_sac_ent_coef_grad(dbl, -2.0, None, None), "null")
    _refused(L.tma_sac_ent_coef_grad(dbl, float("nan"), p, None), "NaN")
    # tma_adam_step_flat
    adam = lambda params=p, grad=p, m=p, v=p, n=8, step=1, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8: L.tma_adam_step_flat(  # noqa: E731
        params, grad, m, v, n, step, lr, b1, b2, eps, None)
    for kw in (dict(params=None), dict(grad=None), dict(m=None), dict(v=None)):
        _refused(adam(**kw), "tma_adam_step_flat", "null")
    _refused(adam(n=0), "n must be at least 1")
    _refused(adam(step=0), "step must be at least 1")
    for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1e-8)):
        _refused(adam(**kw), "betas")
    # tma_polyak_update
    q = _host()
    for tau in (0.0, -0.5, 1.0001, float("nan")):
        _refused(L.tma_polyak_update(p, q, 8, tau, None), "tau", "(0, 1]")
    _refused(L.tma_polyak_update(None, q, 8, 0.5, None), "tma_polyak_update", "null")
    _refused(L.tma_polyak_update(p, None, 8, 0.5, None), "null")
    _refused(L.tma_polyak_update(p, q, 0, 0.5, None), "n must be at least 1")
    _refused(L.tma_polyak_update(p, p, 8, 0.5, None), "same buffer")
    # tma_sac_iterations_local
    vp = C.cast(p, C.c_void_p)
    hp = _lib.SACHParams(16, 32, 1, 1, 1, 1, 1, 0.005, 0.99, 3e-4, -2.0, 1, 1, 0)
    rb = _lib.Replay(*([vp] * 6), 48, 1, 6, 2, 1)
    bufs = _lib.SACBuffers(*([vp] * 25), 1 << 30)
    c = _lib.SACCounters()
    call = lambda **kw: L.tma_sac_iterations_local(kw.get("env", vp), p, p, q, p, C.byref(kw.get("d", d)), C.byref(kw.get("rb", rb)),  # noqa: E731
                                                   C.byref(kw.get("bufs", bufs)), C.byref(kw.get("hp", hp)), C.byref(kw.get("c", c)), kw.get("n", 1), None)
    _refused(call(env=None), "tma_sac_iterations_local", "null")
    _refused(call(n=0), "n_iters")
    _refused(call(bufs=_lib.SACBuffers()), "buffer")
    for field, value in (("train_freq", 0), ("batch_size", 0), ("target_update_interval", 0), ("gradient_steps", 0), ("gradient_steps", -2)):
        bad = _lib.SACHParams.from_buffer_copy(hp)
        setattr(bad, field, value)
        _refused(call(hp=bad), "train_freq")
    _refused(call(rb=_lib.Replay(*([vp] * 6), 48, 1, 6, 2, 0)), "replay view", "Box")
    _refused(call(rb=_lib.Replay(*([vp] * 6), 48, 1, 7, 2, 1)), "replay view")
    _refused(call(rb=_lib.Replay(*([vp] * 6), 48, 1, 6, 3, 1)), "replay view")
    _refused(call(c=_lib.SACCounters(0, 0, 48, 0, 0, 0, 0, 0)), "counters")
    _refused(call(d=_dims(H=192)), "hidden 192")


def test_constructor_defaults_and_refusals():
    import three_mlagents_amd
    from three_mlagents_amd.sac import SAC

    assert three_mlagents_amd.SAC is SAC and "SAC" in three_mlagents_amd.__all__
    sig = inspect.signature(SAC.__init__).parameters
    want = dict(policy="MlpPolicy", learning_rate=3e-4, buffer_size=1_000_000, learning_starts=100, batch_size=256, tau=0.005, gamma=0.99, train_freq=1,
                gradient_steps=1, action_noise=None, optimize_memory_usage=False, n_steps=1, ent_coef="auto", target_update_interval=1,
                target_entropy="auto", use_sde=False, stats_window_size=100, tensorboard_log=None, policy_kwargs=None, verbose=0, seed=None, device="auto")
    assert {k: sig[k].default for k in want} == want
    assert [k for k in sig if k != "self"][:2] == ["policy", "env"]
    m = SAC("MlpPolicy", None, ent_coef="auto_0.1", gradient_steps=-1, train_freq=(2, "step"))
    assert m._auto_ent and m._log_ent_coef_init == math.log(0.1) and m.gradient_steps == -1 and m.train_freq == 2
    m = SAC("MlpPolicy", None, ent_coef=0.2)
    assert not m._auto_ent and m._log_ent_coef_init == math.log(0.2) and m.ent_coef_optimizer is None
    assert SAC._arch({}) == (256, "relu") and SAC._arch({"net_arch": [64, 64], "activation_fn": torch.nn.Tanh}) == (64, "tanh")
    assert SAC._arch({"net_arch": {"pi": [128, 128], "qf": [128, 128]}}) == (128, "relu")
    for kw, word in ((dict(policy="CnnPolicy"), "MlpPolicy"), (dict(learning_rate=lambda p: 1e-3), "schedules"), (dict(use_sde=True), "use_sde"),
                     (dict(action_noise=object()), "action_noise"), (dict(train_freq=(1, "episode")), "per episode"),
                     (dict(optimize_memory_usage=True), "optimize_memory_usage"), (dict(policy_kwargs={"n_critics": 3}), "n_critics"),
                     (dict(gradient_steps=0), "gradient_steps"), (dict(tau=0.0), "tau"), (dict(batch_size=0), "batch_size"),
                     (dict(ent_coef="fixed"), "ent_coef"), (dict(ent_coef=0.0), "ent_coef"), (dict(ent_coef="auto_0"), "ent_coef"),
                     (dict(target_entropy="high"), "target_entropy")):
        with pytest.raises(ValueError, match=word):
            SAC(**{"policy": "MlpPolicy", "env": None, **kw})
    for pk in ({"net_arch": [64, 32]}, {"net_arch": [64]}, {"net_arch": {"pi": [64, 64], "qf": [128, 128]}}):
        with pytest.raises(ValueError, match="net_arch"):
            SAC._arch(pk)
    with pytest.raises(ValueError, match="HipVecEnv"):
        SAC("MlpPolicy", object())


def test_harness_knows_sac_and_keeps_refusing_dqn():
    from three_mlagents_amd import harness, tasks
    from three_mlagents_amd.sac import SAC

    assert harness.ALGORITHMS["sac"] is SAC
    assert harness._algorithm_for("sac", tasks.resolve("ball3d")) == ("sac", None)
    assert harness._algorithm_for(None, tasks.resolve("ball3d"))[0] == "ppo"
    for name in ("dqn", "td3"):
        with pytest.raises(ValueError, match="Unsupported algorithm"):
            harness._algorithm_for(name, tasks.resolve("gridworld"))
    # the reference's table (training.py:392-403) at three budgets: both clamps of buffer_size and of learning_starts
    table = lambda total: dict(learning_rate=3e-4, buffer_size=max(100_000, min(1_000_000, total)), learning_starts=min(10_000, max(1_000, total // 20)),  # noqa: E731
                               batch_size=256, gamma=0.99, tau=0.005, train_freq=1, gradient_steps=1)
    for total in (600, 150_000, 5_000_000):
        assert harness.model_defaults("sac", tasks.resolve("ball3d"), 8, total) == table(total)
    task = tasks.resolve("ball3d")
    assert harness.model_defaults("sac", task) == table(task.total_timesteps)
    assert harness.model_defaults("a2c", task) == {} and harness.model_defaults("ppo", task, 8) == harness.ppo_defaults(task, 8)
    # refused before any env exists: a Discrete task (ball3d is one: Discrete(5)), VecNormalize
    with pytest.raises(ValueError, match="Box action space"):
        harness.train_task(harness.TrainConfig("ball3d", algorithm="sac", total_timesteps=100, verbose=0))
    with pytest.raises(ValueError, match="Box action space"):
        harness.train_task(harness.TrainConfig("gridworld", algorithm="sac", total_timesteps=100, verbose=0))
    with pytest.raises(ValueError, match="normalize"):
        harness.train_task(harness.TrainConfig("ant", algorithm="sac", total_timesteps=100, verbose=0, normalize=True))
    from three_mlagents_amd.__main__ import parser

    assert parser().parse_args(["train", "ball3d", "--algorithm", "sac"]).algorithm == "sac"


@pytest.mark.parametrize("D,A,H", [(6, 2, 256), (105, 8, 256), (1, 1, 64), (21, 3, 128)])
def test_param_offsets_follow_sb3_tensor_order(D, A, H):
    from three_mlagents_amd.sac import actor_tensors, critic_tensors, flat_from_named, named_from_flat, param_offsets, sac_dims

    off = param_offsets(sac_dims(D, A, H))
    shapes = ref.tensor_shapes(D, A, H)
    o = 0
    for name, w, b, n_in, n_out in actor_tensors(off, D, A, H):  # packed, in SB3's order
        assert (w, b) == (o, o + n_in * n_out) and shapes[f"actor.{name}.weight"] == (n_out, n_in) and shapes[f"actor.{name}.bias"] == (n_out,)
        o = b + n_out
    assert o == off.n_actor == sum(math.prod(shapes[k]) for k in ref.actor_keys())
    o = 0
    for name, w, b, n_in, n_out in critic_tensors(off, D, A, H):
        assert (w, b) == (o, o + n_in * n_out) and shapes[f"critic.{name}.weight"] == (n_out, n_in)
        o = b + n_out
    assert o == off.n_critic == 2 * off.n_q == sum(math.prod(shapes[k]) for k in ref.critic_keys())
    # [in][out] in the buffer, [out][in] in SB3's names; the round trip is exact
    flat = torch.arange(off.n_critic, dtype=torch.float32)
    named = named_from_flat(flat, critic_tensors(off, D, A, H), "critic")
    assert named["critic.qf1.0.weight"][3, D].item() == off.n_q + D * H + 3  # qf1, W1, input row D (the first action row), output 3
    assert torch.equal(flat_from_named(named, critic_tensors(off, D, A, H), "critic", off.n_critic), flat)


def test_plan_counts_what_the_plain_loop_does():
    from three_mlagents_amd.sac import plan_iterations

    for n_envs, train_freq, gs, starts, every, n_iters, cap in ((1, 1, 1, 100, 1, 300, 64), (3, 2, -1, 20, 3, 40, 16), (1, 4, 2, 0, 2, 10, 1000), (2, 1, 3, 50, 5, 60, 7)):
        c = ref.new_counters()
        ev = list(ref.iteration_events(c, n_iters, n_envs=n_envs, capacity=cap, train_freq=train_freq, gradient_steps=gs, learning_starts=starts,
                                       target_update_interval=every))
        plan = plan_iterations(0, 0, n_iters, n_envs, train_freq, gs, starts, every)
        assert plan == dict(num_timesteps=c["num_timesteps"], n_calls=c["n_calls"], n_updates=c["n_updates"],
                            target_updates=sum(e[0] == "train" and e[5] for e in ev), uniform_steps=sum(e[0] == "step" and e[1] for e in ev))
        assert c["n_calls"] == n_iters * train_freq and c["draw"] == c["adam_step"] == c["n_updates"]
        assert c["pos"] == c["n_calls"] % cap and c["full"] == (c["n_calls"] >= cap)
    # the first optimizer step follows the first vector step that takes num_timesteps past learning_starts; warm-up steps are uniform
    c = ref.new_counters()
    ev = list(ref.iteration_events(c, 12, n_envs=1, capacity=8, train_freq=1, gradient_steps=1, learning_starts=10, target_update_interval=1))
    assert [e[0] for e in ev] == ["step"] * 11 + ["train", "step", "train"] and [e[1] for e in ev if e[0] == "step"] == [True] * 10 + [False] * 2
    assert ev[11][1:] == (8, 2, 0, 1, True)  # size 8 (wrapped), newest row 2, draw 0, Adam step 1, polyak


def _hand_case():
    """D = 1, H = 2, A = 1, ReLU, one row: obs 2, replayed action 0, noise 0 everywhere -> a = 0, Q0 = 3, Q1 = 4."""
    t = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    sd = {"actor.latent_pi.0.weight": t([1.0], [-1.0]), "actor.latent_pi.0.bias": t(0.0, 0.0), "actor.latent_pi.2.weight": t([1.0, 0.0], [0.0, 1.0]),
          "actor.latent_pi.2.bias": t(0.0, 1.0), "actor.mu.weight": t([0.5, -1.0]), "actor.mu.bias": t(0.0), "actor.log_std.weight": t([0.0, 0.0]),
          "actor.log_std.bias": t(0.0)}
    for prefix in ("critic", "critic_target"):
        for i, (wa, b3) in enumerate(((1.0, 0.0), (2.0, 1.0))):
            sd.update({f"{prefix}.qf{i}.0.weight": t([1.0, wa], [0.0, 0.0]), f"{prefix}.qf{i}.0.bias": t(0.0, 1.0),
                       f"{prefix}.qf{i}.2.weight": t([1.0, 0.0], [0.0, 1.0]), f"{prefix}.qf{i}.2.bias": t(0.0, 0.0),
                       f"{prefix}.qf{i}.4.weight": t([1.0, 1.0]), f"{prefix}.qf{i}.4.bias": t(b3)})
    batch = dict(obs=t([2.0]), actions=t([0.0]), next_obs=t([2.0]), dones=t(1.0), rewards=t(1.0), discounts=t(0.99), noise_next=t([0.0]), noise_pi=t([0.0]))
    return sd, batch


def test_reference_gradients_match_hand_worked_values():
    sd, batch = _hand_case()
    t = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    lp = -0.5 * math.log(2 * math.pi) - math.log(1 + 1e-6)  # logp at z = 0, log_std = 0, a = 0
    # critic: y = r (done); loss = ((3 - 1)^2 + (4 - 1)^2) / 2; cotangents 2 and 3
    g, stats, q, y = ref.critic_grad(sd, batch, 0.0)
    assert q.tolist() == [[3.0, 4.0]] and y.tolist() == [1.0] and stats == dict(loss_sum=6.5, q0_sum=3.0, q1_sum=4.0)
    for i, c in ((0, 2.0), (1, 3.0)):
        assert torch.equal(g[f"critic.qf{i}.4.weight"], c * t([2.0, 1.0])) and torch.equal(g[f"critic.qf{i}.4.bias"], t(c))
        assert torch.equal(g[f"critic.qf{i}.2.weight"], c * t([2.0, 1.0], [2.0, 1.0])) and torch.equal(g[f"critic.qf{i}.2.bias"], t(c, c))
        assert torch.equal(g[f"critic.qf{i}.0.weight"], c * t([2.0, 0.0], [2.0, 0.0])) and torch.equal(g[f"critic.qf{i}.0.bias"], t(c, c))
    # not done: y = r + discount * (min(3, 4) - alpha * logp'), alpha = exp(log 0.5) in float32
    nd = dict(batch, dones=t(0.0))
    _, _, _, y = ref.critic_grad(sd, nd, math.log(0.5))
    alpha = float(torch.exp(torch.tensor(math.log(0.5), dtype=torch.float32)))
    assert y.item() == pytest.approx(1.0 + 0.99 * (3.0 - alpha * lp), abs=1e-12)
    # actor: loss = alpha logp - Q0 (Q0 < Q1); dQ0/da = 1, d logp / da = 0 at a = 0, d logp / d log_std = -1
    g, stats, a, logp = ref.actor_grad(sd, batch, 0.0)
    assert a.tolist() == [[0.0]] and logp.item() == pytest.approx(lp, abs=1e-12) and stats["loss_sum"] == pytest.approx(lp - 3.0, abs=1e-12)
    assert torch.equal(g["actor.mu.weight"], t([-2.0, -1.0])) and torch.equal(g["actor.mu.bias"], t(-1.0))
    assert torch.equal(g["actor.log_std.weight"], t([-2.0, -1.0])) and torch.equal(g["actor.log_std.bias"], t(-1.0))
    assert torch.equal(g["actor.latent_pi.2.weight"], t([-1.0, 0.0], [2.0, 0.0])) and torch.equal(g["actor.latent_pi.2.bias"], t(-0.5, 1.0))
    assert torch.equal(g["actor.latent_pi.0.weight"], t([-1.0], [0.0])) and torch.equal(g["actor.latent_pi.0.bias"], t(-0.5, 0.0))
    # the second critic wins once its action weight is negative enough: Q1(a) = 4 + w a; here a = 0, so make its bias smaller instead
    sd2 = dict(sd)
    sd2["critic.qf1.4.bias"] = t(-2.0)  # Q1 = 1 < Q0 = 3: dQ1/da = 2
    g, *_ = ref.actor_grad(sd2, batch, 0.0)
    assert torch.equal(g["actor.mu.bias"], t(-2.0)) and torch.equal(g["actor.log_std.bias"], t(-1.0))
    # the clamp stops the log_std gradient outside [-20, 2] (torch's rule)
    sd3 = dict(sd)
    sd3["actor.log_std.bias"] = t(2.5)
    g, _, _, logp = ref.actor_grad(sd3, batch, 0.0)
    assert torch.equal(g["actor.log_std.bias"], t(0.0)) and logp.item() == pytest.approx(lp - 2.0, abs=1e-12)
    # ent_coef: d/d log_ent_coef of -(log_ent_coef (logp + target_entropy)).mean()
    lec = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    ref.ent_coef_loss(lec, torch.tensor([1.0, 3.0], dtype=torch.float64), -1.0).backward()
    assert lec.grad.item() == -(2.0 - 1.0)
