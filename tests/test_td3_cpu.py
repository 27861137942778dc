"""TD3 without a GPU (include/tma.h ABI 227, three_mlagents_amd/td3.py): the symbols and their refusals, the constructor, the parameter layout
against the restatement's tensor shapes, the delayed-update plan against a literal loop of SB3's train(), the restatement's hand-written
cotangents against float64 autograd, the loop's counters against a plain-loop restatement, and the harness, which still refuses "td3"."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

import _td3_ref as ref
from three_mlagents_amd import _lib

NEW_SYMBOLS = ["tma_td3_param_offsets", "tma_td3_act", "tma_td3_workspace_bytes", "tma_td3_critic_grad", "tma_td3_actor_grad", "tma_td3_iterations_local"]


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
    assert L.tma_version() >= 227
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes is not None


def _noise(sigma=0.1):
    return _lib.TD3Noise((C.c_float * 8)(*([0.0] * 8)), (C.c_float * 8)(*([sigma] * 8)))


def _act_call(L, d, p, **kw):
    args = dict(actor=p, obs=p, n=4, mode=_lib.TD3_DETERMINISTIC, an=None, noise=None, out=p, nout=None, head=None)
    args.update(kw)
    an = C.byref(args["an"]) if args["an"] is not None else None
    return L.tma_td3_act(args["actor"], d, args["obs"], args["n"], args["mode"], an, 1, 0, 0, args["noise"], args["out"], args["nout"], args["head"], None)


def _critic_call(L, d, p, **kw):
    args = dict(actor_target=p, critic=p, target=p, obs=p, actions=p, next_obs=p, dones=p, rewards=p, discounts=p, n=4, pn=0.2, clip=0.5, grad=p, ws=p,
                ws_bytes=1 << 30)
    args.update(kw)
    return L.tma_td3_critic_grad(args["actor_target"], args["critic"], args["target"], d, args["obs"], args["actions"], args["next_obs"], args["dones"],
                                 args["rewards"], args["discounts"], args["n"], args["pn"], args["clip"], 1, 0, None, args["grad"], None, None, None, None, None,
                                 args["ws"], args["ws_bytes"], None)


def _actor_call(L, d, p, **kw):
    args = dict(actor=p, critic=p, obs=p, n=4, grad=p, ws=p, ws_bytes=1 << 30)
    args.update(kw)
    return L.tma_td3_actor_grad(args["actor"], args["critic"], d, args["obs"], args["n"], args["grad"], None, None, None, args["ws"], args["ws_bytes"], None)


def _loop_args():
    p, q = _host(), _host()
    vp = C.cast(p, C.c_void_p)
    hp = _lib.TD3HParams(16, 32, 2, 1, 1, 1, 0, 0.005, 0.99, 1e-3, 0.2, 0.5, _noise(), 1, 1, 0)
    rb = _lib.Replay(*([vp] * 6), 48, 1, 6, 2, 1)
    bufs = _lib.TD3Buffers(*([vp] * 22), 1 << 30)
    return p, q, vp, hp, rb, bufs


def _loop_call(L, **kw):
    p, q, vp, hp, rb, bufs = _loop_args()
    c = kw.get("c", _lib.TD3Counters())
    return L.tma_td3_iterations_local(kw.get("env", vp), p, q, p, q, C.byref(kw.get("d", _dims())), C.byref(kw.get("rb", rb)), C.byref(kw.get("bufs", bufs)),
                                      C.byref(kw.get("hp", hp)), C.byref(c), kw.get("n", 1), None)


# (dims, words of the message): what every entry point refuses on its shape argument, SAC's contract.  Crawler (172 / 20) is the last one.
BAD_DIMS = [(_dims(H=192), ("hidden 192",)), (_dims(H=100), ("hidden",)), (_dims(A=9), ("act_dim 9", "[1, 8]")), (_dims(A=0), ("[1, 8]",)),
            (_dims(D=121, A=8), ("obs_dim 121", "128")), (_dims(D=0), ("obs_dim 0",)), (_dims(act=2), ("activation 2",)), (_dims(D=172, A=20), ("act_dim 20",)),
            (_dims(H=400), ("hidden 400",)), (_dims(H=300), ("hidden 300",))]


@pytest.mark.parametrize("d,words", BAD_DIMS)
def test_every_entry_refuses_unsupported_shapes_before_any_hip_call(d, words):
    L, p = _lib.lib(), _host()
    _refused(L.tma_td3_param_offsets(C.byref(d), C.byref(_lib.TD3Offsets())), "tma_td3_param_offsets", *words)
    for mode in (_lib.TD3_DETERMINISTIC, _lib.TD3_NOISY, _lib.TD3_UNIFORM):
        _refused(_act_call(L, C.byref(d), p, mode=mode, an=_noise()), "tma_td3_act", *words)
    _refused(_critic_call(L, C.byref(d), p), "tma_td3_critic_grad", *words)
    _refused(_actor_call(L, C.byref(d), p), "tma_td3_actor_grad", *words)
    _refused(_loop_call(L, d=d), "tma_td3_iterations_local", *words)
    assert L.tma_td3_workspace_bytes(C.byref(d), 4) == 0
    for w in ("tma_td3_workspace_bytes",) + words:
        assert w in _lib.last_error()


def test_argument_refusals_on_host_pointers():
    L, d, p = _lib.lib(), _dims(), _host()
    dd = C.byref(d)
    # tma_td3_param_offsets
    _refused(L.tma_td3_param_offsets(None, C.byref(_lib.TD3Offsets())), "tma_td3_param_offsets", "null")
    _refused(L.tma_td3_param_offsets(dd, None), "tma_td3_param_offsets", "null")
    # tma_td3_act
    _refused(_act_call(L, None, p), "tma_td3_act", "null")
    _refused(_act_call(L, dd, p, actor=None), "tma_td3_act", "null")
    _refused(_act_call(L, dd, p, obs=None), "tma_td3_act", "null")
    _refused(_act_call(L, dd, p, out=None), "tma_td3_act", "null")
    _refused(_act_call(L, dd, p, mode=_lib.TD3_UNIFORM, out=None), "tma_td3_act", "null")
    _refused(_act_call(L, dd, p, n=0), "tma_td3_act", "n must be at least 1")
    _refused(_act_call(L, dd, p, mode=3), "tma_td3_act", "mode 3")
    _refused(_act_call(L, dd, p, mode=-1), "tma_td3_act", "mode -1")
    _refused(_act_call(L, dd, p, noise=p), "tma_td3_act", "deterministic", "noise_in")
    _refused(_act_call(L, dd, p, mode=_lib.TD3_NOISY), "tma_td3_act", "noisy", "action_noise")
    _refused(_act_call(L, dd, p, mode=_lib.TD3_NOISY, an=_noise(-0.1)), "tma_td3_act", "sigma", "negative")
    _refused(_act_call(L, dd, p, mode=_lib.TD3_NOISY, an=_noise(float("nan"))), "tma_td3_act", "sigma")
    bad_mean = _noise()
    bad_mean.mean[1] = float("nan")
    _refused(_act_call(L, dd, p, mode=_lib.TD3_NOISY, an=bad_mean), "tma_td3_act", "column 1", "NaN")
    for kw in (dict(noise=p), dict(nout=p), dict(head=p)):
        _refused(_act_call(L, dd, p, mode=_lib.TD3_UNIFORM, **kw), "tma_td3_act", "uniform", "NULL")
    # the workspace: one slab of the wider buffer behind one record of four doubles per workgroup, at most 64 workgroups
    off = _lib.TD3Offsets()
    assert L.tma_td3_param_offsets(dd, C.byref(off)) == 0
    widest = max(off.n_actor, off.n_critic)
    assert L.tma_td3_workspace_bytes(dd, 4) == 32 + widest * 4 and L.tma_td3_workspace_bytes(dd, 64) == 4 * (32 + widest * 4)
    assert L.tma_td3_workspace_bytes(dd, 10 ** 9) == 64 * (32 + widest * 4)
    assert L.tma_td3_workspace_bytes(dd, 0) == 0 and "n must be at least 1" in _lib.last_error() and "tma_td3_workspace_bytes" in _lib.last_error()
    assert L.tma_td3_workspace_bytes(None, 4) == 0 and "null" in _lib.last_error()
    need = L.tma_td3_workspace_bytes(dd, 4)
    # tma_td3_critic_grad / tma_td3_actor_grad: every pointer in turn, n, the smoothing parameters, the workspace
    for name in ("actor_target", "critic", "target", "obs", "actions", "next_obs", "dones", "rewards", "discounts", "grad"):
        _refused(_critic_call(L, dd, p, **{name: None}), "tma_td3_critic_grad", "null")
    _refused(_critic_call(L, None, p), "tma_td3_critic_grad", "null")
    _refused(_critic_call(L, dd, p, n=0), "tma_td3_critic_grad", "n must be at least 1")
    for kw in (dict(pn=-0.1), dict(clip=-0.5), dict(pn=float("nan")), dict(clip=float("nan"))):
        _refused(_critic_call(L, dd, p, **kw), "tma_td3_critic_grad", "target_policy_noise", "target_noise_clip", "at least 0")
    _refused(_critic_call(L, dd, p, ws_bytes=need - 1), "tma_td3_critic_grad", "workspace", str(need))
    _refused(_critic_call(L, dd, p, ws=None), "tma_td3_critic_grad", "workspace")
    for name in ("actor", "critic", "obs", "grad"):
        _refused(_actor_call(L, dd, p, **{name: None}), "tma_td3_actor_grad", "null")
    _refused(_actor_call(L, None, p), "tma_td3_actor_grad", "null")
    _refused(_actor_call(L, dd, p, n=0), "tma_td3_actor_grad", "n must be at least 1")
    _refused(_actor_call(L, dd, p, ws_bytes=need - 1), "tma_td3_actor_grad", "workspace", str(need))
    _refused(_actor_call(L, dd, p, ws=None), "tma_td3_actor_grad", "workspace")
    # tma_td3_iterations_local
    _, _, vp, hp, _, _ = _loop_args()
    _refused(_loop_call(L, env=None), "tma_td3_iterations_local", "null")
    _refused(_loop_call(L, n=0), "tma_td3_iterations_local", "n_iters")
    _refused(_loop_call(L, bufs=_lib.TD3Buffers()), "tma_td3_iterations_local", "buffer")
    for field, value in (("train_freq", 0), ("batch_size", 0), ("policy_delay", 0), ("gradient_steps", 0), ("gradient_steps", -2)):
        bad = _lib.TD3HParams.from_buffer_copy(hp)
        setattr(bad, field, value)
        _refused(_loop_call(L, hp=bad), "tma_td3_iterations_local", "train_freq", "policy_delay")
    for field in ("target_policy_noise", "target_noise_clip"):
        bad = _lib.TD3HParams.from_buffer_copy(hp)
        setattr(bad, field, -0.1)
        _refused(_loop_call(L, hp=bad), "tma_td3_iterations_local", field, "at least 0")
    _refused(_loop_call(L, rb=_lib.Replay(*([vp] * 6), 48, 1, 6, 2, 0)), "tma_td3_iterations_local", "replay view", "Box")
    _refused(_loop_call(L, rb=_lib.Replay(*([vp] * 6), 48, 1, 7, 2, 1)), "tma_td3_iterations_local", "replay view")
    _refused(_loop_call(L, rb=_lib.Replay(*([vp] * 6), 48, 1, 6, 3, 1)), "tma_td3_iterations_local", "replay view")
    _refused(_loop_call(L, c=_lib.TD3Counters(0, 0, 48, 0, 0, 0, 0, 0, 0)), "tma_td3_iterations_local", "counters")
    _refused(_loop_call(L, c=_lib.TD3Counters(0, 0, 0, 0, 0, 0, 0, -1, 0)), "tma_td3_iterations_local", "counters")


def test_constructor_defaults_and_refusals():
    import three_mlagents_amd
    from three_mlagents_amd.td3 import TD3, NormalActionNoise, noise_struct

    assert three_mlagents_amd.TD3 is TD3 and "TD3" in three_mlagents_amd.__all__ and three_mlagents_amd.NormalActionNoise is NormalActionNoise
    sig = inspect.signature(TD3.__init__).parameters
    want = dict(policy="MlpPolicy", learning_rate=1e-3, buffer_size=1_000_000, learning_starts=100, batch_size=256, tau=0.005, gamma=0.99, train_freq=1,
                gradient_steps=1, action_noise=None, optimize_memory_usage=False, n_steps=1, policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5,
                stats_window_size=100, tensorboard_log=None, policy_kwargs=None, verbose=0, seed=None, device="auto")
    assert {k: sig[k].default for k in want} == want
    assert [k for k in sig if k != "self"][:2] == ["policy", "env"]
    noise = NormalActionNoise(np.zeros(8), 0.1 * np.ones(8))
    m = TD3("MlpPolicy", None, action_noise=noise, gradient_steps=-1, train_freq=(2, "step"), policy_delay=3)
    assert m.action_noise is noise and m.gradient_steps == -1 and m.train_freq == 2 and m.policy_delay == 3 and m.ALGORITHM == "td3"
    assert np.array_equal(noise.mean, np.zeros(8)) and np.array_equal(noise.sigma, 0.1 * np.ones(8)) and "NormalActionNoise" in repr(noise)
    s = noise_struct(NormalActionNoise(0.25, [0.5, 0.125, 1.0]), 3)
    assert list(s.mean)[:4] == [0.25, 0.25, 0.25, 0.0] and list(s.sigma)[:4] == [0.5, 0.125, 1.0, 0.0] and list(noise_struct(None, 3).sigma) == [0.0] * 8
    for bad in (NormalActionNoise(np.zeros(2), np.ones(2)), NormalActionNoise(0.0, -1.0), NormalActionNoise(float("nan"), 1.0)):
        with pytest.raises(ValueError, match="action_noise"):
            noise_struct(bad, 3)
    # the one stated deviation: the default arch is [256, 256]; SB3's [400, 300] and every other arch is refused, naming the widths
    assert TD3._arch({}) == (256, "relu") and TD3._arch({"net_arch": [64, 64], "activation_fn": torch.nn.Tanh}) == (64, "tanh")
    assert TD3._arch({"net_arch": {"pi": [128, 128], "qf": [128, 128]}}) == (128, "relu")
    for pk in ({"net_arch": [400, 300]}, {"net_arch": [64, 32]}, {"net_arch": [64]}, {"net_arch": [32, 32]}, {"net_arch": [512, 512]},
               {"net_arch": {"pi": [64, 64], "qf": [128, 128]}}):
        with pytest.raises(ValueError, match="net_arch") as info:
            TD3("MlpPolicy", None, policy_kwargs=pk)
        if not isinstance(pk["net_arch"], dict):
            assert "64, 128 or 256" in str(info.value)

    class OrnsteinUhlenbeckActionNoise:
        pass

    for kw, word in ((dict(policy="CnnPolicy"), "MlpPolicy"), (dict(learning_rate=lambda p: 1e-3), "schedules"),
                     (dict(action_noise=OrnsteinUhlenbeckActionNoise()), "Ornstein-Uhlenbeck"), (dict(action_noise=object()), "NormalActionNoise"),
                     (dict(train_freq=(1, "episode")), "per episode"), (dict(optimize_memory_usage=True), "optimize_memory_usage"),
                     (dict(policy_kwargs={"n_critics": 3}), "n_critics"), (dict(policy_kwargs={"n_critics": 1}), "n_critics"),
                     (dict(gradient_steps=0), "gradient_steps"), (dict(tau=0.0), "tau"), (dict(batch_size=0), "batch_size"),
                     (dict(policy_delay=0), "policy_delay"), (dict(policy_delay=-2), "policy_delay"), (dict(target_policy_noise=-0.1), "target_policy_noise"),
                     (dict(target_noise_clip=-0.5), "target_noise_clip")):
        with pytest.raises(ValueError, match=word):
            TD3(**{"policy": "MlpPolicy", "env": None, **kw})
    with pytest.raises(ValueError, match="HipVecEnv"):
        TD3("MlpPolicy", object())


def test_harness_still_refuses_td3():
    from three_mlagents_amd import harness, tasks

    assert "td3" not in harness.ALGORITHMS
    for name in ("dqn", "td3"):
        with pytest.raises(ValueError, match="Unsupported algorithm"):
            harness._algorithm_for(name, tasks.resolve("ant"))


@pytest.mark.parametrize("D,A,H", [(6, 2, 256), (105, 8, 256), (1, 1, 64), (21, 3, 128)])
def test_param_offsets_follow_sb3_tensor_order(D, A, H):
    from three_mlagents_amd import sac
    from three_mlagents_amd.td3 import actor_tensors, critic_tensors, flat_from_named, named_from_flat, param_offsets, sac_dims

    off = param_offsets(sac_dims(D, A, H))
    shapes = ref.tensor_shapes(D, A, H)
    o = 0
    for name, w, b, n_in, n_out in actor_tensors(off, D, A, H):  # packed, in SB3's order: actor.mu.{0,2,4}
        assert (w, b) == (o, o + n_in * n_out) and shapes[f"actor.{name}.weight"] == (n_out, n_in) and shapes[f"actor.{name}.bias"] == (n_out,)
        o = b + n_out
    assert o == off.n_actor == sum(math.prod(shapes[k]) for k in ref.actor_keys()) == D * H + H + H * H + H + H * A + A
    assert [k for k in shapes if k.startswith("actor.")] == ref.actor_keys()
    o = 0
    for name, w, b, n_in, n_out in critic_tensors(off, D, A, H):
        assert (w, b) == (o, o + n_in * n_out) and shapes[f"critic.{name}.weight"] == (n_out, n_in)
        o = b + n_out
    assert o == off.n_critic == 2 * off.n_q == sum(math.prod(shapes[k]) for k in ref.critic_keys())
    # the critic pair is SAC's layout exactly
    soff = sac.param_offsets(sac_dims(D, A, H))
    for k in ("q_W1", "q_b1", "q_W2", "q_b2", "q_W3", "q_b3", "n_q", "n_critic"):
        assert getattr(off, k) == getattr(soff, k), k
    # [in][out] in the buffer, [out][in] in SB3's names; the round trip is exact
    flat = torch.arange(off.n_actor, dtype=torch.float32)
    named = named_from_flat(flat, actor_tensors(off, D, A, H), "actor_target")
    assert named["actor_target.mu.4.weight"][A - 1, 3].item() == off.a_Wmu + 3 * A + A - 1  # Wmu, input row 3, output A - 1
    assert torch.equal(flat_from_named(named, actor_tensors(off, D, A, H), "actor_target", off.n_actor), flat)


@pytest.mark.parametrize("policy_delay", [1, 2, 3])
def test_delayed_update_plan_follows_sb3_train_across_a_resumed_call(policy_delay):
    from three_mlagents_amd.td3 import plan_iterations, plan_updates

    # one call of seven steps, then a resumed call of five from the counter the first left: the same decisions as twelve steps in one call
    first, n = ref.sb3_train_plan(0, 7, policy_delay)
    second, n2 = ref.sb3_train_plan(n, 5, policy_delay)
    whole, _ = ref.sb3_train_plan(0, 12, policy_delay)
    assert plan_updates(0, 7, policy_delay) == first and plan_updates(7, 5, policy_delay) == second and first + second == whole and (n, n2) == (7, 12)
    assert sum(whole) == 12 // policy_delay and whole[policy_delay - 1] and (policy_delay == 1 or not whole[0])
    for start in range(7):
        assert plan_updates(start, 9, policy_delay) == ref.sb3_train_plan(start, 9, policy_delay)[0]
    # the loop's counters against the plain loop
    for n_envs, train_freq, gs, starts, n_iters, cap in ((1, 1, 1, 100, 300, 64), (3, 2, -1, 20, 40, 16), (1, 4, 2, 0, 10, 1000), (2, 1, 3, 50, 60, 7)):
        c = ref.new_counters()
        ev = list(ref.iteration_events(c, n_iters, n_envs=n_envs, capacity=cap, train_freq=train_freq, gradient_steps=gs, learning_starts=starts,
                                       policy_delay=policy_delay))
        plan = plan_iterations(0, 0, n_iters, n_envs, train_freq, gs, starts, policy_delay)
        assert plan == dict(num_timesteps=c["num_timesteps"], n_calls=c["n_calls"], n_updates=c["n_updates"], actor_updates=c["actor_adam_step"],
                            uniform_steps=sum(e[0] == "step" and e[1] for e in ev))
        assert c["n_calls"] == n_iters * train_freq and c["draw"] == c["critic_adam_step"] == c["n_updates"]
        assert c["actor_adam_step"] == c["n_updates"] // policy_delay == sum(e[0] == "train" and e[5] is not None for e in ev)
        # resumed half way: the same counters
        c2 = ref.new_counters()
        list(ref.iteration_events(c2, n_iters // 2, n_envs=n_envs, capacity=cap, train_freq=train_freq, gradient_steps=gs, learning_starts=starts,
                                  policy_delay=policy_delay))
        half = plan_iterations(0, 0, n_iters // 2, n_envs, train_freq, gs, starts, policy_delay)
        rest = plan_iterations(half["num_timesteps"], half["n_updates"], n_iters - n_iters // 2, n_envs, train_freq, gs, starts, policy_delay)
        assert half["n_updates"] + rest["n_updates"] == plan["n_updates"] and half["actor_updates"] + rest["actor_updates"] == plan["actor_updates"]
        assert rest["num_timesteps"] == plan["num_timesteps"]


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_hand_written_cotangents_match_float64_autograd(act):
    D, H, A, n = 7, 64, 3, 40
    sd = ref.make_sd(D, H, A, act, seed=5)
    batch, _ = ref.make_batch(sd, D, A, n, act, seed=9)
    ref.check_batch(sd, batch, act)
    g, stats, q, y = ref.critic_grad(sd, batch, activation=act)
    hand = ref.critic_grad_by_hand(sd, batch, activation=act)
    scale = max(float(v.abs().max()) for v in g.values())
    assert scale > 1e-3 and max(float((g[k] - hand[k]).abs().max()) for k in g) <= 1e-13 * max(scale, 1.0)
    # the factor 2: SAC's loss on the same tensors carries a 1/2 and half the gradient
    half = {k: v / 2 for k, v in hand.items()}
    assert max(float((g[k] - half[k]).abs().max()) for k in g) > 0.4 * scale
    assert stats["loss_sum"] == pytest.approx(float(((q - y[:, None]) ** 2).sum()), rel=1e-12)
    g, stats, a_pi, q0 = ref.actor_grad(sd, batch, act)
    hand = ref.actor_grad_by_hand(sd, batch, act)
    scale = max(float(v.abs().max()) for v in g.values())
    assert scale > 1e-4 and max(float((g[k] - hand[k]).abs().max()) for k in g) <= 1e-13 * max(scale, 1.0)
    assert stats["loss_sum"] == pytest.approx(-float(q0.sum()), rel=1e-12)
    # the qf0-only path: qf1 does not enter the actor loss; qf0 does
    other = {k: (v * 1.5 if k.startswith("critic.qf1.") else v) for k, v in sd.items()}
    g1 = ref.actor_grad(other, batch, act)[0]
    assert all(torch.equal(g1[k], g[k]) for k in g)
    other = {k: (v * 1.5 if k.startswith("critic.qf0.4") else v) for k, v in sd.items()}
    assert not torch.equal(ref.actor_grad(other, batch, act)[0]["actor.mu.4.bias"], g["actor.mu.4.bias"])


def test_hand_worked_values():
    """D = 1, H = 2, A = 1, ReLU, one row: obs 2, replayed action 0, mu = 0 -> a = 0, Q0 = 3, Q1 = 4 (tests/test_sac_cpu.py's nets)."""
    t = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    sd = {}
    for prefix in ("actor", "actor_target"):
        sd.update({f"{prefix}.mu.0.weight": t([1.0], [-1.0]), f"{prefix}.mu.0.bias": t(0.0, 0.0), f"{prefix}.mu.2.weight": t([1.0, 0.0], [0.0, 1.0]),
                   f"{prefix}.mu.2.bias": t(0.0, 1.0), f"{prefix}.mu.4.weight": t([0.5, -1.0]), f"{prefix}.mu.4.bias": t(0.0)})
    for prefix in ("critic", "critic_target"):
        for i, (wa, b3) in enumerate(((1.0, 0.0), (2.0, 1.0))):
            sd.update({f"{prefix}.qf{i}.0.weight": t([1.0, wa], [0.0, 0.0]), f"{prefix}.qf{i}.0.bias": t(0.0, 1.0),
                       f"{prefix}.qf{i}.2.weight": t([1.0, 0.0], [0.0, 1.0]), f"{prefix}.qf{i}.2.bias": t(0.0, 0.0),
                       f"{prefix}.qf{i}.4.weight": t([1.0, 1.0]), f"{prefix}.qf{i}.4.bias": t(b3)})
    batch = dict(obs=t([2.0]), actions=t([0.0]), next_obs=t([2.0]), dones=t(1.0), rewards=t(1.0), discounts=t(0.99), noise=t([1.0]))
    # critic: y = r (done); loss = (3 - 1)^2 + (4 - 1)^2 = 13; cotangents 2 * 2 and 2 * 3
    g, stats, q, y = ref.critic_grad(sd, batch, 0.2, 0.5)
    assert q.tolist() == [[3.0, 4.0]] and y.tolist() == [1.0] and stats == dict(loss_sum=13.0, q0_sum=3.0, q1_sum=4.0)
    for i, c in ((0, 4.0), (1, 6.0)):
        assert torch.equal(g[f"critic.qf{i}.4.weight"], c * t([2.0, 1.0])) and torch.equal(g[f"critic.qf{i}.4.bias"], t(c))
        assert torch.equal(g[f"critic.qf{i}.0.weight"], c * t([2.0, 0.0], [2.0, 0.0])) and torch.equal(g[f"critic.qf{i}.0.bias"], t(c, c))
    # not done: a' = clamp(0 + clamp(0.2 z, -0.5, 0.5), -1, 1); Qt0 = 3 + a', Qt1 = 4 + 2 a'; y = 1 + 0.99 min
    for z, a_next in ((1.0, 0.2), (4.0, 0.5), (-4.0, -0.5)):
        nd = dict(batch, dones=t(0.0), noise=t([z]))
        assert ref.critic_grad(sd, nd, 0.2, 0.5)[3].item() == pytest.approx(1.0 + 0.99 * min(3.0 + a_next, 4.0 + 2.0 * a_next), abs=1e-12)
    assert ref.critic_grad(sd, dict(batch, dones=t(0.0), noise=t([4.0])), 2.0, 5.0)[3].item() == pytest.approx(1.0 + 0.99 * 4.0, abs=1e-12)  # a' clamped at 1
    # actor: loss = -Q0; dQ0/da = 1 at a = 0 (1 - a^2 = 1): the mu cotangent is -1
    g, stats, a, q0 = ref.actor_grad(sd, batch)
    assert a.tolist() == [[0.0]] and q0.tolist() == [3.0] and stats == dict(loss_sum=-3.0)
    assert torch.equal(g["actor.mu.4.weight"], t([-2.0, -1.0])) and torch.equal(g["actor.mu.4.bias"], t(-1.0))
    assert torch.equal(g["actor.mu.2.weight"], t([-1.0, 0.0], [2.0, 0.0])) and torch.equal(g["actor.mu.2.bias"], t(-0.5, 1.0))
    assert torch.equal(g["actor.mu.0.weight"], t([-1.0], [0.0])) and torch.equal(g["actor.mu.0.bias"], t(-0.5, 0.0))
    # tma_td3_act's arithmetic
    mu = t([0.0, 2.0, -2.0])  # (one row of three columns)
    assert torch.equal(ref.act(mu), torch.tanh(mu))
    assert ref.act(mu, t([1.0, 1.0, -1.0]), t(0.25), t(0.5)).tolist() == [[0.75, 1.0, -1.0]]
