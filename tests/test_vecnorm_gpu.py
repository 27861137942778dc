"""GPU tests of VecNormalize on the device: the kernels (csrc/tma_vecnorm.hip) against the float64 restatement tests/_vecnorm_ref.py on synthetic
arrays, the Python wrapper on real envs, tma_rollout_collect_norm against the stepped composition, PPO / evaluation / the harness end to end.

Bounds on the statistics (eps = 2^-53, n rows, k merges so far), derived in tests/test_vecnorm_cpu.py and applied here between the device and the
restatement, which sum in different orders: mean within 8 k n eps max|x|, variance within 8 k n eps of itself.  Everything the kernels compute FROM
the statistics is checked bit for bit against the restatement evaluated with the device's own read-back statistics: that is the IEEE contract
(float64 subtract, sqrt, divide, no fused multiply-add)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vecnorm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
STEPS = 6


def _bound():
    from three_mlagents_amd import _lib

    return _lib.VECNORM_ONE_LAUNCH_MAX


def _dev():
    return torch.device("cuda", 0)


class _Handle:
    """A raw tma_vecnorm handle driven through the C ABI with torch tensors."""

    def __init__(self, D, N, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8):
        from three_mlagents_amd import _lib

        self.lib, self.L, self.D, self.N = _lib, _lib.lib(), D, N
        self.h = C.c_void_p()
        _lib.check(self.L.tma_vecnorm_create(D, N, int(norm_obs), int(norm_reward), clip_obs, clip_reward, gamma, epsilon, 0, C.byref(self.h)))

    def close(self):
        self.lib.check(self.L.tma_vecnorm_destroy(self.h))

    def stats(self):
        mean, var, sc = np.empty(self.D), np.empty(self.D), np.empty(4)
        p = self.lib.ptr
        self.lib.check(self.L.tma_vecnorm_get_stats(self.h, p(mean), p(var), p(sc), self.lib.stream_ptr()))
        return dict(obs_mean=mean, obs_var=var, obs_count=sc[0], ret_mean=sc[1], ret_var=sc[2], ret_count=sc[3])

    def returns(self):
        out = np.empty(self.N)
        self.lib.check(self.L.tma_vecnorm_get_returns(self.h, self.lib.ptr(out), self.lib.stream_ptr()))
        return out

    def reset(self, obs, training=True):
        t = torch.from_numpy(obs).to(_dev())
        self.lib.check(self.L.tma_vecnorm_reset(self.h, self.lib.ptr(t), self.N, int(training), self.lib.stream_ptr()))
        return t.cpu().numpy()

    def step(self, obs, rew, tobs, term, trunc, training=True):
        p = self.lib.ptr
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) for a in (obs, rew, tobs, term, trunc)]
        self.lib.check(self.L.tma_vecnorm_step(self.h, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), self.N, int(training), self.lib.stream_ptr()))
        return t[0].cpu().numpy(), t[1].cpu().numpy(), t[2].cpu().numpy()

    def original(self):
        o = torch.empty((self.N, self.D), dtype=torch.float32, device=_dev())
        r = torch.empty((self.N,), dtype=torch.float32, device=_dev())
        self.lib.check(self.L.tma_vecnorm_get_original(self.h, self.lib.ptr(o), self.lib.ptr(r), self.lib.stream_ptr()))
        return o.cpu().numpy(), r.cpu().numpy()


def _synthetic(n, D, kind, seed=11):
    rng = np.random.default_rng(seed + 1000 * n + D)
    if kind == "offset":  # 1e5 + k / 64: float32-exact, spread ~ 1, where E[x^2] - E[x]^2 is wrong in the sixth digit
        obs = (1e5 + rng.integers(0, 64, size=(STEPS + 1, n, D)) / 64.0).astype(np.float32)
        tobs = (1e5 + rng.integers(0, 64, size=(STEPS, n, D)) / 64.0).astype(np.float32)
    else:  # magnitudes up to 1e3, a different scale per column
        scale = np.logspace(-2, 3, D).astype(np.float64)
        obs = (rng.uniform(-1.0, 1.0, size=(STEPS + 1, n, D)) * scale).astype(np.float32)
        tobs = (rng.uniform(-1.0, 1.0, size=(STEPS, n, D)) * scale).astype(np.float32)
    rew = (rng.normal(0.0, 10.0, size=(STEPS, n)) + (500.0 if kind == "offset" else 0.0)).astype(np.float32)
    done = rng.random((STEPS, n)) < 0.3
    done[1] = False  # a step with no finished env
    done[2, 0] = True
    term = (done & (rng.random((STEPS, n)) < 0.5)).astype(np.uint8)
    trunc = (done & ~term.astype(bool)).astype(np.uint8)
    return obs, rew, tobs, term, trunc


def _check_stats(dev, ref, n, k, amax_obs, amax_ret, tag):
    """k: merges into the observation statistics so far (the reset and every step); the return statistics have had k - 1 (no merge at the
    reset, where the bound is 0: they must still be the initial ones).  amax_obs / amax_ret: the largest |x| that entered either statistic --
    for the returns, returns * gamma + reward BEFORE the rows of finished envs are zeroed, as the restatement forms them."""
    b, b_ret = 8 * k * n * EPS, 8 * (k - 1) * n * EPS
    assert np.all(np.abs(dev["obs_mean"] - ref.obs_rms.mean) <= b * amax_obs), (tag, "obs mean", float(np.abs(dev["obs_mean"] - ref.obs_rms.mean).max()), b * amax_obs)
    assert np.all(np.abs(dev["obs_var"] - ref.obs_rms.var) <= b * ref.obs_rms.var), (tag, "obs var", float((np.abs(dev["obs_var"] - ref.obs_rms.var) / ref.obs_rms.var).max()), b)
    assert dev["obs_count"] == ref.obs_rms.count and dev["ret_count"] == ref.ret_rms.count, tag  # (the same additions in the same order)
    assert abs(dev["ret_mean"] - float(ref.ret_rms.mean)) <= b_ret * amax_ret, (tag, "ret mean", abs(dev["ret_mean"] - float(ref.ret_rms.mean)), b_ret * amax_ret)
    assert abs(dev["ret_var"] - float(ref.ret_rms.var)) <= b_ret * float(ref.ret_rms.var), (tag, "ret var")


def _run_synthetic(n, D, kind):
    """reset + STEPS steps on one fresh handle: every output and every statistic of every step, for the checks and for the run-to-run comparison."""
    obs, rew, tobs, term, trunc = _synthetic(n, D, kind)
    h = _Handle(D, n)
    ref = R.VecNormalizeRef(n, D)
    trace = []
    try:
        d_obs = h.reset(obs[0].copy())
        r_obs = ref.reset(obs[0])
        st = h.stats()
        amax = float(np.abs(obs[0].astype(np.float64)).max())
        _check_stats(st, ref, n, 1, amax, 0.0, (n, D, kind, "reset"))
        assert np.array_equal(d_obs, R.normalize_obs_with(obs[0], st["obs_mean"], st["obs_var"], 1e-8, 10.0))
        assert np.array_equal(h.returns(), np.zeros(n))
        if n == 1:  # one row: the batch variance is exactly 0 and the batch mean the row itself, so the merge is the restatement's bit for bit
            assert np.array_equal(st["obs_mean"], ref.obs_rms.mean) and np.array_equal(st["obs_var"], ref.obs_rms.var)
        trace.append((d_obs, st))
        amax_ret = 0.0
        for t in range(STEPS):
            done = (term[t] | trunc[t]).astype(bool)
            d_obs, d_rew, d_tobs = h.step(obs[t + 1].copy(), rew[t].copy(), tobs[t].copy(), term[t], trunc[t])
            entered = ref.returns * ref.gamma + rew[t].astype(np.float64)  # what the restatement merges into ret_rms in this step
            ref.step(obs[t + 1], rew[t], done, tobs[t])
            ret_before_zero = ref.returns.copy()  # (already zeroed where done)
            assert np.array_equal(ret_before_zero[~done], entered[~done])
            st, d_ret = h.stats(), h.returns()
            amax = max(amax, float(np.abs(obs[t + 1].astype(np.float64)).max()))
            amax_ret = max(amax_ret, float(np.abs(entered).max()))
            _check_stats(st, ref, n, t + 2, amax, amax_ret, (n, D, kind, t))
            if n == 1:
                assert np.array_equal(st["obs_mean"], ref.obs_rms.mean) and np.array_equal(st["obs_var"], ref.obs_rms.var)
                assert st["ret_mean"] == float(ref.ret_rms.mean) and st["ret_var"] == float(ref.ret_rms.var)
            # outputs: the restatement evaluated with the device's own statistics, bit for bit
            assert np.array_equal(d_obs, R.normalize_obs_with(obs[t + 1], st["obs_mean"], st["obs_var"], 1e-8, 10.0)), (n, D, kind, t)
            assert np.array_equal(d_rew, R.normalize_reward_with(rew[t], st["ret_var"], 1e-8, 10.0)), (n, D, kind, t)
            assert np.array_equal(d_tobs[~done], tobs[t][~done])  # rows of unfinished envs are not touched
            if done.any():
                assert np.array_equal(d_tobs[done], R.normalize_obs_with(tobs[t][done], st["obs_mean"], st["obs_var"], 1e-8, 10.0)), (n, D, kind, t)
            # returns: returns * gamma + reward in float64 (the same two operations as the restatement), zero exactly where done
            assert np.array_equal(d_ret, ret_before_zero) and np.array_equal(d_ret == 0.0, done | (ret_before_zero == 0.0)), (n, D, kind, t)
            raw_o, raw_r = h.original()
            assert np.array_equal(raw_o, obs[t + 1]) and np.array_equal(raw_r, rew[t])
            trace.append((d_obs, d_rew, d_tobs, st, d_ret))
    finally:
        h.close()
    return trace


def _same_bits(a, b):
    if isinstance(a, dict):
        return all(_same_bits(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return all(_same_bits(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


SHAPES = [(1, 4), (7, 6), (8, 105), (64, 16), (257, 45), (1000, 172), (4096, 4)]


@pytest.mark.parametrize("kind", ["plain", "offset"])
@pytest.mark.parametrize("n,D", SHAPES + [(-1, 7), (0, 7), (1, 7)], ids=[f"{n}x{D}" for n, D in SHAPES] + ["bound-1", "bound", "bound+1"])
def test_kernel_against_restatement(n, D, kind):
    if D == 7:
        n = _bound() + n  # the one-launch bound - 1, the bound, the bound + 1
    first = _run_synthetic(n, D, kind)
    second = _run_synthetic(n, D, kind)
    assert _same_bits(tuple(first), tuple(second)), "two runs differ in some bit"


@pytest.mark.parametrize("n", [8, 300])
def test_flags_and_frozen_statistics(n):
    D = 5
    obs, rew, tobs, term, trunc = _synthetic(n, D, "plain", seed=23)
    # training = 0: nothing moves, outputs use the statistics as they stand
    h = _Handle(D, n)
    try:
        h.reset(obs[0].copy())
        h.step(obs[1].copy(), rew[0].copy(), tobs[0].copy(), term[0], trunc[0])
        before, ret_before = h.stats(), h.returns()
        d_obs, d_rew, d_tobs = h.step(obs[2].copy(), rew[1].copy(), tobs[1].copy(), term[1] | 1, trunc[1], training=False)
        after = h.stats()
        assert _same_bits(before, after)
        assert np.array_equal(d_obs, R.normalize_obs_with(obs[2], after["obs_mean"], after["obs_var"], 1e-8, 10.0))
        assert np.array_equal(d_rew, R.normalize_reward_with(rew[1], after["ret_var"], 1e-8, 10.0))
        assert np.array_equal(d_tobs, R.normalize_obs_with(tobs[1], after["obs_mean"], after["obs_var"], 1e-8, 10.0))  # every env finished
        assert np.array_equal(h.returns(), np.zeros(n)) and ret_before.any()  # step 6 happens whether or not the wrapper trains
        d_obs2 = h.reset(obs[3].copy(), training=False)
        assert _same_bits(before, h.stats()) and np.array_equal(d_obs2, R.normalize_obs_with(obs[3], after["obs_mean"], after["obs_var"], 1e-8, 10.0))
    finally:
        h.close()
    # norm_reward off: rewards pass through, the return statistics still move; norm_obs off: observations pass through, their statistics stay
    for flags in (dict(norm_reward=False), dict(norm_obs=False)):
        h, ref = _Handle(D, n, **flags), R.VecNormalizeRef(n, D, **flags)
        try:
            h.reset(obs[0].copy())
            ref.reset(obs[0])
            for t in range(3):
                done = (term[t] | trunc[t]).astype(bool)
                d_obs, d_rew, d_tobs = h.step(obs[t + 1].copy(), rew[t].copy(), tobs[t].copy(), term[t], trunc[t])
                ref.step(obs[t + 1], rew[t], done, tobs[t])
                st = h.stats()
                if "norm_reward" in flags:
                    assert np.array_equal(d_rew, rew[t]) and st["ret_count"] == pytest.approx(1e-4 + (t + 1) * n, rel=1e-12)
                    assert abs(st["ret_var"] - float(ref.ret_rms.var)) <= 8 * (t + 1) * n * EPS * float(ref.ret_rms.var)
                else:
                    assert np.array_equal(d_obs, obs[t + 1]) and np.array_equal(d_tobs, tobs[t]) and st["obs_count"] == 1e-4
                    assert np.array_equal(st["obs_var"], np.ones(D)) and np.array_equal(d_rew, R.normalize_reward_with(rew[t], st["ret_var"], 1e-8, 10.0))
        finally:
            h.close()


def test_stateless_helpers_and_set_stats():
    from three_mlagents_amd import _lib

    D, n = 7, 13
    h = _Handle(D, 4, clip_obs=5.0, clip_reward=2.0)
    rng = np.random.default_rng(2)
    mean, var = rng.normal(0, 100, D), rng.uniform(0.1, 50, D)
    sc = np.array([123.0, -4.0, 9.5, 77.0])
    p = _lib.ptr
    try:
        _lib.check(h.L.tma_vecnorm_set_stats(h.h, p(mean), p(var), p(sc), _lib.stream_ptr()))
        st = h.stats()
        assert np.array_equal(st["obs_mean"], mean) and np.array_equal(st["obs_var"], var) and [st["obs_count"], st["ret_mean"], st["ret_var"], st["ret_count"]] == list(sc)
        x = (rng.normal(0, 150, (n, D))).astype(np.float32)
        r = (rng.normal(0, 5, n)).astype(np.float32)
        tx, tr = torch.from_numpy(x).to(_dev()), torch.from_numpy(r).to(_dev())
        ox, orr = torch.empty_like(tx), torch.empty_like(tr)
        _lib.check(h.L.tma_vecnorm_normalize_obs(h.h, p(tx), p(ox), n, _lib.stream_ptr()))
        assert np.array_equal(ox.cpu().numpy(), R.normalize_obs_with(x, mean, var, 1e-8, 5.0))
        _lib.check(h.L.tma_vecnorm_unnormalize_obs(h.h, p(tx), p(ox), n, _lib.stream_ptr()))
        assert np.array_equal(ox.cpu().numpy(), (x.astype(np.float64) * np.sqrt(var + 1e-8) + mean).astype(np.float32))
        _lib.check(h.L.tma_vecnorm_normalize_reward(h.h, p(tr), p(orr), n, _lib.stream_ptr()))
        assert np.array_equal(orr.cpu().numpy(), R.normalize_reward_with(r, 9.5, 1e-8, 2.0))
        _lib.check(h.L.tma_vecnorm_unnormalize_reward(h.h, p(tr), p(orr), n, _lib.stream_ptr()))
        assert np.array_equal(orr.cpu().numpy(), (r.astype(np.float64) * np.sqrt(9.5 + 1e-8)).astype(np.float32))
    finally:
        h.close()


# ---- the wrapper on real envs ----------------------------------------------------------------------------------------------------------

def _within_one_ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))))


@pytest.mark.parametrize("task", ["ball3d", "basic"])
def test_wrapper_on_real_envs(task, tmp_path):
    from three_mlagents_amd.vec_env import HipVecEnv
    from three_mlagents_amd.vec_normalize import VecNormalize, sync_envs_normalization

    N, T = 8, 64
    plain, venv = HipVecEnv(task, N, seed=5), VecNormalize(HipVecEnv(task, N, seed=5))
    D = plain.engine.obs_dim
    tape = np.random.default_rng(4).integers(0, plain.engine.num_actions, size=(T, N))
    ref = R.VecNormalizeRef(N, D)
    raw = plain.reset()
    assert _within_one_ulp(venv.reset(), ref.reset(raw)) and np.array_equal(venv.get_original_obs(), raw)
    amax, amax_ret, n_terminal = float(np.abs(raw).max()), 0.0, 0
    for t in range(T):
        raw, rew, dones, infos = plain.step(tape[t])
        amax_ret = max(amax_ret, float(np.abs(ref.returns * ref.gamma + rew.astype(np.float64)).max()))  # the returns this step merges, before zeroing
        obs_n, rew_n, dones_n, infos_n = venv.step(tape[t])
        tobs = np.zeros((N, D), np.float32)
        for i in np.nonzero(dones)[0]:
            tobs[i] = infos[i]["terminal_observation"]
        r_obs, r_rew, r_tobs = ref.step(raw, rew, dones, tobs)
        assert np.array_equal(dones, dones_n) and [i["TimeLimit.truncated"] for i in infos] == [i["TimeLimit.truncated"] for i in infos_n], t
        assert _within_one_ulp(obs_n, r_obs) and _within_one_ulp(rew_n, r_rew), t
        for i in np.nonzero(dones)[0]:
            n_terminal += 1
            assert _within_one_ulp(infos_n[i]["terminal_observation"], r_tobs[i]), (t, i)
            assert infos_n[i]["episode"]["r"] == infos[i]["episode"]["r"] and infos_n[i]["episode"]["l"] == infos[i]["episode"]["l"]  # Monitor stays raw
        assert np.array_equal(venv.get_original_obs(), raw) and np.array_equal(venv.get_original_reward(), rew), t
        amax = max(amax, float(np.abs(raw).max()))
        b, b_ret = 8 * (t + 2) * N * EPS, 8 * (t + 1) * N * EPS  # (the observation statistics have had one merge more: the reset)
        assert np.all(np.abs(venv.obs_rms.mean - ref.obs_rms.mean) <= b * amax) and np.all(np.abs(venv.obs_rms.var - ref.obs_rms.var) <= b * ref.obs_rms.var), t
        assert abs(venv.ret_rms.var - float(ref.ret_rms.var)) <= b_ret * float(ref.ret_rms.var) and venv.obs_rms.count == ref.obs_rms.count, t
        assert abs(venv.ret_rms.mean - float(ref.ret_rms.mean)) <= b_ret * amax_ret and venv.ret_rms.count == ref.ret_rms.count, t
    assert n_terminal > 0 or task != "basic"  # basic truncates at 50 steps: terminal observations occurred
    assert venv.obs_rms.mean.dtype == np.float64 and venv.obs_rms.mean.shape == (D,)
    # normalize_obs / unnormalize_obs with the current statistics
    st = venv.get_stats()
    assert np.array_equal(venv.normalize_obs(raw), R.normalize_obs_with(raw, st["obs_mean"], st["obs_var"], 1e-8, 10.0))
    assert np.allclose(venv.unnormalize_obs(venv.normalize_obs(raw)), raw, rtol=1e-5, atol=1e-5)
    # save / load round-trips the statistics bit for bit; sync copies them
    path = tmp_path / "vecnormalize.npz"
    venv.save(path)
    other = VecNormalize.load(path, HipVecEnv(task, N, seed=9))
    assert _same_bits(st, other.get_stats()) and (other.clip_obs, other.clip_reward, other.gamma, other.epsilon, other.norm_obs, other.norm_reward) == (10.0, 10.0, 0.99, 1e-8, True, True)
    third = VecNormalize(HipVecEnv(task, 4, seed=2), training=False)
    assert not _same_bits(st, third.get_stats())
    sync_envs_normalization(venv, third)
    assert _same_bits(st, third.get_stats())
    for e in (plain, venv, other, third):
        e.close()


def test_wrapper_carries_every_attribute_of_the_vector():
    """VecNormalize shares the wrapped vector's engine instead of calling HipVecEnv.__init__: whatever that (or make_vector_env) sets on a vector
    must exist on the wrapper too."""
    from three_mlagents_amd.harness import make_vector_env
    from three_mlagents_amd.vec_normalize import VecNormalize

    vec = make_vector_env("basic", n_envs=4, seed=1, monitor_dir="somewhere")
    venv = VecNormalize(vec)
    missing = set(vars(vec)) - set(vars(venv))
    assert not missing, missing
    assert venv.engine is vec.engine and venv.monitor_dir == "somewhere" and venv.num_envs == 4 and venv.observation_space is vec.observation_space
    venv.close()


# ---- the native driver equals the stepped composition -----------------------------------------------------------------------------------

@pytest.mark.parametrize("task,N,T,hidden,slots", [("ball3d", 8, 16, 256, None), ("gridworld", 64, 12, 64, None), ("basic", 8, 60, 64, None), ("basic", 8, 60, 64, 1),
                                                   ("basic", 64, 60, 64, None), ("basic", 64, 60, 64, 1), ("ant", 16, 8, 64, None)])
def test_native_driver_equals_stepped_composition(task, N, T, hidden, slots):
    from three_mlagents_amd import _lib
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv
    from three_mlagents_amd.vec_normalize import VecNormalize

    env = VecNormalize(HipVecEnv(task, N, seed=3, ring_depth=16))
    model = PPO("MlpPolicy", env, n_steps=T, batch_size=256, n_epochs=1, seed=3, policy_kwargs={"net_arch": [hidden, hidden]})
    if slots is not None:  # one terminal-observation slot: the driver's other branch (the bootstrap rides in the next step's forward launch)
        model._rb.terminal_obs_slots = slots
    else:
        assert model._rb.terminal_obs_slots > 1
    assert model.collect_rollouts()
    b = {k: v.clone() for k, v in model.buf.items()}
    assert all(torch.isfinite(b[k]).all() for k in ("values", "log_probs", "rewards", "obs"))
    assert float(b["obs"].abs().max()) <= 10.0 and float(b["rewards"].abs().max()) <= 10.0 + 0.99 * float(b["values"].abs().max()) + 1.0
    env2 = VecNormalize(HipVecEnv(task, N, seed=3, ring_depth=16))
    obs = env2.reset_device().clone()
    assert torch.equal(obs, b["obs"][0])
    for t in range(T):
        a, v, lp = model.policy.act(obs, rng_seed=3, rng_step=t, env_offset=0)
        out = env2.step_device(a)
        rew = out["rew"][0].clone()
        _lib.check(_lib.lib().tma_policy_bootstrap(_lib.ptr(model.policy.params), C.byref(model.policy.dims), _lib.ptr(out["term_obs"][0]),
                                                   _lib.ptr(out["trunc"][0]), N, 0.99, _lib.ptr(rew), _lib.stream_ptr()))
        assert torch.equal(a, b["actions"][t]) and torch.equal(v, b["values"][t]) and torch.equal(lp, b["log_probs"][t]), t
        assert torch.equal(rew, b["rewards"][t]) and torch.equal(out["term"][0], b["terminated"][t]) and torch.equal(out["trunc"][0], b["truncated"][t]), t
        obs = out["obs"][0].clone()
        assert torch.equal(obs, b["obs"][t + 1]), t
    assert torch.equal(model.policy.predict_values(obs), b["last_values"])
    assert int((b["terminated"] | b["truncated"]).sum()) > 0 or task not in ("basic", "gridworld")  # terminal observations occurred
    if task == "basic" and N >= 40:  # (eight envs of an untrained policy mostly reach a goal before the 50-step limit; sixty-four do not all)
        assert int(b["truncated"].sum()) > 0  # truncations inside the window: the timeout bootstrap read normalised terminal observations
    st = env.get_stats()
    assert _same_bits(st, env2.get_stats()) and np.array_equal(env.get_returns(), env2.get_returns())
    assert st["obs_count"] == env2.obs_rms.count and abs(st["obs_count"] - (1e-4 + N * (T + 1))) < 1e-6
    # training = 0: a further rollout leaves every bit of the statistics where it was
    env.training = False
    assert model.collect_rollouts()
    torch.cuda.synchronize()
    assert _same_bits(st, env.get_stats())
    env.close()
    env2.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------

def _dispatch_ids():
    from three_mlagents_amd import _lib

    f, g, o = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    _lib.lib().tma_debug_last_dispatch(C.byref(f), C.byref(g), C.byref(o))
    return f.value, g.value, o.value, _lib.lib().tma_debug_last_rollout_waves()


def _plain_iteration():
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv

    env = HipVecEnv("ball3d", 8, seed=1)
    model = PPO("MlpPolicy", env, n_steps=64, batch_size=256, seed=1)
    model.collect_rollouts()
    ids_roll = _dispatch_ids()
    model.train()
    ids = (ids_roll, _dispatch_ids())
    params = model.policy.params.clone()
    env.close()
    return ids, params


def test_ppo_end_to_end_and_plain_env_unchanged():
    from three_mlagents_amd.evaluation import evaluate_policy
    from three_mlagents_amd.harness import make_vector_env
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv
    from three_mlagents_amd.vec_normalize import VecNormalize, sync_envs_normalization

    ids_before, params_before = _plain_iteration()
    assert ids_before[0][0] != 0  # (a forward kernel was recorded; the update's ids may be NONE where a persistent epoch kernel takes the shape)
    env = VecNormalize(make_vector_env("ball3d", n_envs=8, seed=1))
    model = PPO("MlpPolicy", env, n_steps=64, batch_size=256, seed=1)
    replay = HipVecEnv("ball3d", 8, seed=1)  # the same envs driven by the actions the model took: the RAW episode returns
    replay.engine.reset()
    episodes = 0
    for it in range(2):
        model.learn(8 * 64, reset_num_timesteps=(it == 0))
        s_ret, cnt = 0.0, 0
        for t in range(64):
            out = replay.engine.step(model.buf["actions"][t])
            done = (out["term"][0] | out["trunc"][0]).bool()
            s_ret += float(out["ep_ret"][0][done].sum())
            cnt += int(done.sum())
        logged = model.logger_values["rollout/ep_rew_mean"]
        assert model.logger_values["rollout/episodes"] == cnt
        assert (np.isnan(logged) and cnt == 0) or logged == pytest.approx(s_ret / cnt, rel=1e-12), (it, logged, s_ret, cnt)
        episodes += cnt
    assert episodes > 0
    assert bool(torch.isfinite(model.policy.params).all())
    count = 1e-4
    for _ in range(1 + 2 * 64):  # the reset and 2 x 64 steps of 8 rows, added one batch at a time
        count += 8.0
    assert env.obs_rms.count == count == pytest.approx(1e-4 + 8 * (1 + 2 * 64), rel=1e-12) and env.ret_rms.count == pytest.approx(1e-4 + 8 * 2 * 64, rel=1e-12)
    assert float(model.buf["obs"].abs().max()) <= env.clip_obs
    # predict does not normalise: the caller does
    act, _ = model.predict(env.normalize_obs(env.get_original_obs()), deterministic=True)
    assert act.shape == (8,)
    # evaluation on a synced, frozen wrapper leaves its statistics alone
    eval_env = VecNormalize(HipVecEnv("ball3d", 8, seed=77), training=False)
    sync_envs_normalization(env, eval_env)
    st = eval_env.get_stats()
    assert _same_bits(st, env.get_stats())
    mean, std = evaluate_policy(model, eval_env, n_eval_episodes=8)
    assert np.isfinite(mean) and _same_bits(st, eval_env.get_stats())
    env.close()
    eval_env.close()
    replay.close()
    # a plain HipVecEnv launches what it launched before a wrapper existed in the process, and computes the same bits
    ids_after, params_after = _plain_iteration()
    assert ids_after == ids_before and torch.equal(params_after, params_before)


def test_refusals():
    from three_mlagents_amd.a2c import A2C
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv
    from three_mlagents_amd.vec_normalize import VecNormalize

    env = VecNormalize(HipVecEnv("ball3d", 8, seed=1))
    with pytest.raises(ValueError, match="A2C"):
        A2C("MlpPolicy", env)
    model = PPO("MlpPolicy", env, n_steps=16, batch_size=128, _init_setup_model=False)
    model.world_size = 2  # a faked data-parallel job
    with pytest.raises(ValueError, match="world_size"):
        model._setup_model()
    with pytest.raises(ValueError):
        VecNormalize(env)
    with pytest.raises(ValueError):
        env.step_device(torch.zeros(2 * 8, dtype=torch.int32, device=_dev()), n_steps=2)
    env.close()


# ---- harness ----------------------------------------------------------------------------------------------------------------------------

def test_train_task_with_normalize(tmp_path, monkeypatch):
    from three_mlagents_amd import harness
    from three_mlagents_amd.vec_normalize import VecNormalize

    monkeypatch.chdir(tmp_path)
    res = harness.train_task(harness.TrainConfig("ball3d", total_timesteps=2048, normalize=True, verbose=0))
    meta = json.load(open(res.metadata_path))
    stats_path = res.model_path[:-len(".zip")] + ".vecnormalize.npz"
    assert meta["normalize"] is True and meta["config"]["normalize"] is True and meta["vecnormalize_path"] == stats_path
    assert os.path.isfile(stats_path) and os.path.dirname(stats_path) == os.path.dirname(res.model_path)
    with np.load(stats_path) as z:
        assert float(z["obs_count"]) > 2048 and z["obs_mean"].shape == (6,) and z["obs_mean"].dtype == np.float64
    loaded = []
    real_load = VecNormalize.load.__func__
    monkeypatch.setattr(VecNormalize, "load", classmethod(lambda cls, path, venv: loaded.append(str(path)) or real_load(cls, path, venv)))
    ev = harness.evaluate_model("ball3d", res.model_filename, episodes=4)
    assert loaded == [stats_path] and ev["episodes"] == 4 and np.isfinite(ev["mean_reward"])
    # the default: no such file, no such key
    res2 = harness.train_task(harness.TrainConfig("ball3d", total_timesteps=2048, verbose=0))
    meta2 = json.load(open(res2.metadata_path))
    assert "normalize" not in meta2 and meta2["config"]["normalize"] is False
    assert not os.path.exists(res2.model_path[:-len(".zip")] + ".vecnormalize.npz")
    assert [p for p in os.listdir(os.path.dirname(res2.model_path)) if p.endswith(".npz")] == [os.path.basename(stats_path)]
    loaded.clear()
    harness.evaluate_model("ball3d", res2.model_filename, episodes=4)
    assert loaded == []
