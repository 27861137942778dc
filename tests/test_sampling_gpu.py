"""Every action sampler draws from the policy's distribution.  Exploration noise is matched to the reference in distribution only (torch's
generator is not reproduced), so the distribution is the contract; this file asserts it for every forward family -- the Gumbel-max sampler
of the H = 64 kernel, the inverse-CDF samplers of the generic and column-parallel kernels, Box-Muller on libm (generic) and on the hardware
units (column-parallel, f32 and bf16) -- and once end to end through the fused rollout.

SAMPLING_CASES is importable without a GPU; every case names the TMA_DISPATCH_FWD_* id it expects and asserts it through
tma_debug_last_dispatch.  tests/test_sampling_cpu.py checks that every FWD id has a case, that the statistics reject emulated defective
samplers at the sizes used here and accept numpy's own sampler, and the bf16 precondition of the per-row cases.

One significance level: the family-wise level _sampling_stats.FAMILY_ALPHA (1e-6), split Bonferroni over ALL p-value assertions of this file;
the count, N_PVALUES, comes from the case table below.  Seeds are fixed, so the outcome is deterministic: a correct sampler fails this file
by chance once in a million choices of the seeds.  A seed is never changed to make a case pass.  Every p-value is recorded with
record_property."""
import numpy as np
import pytest
import torch

import _sampling_stats as S
from oracle import sb3_ref
from test_policy_dispatch_gpu import _FWD_BF_SHAPES, _FWD_SHAPES, _emulated_forward64, _last_dispatch, _name, expected_value

pytestmark = pytest.mark.gpu

DRAWS = 1 << 20  # draws (Discrete) or N(0, 1) variates (Box) per case: tests/test_sampling_cpu.py shows every mutant rejected at this size
# the peaked distribution of 2a: its rare cells (probability e^-12 each) expect 6 draws apiece at 2^20.  Against a softmax at temperature 1.05
# (rare mass x 1.77) the smallest p-value of the kind's assertions, in tests/test_sampling_cpu.py's emulation, is 6e-4 / 2e-7 / 8e-13 at
# 2^20 / 2^21 / 2^22 draws for A = 5 (the Poisson test of the rare total alone: 9e-12 at 2^22) and 5e-18 at 2^20 for A = 16: hence 2^22, the cap,
# below 16 actions.  NOT seen by this kind under the cap: that mutant at A = 2 (3e-7 at 2^22); borderline at A = 3 (2.7e-10 against the
# threshold's 6.4e-10).  The random kind of the same cases sees it.
def draws_for(c, kind):
    return 1 << 22 if kind == "peaked" and c[2] < 16 else DRAWS


STREAM_DRAWS = 1 << 18  # per seed in the stream tests
N_ROWS = 4096 + 13  # a ragged tail behind 128 full 32-row groups / 256 full 16-row tiles
SEED = 3

# (D, H, A, continuous, dtype, expected dispatch id, rows per call).  The shapes of test_policy_dispatch_gpu.py's forward tables, then what they lack:
# Discrete A in {2, 5, 16} on the H = 64 and the generic kernel, Box A in {1, 8, 20, 32} on a column-parallel f32, a bf16 and the generic kernel
# (columns >= 16 sit in the second accumulator tile, with stream keys of their own), and the generic kernel at four and two waves per block.
_EXTRA = [
    (4, 64, 2, False, "f32", "FWD_H64", N_ROWS),
    (21, 64, 2, False, "f32", "FWD_GENERIC_W1", N_ROWS), (21, 64, 5, False, "f32", "FWD_GENERIC_W1", N_ROWS), (21, 64, 16, False, "f32", "FWD_GENERIC_W1", N_ROWS),
    (8, 128, 8, True, "f32", "FWD_F32_NTW2_BOX", N_ROWS), (8, 128, 20, True, "f32", "FWD_F32_NTW2_BOX", N_ROWS),
    (8, 128, 20, True, "bf16", "FWD_BF16_NTW2_BOX", N_ROWS), (8, 256, 1, True, "bf16", "FWD_BF16_NTW4_BOX", N_ROWS),
    (6, 64, 1, True, "f32", "FWD_GENERIC_W1", N_ROWS), (6, 64, 8, True, "f32", "FWD_GENERIC_W1", N_ROWS), (6, 64, 20, True, "f32", "FWD_GENERIC_W1", N_ROWS),
    (6, 64, 32, True, "f32", "FWD_GENERIC_W1", N_ROWS),
    (4, 64, 2, True, "f32", "FWD_GENERIC_W4", 16384 + 13), (200, 64, 3, False, "f32", "FWD_GENERIC_W2", 16384 + 13),
]
SAMPLING_CASES = ([(D, H, A, cont, "f32", ident, N_ROWS) for (D, H, A, cont, ident) in _FWD_SHAPES]
                  + [(D, H, A, cont, "bf16", ident, N_ROWS) for (D, H, A, cont, ident) in _FWD_BF_SHAPES] + _EXTRA)


def case_id(c):
    D, H, A, cont, dtype, ident, n = c
    return f"{D}x{H}x{A}{'C' if cont else 'D'}-{dtype}-{n}"


def env_offset(c):
    """nonzero in every second case"""
    i = SAMPLING_CASES.index(c)
    return 0 if i % 2 == 0 else 100003 + 64 * i + 5


def steps(c, draws=DRAWS):
    D, H, A, cont, dtype, ident, n = c
    return max(4, draws // (n * (A if cont else 1)))


KINDS = ("random", "peaked", "zeros")


def _assertions():
    """(test, case id, kind) -> the names of its p-values: the whole file's p-value assertions, from the case table"""
    out = {}
    for c in SAMPLING_CASES:
        D, H, A, cont, dtype, ident, n = c
        cid = case_id(c)
        if cont:
            out[("known", cid, "box")] = S.normal_names(A)
            out[("rows", cid, "")] = S.normal_names(A)
        else:
            for kind in KINDS:
                out[("known", cid, kind)] = S.categorical_shared_names(kind == "peaked")
            out[("rows", cid, "")] = S.categorical_rows_names()
        out[("streams", cid, "")] = ["seed_" + x for x in S.independence_names(cont)] + ["step_" + x for x in S.independence_names(cont)]
    out[("rollout", "crawler", "")] = S.independence_names(True) + ["noise_" + x for x in S.normal_names(20)]
    return out


ASSERTIONS = _assertions()
N_PVALUES = sum(len(v) for v in ASSERTIONS.values())
ALPHA = S.FAMILY_ALPHA / N_PVALUES


def check_pvalues(key, pvals, record_property):
    assert list(pvals) == ASSERTIONS[key], (list(pvals), ASSERTIONS[key])  # (the Bonferroni split counted exactly these)
    for k, v in pvals.items():
        record_property(f"p_{k}", repr(v))
    record_property("p_min", repr(min(pvals.values())))
    print(key, "alpha", ALPHA, {k: float(f"{v:.3g}") for k, v in pvals.items()})
    bad = {k: v for k, v in pvals.items() if not v >= ALPHA}
    assert not bad, (key, bad, ALPHA)


# ---- distributions of 2a -----------------------------------------------------------------------------------------------------------------
def known_logits(A, kind):
    """float32 logits loaded as action_net.bias under an all-zero action_net.weight"""
    if kind == "random":
        return (2.0 * torch.randn(A, generator=torch.Generator().manual_seed(100 + A))).float()
    if kind == "peaked":  # one logit 12 above the rest: every other action is a rare cell
        x = torch.full((A,), -12.0)
        x[A // 2] = 0.0
        return x
    if kind == "zeros":  # exp(-200 - max) == 0 in float32: the first, a middle and the LAST action have probability exactly zero
        x = torch.linspace(-1.0, 1.0, A) if A > 1 else torch.zeros(1)
        x[A - 1] = -200.0  # (A = 2, 3: only the last fits beside a support of one / two; A = 2 is p = [1, 0], carried by the exact assertion alone)
        if A >= 4:
            x[0] = -200.0
        if A >= 5:
            x[A // 2] = -200.0
        return x.float()
    if kind == "ties":  # [1, 3, 3, 0, 3] repeated / cut to A entries: the first of several maxima is index 1; A = 2: [3, 3], index 0
        return torch.tensor(([1.0, 3.0, 3.0, 0.0, 3.0] * 4)[:A]) if A >= 3 else torch.full((A,), 3.0)
    raise KeyError(kind)


BOX_LOG_STD = (-2.0, 0.0, 1.0)


def box_known(A):
    """(means = action_net.bias, log_std cycling over BOX_LOG_STD)"""
    mean = (1.5 * torch.randn(A, generator=torch.Generator().manual_seed(200 + A))).float()
    return mean, torch.tensor([BOX_LOG_STD[j % 3] for j in range(A)])


def cpu_state_dict(D, H, A, cont, seed=5):
    """the state dict test_ppo_gpu._policy / test_bf16_gpu._policies load, formed without a device by the same two functions
    (test_sampling_cpu.py needs the per-row distributions); test_per_row_distribution asserts it equal, bit for bit"""
    from test_ppo_gpu import _nontrivial_heads
    from three_mlagents_amd.ppo import orthogonal_init

    return _nontrivial_heads(orthogonal_init(D, H, A, cont, seed), A, cont, seed)


def row_observations(c):
    D, H, A, cont, dtype, ident, n = c
    return torch.randn(n, D, generator=torch.Generator().manual_seed(1000 + D))


def row_reference64(c, sd, obs):
    """float64 head outputs [n, A] of the rows: sb3_ref.forward on .double() copies, or the float64 emulation of the bf16 rounding points"""
    with torch.no_grad():
        if c[4] == "bf16":
            return _emulated_forward64(sd, obs)[0]
        return sb3_ref.forward({k: v.double() for k, v in sd.items()}, obs.double())[0]


# ---- device helpers ---------------------------------------------------------------------------------------------------------------------
def _policy(c):
    from test_policy_dispatch_gpu import _policy as make

    D, H, A, cont, dtype, ident, n = c
    return make(D, H, A, cont, dtype)


def _zero_weight_policy(c, bias, log_std=None):
    pol, sd = _policy(c)
    sd = dict(sd)
    sd["action_net.weight"] = torch.zeros_like(sd["action_net.weight"])
    sd["action_net.bias"] = bias.clone()
    if log_std is not None:
        sd["log_std"] = log_std.clone()
    pol.load_state_dict(sd)
    return pol


def _check_id(c):
    got = _last_dispatch()[0]
    assert got == expected_value(c[5]), (c[5], _name(got))


def _draw(pol, obs_d, c, n_steps, seed=SEED, step0=0, offset=None):
    """actions of n_steps consecutive rng_steps, stacked [n_steps, n(, A)], as numpy"""
    o = env_offset(c) if offset is None else offset
    out = [pol.act(obs_d, rng_seed=seed, rng_step=step0 + t, env_offset=o)[0] for t in range(n_steps)]
    _check_id(c)
    return torch.stack(out).cpu().numpy()


def _cases(pred=lambda c: True):
    return [pytest.param(c, id=case_id(c)) for c in SAMPLING_CASES if pred(c)]


def _discrete_premise(pol, obs_d, logits, c):
    """the kernel's distribution IS softmax(bias): evaluate_actions against the float64 log_softmax, 1e-6 absolute.  Cells of logit -200
    (log-probability near -201, where neighbouring float32 values are 1.5e-5 apart) cannot be held to 1e-6 by any float32 output: they get the
    1e-6 plus one float32 rounding of their own magnitude, and their probability, exp of it, must be exactly zero in float32."""
    A, n = c[2], c[6]
    ref = torch.log_softmax(logits.double(), dim=0)
    acts = (torch.arange(n) % A).to(torch.int32)
    _, lp, _ = pol.evaluate_actions(obs_d, acts.cuda())
    _check_id(c)
    err = (lp.cpu().double() - ref[acts.long()]).abs()
    tol = torch.where(ref[acts.long()] < -100.0, 1e-6 + 2.0 ** -24 * ref[acts.long()].abs(), torch.full_like(err, 1e-6))
    assert bool((err <= tol).all()), (float(err.max()), ref)
    assert bool((torch.exp(lp.cpu())[ref[acts.long()] < -100.0] == 0.0).all())
    return float(err.max())


# ---- 2a: known distribution, isolated from the forward pass ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", _cases(lambda c: not c[3]))
def test_discrete_known_distribution(c, kind, record_property):
    """action_net.weight = 0: every row's logits are action_net.bias exactly, in every dtype, whatever the observation.
    zeros: the actions of probability exactly zero must NEVER be drawn, over the draws made.  The inverse-CDF samplers clamp with
    min(count, A - 1), and the float32 prefix sum of e / s can end below 1: a uniform above it lands on the last action even where its
    probability is zero.  The draws of this case may or may not contain such a uniform, so a pass does NOT prove the clamp safe."""
    D, H, A, cont, dtype, ident, n = c
    logits = known_logits(A, kind)
    pol = _zero_weight_policy(c, logits)
    obs_d = row_observations(c).cuda()
    record_property("premise_err", repr(_discrete_premise(pol, obs_d, logits, c)))
    a = _draw(pol, obs_d, c, steps(c, draws_for(c, kind)))
    assert a.min() >= 0 and a.max() < A
    p = torch.softmax(logits.double(), dim=0).numpy()
    if kind == "zeros":
        never = np.flatnonzero(logits.numpy() < -100.0)
        drawn = {int(k): int((a == k).sum()) for k in never}
        assert not any(drawn.values()), f"actions of probability zero were drawn: {drawn}"
        p = np.where(logits.numpy() < -100.0, 0.0, p)
        p = p / p.sum()
    check_pvalues(("known", case_id(c), kind), S.categorical_shared(a, p, peaked=kind == "peaked"), record_property)


@pytest.mark.parametrize("c", _cases(lambda c: not c[3]))
def test_discrete_ties_take_the_first_maximum(c):
    """deterministic=True on exact ties returns the first maximum on every row (SB3's argmax)"""
    logits = known_logits(c[2], "ties")
    pol = _zero_weight_policy(c, logits)
    a, _, _ = pol.act(row_observations(c).cuda(), deterministic=True)
    _check_id(c)
    first = int(torch.nonzero(logits == logits.max())[0])
    assert int((logits == logits.max()).sum()) >= 2 and first == (1 if c[2] >= 3 else 0)
    assert bool((a.cpu() == first).all()), torch.bincount(a.cpu().long(), minlength=c[2])


@pytest.mark.parametrize("c", _cases(lambda c: c[3]))
def test_box_known_distribution(c, record_property):
    """action_net.weight = 0: the mean of every row is action_net.bias exactly (asserted: deterministic act returns it bit for bit), so
    z = (a - bias) / exp(log_std), in float64, is the sampler's noise: N(0, 1)"""
    D, H, A, cont, dtype, ident, n = c
    mean, log_std = box_known(A)
    pol = _zero_weight_policy(c, mean, log_std)
    obs_d = row_observations(c).cuda()
    a_det, _, _ = pol.act(obs_d, deterministic=True)
    _check_id(c)
    assert torch.equal(a_det.cpu(), mean.expand(n, A))
    a = _draw(pol, obs_d, c, steps(c))
    z = (a.astype(np.float64) - mean.double().numpy()) / np.exp(log_std.double().numpy())
    check_pvalues(("known", case_id(c), "box"), S.normal(z), record_property)


# ---- 2b: per-row distributions, real weights -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _cases())
def test_per_row_distribution(c, record_property):
    """non-trivial heads, 4096 + 13 distinct observation rows (the same at every step); the reference distribution of each row comes from
    float64 (never from the kernel's outputs).  A row that draws from another row's CDF, or with another row's mean, fails here."""
    D, H, A, cont, dtype, ident, n = c
    pol, sd = _policy(c)
    sd_cpu = cpu_state_dict(D, H, A, cont)
    assert all(torch.equal(sd[k], sd_cpu[k]) for k in sd) and set(sd) == set(sd_cpu)
    obs = row_observations(c)
    out64 = row_reference64(c, sd, obs)
    a = _draw(pol, obs.cuda(), c, steps(c))
    if cont:
        z = (a.astype(np.float64) - out64.numpy()) / np.exp(sd["log_std"].double().numpy())
        pvals = S.normal(z)
    else:
        pvals = S.categorical_rows(a, torch.softmax(out64, dim=1).numpy())
    check_pvalues(("rows", case_id(c), ""), pvals, record_property)


# ---- 2c: streams ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _cases())
def test_streams(c, record_property):
    """counter-based: a draw depends on (seed, global env, step) only -- bit-equal whether the env is reached by row or by env_offset -- and
    draws of seeds s / s + 1 and of steps t / t + 1 are independent.  Known distribution (zero head weight), so only the streams are tested."""
    D, H, A, cont, dtype, ident, n = c
    if cont:
        mean, log_std = box_known(A)
        pol = _zero_weight_policy(c, mean, log_std)
    else:
        logits = known_logits(A, "random")
        pol = _zero_weight_policy(c, logits)
        p = torch.softmax(logits.double(), dim=0).numpy()
    obs = row_observations(c)
    obs_d = obs.cuda()
    o = env_offset(c)
    a1 = pol.act(obs_d, rng_seed=SEED, rng_step=7, env_offset=o)[0]
    a2 = pol.act(obs_d, rng_seed=SEED, rng_step=7, env_offset=o)[0]
    a3 = pol.act(obs[37:37 + 1001].cuda(), rng_seed=SEED, rng_step=7, env_offset=o + 37)[0]
    assert torch.equal(a1, a2) and torch.equal(a1[37:37 + 1001], a3)
    T = 2 * (steps(c, STREAM_DRAWS) // 2 + 1)
    x = _draw(pol, obs_d, c, T, seed=SEED)
    y = _draw(pol, obs_d, c, T, seed=SEED + 1)
    if cont:
        sdv = np.exp(log_std.double().numpy())
        x, y = (x.astype(np.float64) - mean.double().numpy()) / sdv, (y.astype(np.float64) - mean.double().numpy()) / sdv
        pv = {"seed_" + k: v for k, v in S.independence(x, y, True).items()}
        pv.update({"step_" + k: v for k, v in S.independence(x[0::2], x[1::2], True).items()})
    else:
        pv = {"seed_" + k: v for k, v in S.independence(x, y, False, p).items()}
        pv.update({"step_" + k: v for k, v in S.independence(x[0::2], x[1::2], False, p).items()})
    check_pvalues(("streams", case_id(c), ""), pv, record_property)


def test_rollout_noise_across_rollouts(record_property):
    """two consecutive PPO.collect_rollouts() on crawler (64 envs, n_steps = 64, parameters frozen) through the fused rollout: the noise
    z = (action - float64 mean) / exp(log_std) of the second must be independent of the first's at the same (step, env, column) -- the step
    counter _rollout_counter * T + t is what keeps the two apart -- and the 163 840 variates of both together N(0, 1) (a standard deviation
    x 1.02 gives the variance test a z of 11.6 there)."""
    from three_mlagents_amd.ppo import PPO
    from three_mlagents_amd.vec_env import HipVecEnv

    T, N = 64, 64
    env = HipVecEnv("crawler", N, seed=3)
    try:
        model = PPO("MlpPolicy", env, n_steps=T, batch_size=256, n_epochs=1, seed=3, policy_kwargs={"net_arch": [256, 256]})
        sd64 = {k: v.double() for k, v in model.policy.state_dict().items()}
        zs = []
        for _ in range(2):
            assert model.collect_rollouts()
            obs = model.buf["obs"][:T].cpu().double().reshape(T * N, -1)
            with torch.no_grad():
                mean64 = sb3_ref.forward(sd64, obs)[0]
            act = model.buf["actions"][:T].cpu().double().reshape(T * N, -1)
            zs.append(((act - mean64) / torch.exp(sd64["log_std"])).numpy())
        pv = S.independence(zs[0], zs[1], True)
        # the noise of both rollouts, [2 T, N, A], against N(0, 1): what the fused kernel stored, not what `act` would have drawn
        pv.update({"noise_" + k: v for k, v in S.normal(np.concatenate(zs).reshape(2 * T, N, -1)).items()})
        check_pvalues(("rollout", "crawler", ""), pv, record_property)
    finally:
        env.close()
