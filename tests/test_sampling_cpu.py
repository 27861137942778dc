"""CPU side of the sampling tests (tests/test_sampling_gpu.py, tests/_sampling_stats.py):

 * every TMA_DISPATCH_FWD_* id of include/tma.h has a sampling case;
 * the statistics have teeth at the sizes the GPU file uses and at ITS Bonferroni threshold: numpy samplers with one realistic defect each
   (MUTANTS) fall below it in at least one assertion, numpy's own sampler of the true distribution stays above it in all;
 * the precondition of the bf16 per-row cases: a sampler drawing from the float32 emulation of the bf16 forward passes against the float64
   emulation's distribution at the case's size;
 * the minibatch permutation (tma_ppo_permutation, a host function: a 4-round Feistel network with cycle walking) stands in for
   np.random.permutation: at the headline size and at ragged ones a minibatch is no structured slice of indices, envs or steps.  Mutants: the same
   network with two rounds (restated in numpy and checked equal to the library at four), and a rotation.

Which bundle of assertions sees which mutant (each evaluated on its own, at its own draw count): 2a's shared-p statistics reject temperature,
row_pair, step_independent and last_never; 2b's per-row PIT statistics reject row_pair, step_independent, last_never and row_swap (row i drawing
from row i ^ 1's distribution: what 2b is for); the N(0, 1) statistics of 2a / 2b (the same bundle at the same size) reject sd, radians, row_pair,
step_independent, col16 and, against per-row means, row_swap.
Mutants NOT seen (NOT_SEEN below, with the figures): temperature by 2b's per-row statistics at any A, also at the cap of 2^22 draws (smallest p
1e-8 at A = 2 and 5, 1.6e-4 at A = 16, against 6.3e-10: pooled over 4109 different rows a flatter softmax moves the PIT little), so 2b stays at
2^20; temperature by the PEAKED kind of 2a at A = 2 (borderline at A = 3; draws_for in tests/test_sampling_gpu.py); the two-round Feistel
network at the two smallest permutation sizes (TWO_ROUNDS_NOT_SEEN)."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _sampling_stats as S  # noqa: E402
import test_sampling_gpu as G  # noqa: E402


def test_every_forward_id_has_a_sampling_case():
    assert not torch.cuda.is_initialized()
    text = open(os.path.join(ROOT, "include", "tma.h")).read()
    fwd = set(re.findall(r"\bTMA_DISPATCH_(FWD_[A-Z0-9_]+)\s*=", text))
    assert len(fwd) >= 16
    covered = {c[5] for c in G.SAMPLING_CASES}
    assert covered <= fwd, sorted(covered - fwd)
    assert not fwd - covered, f"forward ids without a case in tests/test_sampling_gpu.py: {sorted(fwd - covered)}"
    ids = [G.case_id(c) for c in G.SAMPLING_CASES]
    assert len(ids) == len(set(ids))
    assert sum(G.env_offset(c) != 0 for c in G.SAMPLING_CASES) == len(G.SAMPLING_CASES) // 2
    # what the forward tables of test_policy_dispatch_gpu.py lack
    have = {(c[5].startswith("FWD_H64"), c[5].startswith("FWD_GENERIC"), c[4], c[2], c[3]) for c in G.SAMPLING_CASES}
    for A in (2, 5, 16):
        assert (True, False, "f32", A, False) in have and (False, True, "f32", A, False) in have, A
    for A in (1, 8, 20, 32):
        assert (False, True, "f32", A, True) in have, A
        assert any(c[2] == A and c[3] and c[4] == "f32" and c[5].startswith("FWD_F32") for c in G.SAMPLING_CASES), A
        assert any(c[2] == A and c[3] and c[4] == "bf16" for c in G.SAMPLING_CASES), A
    # every Discrete case's tie vector holds its maximum at least twice (a vector without a tie passes under any tie-breaking rule)
    for c in G.SAMPLING_CASES:
        if not c[3]:
            t = G.known_logits(c[2], "ties")
            assert int((t == t.max()).sum()) >= 2, G.case_id(c)
    # the Bonferroni split is the table's
    assert G.N_PVALUES == sum(len(v) for v in G.ASSERTIONS.values()) and G.ALPHA == S.FAMILY_ALPHA / G.N_PVALUES
    assert all(1 << 19 <= G.steps(c) * c[6] * (c[2] if c[3] else 1) <= 1 << 22 for c in G.SAMPLING_CASES)


# ---- emulated samplers: numpy's generator, the kernels' constructions, one defect each -------------------------------------------------------
def _uniforms(rng, T, N, mutant, cols=None):
    shape = (T, N) if cols is None else (T, N, cols)
    u = rng.random(shape)
    if mutant == "row_pair":  # row i uses row (i & ~1)'s uniform
        u = u[:, np.arange(N) & ~1]
    if mutant == "step_independent":
        u = np.broadcast_to(u[:1], shape).copy()
    return u


def sample_discrete(rng, P, T, mutant=None, logits=None):
    """inverse CDF, as the generic and column-parallel kernels draw; P [N, A] float64"""
    N, A = P.shape
    if mutant == "temperature":
        x = logits / 1.05
        P = np.exp(x - x.max(axis=1, keepdims=True))
        P = P / P.sum(axis=1, keepdims=True)
    if mutant == "last_never":
        P = P.copy()
        P[:, A - 1] = 0.0
        P = P / P.sum(axis=1, keepdims=True)
    u = _uniforms(rng, T, N, mutant)
    cdf = np.cumsum(P, axis=1)
    cdf[:, -1] = 1.0
    a = np.zeros((T, N), dtype=np.int64)
    for k in range(A - 1):
        a += cdf[None, :, k] <= u
    return a


def sample_normal(rng, T, N, A, mutant=None):
    """Box-Muller from two uniforms per (step, env, column), as the kernels form it"""
    u1 = np.maximum(_uniforms(rng, T, N, mutant, A), 2.0 ** -24)
    u2 = _uniforms(rng, T, N, mutant, A)
    angle = u2 if mutant == "radians" else 2.0 * math.pi * u2  # (the hardware cosine takes revolutions: passing radians to it, or revolutions to cosf)
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(angle)
    if mutant == "sd":
        z = 1.02 * z
    if mutant == "col16":
        z[:, :, 16:] = z[:, :, :A - 16]
    return z


SHARED_MUTANTS = ("temperature", "row_pair", "step_independent", "last_never")  # against 2a's shared-p bundle
ROWS_MUTANTS = SHARED_MUTANTS + ("row_swap",)  # against 2b's per-row bundle
BOX_MUTANTS = ("sd", "radians", "row_pair", "step_independent", "col16")
# (bundle, mutant): smallest p-value at 2^20 / 2^22 draws for A = 2, 5, 16: 1.6e-3 / 1e-8, 8.7e-4 / 1e-8, 0.063 / 1.6e-4
NOT_SEEN = {("rows", "temperature")}

_ROWS = {}


def _row_logits(c):
    """float64 head outputs of a case's rows, once per case"""
    cid = G.case_id(c)
    if cid not in _ROWS:
        D, H, A, cont, dtype, ident, n = c
        _ROWS[cid] = G.row_reference64(c, G.cpu_state_dict(D, H, A, cont), G.row_observations(c)).numpy()
    return _ROWS[cid]


def _case(D, H, A, cont, dtype="f32"):
    return next(c for c in G.SAMPLING_CASES if c[:5] == (D, H, A, cont, dtype))


def _softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


_DISCRETE_MUTANT_CASES = [(4, 64, 2, False), (4, 64, 5, False), (21, 64, 16, False)]


def _swap(n):
    """row i -> row i ^ 1 (the last row of an odd count keeps itself)"""
    return np.minimum(np.arange(n) ^ 1, n - 1)


def _worst(pv):
    return min(pv.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("D,H,A,cont", _DISCRETE_MUTANT_CASES)
def test_discrete_statistics_reject_the_mutants_and_accept_numpy(D, H, A, cont, record_property):
    """shared p (the `random` logits of 2a) and per-row P (2b), EACH bundle on its own, at the case's draw count and the GPU file's threshold"""
    c = _case(D, H, A, cont)
    T, n = G.steps(c), c[6]
    logits = G.known_logits(A, "random").double().numpy()
    shared_logits = np.broadcast_to(logits, (n, A))
    rows_logits = _row_logits(c)
    P_rows = _softmax(rows_logits)
    for bundle, mutants in (("known", SHARED_MUTANTS), ("rows", ROWS_MUTANTS)):
        unseen = {}
        for mutant in (None,) + mutants:
            rng = np.random.default_rng(7)
            if bundle == "known":
                pv = S.categorical_shared(sample_discrete(rng, _softmax(shared_logits), T, mutant, shared_logits), _softmax(logits))
            elif mutant == "row_swap":
                pv = S.categorical_rows(sample_discrete(rng, P_rows[_swap(n)], T), P_rows)
            else:
                pv = S.categorical_rows(sample_discrete(rng, P_rows, T, mutant, rows_logits), P_rows)
            record_property(f"p_min_{bundle}_{mutant}", repr(_worst(pv)))
            if mutant is None:
                assert min(pv.values()) >= G.ALPHA, ("numpy's sampler of the true distribution is rejected", bundle, pv)
            elif min(pv.values()) >= G.ALPHA and (bundle, mutant) not in NOT_SEEN:
                unseen[mutant] = _worst(pv)
        assert not unseen, (bundle, unseen)


_BOX_MUTANT_CASES = [(8, 128, 1, True), (105, 256, 8, True), (8, 128, 20, True), (8, 192, 32, True)]


@pytest.mark.parametrize("D,H,A,cont", _BOX_MUTANT_CASES)
def test_normal_statistics_reject_the_mutants_and_accept_numpy(D, H, A, cont, record_property):
    c = _case(D, H, A, cont)
    T, n = G.steps(c), c[6]
    mutants = [m for m in BOX_MUTANTS if m != "col16" or A > 16]
    results = {}
    for mutant in [None] + mutants:
        results[mutant] = S.normal(sample_normal(np.random.default_rng(11), T, n, A, mutant))
        record_property(f"p_min_{mutant}", repr(min(results[mutant].items(), key=lambda kv: kv[1])))
    assert min(results[None].values()) >= G.ALPHA, ("numpy's sampler of the true distribution is rejected", results[None])
    pv = S.normal(np.random.default_rng(12).standard_normal((T, n, A)))
    assert min(pv.values()) >= G.ALPHA, pv
    unseen = [m for m in mutants if min(results[m].values()) >= G.ALPHA]
    assert not unseen, {m: min(results[m].items(), key=lambda kv: kv[1]) for m in unseen}
    # 2b: a row drawing with its neighbour's mean, z formed from its own float64 mean
    mean = _row_logits(c)
    sdv = np.exp(G.cpu_state_dict(D, H, A, cont)["log_std"].double().numpy())
    a = mean[_swap(n)] + sdv * np.random.default_rng(13).standard_normal((T, n, A))
    assert min(S.normal((a - mean) / sdv).values()) < G.ALPHA


@pytest.mark.parametrize("D,H,A", [(4, 64, 5), (4, 64, 16)])
def test_peaked_statistics_see_a_wrong_temperature(D, H, A):
    """the peaked kind of 2a at its draw count (draws_for in tests/test_sampling_gpu.py, with the sizes tried and what stays unseen)"""
    c = _case(D, H, A, False)
    n, T = c[6], G.steps(c, G.draws_for(c, "peaked"))
    logits = G.known_logits(A, "peaked").double().numpy()
    p = _softmax(logits)
    rng = np.random.default_rng(3)
    ok = S.categorical_shared(sample_discrete(rng, np.broadcast_to(p, (n, A)), T), p, peaked=True)
    assert min(ok.values()) >= G.ALPHA, ok
    x = np.broadcast_to(logits, (n, A))
    bad = S.categorical_shared(sample_discrete(rng, _softmax(x), T, "temperature", x), p, peaked=True)
    assert bad["rare_poisson"] < 1e-8 and min(bad.values()) < G.ALPHA, bad  # (temperature 1.05 raises the rare mass by e^(12 * 0.05 / 1.05) = 1.77)


def test_independence_statistics():
    """the cross tests of the stream and rollout cases see reused noise"""
    A, n = 5, G.N_ROWS
    rng = np.random.default_rng(3)
    p = _softmax(G.known_logits(A, "peaked").double().numpy())
    z1, z2 = rng.standard_normal((64, 64, 20)), rng.standard_normal((64, 64, 20))
    assert min(S.independence(z1, z2, True).values()) >= G.ALPHA
    assert all(v < G.ALPHA for v in S.independence(z1, z1 + 1e-6 * z2, True).values())
    z3 = z2.copy()
    z3[:, :, 0] = z1[:, :, 0]  # one column in twenty reuses its noise
    assert S.independence(z1, z3, True)["cross_near_equal"] < G.ALPHA
    a1, a2 = sample_discrete(rng, np.broadcast_to(p, (n, A)), 64), sample_discrete(rng, np.broadcast_to(p, (n, A)), 64)
    assert S.independence(a1, a2, False, p)["cross_joint"] >= G.ALPHA
    pr = _softmax(G.known_logits(A, "random").double().numpy())
    a1 = sample_discrete(rng, np.broadcast_to(pr, (n, A)), 64)
    assert S.independence(a1, a1, False, pr)["cross_joint"] < G.ALPHA


@pytest.mark.parametrize("c", [pytest.param(c, id=G.case_id(c)) for c in G.SAMPLING_CASES if c[4] == "bf16"])
def test_bf16_per_row_precondition(c):
    """the kernel's bf16 logits differ from the float64 emulation where a sum lands on a rounding boundary; the float32 emulation differs from it
    in the same way.  A numpy sampler that draws from the float32 emulation must pass against the float64 emulation's distribution at the case's
    size, or the case could not tell a defective sampler from that noise."""
    from test_bf16_gpu import _emulated_forward

    D, H, A, cont, dtype, ident, n = c
    sd = G.cpu_state_dict(D, H, A, cont)
    obs = G.row_observations(c)
    with torch.no_grad():
        out32 = _emulated_forward(sd, obs)[0].double().numpy()
    out64 = _row_logits(c)
    T = G.steps(c)
    rng = np.random.default_rng(5)
    if cont:
        sdv = np.exp(sd["log_std"].double().numpy())
        a = (out32 + sdv * rng.standard_normal((T, n, A))).astype(np.float32)
        pv = S.normal((a.astype(np.float64) - out64) / sdv)
    else:
        pv = S.categorical_rows(sample_discrete(rng, _softmax(out32), T), _softmax(out64))
    assert min(pv.values()) >= G.ALPHA, pv


def test_zero_probability_draws_stay_short_of_the_clamp():
    """what the `zeros` kind of 2a does NOT reach: the inverse-CDF samplers take u = (mix32(seed, env, step) >> 8) / 2^24 and clamp the count of
    c <= u with min(count, A - 1), and the float32 prefix sum of e / s may end at 1 - 2^-24 (restated below with sequential float32 sums: it
    does at A = 16).  Over the (seed, env, step) range those cases draw, the largest u is 1 - 4 * 2^-24: no tested draw has a uniform at or
    above the end of its prefix sum, so the clamp onto a zero-probability last action stays untested."""
    ends = {}
    worst = 0
    with np.errstate(over="ignore"):
        for c in G.SAMPLING_CASES:
            D, H, A, cont, dtype, ident, n = c
            if cont or ident == "FWD_H64":  # (Gumbel-max has no prefix sum)
                continue
            x = G.known_logits(A, "zeros").numpy().astype(np.float32)
            e = np.exp(x - x.max()).astype(np.float32)
            total = end = np.float32(0)
            for v in e:
                total = np.float32(total + v)
            for v in e:
                end = np.float32(end + np.float32(v / total))
            ends[A] = round((1.0 - float(end)) * 2 ** 24)
            gi = (np.arange(n, dtype=np.uint64) + G.env_offset(c)).astype(np.uint32)
            k = max(int((_mix32(G.SEED, gi, t) >> np.uint32(8)).max()) for t in range(G.steps(c, G.draws_for(c, "zeros"))))
            worst = max(worst, k)
            assert k < (1 << 24) - ends[A], (G.case_id(c), k, ends[A])
    assert worst == (1 << 24) - 4 and ends[16] == 1 and ends[5] == 0, (worst, ends)


# ---- the minibatch permutation ------------------------------------------------------------------------------------------------------------
def _mix32(seed, i, t):
    x = (np.uint32(seed) * np.uint32(0x9E3779B1)) ^ (i.astype(np.uint32) * np.uint32(0x85EBCA77)) ^ (np.uint32(t) * np.uint32(0xC2B2AE3D))
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def feistel_permutation(seed, epoch, n, rounds=4):
    """perm_index (csrc/tma_mlp.h) for j = 0 .. n - 1, with `rounds` rounds"""
    b = 2
    while (1 << b) < n:
        b += 2
    half = np.uint32(b >> 1)
    mask = np.uint32((1 << (b >> 1)) - 1)
    with np.errstate(over="ignore"):
        key = np.uint32(seed) ^ (np.uint32(epoch) * np.uint32(0x9E3779B9))
        x = np.arange(n, dtype=np.uint32)
        todo = np.arange(n)
        while todo.size:
            v = x[todo]
            L, R = v >> half, v & mask
            for rd in range(rounds):
                L, R = R, L ^ (_mix32(key, R, rd) & mask)
            v = (L << half) | R
            x[todo] = v
            todo = todo[v >= n]
    return x.astype(np.int64)


def library_permutation(seed, epoch, n):
    from three_mlagents_amd import _lib

    out = np.zeros(n, dtype=np.int64)
    _lib.check(_lib.lib().tma_ppo_permutation(seed, epoch, n, out.ctypes.data_as(C.c_void_p)))
    return out


PPO_SEED = 1
PERM_SEED = (PPO_SEED * 2654435761 + 12345) & 0xFFFFFFFF  # as PPO.train forms it
# (T, N, B): the headline rollout at the flagship minibatch and at the reference's literal one, then ragged sizes
PERM_CASES = [(1024, 4096, 131072), (1024, 4096, 256), (128, 8, 256), (20, 19, 80), (64, 100, 256)]
PERM_EPOCHS = (0, 1)
# the two-round network is NOT seen at the two smallest ragged sizes (smallest p-value 0.012 at 380 indices, 1.7e-4 at 6400: the sizes are the
# issue's, there is nothing to enlarge); the rotation is seen everywhere
TWO_ROUNDS_NOT_SEEN = {(20, 19, 80), (64, 100, 256)}
N_PERM_PVALUES = len(PERM_CASES) * (len(PERM_EPOCHS) * len(S.permutation_names()) + len(S.permutation_pair_names()))
PERM_ALPHA = S.FAMILY_ALPHA / N_PERM_PVALUES


@pytest.mark.parametrize("T,N,B", PERM_CASES)
def test_minibatch_permutation_stands_in_for_a_uniform_one(T, N, B, record_property):
    total = T * N
    perms = [library_permutation(PERM_SEED, e, total) for e in PERM_EPOCHS]
    if total <= 1 << 17:
        assert all(np.array_equal(perms[e], feistel_permutation(PERM_SEED, e, total)) for e in PERM_EPOCHS)  # (the restatement the mutant is cut from)
    pv = {}
    for e in PERM_EPOCHS:
        assert np.array_equal(np.sort(perms[e]), np.arange(total))
        pv.update({f"e{e}_{k}": v for k, v in S.permutation(perms[e], T, B).items()})
    pv.update(S.permutation_pair(perms[0], perms[1]))
    assert len(pv) == N_PERM_PVALUES // len(PERM_CASES)
    for k, v in pv.items():
        record_property(f"p_{k}", repr(v))
    bad = {k: v for k, v in pv.items() if not v >= PERM_ALPHA}
    assert not bad, (bad, PERM_ALPHA)


@pytest.mark.parametrize("T,N,B", PERM_CASES)
def test_permutation_statistics_reject_the_mutants_and_accept_numpy(T, N, B):
    total = T * N
    rng = np.random.default_rng(9)
    ref = [rng.permutation(total) for _ in PERM_EPOCHS]
    pv = {}
    for e in PERM_EPOCHS:
        pv.update({f"e{e}_{k}": v for k, v in S.permutation(ref[e], T, B).items()})
    pv.update(S.permutation_pair(ref[0], ref[1]))
    assert min(pv.values()) >= PERM_ALPHA, pv
    two = S.permutation(feistel_permutation(PERM_SEED, 0, total, rounds=2), T, B)
    assert min(two.values()) < PERM_ALPHA or (T, N, B) in TWO_ROUNDS_NOT_SEEN, two
    rot = S.permutation((np.arange(total, dtype=np.int64) + total // 3 + 1) % total, T, B)
    assert min(rot.values()) < PERM_ALPHA, rot
    assert S.permutation_pair(ref[0], ref[0])["equal_positions"] < PERM_ALPHA  # an epoch counter that does not advance
