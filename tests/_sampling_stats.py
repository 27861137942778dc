"""Statistics for tests of the action samplers and of the minibatch permutation (tests/test_sampling_gpu.py, tests/test_sampling_cpu.py).
Plain numpy; importable without a GPU.  Every test function returns p-values under the null "independent draws from the stated
distribution", by name, and for every bundle a *_names function lists those names without any data: the test files count their p-value
assertions from their case tables with it and split ONE family-wise level, FAMILY_ALPHA, Bonferroni over all of them.

Conventions: draws are arrays [T steps, N envs] (Discrete) or [T, N, A columns] (Box).  Moments under the null are the KNOWN ones (uniform:
1/2, 1/12; normal: 0, 1, 3, E z^8 = 105), never sample estimates, so every z-statistic is standard normal under the null.  Pair statistics
use disjoint pairs only, so the chi-square degrees of freedom are the plain ones."""
import math

import numpy as np

FAMILY_ALPHA = 1e-6
ENV_LAGS = (1, 2, 4, 8, 16, 32, 64)

# ---- tail functions: scipy where it is installed, torch.special otherwise -------------------------------------------------------------
try:
    from scipy import special as _sp

    def _gammaincc(a, x):
        return float(_sp.gammaincc(a, x))

    def _gammainc(a, x):
        return float(_sp.gammainc(a, x))

    def _binom_tails(k, n, p):
        return float(_sp.bdtr(k, n, p)), float(_sp.bdtrc(k - 1, n, p)) if k > 0 else 1.0
except ImportError:  # pragma: no cover
    import torch

    def _gammaincc(a, x):
        return float(torch.special.gammaincc(torch.tensor(float(a), dtype=torch.float64), torch.tensor(float(x), dtype=torch.float64)))

    def _gammainc(a, x):
        return float(torch.special.gammainc(torch.tensor(float(a), dtype=torch.float64), torch.tensor(float(x), dtype=torch.float64)))

    def _binom_tails(k, n, p):  # rare events of many trials: the Poisson limit (relative error of the tails O(p))
        return _poisson_tails(k, n * p)


def _poisson_tails(k, mu):
    """(P(X <= k), P(X >= k)) for X ~ Poisson(mu)."""
    return _gammaincc(k + 1, mu), (_gammainc(k, mu) if k > 0 else 1.0)


def _two_sided(lo, hi):
    return min(1.0, 2.0 * min(lo, hi))


def chi2_sf(stat, df):
    return _gammaincc(0.5 * df, 0.5 * stat) if df > 0 else 1.0


def normal_sf2(z):
    """two-sided tail of a standard normal statistic"""
    return math.erfc(abs(float(z)) / math.sqrt(2.0))


def poisson_p(k, mu):
    return _two_sided(*_poisson_tails(int(k), float(mu)))


def binom_p(k, n, p):
    return _two_sided(*_binom_tails(int(k), int(n), float(p)))


def kolmogorov_sf(d, n):
    """P(D_n > d), asymptotic series with Stephens' finite-n correction"""
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * d
    if lam < 0.2:
        return 1.0
    s = sum((-1) ** (k - 1) * math.exp(-2.0 * k * k * lam * lam) for k in range(1, 101))
    return min(1.0, max(0.0, 2.0 * s))


def ks_uniform(w):
    x = np.sort(np.asarray(w, dtype=np.float64).ravel())
    n = x.size
    i = np.arange(1, n + 1, dtype=np.float64)
    d = max(float((i / n - x).max()), float((x - (i - 1) / n).max()))
    return kolmogorov_sf(d, n)


def _ndtr(z):
    try:
        return _sp.ndtr(z)
    except NameError:  # pragma: no cover
        import torch

        return torch.special.ndtr(torch.from_numpy(np.ascontiguousarray(z))).numpy()


# ---- chi-square with known expectations --------------------------------------------------------------------------------------------------
def _chi2_stat(obs, exp):
    """(statistic, degrees of freedom); cells of expectation < 5 are pooled into one, which takes the smallest other cell too while it stays < 5"""
    obs, exp = np.asarray(obs, dtype=np.float64).ravel(), np.asarray(exp, dtype=np.float64).ravel()
    order = np.argsort(exp, kind="stable")
    obs, exp = obs[order], exp[order]
    k = int((exp < 5.0).sum())
    if k:
        while k < exp.size and exp[:k].sum() < 5.0:
            k += 1
        obs = np.concatenate([[obs[:k].sum()], obs[k:]])
        exp = np.concatenate([[exp[:k].sum()], exp[k:]])
    keep = exp > 0
    if (obs[~keep] != 0).any():
        return math.inf, 1
    obs, exp = obs[keep], exp[keep]
    if exp.size < 2:
        return 0.0, 0
    return float((((obs - exp) ** 2) / exp).sum()), exp.size - 1


def chi2_counts(idx, p):
    """idx: draws (any shape) from the categorical p (float64)"""
    p = np.asarray(p, dtype=np.float64)
    idx = np.asarray(idx).ravel()
    return chi2_sf(*_chi2_stat(np.bincount(idx, minlength=p.size), idx.size * p))


def chi2_pairs(a, b, p):
    """joint of two aligned arrays of draws against p x p"""
    p = np.asarray(p, dtype=np.float64)
    A = p.size
    j = np.asarray(a).ravel().astype(np.int64) * A + np.asarray(b).ravel().astype(np.int64)
    return chi2_sf(*_chi2_stat(np.bincount(j, minlength=A * A), j.size * np.outer(p, p).ravel()))


def _disjoint_pairs(x, k, axis):
    """(x[i], x[i + k]) along `axis` for i with (i // k) even: no element in two pairs"""
    x = np.moveaxis(x, axis, 0)
    n = x.shape[0]
    i = np.arange(n - k)
    i = i[(i // k) % 2 == 0]
    return x[i], x[i + k]


def categorical_shared_names(peaked=False):
    return ["counts", "step_pairs"] + [f"env_pairs_{k}" for k in ENV_LAGS] + ["lane64"] + (["rare_poisson"] if peaked else [])


def categorical_shared(a, p, peaked=False):
    """a: int [T, N] draws, every one from the same p.  peaked: adds the Poisson test of the total outside the mode."""
    a = np.asarray(a).astype(np.int64)
    p = np.asarray(p, dtype=np.float64)
    T, N = a.shape
    out = {"counts": chi2_counts(a, p)}
    out["step_pairs"] = chi2_pairs(*_disjoint_pairs(a, 1, 0), p)
    for k in ENV_LAGS:
        out[f"env_pairs_{k}"] = chi2_pairs(*_disjoint_pairs(a, k, 1), p)
    stat = df = 0
    lane = np.arange(N) % 64
    for ln in range(64):
        sel = a[:, lane == ln]
        s, d = _chi2_stat(np.bincount(sel.ravel(), minlength=p.size), sel.size * p)
        stat, df = stat + s, df + d
    out["lane64"] = chi2_sf(stat, df)
    if peaked:
        mode = int(np.argmax(p))
        out["rare_poisson"] = poisson_p(int((a != mode).sum()), a.size * (1.0 - p[mode]))  # (1 - p[mode] ~ 1e-5: binomial = Poisson)
    assert list(out) == categorical_shared_names(peaked)
    return out


# ---- known-moment correlation statistics ------------------------------------------------------------------------------------------------
def _corr_p(x, y, var):
    """x, y centred with known variance `var`, independent under the null: sum(x y) / (sqrt(n) var) is standard normal"""
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    if x.size == 0:  # (a lag as long as the axis: no pair, nothing to reject)
        return 1.0
    return normal_sf2(float(np.dot(x, y)) / (math.sqrt(x.size) * var))


def _lag_p(c, k, axis, var):
    return _corr_p(*_disjoint_pairs(c, k, axis), var)


def pit(a, P, rng):
    """randomized probability-integral transform of draws a [T, N] from the rows of P [N, A] (float64): Uniform(0, 1) under the null"""
    a = np.asarray(a).astype(np.int64)
    P = np.asarray(P, dtype=np.float64)
    upper = np.cumsum(P, axis=1)
    rows = np.broadcast_to(np.arange(P.shape[0]), a.shape)
    pa = P[rows, a]
    return upper[rows, a] - pa + rng.random(a.shape) * pa


def categorical_rows_names():
    return ["pit_ks", "pit_lag_step1", "pit_lag_step2"] + [f"pit_lag_env{k}" for k in ENV_LAGS]


def categorical_rows(a, P, seed=12345):
    """a: int [T, N]; row i of every step is drawn from P[i]"""
    w = pit(a, P, np.random.default_rng(seed))
    out = {"pit_ks": ks_uniform(w)}
    c = w - 0.5
    for k in (1, 2):
        out[f"pit_lag_step{k}"] = _lag_p(c, k, 0, 1.0 / 12.0)
    for k in ENV_LAGS:
        out[f"pit_lag_env{k}"] = _lag_p(c, k, 1, 1.0 / 12.0)
    assert list(out) == categorical_rows_names()
    return out


def normal_names(A):
    names = ["ks", "mean", "var", "kurt", "tail3", "tail4"]
    for q in ("z", "z2"):
        names += [f"{q}_lag_step1", f"{q}_lag_step2"] + [f"{q}_lag_env{k}" for k in ENV_LAGS]
        names += ([f"{q}_lag_col1"] if A > 1 else []) + ([f"{q}_lag_col16"] if A > 16 else [])
    return names + (["colcorr"] if A > 1 else [])


def normal(z):
    """z: float64 [T, N, A], N(0, 1) under the null"""
    z = np.asarray(z, dtype=np.float64)
    T, N, A = z.shape
    n = z.size
    flat = z.ravel()
    out = {"ks": ks_uniform(_ndtr(flat))}
    out["mean"] = normal_sf2(flat.mean() * math.sqrt(n))
    z2 = z * z
    out["var"] = normal_sf2((z2.mean() - 1.0) * math.sqrt(n / 2.0))
    out["kurt"] = normal_sf2(((z2 * z2).mean() - 3.0) * math.sqrt(n / 96.0))
    for lim in (3.0, 4.0):
        out[f"tail{int(lim)}"] = binom_p(int((np.abs(flat) > lim).sum()), n, math.erfc(lim / math.sqrt(2.0)))
    for q, c, var in (("z", z, 1.0), ("z2", z2 - 1.0, 2.0)):
        for k in (1, 2):
            out[f"{q}_lag_step{k}"] = _lag_p(c, k, 0, var)
        for k in ENV_LAGS:
            out[f"{q}_lag_env{k}"] = _lag_p(c, k, 1, var)
        if A > 1:
            out[f"{q}_lag_col1"] = _lag_p(c, 1, 2, var)
        if A > 16:
            out[f"{q}_lag_col16"] = _lag_p(c, 16, 2, var)
    if A > 1:  # all A (A - 1) / 2 column correlations at once: m r_ij^2 summed is chi-square with that many degrees of freedom
        m = T * N
        zc = z.reshape(m, A)
        r = (zc.T @ zc) / m
        iu = np.triu_indices(A, 1)
        out["colcorr"] = chi2_sf(float(m * (r[iu] ** 2).sum()), iu[0].size)
    assert list(out) == normal_names(A)
    return out


def independence_names(cont):
    return ["cross_z", "cross_z2", "cross_near_equal"] if cont else ["cross_joint"]


NEAR = 1e-4


def independence(x, y, cont, p=None):
    """two aligned sets of draws that must be independent (another seed, another rollout).  Discrete (shared p): the joint table.
    Box (z values): correlation of z and of z^2, and the number of aligned pairs closer than NEAR against its chance expectation
    n * 2 NEAR * integral(phi^2) = n * NEAR / sqrt(pi), upper tail (float32 rounding of mean + sd z moves a recovered z by far less
    than NEAR, so reused noise lands inside)."""
    if not cont:
        return {"cross_joint": chi2_pairs(x, y, p)}
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    close = int((np.abs(x - y) < NEAR).sum())
    return {"cross_z": _corr_p(x, y, 1.0), "cross_z2": _corr_p(x * x - 1.0, y * y - 1.0, 2.0),
            "cross_near_equal": min(1.0, _poisson_tails(close, x.size * NEAR / math.sqrt(math.pi))[1])}


# ---- permutations ---------------------------------------------------------------------------------------------------------------------------
def permutation_names():
    return ["mb_index_bins", "mb_env_bins", "mb_step_bins", "spearman", "successive_joint", "fixed_points"]


def _mb_bins_p(keys, K, B):
    """keys: the permuted order mapped to [0, K) with every key equally often.  For every full minibatch of B positions, the chi-square of
    its keys over nb near-equal-width bins (expectation >= 8 a bin), with the finite-population factor of a draw without replacement;
    the smallest p-value times the number of minibatches (Bonferroni)."""
    total = keys.size
    nb = max(2, min(K, 64, B // 8))
    edges = (np.arange(K, dtype=np.int64) * nb) // K
    frac = np.bincount(edges, minlength=nb) / K
    n_mb = total // B
    if n_mb == 0:
        return 1.0
    b = edges[keys[: n_mb * B]].reshape(n_mb, B)
    counts = np.bincount((np.arange(n_mb, dtype=np.int64)[:, None] * nb + b).ravel(), minlength=n_mb * nb).reshape(n_mb, nb).astype(np.float64)
    exp = B * frac
    stat = (((counts - exp) ** 2) / exp).sum(axis=1) * ((total - 1.0) / max(total - B, 1.0))
    return min(1.0, n_mb * chi2_sf(float(stat.max()), nb - 1))


def permutation(perm, T, B):
    """perm: a permutation of [0, T * N) (flat index f = env * T + step), consumed in minibatches of B positions"""
    perm = np.asarray(perm, dtype=np.int64)
    total = perm.size
    N = total // T
    out = {"mb_index_bins": _mb_bins_p(perm, total, B), "mb_env_bins": _mb_bins_p(perm // T, N, B), "mb_step_bins": _mb_bins_p(perm % T, T, B)}
    j = np.arange(total, dtype=np.float64)
    c = (total - 1) / 2.0
    r = float(np.dot(j - c, perm - c)) / float(np.dot(j - c, j - c))
    out["spearman"] = normal_sf2(r * math.sqrt(total - 1.0))
    nb = 8 if total // 2 >= 64 * 5 else 4  # (8 x 8 where every cell expects >= 5 pairs)
    q = (perm * nb) // total
    cells = np.bincount(q[0:total - 1:2] * nb + q[1:total:2], minlength=nb * nb)
    size = np.bincount((np.arange(total, dtype=np.int64) * nb) // total, minlength=nb).astype(np.float64)
    joint = np.outer(size, size) - np.diag(size)  # ordered pairs of distinct indices per cell
    out["successive_joint"] = chi2_sf(*_chi2_stat(cells, (total // 2) * joint / joint.sum()))
    out["fixed_points"] = poisson_p(int((perm == np.arange(total)).sum()), 1.0)
    assert list(out) == permutation_names()
    return out


def permutation_pair_names():
    return ["equal_positions"]


def permutation_pair(p0, p1):
    """two epochs' permutations: the positions holding the same index are Poisson(1) for independent uniform permutations"""
    return {"equal_positions": poisson_p(int((np.asarray(p0) == np.asarray(p1)).sum()), 1.0)}
