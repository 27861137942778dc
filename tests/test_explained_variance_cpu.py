"""The yardstick of tests/test_explained_variance_gpu.py, checked without a GPU: for the synthetic inputs that test uses, numpy's float64
`1 - var(returns - values) / var(returns)` against the EXACT value (integer arithmetic on the float32 inputs, a Fraction at the end) stays far
inside the bound the device kernel is held to, 2e-9 * max(1, |1 - ev|) -- so a device result outside the bound is the kernel's error, not the
reference's."""
from fractions import Fraction

import numpy as np
import pytest

SIZES = (1000, 131072, 2 ** 22 + 3)
NOISE = (0.3, 3.0)


def synthetic(n, noise, seed=0):
    """returns = 100 + N(0, 1), values = returns + noise * N(0, 1), float32 (the generator of the GPU test)."""
    rng = np.random.default_rng(seed + n)
    returns = (100.0 + rng.standard_normal(n)).astype(np.float32)
    values = (returns.astype(np.float64) + noise * rng.standard_normal(n)).astype(np.float32)
    return values, returns


def bound(ev):
    return 2e-9 * max(1.0, abs(1.0 - ev))


def numpy_ev(values, returns):
    y, p = returns.astype(np.float64), values.astype(np.float64)
    var_y = np.var(y)
    return float("nan") if var_y == 0 else float(1.0 - np.var(y - p) / var_y)


def exact_ev(values, returns) -> Fraction:
    """Both inputs are float32 of magnitude >= 8: integers after scaling by 2^20.  Population variance of integers d_i (centred on an integer near
    the mean so that the squares fit int64): (n sum d^2 - (sum d)^2) / n^2, summed in chunks that cannot overflow, folded as Python integers."""
    def ints(x):
        s = np.ldexp(x.astype(np.float64), 20)
        assert np.all(np.abs(x) >= 8.0) and np.all(s == np.rint(s)) and np.all(np.abs(s) < 2.0 ** 40)
        return s.astype(np.int64)

    def var_times_n2(d):
        d = d - int(np.rint(d.mean()))
        assert np.abs(d).max() < 2 ** 25
        s1 = sum(int(c.sum()) for c in np.array_split(d, max(1, len(d) // 4096)))
        s2 = sum(int((c * c).sum()) for c in np.array_split(d, max(1, len(d) // 4096)))
        return len(d) * s2 - s1 * s1

    y, p = ints(returns), ints(values)
    return 1 - Fraction(var_times_n2(y - p), var_times_n2(y))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("noise", NOISE)
def test_numpy_float64_is_far_inside_the_bound_of_the_device_test(n, noise):
    values, returns = synthetic(n, noise)
    ev64, ev = numpy_ev(values, returns), exact_ev(values, returns)
    err = abs(float(Fraction(ev64) - ev))
    print(f"n = {n}, noise {noise}: ev = {float(ev):.12f}, |numpy f64 - exact| = {err:.3g}, bound {bound(float(ev)):.3g}")
    assert err <= 1e-3 * bound(float(ev))  # (measured: at most a few 1e-15)


def test_exact_helper_on_a_case_with_a_known_answer():
    returns = np.array([96.0, 98.0, 102.0, 104.0], np.float32)  # variance 10
    values = returns + np.array([1.0, -1.0, 1.0, -1.0], np.float32)  # residual variance 1
    assert exact_ev(values, returns) == Fraction(9, 10) and abs(numpy_ev(values, returns) - 0.9) < 1e-15
    assert np.isnan(numpy_ev(values, np.full(4, 100.0, np.float32)))
