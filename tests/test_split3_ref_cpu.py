"""The float64 emulation of the three-term bf16 split (tests/_split3_ref.py) checked on its own, and the inputs of every bf16x3 gradient row of
tests/test_policy_dispatch_gpu.py checked from the references alone: the comparator those rows use must see their last row tile go.
None of this touches a GPU."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_policy_dispatch_gpu as t  # noqa: E402
from _split3_ref import emulated_grads, split3  # noqa: E402


def test_split_is_exact_and_every_term_is_a_bf16():
    g = torch.Generator().manual_seed(0)
    special = [0.0, -0.0, 1.0, -1.0, 2.0 ** -60, 2.0 ** 60, -(2.0 ** 17), 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 1.0 - 2.0 ** -24,
               1.0 + 2.0 ** -7,   # a bf16: mid and lo are zero
               1.0 + 2.0 ** -10,  # hi = 1, mid = 2^-10, lo = 0
               1.0 + 2.0 ** -7 + 2.0 ** -20,  # mid = 0 would need the residual below a bf16 ulp of it: hi = 1 + 2^-7, mid = 2^-20, lo = 0
               1.0 + 2.0 ** -8,   # a tie of the first rounding (to even: hi = 1, mid = 2^-8)
               1.0 + 3 * 2.0 ** -8, 1e30, -1e30, 1e-30, -1e-30, 3.0e38, 0.1, 1 / 3]  # (beyond 3.396e38 the first term rounds to infinity)
    x = torch.cat([torch.tensor(special, dtype=torch.float32), torch.randn(4096, generator=g),
                   torch.randn(4096, generator=g) * torch.exp2(torch.randint(-90, 90, (4096,), generator=g).float())])
    hi, mid, lo = split3(x)
    for term in (hi, mid, lo):
        assert term.dtype == torch.float32 and torch.equal(term.to(torch.bfloat16).to(torch.float32), term)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    assert torch.equal((hi + mid) + lo, x)  # unsplit_quad's float32 sum gives the value back as well
    # signed zeros split into zeros; the terms of a bf16 value beyond the first are zero
    assert hi[0] == 0 and mid[0] == 0 and lo[0] == 0 and hi[1] == 0 and mid[1] == 0 and lo[1] == 0
    assert hi[10] == x[10] and mid[10] == 0 and lo[10] == 0
    assert hi[11] == 1 and mid[11] == 2.0 ** -10 and lo[11] == 0
    assert hi[13] == 1 and mid[13] == 2.0 ** -8
    # each term is at most half a bf16 ulp of the one before (what makes three 8-bit pieces cover 24 bits): relative 2^-8 per step
    big = x.abs() >= 2.0 ** -90
    assert bool((mid[big].abs() <= hi[big].abs() * 2.0 ** -8).all()) and bool((lo[big].abs() <= hi[big].abs() * 2.0 ** -16).all())
    # Nothing is asserted below |x| ~ 2^-110: bf16 has float32's exponent range, so there the third term (2^-16 of x) is a bf16 subnormal -- it
    # keeps fewer than 8 bits (the split is then inexact by up to 2^-134) and a conversion that flushes denormals makes it zero.  No gradient
    # operand of a trained policy is that small, and such a loss is 2^-16 relative at worst.


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("D,A", [(6, 2), (17, 5), (32, 16)])
def test_manual_backward_with_every_product_equals_float64_autograd(D, A, normalize):
    """emulated_grads(products="all") -- the same manual backward, every split term kept -- against float64 autograd of sb3_ref.ppo_loss: 1e-12 of
    max |g| per segment (observed 1e-15 .. 6e-15).  With the kernel's three products the weight segments move and the bias segments do not."""
    B, T = 300, 16
    N = B // T + 2
    sd = t.case_state_dict(D, 256, A, False)
    _, rows = t._rollout(sd, D, A, False, T, N, seed=D)
    idx = torch.randperm(T * N, generator=torch.Generator().manual_seed(A))[:B]
    hp = dict(t.HP, normalize_advantage=normalize)
    ref, s_ref = t._grads(sd, rows, idx, torch.float64, hp)
    full, s_full = emulated_grads(sd, rows, idx, torch.float64, hp, products="all")
    kern, _ = emulated_grads(sd, rows, idx, torch.float64, hp)
    assert set(full) == set(ref) == set(kern)
    assert 0.05 < s_ref["clip_fraction"] < 0.95  # both branches of the clipped surrogate
    for key in ref:
        m = float(ref[key].abs().max())
        assert full[key].shape == ref[key].shape and m > 0
        assert float((full[key] - ref[key]).abs().max()) <= 1e-12 * m, (key, float((full[key] - ref[key]).abs().max()) / m)
        d = float((kern[key] - full[key]).abs().max())
        if key.endswith("bias"):
            assert d == 0.0, key
        else:  # three products of order 2 dropped: 2^-16 of a product, less after the sum
            assert 0.0 < d <= 2.0 ** -14 * m, (key, d / m)
    for key in ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction"):
        assert s_full[key] == s_ref[key]


S3_GRAD_CASES = [c for c in t.CASES if c[0].startswith("grad") and t.entry_dtype_kind(c[0])[0] == "bf16x3"]


def test_the_issue_rows_are_all_there():
    have = {(e, D, A, B) for e, D, H, A, cont, B, ident in S3_GRAD_CASES}
    want = {("grad_bf16x3", 6, 5, 4096)} | {("grad_bf16x3", 16, 5, B) for B in (4096, 4097, 4111, 4112, 4113, 4127, 8192, 8193, 12289)}
    want |= {("grad_bf16x3", D, 5, 4097) for D in (1, 16, 17, 32)} | {("grad_bf16x3", 6, A, 4127) for A in (2, 16)} | {("grad_bf16x3", 32, A, 4096) for A in (2, 16)}
    want |= {("grad_perm_bf16x3", 6, 5, 4113), ("grad_noadv_bf16x3", 21, 3, 4097), ("grad_corr_bf16x3", 17, 2, 12289),
             ("grad_nw8_bf16x3", 16, 5, 4097), ("grad_nw8_bf16x3", 17, 16, 4127)}
    assert want <= have, sorted(want - have)
    assert all(H == 256 and not cont and ident == "GRAD_BF16X3" for e, D, H, A, cont, B, ident in S3_GRAD_CASES)


@pytest.mark.parametrize("entry,D,H,A,cont,B,ident", [pytest.param(*c, id=t._case_id(c)) for c in S3_GRAD_CASES])
def test_comparator_sees_the_last_row_tile_of_every_bf16x3_row_dropped(entry, D, H, A, cont, B, ident, record_property):
    """A condition on the test inputs, not a measurement of the kernel: with the float64 emulation as reference and the float32 emulation as
    calibration, the comparator (K_S3, F_S3) rejects the float64 emulation of the same minibatch without its last row tile, and the dropped
    tile overshoots the budget at least fourfold."""
    sd = t.case_state_dict(D, H, A, cont)
    c = t.grad_case_inputs(entry, D, A, cont, B, sd)
    rows, idx, hp, drop = c["rows"], c["idx"], c["hp"], c["drop"]
    if entry == "grad_corr_bf16x3":
        assert len(torch.unique(rows["obs"][idx], dim=0)) == 4
    g64, s64 = emulated_grads(sd, rows, idx, torch.float64, hp)
    g32, _ = emulated_grads(sd, rows, idx, torch.float32, hp)
    gdrop, _ = emulated_grads(sd, rows, idx[:B - drop], torch.float64, hp)
    assert 0.05 < s64["clip_fraction"] < 0.95
    errs_cal = t._segment_errors(g32, g64, g32)
    errs_drop = t._segment_errors(gdrop, g64, g32)
    over = max(t.budget_use(*v, t.K_S3, t.F_S3) for v in errs_drop.values())
    record_property("drop_overshoot", over)
    print(f"{t._case_id((entry, D, H, A, cont, B, ident))}: drop of {drop} rows overshoots {over:.1f}-fold; calibration error / max|g| "
          f"{max(v[0] / v[2] for v in errs_cal.values()):.2e}")
    assert t._rejects(errs_drop, t.K_S3, t.F_S3)
    assert over >= 4.0, (over, errs_drop)
