"""Every specialisation the policy's three dispatchers can pick -- the forward (launch_fwd), the minibatch gradient (minibatch_grad_impl) and
the optimizer step (tma_ppo_adam_step / _local), each of which launches what its pure plan function (plan_fwd / plan_grad / plan_opt,
csrc/tma_policy_plan.h) decides -- against an independent float64 reference (oracle/sb3_ref.py run on .double() copies of
the exact f32 parameters and inputs), at the shapes where tile code breaks.  Each case names the branch it is meant to reach and asserts
it through tma_debug_last_dispatch, so a threshold change cannot quietly move a case onto another kernel; the host-only query
tma_debug_plan_dispatch must name the same branch for the same arguments.

Gradient comparison, per parameter segment s:  err_kernel,s <= K * err_torch32,s + F * max|g64,s|, where err_torch32 is the error of
float32 torch CPU autograd on the same data (the calibration: what an honest f32 implementation of the same sums is off by).  Every
gradient case also checks that the comparator REJECTS the float64 gradient of the same minibatch without its last row tile -- the
tolerance is tight enough to see a dropped partial tile at that size.

The bf16 rows and the bf16x3 rows (mfma_dtype = 2, the three-term split of the 256 x 256 f32 update: csrc/tma_split3.h) are held to the same
comparator with an emulation of the kernel's documented rounding as the reference (float64) and the calibration (float32): the bf16 rounding
points of tests/test_bf16_gpu.py, and for the split the three weight-gradient products it keeps (tests/_split3_ref.py).  Against plain float64
the split's dropped products alone would use 0.15 .. 0.7 of an f32-class budget; with them in the reference, what is left of the kernel's
error is f32-class and K_S3, F_S3 are the f32 rows' constants.  The bf16x3 rows cover the 32-row-group edges from 4096 samples (where the update
switches to this kernel) on, both compile-time observation classes at both ends, head widths 2 and 16, the on-device permutation,
normalize_advantage off, a minibatch of four distinct observations, the eight-wave instantiations (TMA_S3_NW8) and the optimizer's three-plane
scatter (a gradient at the stepped parameters); each row also records its distance from plain float64 autograd.

CASES is importable without a GPU: tests/test_policy_dispatch_table_cpu.py checks that every branch id of include/tma.h has a case, and
that the query alone gives every case its id."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import sb3_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

# comparator constants, one pair for the whole file (f32 rows); bf16 forward rows are compared with the bf16-rounded emulation and get their own.
# First MI355X run (K = 8, F = 2e-6): every gradient case used at most 0.82 of that budget (Basic, 21 x 64, 131 072 samples: the generic kernel's
# float atomics); the forward rows at most 0.18.  With the constants below: at most 0.41, i.e. 2.4x headroom.  The dropped-tile reference
# overshoots the same budget at least 129-fold (Box 6 x 64, 8 177 samples).  Worst err_kernel / err_torch32 over a case's segments, by
# family: H = 64 kernels 3.1, f32 kt1 = 107 5.4, kt1 = 0 22.7, small7 26.7, kt1 = 2 31.9, kt1 = 11 127, generic 194, kt1 = 1 242 (the large
# ones on segments where float32 autograd happens to be almost exact, so the F term carries them).
# The H = 64 class rows (H64_CLASS_CASES: eight (D, A) at seven sizes, every DT / AT variant of both kernels), MI355X, same constants, nothing raised:
# small kernel at most 0.120 (4 x 64 x 4, 2033 samples, value_net.bias), eight-wave kernel 0.115 (1 x 64 x 2, 16 385 samples, action_net.bias),
# forward rows 0.059 (6 x 64 x 5, n = 17, values); their worst err_kernel / err_torch32 is 12.5 (1 x 64 x 2, 4112 samples: one observation column,
# float32 autograd almost exact).  Optimizer rows, in units of the entry's own bounds: parameters 0.50 of 2^-19 |p| + 4e-5 lr (7 x 64 x 3, no clip,
# step 3), exp_avg_sq 0.50 of 2.6e-5 (1 x 64 x 2), IEEE float32 Adam 167 of 256 (7 x 64 x 3, step 3: what three steps of the float32 1 - beta2
# offset come to on a parameter far smaller than lr), tma_policy_sync changed no bit; opt and opt_local give the same figures.  Statistics at most 4.5e-8
# (9 x 64 x 7, 2033 samples, entropy_loss).  The dropped-tile reference of these rows overshoots at least 229-fold (16 x 64 x 5, 16 385 samples:
# one row), which tests/test_policy_dispatch_table_cpu.py holds to a floor of four from the references alone.
K, F = 16.0, 4e-6
K_BF, F_BF = 8.0, 4e-3  # (a sum that lands on a bf16 rounding boundary flips one activation by one bf16 ulp: test_bf16_gpu.py's 4e-3)
CLIP_MARGIN = 2e-2  # |ratio - 1| kept this far from clip_range in float64 (tests/test_ppo_gpu.py's _rollout keeps 5e-3 in float32)
# bf16 gradient rows: reference = test_bf16_gpu._emulated_grad (the kernel's bf16 rounding points) in float64, calibration = the same in float32.
# Where no float32 sum lands on the other side of a bf16 rounding boundary the kernels sit 1e-7 .. 2e-6 of max |g| from the reference; one such flip
# of an activation or a delta moves one sample's terms by 2^-8 of themselves, and the float32 emulation has flips of its own, in other places
# (its sums are in yet another order).  In a large minibatch both average out (kernel and calibration 1e-4 .. 1e-3 of max |g|, ratio 0.3 .. 3);
# in a small one a flip is a rare whole event that the calibration may not have, so F has to carry it: at B = 1 a flip is up to 2.2 * 2^-8
# of max |g|.  MI355X run with these constants: worst budget use 0.48 (17 x 256 x 3 Discrete, B = 1, action_net.weight: 8.7e-3 of max |g|,
# calibration exact), next 0.12; the dropped-tile reference overshoots at least 2.0-fold (Box 32 x 256 x 4, 4096 samples), the heavy-tile rows
# at least 6-fold; statistics at most 1.03e-3 (Box 105 x 256 x 8, B = 1: policy_loss of the one sample), 0.41 of S_BF_G, next 1.8e-4.
# First run, K = 8, F = 4e-6: worst use 412 (Box 172 x 256 x 20, B = 77) -- F cannot be the float32 rows' F.
K_BF_G, F_BF_G = 8.0, 1.8e-2
S_BF_G = 2.5e-3  # the four averaged statistics, relative to max(1, |reference|)
# A dropped tile of `drop` rows out of B moves a segment by about sqrt(drop / B) of its max |g| (a sum of B terms of either sign), and the
# budget above is 2e-2 .. 3e-2 of it: where the last row tile holds less than a thousandth of the minibatch the comparator could not see
# it go.  Those rows make the tile heavy instead: its advantages and returns times BF_HEAVY, normalize_advantage off (so that the factor
# is not divided out again).
BF_HEAVY = 100.0
# bf16x3 rows: reference = _split3_ref.emulated_grads in float64 (the three weight-gradient products the kernel keeps), calibration = the same in
# float32.  The emulation carries the truncation, what remains is f32-class (tma_split3.h): the f32 rows' constants under names of their own.
# First MI355X run, with these constants: worst budget use 0.173 (6 x 256 x 5, B = 4096: the gradient after three tma_ppo_adam_step steps with
# max_norm 1e3, on the scattered planes), among the gradient rows 0.172 (6 x 256 x 16, B = 4127, value_net layer-2 bias), every other row
# 0.07 .. 0.17, the gradient rows always on a bias segment (plain f32 sums, where the float32 calibration happens to be closest); the eight-wave rows 0.10 / 0.11.
# Kernel against the emulation 1.4e-6 .. 3.1e-6 of max |g| on weight segments (5.1e-6 on the four-observation minibatch, whose calibration is
# 2.5e-5 off), 0.5e-6 .. 2.7e-6 on bias segments; the float32 emulation itself 1.5e-6 .. 2.7e-6.  Statistics at most 7.0e-8 (value_loss,
# four-observation minibatch), 0.035 of the 2e-6.  The dropped-tile reference overshoots at least 399-fold (16 x 256 x 5, B = 4113: one row).
# Nothing was raised: the constants are the f32 rows' (5.8x headroom here against their 2.4x; not tightened, so that both families keep one budget).
K_S3, F_S3 = 16.0, 4e-6
S3_SEED = 60000  # data seed offset of the bf16x3 rows (tests/test_split3_ref_cpu.py: every dropped-tile reference overshoots K_S3, F_S3 at least fourfold)


def bf_heavy_tile(B):
    return (B % 16 or 16) * 1024 < B

# (entry, D, H, A, continuous, B or n, expected dispatch id: TMA_DISPATCH_ name without the prefix, "|GRID_CAPPED" where the grid is capped)
# entries: grad (explicit indices) / grad_perm (Feistel permutation) / grad_noadv (normalize_advantage off) / grad_nodz1 (TMA_NO_DZ1_CACHE) /
# grad_nodefer (TMA_NO_DEFER_W2, in a child process: read once per process) / fwd / fwd_bf16 /
# opt / opt_bf16 / opt_bf16x3 (tma_ppo_adam_step after a gradient of B samples) /
# opt_local / opt_local_bf16 / opt_local_bf16x3 (tma_ppo_adam_step_local with last_count = B)
# bf16x3 gradient rows (float64 emulation of the split's weight-gradient products): grad_bf16x3 / grad_perm_bf16x3 / grad_noadv_bf16x3 /
# grad_corr_bf16x3 (observations of four distinct values) and, in a child process, grad_nw8_bf16x3 (TMA_S3_NW8: eight waves of 32 columns)
# bf16 gradient rows (float64 emulation with the kernel's rounding points): grad_bf16 / grad_perm_bf16 / grad_noadv_bf16 / grad_nodz1_bf16 and, in a
# child process each (read once per process), grad_nw4_bf16 (TMA_BF_NW4: four waves throughout) / grad_mt2_bf16 (TMA_BF_MT2: 32-row groups)
_N_EDGES = (1, 15, 16, 17, 31, 32, 33)
_FWD_SHAPES = [  # (D, H, A, cont, id) -- Discrete A = 2 / 16 and Box A = 1 / 32 among them
    (4, 64, 5, False, "FWD_H64"), (4, 64, 16, False, "FWD_H64"),
    (6, 128, 2, False, "FWD_F32_NTW2_DISCRETE"), (6, 192, 16, False, "FWD_F32_NTW3_DISCRETE"), (21, 256, 5, False, "FWD_F32_NTW4_DISCRETE"),
    (8, 128, 1, True, "FWD_F32_NTW2_BOX"), (8, 192, 32, True, "FWD_F32_NTW3_BOX"), (105, 256, 8, True, "FWD_F32_NTW4_BOX"),
    (21, 64, 3, False, "FWD_GENERIC_W1"), (6, 64, 4, True, "FWD_GENERIC_W1"),
]
_FWD_BF_SHAPES = [
    (6, 128, 2, False, "FWD_BF16_NTW2_DISCRETE"), (6, 192, 16, False, "FWD_BF16_NTW3_DISCRETE"), (21, 256, 5, False, "FWD_BF16_NTW4_DISCRETE"),
    (8, 128, 1, True, "FWD_BF16_NTW2_BOX"), (8, 192, 32, True, "FWD_BF16_NTW3_BOX"), (105, 256, 8, True, "FWD_BF16_NTW4_BOX"),
]


def _wide_grad_cases():
    out = []
    for H in (128, 192, 256):
        w8 = H == 256
        for cont, A in ((False, 5), (True, 3)):
            for B in (113, 256, 1000, 1024, 1025, 33000):  # kt1 = 1: half groups up to 1024 samples, full row groups beyond
                half = B <= 1024
                ident = ("KT1_HALF_W8_DEFER" if half else "KT1_FULL_W8") if w8 else ("KT1_HALF_W4" if half else "KT1_FULL_W4")
                out.append(("grad", 16, H, A, cont, B, "GRAD_F32_" + ident))
            for D, B in ((17, 1000), (17, 2048), (32, 1024), (32, 1025)):  # kt1 = 2
                half = B <= 1024
                ident = ("KT2_HALF_W8_DEFER" if half else "KT2_FULL_W8") if w8 else ("KT2_HALF_W4" if half else "KT2_FULL_W4")
                out.append(("grad", D, H, A + 1, cont, B, "GRAD_F32_" + ident))
    return out


_BF_EDGES = (1, 31, 32, 33, 77)  # row-group edges of the 32-row leaves


def _bf_grad_cases():
    """Every leaf of plan_grad_bf (csrc/tma_policy_plan.h) at every hidden width and head it takes, both ends of every observation-width class
    (16 / 17, 32 / 33, 64 / 65, 96 / 97, 128 / 129, 160 / 161, 192 / 193), head widths Discrete 2 / 16 and Box 1 / 32 on 32-row and on 64-row
    leaves.  Sizes: the row-group edges; 3841 = 121 groups of 32 (between the value net's block cap and the policy net's: only the value blocks
    loop) with a 1-row last group; 4500 / 4733 = more 32-row groups than blocks (136 / 144 policy blocks); 4096 | 4097 = the switch to 64-row
    groups (65 groups, the last with one row); 7681 = 121 groups of 64, between the two caps of the eight-wave kernel; 9001 / 9301 = more 64-row groups than blocks, ragged; 33000 on the two timed configurations."""
    e, G = "grad_bf16", "GRAD_BF16_"
    out = [(e, 6, 256, 5, False, 1000, G + "KT1_MT2")]
    # dW1 in registers, 32-row groups: up to 4096 samples, and at H = 192 throughout
    out += [(e, 16, 128, 5, False, B, G + "KT1_MT2") for B in _BF_EDGES]
    out += [(e, 16, 192, 16, False, 3841, G + "KT1_MT2"), (e, 6, 192, 2, False, 4500, G + "KT1_MT2"), (e, 16, 256, 2, False, 4096, G + "KT1_MT2"),
            (e, 16, 128, 1, True, 3841, G + "KT1_MT2"), (e, 8, 192, 32, True, 4733, G + "KT1_MT2"), (e, 16, 256, 3, True, 4096, G + "KT1_MT2")]
    out += [(e, 17, 256, 3, False, B, G + "KT2_MT2") for B in _BF_EDGES]
    out += [(e, 32, 128, 16, False, 3841, G + "KT2_MT2"), (e, 21, 192, 3, False, 4500, G + "KT2_MT2"), (e, 17, 128, 1, True, 77, G + "KT2_MT2"),
            (e, 32, 192, 32, True, 4733, G + "KT2_MT2"), (e, 17, 192, 4, True, 3841, G + "KT2_MT2"), (e, 32, 256, 4, True, 4096, G + "KT2_MT2")]
    # 64-row groups beyond 4096 samples; the Discrete head at H = 256 with <= 16 observations on eight waves
    out += [(e, 16, 128, 5, False, 4097, G + "KT1_MT4"), (e, 16, 128, 16, False, 9001, G + "KT1_MT4"), (e, 16, 128, 32, True, 4097, G + "KT1_MT4"),
            (e, 16, 256, 1, True, 9301, G + "KT1_MT4"), (e, 6, 256, 3, True, 4097, G + "KT1_MT4"),
            (e, 16, 256, 5, False, 4097, G + "KT1_MT4_W8"), (e, 16, 256, 2, False, 9001, G + "KT1_MT4_W8"), (e, 4, 256, 16, False, 4097, G + "KT1_MT4_W8"),
            (e, 6, 256, 5, False, 33000, G + "KT1_MT4_W8"),  # Ball3D
            (e, 6, 256, 5, False, 7681, G + "KT1_MT4_W8"),  # 121 groups of 64: between this kernel's 116 value blocks and 140 policy blocks
            (e, 17, 128, 3, False, 4097, G + "KT2_MT4"), (e, 32, 128, 2, False, 9001, G + "KT2_MT4"), (e, 21, 256, 3, False, 4097, G + "KT2_MT4"),  # Basic
            (e, 17, 256, 16, False, 9001, G + "KT2_MT4"), (e, 17, 128, 1, True, 9301, G + "KT2_MT4"), (e, 32, 256, 32, True, 4097, G + "KT2_MT4")]
    # two passes, two layer-1 k-steps (33 .. 64 observations)
    out += [(e, 33, 128, 5, False, B, G + "KS2_CACHED") for B in _BF_EDGES]
    out += [(e, 64, 192, 2, False, 3841, G + "KS2_CACHED"), (e, 64, 256, 16, False, 4733, G + "KS2_CACHED"), (e, 33, 128, 1, True, 3841, G + "KS2_CACHED"),
            (e, 40, 192, 7, True, 4733, G + "KS2_CACHED"), (e, 64, 256, 32, True, 1025, G + "KS2_CACHED"),
            ("grad_nodz1_bf16", 64, 256, 5, False, 4733, G + "KS2_RECOMPUTE"), ("grad_nodz1_bf16", 33, 128, 3, True, 1025, G + "KS2_RECOMPUTE")]
    # ... six (161 .. 192: Crawler's 172), on four waves except for Box heads at H = 256
    out += [(e, 161, 128, 5, False, B, G + "KS6_CACHED") for B in _BF_EDGES]
    out += [(e, 192, 192, 16, False, 3841, G + "KS6_CACHED"), (e, 172, 256, 2, False, 4733, G + "KS6_CACHED"), (e, 161, 128, 20, True, 3841, G + "KS6_CACHED"),
            (e, 192, 192, 1, True, 4733, G + "KS6_CACHED"),
            ("grad_nodz1_bf16", 192, 256, 5, False, 1025, G + "KS6_RECOMPUTE"), ("grad_nodz1_bf16", 172, 192, 32, True, 4733, G + "KS6_RECOMPUTE")]
    out += [(e, 172, 256, 20, True, B, G + "KS6_W8_CACHED") for B in _BF_EDGES + (33000,)]
    out += [(e, 161, 256, 1, True, 3841, G + "KS6_W8_CACHED"), (e, 192, 256, 32, True, 4733, G + "KS6_W8_CACHED"),
            ("grad_nodz1_bf16", 161, 256, 20, True, 4733, G + "KS6_W8_RECOMPUTE")]
    # ... four (97 .. 128 with a Box head at H = 256: the reference's ant task), eight waves
    out += [(e, 105, 256, 8, True, B, G + "KS4_W8_CACHED") for B in _BF_EDGES]
    out += [(e, 97, 256, 1, True, 3841, G + "KS4_W8_CACHED"), (e, 128, 256, 32, True, 4733, G + "KS4_W8_CACHED"),
            ("grad_nodz1_bf16", 128, 256, 8, True, 1025, G + "KS4_W8_RECOMPUTE"), ("grad_nodz1_bf16", 97, 256, 3, True, 4733, G + "KS4_W8_RECOMPUTE")]
    # runtime width: everything else (the Ant width with a Discrete head or at H = 128 among it)
    out += [(e, 65, 128, 5, False, B, G + "RUNTIME") for B in _BF_EDGES]
    out += [(e, 96, 192, 2, False, 3841, G + "RUNTIME"), (e, 129, 256, 16, False, 4733, G + "RUNTIME"), (e, 160, 128, 3, False, 1025, G + "RUNTIME"),
            (e, 193, 256, 4, False, 1025, G + "RUNTIME"), (e, 105, 256, 5, False, 3841, G + "RUNTIME"), (e, 97, 192, 3, False, 77, G + "RUNTIME"),
            (e, 105, 128, 8, True, 4733, G + "RUNTIME"), (e, 128, 192, 32, True, 3841, G + "RUNTIME"), (e, 65, 256, 3, True, 4733, G + "RUNTIME"),
            (e, 96, 192, 6, True, 77, G + "RUNTIME"), (e, 129, 256, 1, True, 1025, G + "RUNTIME"), (e, 160, 128, 4, True, 1025, G + "RUNTIME"),
            (e, 193, 192, 2, True, 1025, G + "RUNTIME")]
    # the Feistel-permutation and normalize_advantage = False entries: a 64-row leaf, a two-pass leaf and the runtime width each
    out += [("grad_perm_bf16", 16, 256, 5, False, 4097, G + "KT1_MT4_W8"), ("grad_noadv_bf16", 21, 256, 3, False, 4097, G + "KT2_MT4"),
            ("grad_perm_bf16", 172, 256, 20, True, 1025, G + "KS6_W8_CACHED"), ("grad_noadv_bf16", 40, 128, 4, False, 1025, G + "KS2_CACHED"),
            ("grad_perm_bf16", 100, 128, 4, False, 1025, G + "RUNTIME"), ("grad_noadv_bf16", 105, 256, 5, False, 1025, G + "RUNTIME")]
    # per-process switches: the four-wave kernels that TMA_BF_NW4 alone reaches; 32-row groups past 4096 samples at H = 256
    out += [("grad_nw4_bf16", 16, 256, 5, False, 4097, G + "KT1_MT4"), ("grad_nw4_bf16", 172, 256, 20, True, 1025, G + "KS6_CACHED"),
            ("grad_nw4_bf16", 105, 256, 8, True, 1025, G + "RUNTIME"), ("grad_mt2_bf16", 6, 256, 5, False, 4500, G + "KT1_MT2")]
    return out


def _s3_grad_cases():
    """The split kernel (ppo_grad_split3_kernel, H = 256, Discrete): 32-row groups of two 16-row tiles, persistent blocks, at most 128 per net.
    The update reaches it from 4096 samples on, so these are its smallest shapes."""
    e, G = "grad_bf16x3", "GRAD_BF16X3"
    out = [(e, 6, 256, 5, False, 4096, G)]
    # group edges: 4096 = 128 groups = both block caps (one group per block); 4097 .. 4127 = a last group of 1 / 15 / 16 / 17 / 31 rows that one block
    # loops for; 8192 | 8193 = two full groups per block, then a one-row third on one block; 12289 = three per block and a one-row group
    out += [(e, 16, 256, 5, False, B, G) for B in (4096, 4097, 4111, 4112, 4113, 4127, 8192, 8193, 12289)]
    # both ends of the two compile-time observation classes (KT1C = 1: D <= 16, KT1C = 2: 17 .. 32)
    out += [(e, D, 256, 5, False, 4097, G) for D in (1, 17, 32)]
    # head widths 2 and 16
    out += [(e, 6, 256, A, False, 4127, G) for A in (2, 16)] + [(e, 32, 256, A, False, 4096, G) for A in (2, 16)]
    out += [("grad_perm_bf16x3", 6, 256, 5, False, 4113, G), ("grad_noadv_bf16x3", 21, 256, 3, False, 4097, G),
            ("grad_corr_bf16x3", 17, 256, 2, False, 12289, G),  # GridWorld early in training: the truncation errors of equal rows do not average out
            ("grad_nw8_bf16x3", 16, 256, 5, False, 4097, G), ("grad_nw8_bf16x3", 17, 256, 16, False, 4127, G)]
    return out


# entries whose switch is read once per process: the case runs in a child process with it set (and so does its plan query in the table test)
SWITCH_ENTRIES = {"grad_nodefer": "TMA_NO_DEFER_W2", "grad_nw4_bf16": "TMA_BF_NW4", "grad_mt2_bf16": "TMA_BF_MT2", "grad_nw8_bf16x3": "TMA_S3_NW8"}


def bf_expected_geometry(ident, cont, B):
    """(grid, block) of a bf16 gradient leaf, restated from the design: one block per CU, the policy net gets 144 (Box), 140 (eight-wave
    Discrete kernel) or 136 of the 256; a block loops once there are more row groups than its net has blocks."""
    groups = -(-B // (64 if "_MT4" in ident else 32))
    cap_pi = 144 if cont else (140 if ident.endswith("KT1_MT4_W8") else 136)
    return min(groups, cap_pi) + min(groups, 256 - cap_pi), (512 if "_W8" in ident else 256)


# The H = 64 LDS-image kernels beyond the headline shape.  One dispatch id covers every compile-time variant tma_launch_grad_h64 (csrc/tma_h64.hip)
# launches -- observation width DT = 4 / 6 / 0 (runtime D: KS1 = (D + 3) >> 2 layer-1 k-steps, columns D .. 4 KS1 - 1 zero-padded), the four-wave
# small kernel or the eight-wave persistent one, head width AT = 5 (4 x 64 x 5 alone) or runtime -- so the ids cannot tell whether a variant has a
# reference row: tests/test_policy_dispatch_table_cpu.py derives the variant of every row and asserts that each one has rows on both kernels.
H64_SHAPES = [(6, 5),    # DT = 6: Ball3D
              (4, 4),    # DT = 4 with a runtime head: WallJump
              (7, 3),    # DT = 0, KS1 = 2, one padded column: Bicycle
              (16, 5),   # KS1 = 4, no padding: Glider
              (1, 2),    # KS1 = 1, three padded columns, the smallest head
              (5, 16),   # KS1 = 2, three padded columns, the full head
              (9, 7),    # KS1 = 3, three padded columns, head rows 5 .. 8
              (13, 12)]  # KS1 = 4, three padded columns, head rows 9 .. 12
# small kernel: 241 = 16 tiles (the first size of the family), one row in the last; 2033 = 128 tiles, the last ragged; 2048 = 128 full tiles, the
# last size before the switch.  Eight-wave kernel: 2049 = 129 tiles, 15 invalid rows in the last; 4112 = 257 tiles over 33 x 8 waves (some waves
# run no tile); 16385 = 1025 tiles over 1024 waves (one wave runs a second tile); 32784 = 2049 tiles (a pair's waves own 3 and 2 tiles)
H64_SMALL_B, H64_WAVE8_B = (241, 2033, 2048), (2049, 4112, 16385, 32784)
# forward: tile edges; 64 tiles (plan_fwd goes to two waves per block), ragged and full; 512 tiles (four waves per block), ragged
H64_FWD_N = (1, 17, 33, 1009, 1024, 8177)
# the optimizer's scatter into the LDS images, whose layout depends on D's padding and on A: the task shapes and the two extremes
H64_OPT_SHAPES = [(6, 5), (4, 4), (7, 3), (16, 5), (1, 2), (5, 16)]
H64_CLASS_CASES = (
    [("grad", D, 64, A, False, B, "GRAD_H64_SMALL") for D, A in H64_SHAPES for B in H64_SMALL_B]
    + [("grad", D, 64, A, False, B, "GRAD_H64") for D, A in H64_SHAPES for B in H64_WAVE8_B]
    + [("grad_perm", 6, 64, 5, False, 4112, "GRAD_H64"), ("grad_noadv", 7, 64, 3, False, 2049, "GRAD_H64")]
    + [("fwd", D, 64, A, False, n, "FWD_H64") for D, A in H64_SHAPES for n in H64_FWD_N]
    + [("opt", D, 64, A, False, 256, "OPT_SCATTER_H64") for D, A in H64_OPT_SHAPES]
    + [("opt_local", D, 64, A, False, 256, "OPT_LOCAL_SCATTER_H64") for D, A in H64_OPT_SHAPES]
)

CASES = (
    # ---- gradient: H = 64 fast path (4, 64, 5, Discrete): one tile per wave up to 2048 samples, then the persistent eight-wave kernel
    [("grad", 4, 64, 5, False, B, "GRAD_H64_SMALL") for B in (241, 255, 256, 2048)]
    + [("grad", 4, 64, 5, False, B, "GRAD_H64") for B in (2049, 16385, 131072)]
    + [("grad", 4, 64, 2, False, 1000, "GRAD_H64_SMALL"), ("grad", 16, 64, 16, False, 3000, "GRAD_H64"),
       ("grad_perm", 4, 64, 5, False, 1000, "GRAD_H64_SMALL"), ("grad_noadv", 4, 64, 5, False, 300, "GRAD_H64_SMALL")]
    # ---- H = 64 at every task shape and width class: gradient on both kernels, forward, the optimizer's scatter
    + H64_CLASS_CASES
    # ---- gradient: generic float-atomic kernel (wpb = 4 from 512 tiles, fewer while the tile exceeds 156 KB; grid capped at 1024 blocks)
    + [("grad", 4, 64, 5, False, B, "GRAD_GENERIC_W1") for B in (1, 2, 15, 17, 240)]
    + [("grad", 21, 64, 3, False, 131072, "GRAD_GENERIC_W4|GRID_CAPPED"),  # Basic at the headline minibatch: grid-stride over float atomics
       ("grad", 6, 64, 4, True, 8176, "GRAD_GENERIC_W1"), ("grad", 6, 64, 4, True, 8177, "GRAD_GENERIC_W4"),  # Box heads: 511 / 512 tiles
       ("grad", 45, 64, 3, False, 65536, "GRAD_GENERIC_W4"),  # BrickBreak: 4096 tiles = exactly the 1024-block cap
       ("grad", 105, 64, 8, True, 65552, "GRAD_GENERIC_W4|GRID_CAPPED"),  # Ant at 64 wide: 4097 tiles, one past the cap
       ("grad", 500, 64, 3, False, 8200, "GRAD_GENERIC_W3"), ("grad", 800, 64, 1, True, 8200, "GRAD_GENERIC_W2"),
       ("grad", 2000, 64, 2, False, 8200, "GRAD_GENERIC_W1"),  # (D 449..656 / 657..1072 / 1073..2384 at H = 64)
       ("grad", 4, 320, 3, False, 300, "GRAD_GENERIC_W1"), ("grad", 4, 512, 32, True, 64, "GRAD_GENERIC_W1"),
       ("grad", 4, 1024, 2, False, 40, "GRAD_GENERIC_W1"),
       ("grad", 16, 128, 4, False, 112, "GRAD_GENERIC_W1"), ("grad", 16, 128, 4, False, 113, "GRAD_F32_KT1_HALF_W4"),  # 7 / 8 tiles
       ("grad_perm", 21, 64, 3, False, 5000, "GRAD_GENERIC_W1"), ("grad_noadv", 21, 64, 3, False, 9000, "GRAD_GENERIC_W4")]
    # ---- gradient: f32 column-parallel kernels
    + _wide_grad_cases()
    + [("grad", 21, 256, 3, False, 256, "GRAD_F32_KT2_HALF_W8_DEFER"),  # Basic at the reference's literal batch_size
       ("grad", 16, 128, 16, False, 500, "GRAD_F32_KT1_HALF_W4"), ("grad", 32, 192, 32, True, 600, "GRAD_F32_KT2_HALF_W4"),
       ("grad_perm", 16, 128, 4, True, 1000, "GRAD_F32_KT1_HALF_W4"), ("grad_noadv", 21, 256, 3, False, 2000, "GRAD_F32_KT2_FULL_W8")]
    # small7: H = 256, 33..112 observations, <= 1024 samples (the reference's ant task at its literal batch), dW2 deferred
    + [("grad", D, 256, A, cont, B, "GRAD_F32_SMALL7") for (D, A, cont) in ((33, 2, False), (105, 8, True), (112, 16, False))
       for B in (256, 1000, 1024)]
    + [("grad", 33, 256, 2, False, 113, "GRAD_F32_SMALL7"), ("grad_perm", 105, 256, 8, True, 700, "GRAD_F32_SMALL7"),
       ("grad_noadv", 112, 256, 1, True, 500, "GRAD_F32_SMALL7")]
    # kt1 = 107: 97..112 observations, Box head, H = 256, past the small7 range; dz1 cached or recomputed
    + [("grad", D, 256, 8, True, B, "GRAD_F32_KT107_CACHED") for D in (97, 105, 112) for B in (1025, 33000)]
    + [("grad_nodz1", 97, 256, 8, True, 1025, "GRAD_F32_KT107_RECOMPUTE"), ("grad_nodz1", 112, 256, 32, True, 33000, "GRAD_F32_KT107_RECOMPUTE"),
       ("grad_perm", 105, 256, 8, True, 2000, "GRAD_F32_KT107_CACHED"), ("grad_noadv", 105, 256, 1, True, 1500, "GRAD_F32_KT107_CACHED")]
    # kt1 = 11: 161..176 observations (Crawler's 172)
    + [("grad", 161, 128, 4, False, 1025, "GRAD_F32_KT11_CACHED"), ("grad", 176, 192, 3, False, 2000, "GRAD_F32_KT11_CACHED"),
       ("grad", 176, 256, 20, True, 33000, "GRAD_F32_KT11_CACHED"), ("grad", 172, 256, 2, False, 500, "GRAD_F32_KT11_CACHED"),
       ("grad_nodz1", 161, 256, 6, True, 1500, "GRAD_F32_KT11_RECOMPUTE"), ("grad_nodz1", 176, 128, 2, False, 1025, "GRAD_F32_KT11_RECOMPUTE"),
       ("grad_perm", 172, 256, 20, True, 2000, "GRAD_F32_KT11_CACHED"), ("grad_noadv", 172, 128, 16, False, 700, "GRAD_F32_KT11_CACHED")]
    # runtime width (kt1 = 0)
    + [("grad", 33, 128, 3, False, 500, "GRAD_F32_KT0"), ("grad", 96, 256, 4, True, 2000, "GRAD_F32_KT0"),
       ("grad", 113, 256, 4, True, 1025, "GRAD_F32_KT0"), ("grad", 113, 256, 2, False, 1000, "GRAD_F32_KT0"),
       ("grad", 177, 256, 5, False, 1000, "GRAD_F32_KT0"), ("grad", 33, 256, 2, False, 1025, "GRAD_F32_KT0"),
       ("grad_perm", 60, 128, 4, False, 600, "GRAD_F32_KT0"), ("grad_noadv", 60, 192, 1, True, 800, "GRAD_F32_KT0")]
    # TMA_NO_DEFER_W2: eight-wave half groups accumulate dW2 in the slabs; the Ant literal batch leaves small7 for the two-pass kernel
    + [("grad_nodefer", 16, 256, 5, False, 1000, "GRAD_F32_KT1_HALF_W8_SLAB"), ("grad_nodefer", 21, 256, 3, False, 256, "GRAD_F32_KT2_HALF_W8_SLAB"),
       ("grad_nodefer", 105, 256, 8, True, 256, "GRAD_F32_KT107_CACHED")]
    # ---- gradient: the three-term bf16 split of the 256 x 256 f32 update
    + _s3_grad_cases()
    # ---- gradient: bf16 column-parallel kernels, every leaf
    + _bf_grad_cases()
    # ---- forward: every launch_fwd leaf at the tile edges; the grid caps (wide: 4096 groups of 32 rows; generic: 8192 blocks)
    + [("fwd", D, H, A, cont, n, ident) for (D, H, A, cont, ident) in _FWD_SHAPES for n in _N_EDGES]
    + [("fwd_bf16", D, H, A, cont, n, ident) for (D, H, A, cont, ident) in _FWD_BF_SHAPES for n in _N_EDGES]
    + [("fwd", 4, 64, 5, False, 131072 + 17, "FWD_H64"), ("fwd", 6, 128, 3, True, 131072 + 17, "FWD_F32_NTW2_BOX|GRID_CAPPED"),
       ("fwd", 6, 256, 5, False, 131072, "FWD_F32_NTW4_DISCRETE"), ("fwd_bf16", 6, 128, 4, False, 131072 + 17, "FWD_BF16_NTW2_DISCRETE|GRID_CAPPED"),
       ("fwd", 4, 64, 2, True, 20000, "FWD_GENERIC_W4"), ("fwd", 4, 64, 2, True, 8192 * 4 * 16 + 17, "FWD_GENERIC_W4|GRID_CAPPED"),
       ("fwd", 200, 64, 3, False, 16400, "FWD_GENERIC_W2"), ("fwd", 400, 64, 3, False, 8192 * 16 + 17, "FWD_GENERIC_W1|GRID_CAPPED")]
    # ---- optimizer: every tma_ppo_adam_step / _local leaf
    + [("opt", 4, 64, 5, False, 256, "OPT_SCATTER_H64"), ("opt", 16, 128, 4, False, 256, "OPT_SCATTER_WIDE"),
       ("opt", 8, 192, 3, True, 256, "OPT_SCATTER_WIDE"), ("opt", 105, 256, 8, True, 256, "OPT_SCATTER_WIDE"),
       ("opt_bf16", 6, 256, 5, False, 1000, "OPT_SCATTER_WIDE"),
       ("opt", 6, 64, 4, True, 256, "OPT_SMALL"), ("opt", 21, 64, 3, False, 256, "OPT_SMALL"),  # (P <= 10240: registers; beyond: a loop)
       ("opt", 8, 320, 4, False, 256, "OPT_ADAM"),
       ("opt_local", 4, 64, 5, False, 256, "OPT_LOCAL_SCATTER_H64"), ("opt_local", 4, 64, 5, False, 255, "OPT_SCATTER_H64"),
       ("opt_local", 16, 128, 4, False, 128, "OPT_LOCAL_SCATTER_WIDE"), ("opt_local", 16, 128, 4, False, 127, "OPT_SCATTER_WIDE"),
       ("opt_local", 105, 256, 8, True, 256, "OPT_LOCAL_SCATTER_WIDE"), ("opt_local", 16, 256, 5, False, 2000, "OPT_LOCAL_SCATTER_WIDE"),
       ("opt_local", 21, 64, 3, False, 256, "OPT_SMALL"), ("opt_local_bf16", 6, 256, 5, False, 1000, "OPT_LOCAL_SCATTER_WIDE"),
       # split policies: the scatter also writes the three weight planes (tma_policy.hip, L.split)
       ("opt_bf16x3", 6, 256, 5, False, 4096, "OPT_SCATTER_WIDE"), ("opt_local_bf16x3", 17, 256, 16, False, 4096, "OPT_LOCAL_SCATTER_WIDE")]
)


def dispatch_ids():
    """TMA_DISPATCH_<NAME> -> value, parsed from include/tma.h."""
    text = open(os.path.join(ROOT, "include", "tma.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\bTMA_DISPATCH_([A-Z0-9_]+)\s*=\s*(\d+)", text)}


def expected_value(name):
    ids = dispatch_ids()
    v = 0
    for part in name.split("|"):
        v |= ids[part]
    return v


def _case_id(c):
    entry, D, H, A, cont, B, ident = c
    return f"{entry}-{D}x{H}x{A}{'C' if cont else 'D'}-{B}"


def _cases(prefix):
    return [pytest.param(*c, id=_case_id(c)) for c in CASES if c[0].split("_")[0] == prefix]


def _last_dispatch():
    from three_mlagents_amd import _lib

    f, g, o = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    _lib.check(_lib.lib().tma_debug_last_dispatch(C.byref(f), C.byref(g), C.byref(o)))
    return f.value, g.value, o.value


PLAN_WHICH = {"fwd": 0, "grad": 1, "opt": 2, "opt_local": 3}  # TMA_PLAN_* of include/tma.h


def planned(dims, which, n):
    """(status, id, grid, block, lds_bytes) of tma_debug_plan_dispatch: what the dispatcher `which` would choose for n rows.  No GPU work."""
    from three_mlagents_amd import _lib

    i, g, b, l = C.c_int32(-1), C.c_int64(-1), C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().tma_debug_plan_dispatch(C.byref(dims), PLAN_WHICH[which], n, C.byref(i), C.byref(g), C.byref(b), C.byref(l))
    return rc, i.value, g.value, b.value, l.value


def _entry_which(entry):
    return "opt_local" if entry.startswith("opt_local") else entry.split("_")[0]


def _name(v):
    names = [k for k, x in dispatch_ids().items() if x == v & 0xFF and k != "GRID_CAPPED"]
    return "|".join(names + (["GRID_CAPPED"] if v & 256 else []))


def case_state_dict(D, H, A, cont, seed=5):
    """The test policies' parameters without a GPU: the engine's orthogonal init with the heads made non-trivial -- what _policy loads (the
    state_dict round trip through the engine's [in][out] layout is exact: tests/test_ppo_gpu.py asserts it)."""
    from test_ppo_gpu import _nontrivial_heads
    from three_mlagents_amd.ppo import orthogonal_init

    return _nontrivial_heads(orthogonal_init(D, H, A, cont, seed), A, cont, seed)


def _policy(D, H, A, cont, dtype="f32", seed=5):
    if dtype == "bf16x3":
        from three_mlagents_amd.ppo import HipActorCriticPolicy

        sd = case_state_dict(D, H, A, cont, seed)
        pol = HipActorCriticPolicy(D, A, cont, H, torch.device("cuda", 0), seed=seed, mfma_dtype="bf16x3")
        pol.load_state_dict(sd)
        back = pol.state_dict()
        assert all(torch.equal(sd[k], back[k]) for k in sd)
        return pol, sd
    if dtype == "f32":
        from test_ppo_gpu import _policy as make
    else:
        from test_bf16_gpu import _policies as make
    return make(D, H, A, cont, seed)


def _rows(D, A, cont, total, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(total, D, generator=g)
    act = torch.randn(total, A, generator=g) * 0.7 if cont else torch.randint(0, A, (total,), generator=g, dtype=torch.int32)
    return g, obs, act


def _sd64(sd):
    return {k: v.detach().double() for k, v in sd.items()}


def _rollout(sd, D, A, cont, T, N, seed=0, bf=False, distinct=0):
    """(T, N, ...) rollout buffers whose old log-probabilities keep every sample CLIP_MARGIN away from the clip boundary in float64
    (bf: in the float64 emulation of the bf16 forward, which is what the bf16 kernels' ratios are near).  distinct > 0: every observation
    row is one of `distinct` rows (a correlated minibatch: GridWorld early in training)."""
    g, flat, act = _rows(D, A, cont, T * N, seed)
    if distinct:
        flat = flat[:distinct][torch.randint(0, distinct, (T * N,), generator=g)].contiguous()
    with torch.no_grad():
        if bf:
            lp64 = _logp(_emulated_forward64(sd, flat)[0], _sd64(sd), act, cont)
        else:
            _, lp64, _ = sb3_ref.evaluate_actions(_sd64(sd), flat.double(), act.double() if cont else act)
    old = (lp64 + 0.25 * torch.randn(T * N, generator=g, dtype=torch.float64)).float()
    for _ in range(10):
        near = (((torch.exp(lp64 - old.double()) - 1.0).abs() - 0.2).abs() < CLIP_MARGIN)
        if not near.any():
            break
        old = torch.where(near, old + 0.05, old)
    assert not near.any()
    adv, ret = torch.randn(T * N, generator=g), torch.randn(T * N, generator=g)
    # the kernels read (T, N, ...) buffers with the flat index f = i*T + t: store row f at [t, i]
    to_tn = lambda x: x.reshape(N, T, *x.shape[1:]).transpose(0, 1).contiguous()  # noqa: E731
    return dict(obs=to_tn(flat), actions=to_tn(act), old_lp=to_tn(old), adv=to_tn(adv), ret=to_tn(ret)), dict(obs=flat, actions=act, old_lp=old, adv=adv, ret=ret)


def _grads(sd, rows, idx, dtype, hp):
    """(grads in SB3 naming, stats) of the PPO loss over rows[idx] in `dtype` (float64: the reference; float32: the calibration)."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    if len(idx) == 0:
        return {k: torch.zeros_like(v) for k, v in p.items()}, None
    cont = "log_std" in sd
    x = {k: v[idx] for k, v in rows.items()}
    acts = x["actions"].to(dtype) if cont else x["actions"]
    loss, stats = sb3_ref.ppo_loss(p, x["obs"].to(dtype), acts, x["old_lp"].to(dtype), x["adv"].to(dtype), x["ret"].to(dtype), **hp)
    loss.backward()
    return {k: v.grad.detach() for k, v in p.items()}, stats


HP = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5, normalize_advantage=True)


def _segment_errors(g, ref, cal):
    """per segment: (err of g against ref, err of the calibration against ref, max |ref|)"""
    return {k: (float((g[k].double() - ref[k]).abs().max()), float((cal[k].double() - ref[k]).abs().max()), float(ref[k].abs().max())) for k in ref}


def _rejects(errs, k=K, f=F):
    return any(e > k * e32 + f * m for e, e32, m in errs.values())


def _emulated_grads(sd, rows, idx, dtype, hp):
    """(grads in SB3 naming, stats) of the PPO loss over rows[idx] with the bf16 kernels' rounding points (test_bf16_gpu._emulated_grad), sums
    and loss in `dtype` (float64: the reference of the bf16 gradient rows; float32: their calibration)."""
    from test_bf16_gpu import _emulated_grad

    if len(idx) == 0:
        return {k: torch.zeros_like(v, dtype=dtype) for k, v in sd.items()}, None
    x = {k: v[idx] for k, v in rows.items()}
    return _emulated_grad(sd, x["obs"], x["actions"], x["old_lp"], x["adv"], x["ret"], hp, dtype)


def _run_child(request, env, record_property=None):
    """Run this very case in a child process with `env` added (switches read once per process); the properties the child records are
    recorded here as well, so that the case's figures reach the parent's report."""
    import tempfile
    import xml.etree.ElementTree as ET

    e = dict(os.environ, **env)
    node = request.node.nodeid.split("::", 1)[1]
    with tempfile.TemporaryDirectory() as tmp:
        report = os.path.join(tmp, "child.xml")
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", f"--junitxml={report}",
                            f"{os.path.join(HERE, os.path.basename(__file__))}::{node}"], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
        if record_property is not None:
            for p in ET.parse(report).getroot().iter("property"):
                record_property(p.get("name"), p.get("value"))


def entry_dtype_kind(entry):
    """("f32" | "bf16" | "bf16x3", the entry without its dtype suffix)"""
    for suffix in ("_bf16x3", "_bf16"):
        if entry.endswith(suffix):
            return suffix[1:], entry[:-len(suffix)]
    return "f32", entry


def s3_emulated_grads(sd, rows, idx, dtype, hp):
    from _split3_ref import emulated_grads

    return emulated_grads(sd, rows, idx, dtype, hp)


def grad_case_inputs(entry, D, A, cont, B, sd):
    """Everything of a gradient case that needs no GPU (tests/test_split3_ref_cpu.py checks the bf16x3 rows' inputs from it): hyper-parameters,
    (T, N, ...) buffers and their flat rows, the permutation and the minibatch's row indices, the rows of the last row tile."""
    dtype, kind = entry_dtype_kind(entry)
    bf = dtype == "bf16"
    drop = B % 16 or 16  # rows of the last row tile
    heavy = bf and bf_heavy_tile(B)
    hp = dict(HP, normalize_advantage=kind != "grad_noadv" and not heavy)
    start = 3
    T = 16
    N = (start + B + T - 1) // T + 1
    # (bf16 rows: a data seed of their own, under which every dropped-tile reference overshoots K_BF_G, F_BF_G at least fourfold: checked on the CPU,
    #  from the float64 and float32 emulations alone.  Under the f32 rows' seed the one row of the 16 x H x 5 Discrete minibatches' last tile is a
    #  clipped sample with a return of 0.006: thirty times nothing.  bf16x3 rows: S3_SEED, for the same reason)
    bufs, rows = _rollout(sd, D, A, cont, T, N, seed=B % 7919 + {"f32": 0, "bf16": 30000, "bf16x3": S3_SEED}[dtype], bf=bf,
                          distinct=4 if kind == "grad_corr" else 0)
    total = T * N
    if kind == "grad_perm":
        from three_mlagents_amd import _lib

        perm_np = np.zeros(total, dtype=np.int64)
        _lib.check(_lib.lib().tma_ppo_permutation(77, 3, total, perm_np.ctypes.data_as(C.c_void_p)))
        perm = torch.from_numpy(perm_np)
    else:
        perm = torch.randperm(total, generator=torch.Generator().manual_seed(B))
    idx = perm[start:start + B]
    if heavy:  # the last row tile's advantages and returns times BF_HEAVY (flat row f lies at [f % T, f // T] of the buffers)
        last = idx[B - drop:]
        for k in ("adv", "ret"):
            rows[k][last] *= BF_HEAVY
            bufs[k][last % T, last // T] *= BF_HEAVY
    return dict(hp=hp, start=start, T=T, N=N, bufs=bufs, rows=rows, perm=perm, idx=idx, drop=drop)


def budget_use(e, e32, m, k, f):
    return e / (k * e32 + f * m) if (e32 or m) else (0.0 if e == 0 else math.inf)


@pytest.mark.parametrize("entry,D,H,A,cont,B,ident", _cases("grad"))
def test_gradient_branch_against_float64(entry, D, H, A, cont, B, ident, monkeypatch, request, record_property):
    """f32 rows: float64 / float32 torch autograd (see the module docstring).  bf16 rows (grad_*_bf16): reference = the emulation with the
    kernel's bf16 rounding points in float64, calibration = the same emulation in float32; per segment (log_std included)
    err_kernel <= K_BF_G * err_emu32 + F_BF_G * max|g64|, exact clip count, the four averaged statistics within S_BF_G, and the comparator
    must reject the float64 emulation of the minibatch without its last row tile.  bf16x3 rows (grad_*_bf16x3): the same with the split's
    emulation (tests/_split3_ref.py), K_S3, F_S3 and the f32 rows' 2e-6 on the statistics; their distance from plain float64 is recorded."""
    from test_ppo_gpu import _hip_grad

    dtype, kind = entry_dtype_kind(entry)
    bf = dtype == "bf16"
    if entry in SWITCH_ENTRIES and os.environ.get(SWITCH_ENTRIES[entry]) != "1":
        return _run_child(request, {SWITCH_ENTRIES[entry]: "1"}, record_property)
    if kind == "grad_nodz1":
        monkeypatch.setenv("TMA_NO_DZ1_CACHE", "1")
    pol, sd = _policy(D, H, A, cont, dtype)
    c = grad_case_inputs(entry, D, A, cont, B, sd)
    hp, start, T, N, bufs, rows, perm, idx, drop = (c[k] for k in ("hp", "start", "T", "N", "bufs", "rows", "perm", "idx", "drop"))
    if kind == "grad_perm":
        grad, st, _ = _hip_grad(pol, bufs, T, N, None, start, B, hp, perm=(77, 3))
    else:
        grad, st, _ = _hip_grad(pol, bufs, T, N, perm, start, B, hp)
    got = _last_dispatch()[1]
    assert got == expected_value(ident), (ident, _name(got))
    plan = planned(pol.dims, "grad", B)
    assert plan[:2] == (0, got)
    g = pol.named_from_flat(grad)
    if bf:
        assert plan[2:4] == bf_expected_geometry(ident, cont, B) and 0 <= plan[4] <= 160 * 1024, plan
        k, f, s_tol, ref_fn = K_BF_G, F_BF_G, S_BF_G, _emulated_grads
    elif dtype == "bf16x3":
        k, f, s_tol, ref_fn = K_S3, F_S3, 2e-6, s3_emulated_grads
    else:
        k, f, s_tol, ref_fn = K, F, 2e-6, _grads
    g64, s64 = ref_fn(sd, rows, idx, torch.float64, hp)
    g32, _ = ref_fn(sd, rows, idx, torch.float32, hp)
    assert dtype == "f32" or set(g) == set(g64)
    errs = _segment_errors(g, g64, g32)
    gdrop, _ = ref_fn(sd, rows, idx[:B - drop], torch.float64, hp)
    errs_drop = _segment_errors(gdrop, g64, g32)
    use = lambda e, e32, m: budget_use(e, e32, m, k, f)  # noqa: E731
    budget = max(use(*v) for v in errs.values())
    record_property("grad_errs", repr({"budget": budget, "drop_overshoot": max(use(*v) for v in errs_drop.values()), "errs": errs,
                                       "drop": {key: v[0] for key, v in errs_drop.items()}}))
    if dtype == "bf16x3":  # the design trade on record: kernel and emulation against plain float64 autograd, in units of the segment's max |g|
        gp, _ = _grads(sd, rows, idx, torch.float64, hp)
        record_property("plain64", repr({key: (float((g[key].double() - gp[key]).abs().max()) / float(gp[key].abs().max()),
                                               float((g64[key] - gp[key]).abs().max()) / float(gp[key].abs().max())) for key in gp}))
    print(f"{_case_id((entry, D, H, A, cont, B, ident))}: budget use {budget:.3f} ({max(errs, key=lambda s: use(*errs[s]))}), dropped tile "
          f"{max(use(*v) for v in errs_drop.values()):.1f}")
    # statistics: sums of {policy_loss, value_sq_err, entropy, approx_kl, clipped, n} (the last two exact); no optimizer step on this workspace
    n = st[5]
    stats = ((st[0] / n, s64["policy_loss"], "policy_loss"), (st[1] / n, s64["value_loss"], "value_loss"),
             (-st[2] / n, s64["entropy_loss"], "entropy_loss"), (st[3] / n, s64["approx_kl"], "approx_kl"))
    record_property("stats_errs", repr({what: abs(got_v - ref_v) / max(1.0, abs(ref_v)) for got_v, ref_v, what in stats}))
    assert n == B
    assert st[4] == round(s64["clip_fraction"] * B), (st[4], s64["clip_fraction"] * B)
    for got_v, ref_v, what in stats:
        assert abs(got_v - ref_v) <= s_tol * max(1.0, abs(ref_v)), (what, got_v, ref_v)
    assert st[6] == 0.0 and st[7] == 0.0
    bad = {key: v for key, v in errs.items() if v[0] > k * v[1] + f * v[2]}
    assert not bad, bad
    assert _rejects(errs_drop, k, f), ("the comparator does not see the last row tile dropped", errs_drop)


def _emulated_forward64(sd, obs):
    from test_bf16_gpu import _bf

    def net(prefix, head):
        h = _bf(obs).double()
        for i in (0, 2):
            h = _bf(torch.tanh(h @ _bf(sd[f"mlp_extractor.{prefix}.{i}.weight"]).double().t() + sd[f"mlp_extractor.{prefix}.{i}.bias"].double()).float()).double()
        return h @ _bf(sd[f"{head}.weight"]).double().t() + sd[f"{head}.bias"].double()

    return net("policy_net", "action_net"), net("value_net", "value_net").squeeze(-1)


def _logp(out, sd, a, cont):
    if cont:
        ls = sd["log_std"].to(out.dtype)
        return (-((a.to(out.dtype) - out) ** 2) / (2 * torch.exp(2 * ls)) - ls - 0.5 * math.log(2 * math.pi)).sum(dim=1)
    return torch.log_softmax(out, dim=1).gather(1, a.long().view(-1, 1)).squeeze(1)


@pytest.mark.parametrize("entry,D,H,A,cont,n,ident", _cases("fwd"))
def test_forward_branch_against_float64(entry, D, H, A, cont, n, ident, record_property):
    from three_mlagents_amd import _lib

    bf = entry == "fwd_bf16"
    pol, sd = _policy(D, H, A, cont, "bf16" if bf else "f32")
    g = torch.Generator().manual_seed(n)
    obs = torch.randn(n, D, generator=g)
    sd64 = _sd64(sd)
    if bf:  # reference: the same rounding points as the kernel (bf16 operands) in float64; calibration: the same in float32
        from test_bf16_gpu import _emulated_forward

        out64, v64 = _emulated_forward64(sd, obs)
        out32, v32 = _emulated_forward(sd, obs)
        k, f = K_BF, F_BF
    else:
        out64, v64 = sb3_ref.forward(sd64, obs.double())
        out32, v32 = sb3_ref.forward(sd, obs)
        k, f = K, F

    def close(got, ref, cal, what):
        e, e32, m = float((got.double() - ref).abs().max()), float((cal.double() - ref).abs().max()), float(ref.abs().max())
        record_property(what, repr((e, e32, m)))
        assert e <= k * e32 + f * max(m, 1.0), (what, e, e32, m)

    def check_id():
        got = _last_dispatch()[0]
        assert got == expected_value(ident), (ident, _name(got))
        assert planned(pol.dims, "fwd", n)[:2] == (0, got)

    a, v, lp = pol.act(obs.cuda(), deterministic=True)
    check_id()
    close(v.cpu(), v64, v32, "values")
    if cont:
        close(a.cpu(), out64, out32, "mean")
    else:
        top2 = out64.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > (2e-2 if bf else 1e-4)  # rows whose argmax is not a near-tie
        assert torch.equal(a.cpu().long()[clear], out64.argmax(dim=1)[clear])
    close(lp.cpu(), _logp(out64, sd64, a.cpu(), cont), _logp(out32, sd, a.cpu(), cont), "logp_det")
    a, v2, lp = pol.act(obs.cuda(), rng_seed=9, rng_step=3, deterministic=False)
    check_id()
    close(lp.cpu(), _logp(out64, sd64, a.cpu(), cont), _logp(out32, sd, a.cpu(), cont), "logp_sampled")
    close(pol.predict_values(obs.cuda()).cpu(), v64, v32, "predict_values")
    check_id()
    trunc = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
    rew = torch.randn(n, generator=g)
    obs_d, trunc_d, rew_d = obs.cuda(), trunc.cuda(), rew.cuda()  # (held: the launch is asynchronous)
    _lib.check(_lib.lib().tma_policy_bootstrap(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs_d), _lib.ptr(trunc_d), n, 0.99,
                                               _lib.ptr(rew_d), _lib.stream_ptr()))
    check_id()
    t = trunc.bool()
    close(rew_d.cpu(), torch.where(t, rew.double() + 0.99 * v64, rew.double()), torch.where(t, rew + 0.99 * v32, rew), "bootstrap")


@pytest.mark.parametrize("entry,D,H,A,cont,B,ident", _cases("opt"))
def test_optimizer_branch_against_float64_adam(entry, D, H, A, cont, B, ident, record_property):
    """The same kernel-produced gradient goes to the device step and to float64 torch.optim.Adam(eps=1e-5) + clip_grad_norm_: three steps
    with the clip engaged, three without, three with grad_scale = 0.5 (tma_ppo_adam_step only); parameters and both moments compared.
    After every run tma_policy_sync must change no bit (the step kept every derived copy consistent).  Split policies (opt_*_bf16x3) take one
    more gradient at the stepped parameters after each run and hold it to the bf16x3 rows' comparator.
    Also measured against IEEE float32 Adam (torch CPU, foreach=False, on the device's own clipped gradient), in units of 2^-23 (|p| + lr):
    see the figure next to the assertion."""
    from test_ppo_gpu import _hip_grad
    from three_mlagents_amd import _lib

    local = entry.startswith("opt_local")
    dtype = entry_dtype_kind(entry)[0]
    T = 16
    N = (B + T - 1) // T + 1
    runs = [(0.05, 1.0), (1e3, 1.0)] + ([] if local else [(0.05, 0.5)])
    lr, b1, b2, eps = 3e-4, 0.9, 0.999, 1e-5
    for max_norm, scale in runs:
        pol, sd = _policy(D, H, A, cont, dtype)
        P = pol.n_trainable
        dev = pol.params.device
        m = torch.zeros(P, device=dev)
        v = torch.zeros(P, device=dev)
        p64 = torch.nn.Parameter(pol.params[:P].detach().cpu().double().clone())
        opt64 = torch.optim.Adam([p64], lr=lr, betas=(b1, b2), eps=eps)
        p32 = torch.nn.Parameter(pol.params[:P].detach().cpu().clone())
        opt32 = torch.optim.Adam([p32], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
        for step in range(1, 4):
            bufs, _ = _rollout(pol.state_dict(), D, A, cont, T, N, seed=step)
            grad, _, ws = _hip_grad(pol, bufs, T, N, torch.arange(T * N), 0, B, HP)
            g = grad.detach().cpu().clone()
            if local:
                rc = _lib.lib().tma_ppo_adam_step_local(_lib.ptr(pol.params), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), C.byref(pol.dims), step, lr, b1, b2,
                                                        eps, max_norm, _lib.ptr(ws), _lib.stream_ptr(), B)
            else:
                rc = _lib.lib().tma_ppo_adam_step(_lib.ptr(pol.params), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), C.byref(pol.dims), step, lr, b1, b2,
                                                  eps, max_norm, scale, _lib.ptr(ws), _lib.stream_ptr())
            got = _last_dispatch()[2]
            _lib.check(rc)
            assert got == expected_value(ident), (ident, _name(got))
            assert planned(pol.dims, _entry_which(entry), B)[:2] == (0, got)
            out = (C.c_double * 8)()
            _lib.check(_lib.lib().tma_ppo_pop_stats(_lib.ptr(ws), out, _lib.stream_ptr()))
            assert float(grad.abs().max()) == 0.0  # re-zeroed for the next minibatch
            # float64 reference
            p64.grad = g.double() * scale
            norm64 = float(torch.nn.utils.clip_grad_norm_([p64], max_norm))
            coef64 = min(1.0, max_norm / (norm64 + 1e-6))
            opt64.step()
            # IEEE float32 Adam on the device's own clipped gradient (the form the scatter kernels approximate with hardware sqrt / rcp)
            p32.grad = (g * np.float32(scale)) * np.float32(out[7])
            opt32.step()
            pd = pol.params[:P].detach().cpu()
            st64 = opt64.state[p64]
            e_p = float(((pd.double() - p64.detach()).abs() / (2.0 ** -19 * p64.detach().abs() + 4e-5 * lr)).max())
            e_ieee = float(((pd - p32.detach()).abs() / (2.0 ** -23 * (p32.detach().abs() + lr))).max())
            e_m = float((m.cpu().double() - st64["exp_avg"]).abs().max()) / max(float(st64["exp_avg"].abs().max()), 1e-30)
            e_v = float((v.cpu().double() - st64["exp_avg_sq"]).abs().max()) / max(float(st64["exp_avg_sq"].abs().max()), 1e-30)
            record_property(f"opt_{max_norm}_{scale}_{step}", repr(dict(e_p=e_p, ieee_per_lr=e_ieee, e_m=e_m, e_v=e_v, norm=(out[6], norm64), coef=(out[7], coef64))))
            assert abs(out[6] - norm64) <= 1e-6 * norm64, (out[6], norm64)
            assert abs(out[7] - coef64) <= 1e-6, (out[7], coef64)
            assert (coef64 < 1.0) == (max_norm < 1.0), "clip engagement is not what the run is meant to test"
            assert e_p <= 1.0, (step, e_p)  # |p - p64| <= 2^-19 |p64| + 4e-5 lr, element by element (observed: 0.32 of it, step 2; 0.50 on 7 x 64 x 3, step 3)
            # (the kernels form 1 - beta1 and 1 - beta2 in float32 from float32 betas: 1 - 0.999f = 0.00099998713, 1.29e-5 off 0.001 -- exp_avg_sq
            #  carries that relative offset, exp_avg 2.4e-7; observed 1.30e-5 / 3.8e-7.  In the parameters it is <= 6.4e-6 of lr per step)
            assert e_m <= 1e-6 and e_v <= 2.6e-5, (step, e_m, e_v)
            # against IEEE float32 Adam, in units of 2^-23 (|p| + lr): observed <= 102 on the wide scatter (hardware sqrt / rcp) and <= 101 on the
            # IEEE-arithmetic kernels alike -- the difference is the float32 1 - beta2 above, not the hardware square root / reciprocal
            # (167 on 7 x 64 x 3 at step 3: what three steps of that 6.4e-6 lr come to where |p| << lr, 161 of these units, plus rounding)
            assert e_ieee <= 256, (step, e_ieee)
        if dtype == "bf16x3":
            # one more gradient, at the stepped parameters, held to the bf16x3 rows' comparator against the emulation on pol.state_dict(): the split
            # kernel reads the three weight planes the scatter maintained, so a plane left stale (the planes of the weights three steps ago are
            # ~1e-3 off) shows in the numbers.  (The sync check below proves the planes equal a rebuild; this one that the rebuild is the right split.)
            sd_now = pol.state_dict()
            bufs, rows = _rollout(sd_now, D, A, cont, T, N, seed=4 + S3_SEED)
            idx = torch.arange(B)
            grad, st, _ = _hip_grad(pol, bufs, T, N, torch.arange(T * N), 0, B, HP)
            assert _last_dispatch()[1] == expected_value("GRAD_BF16X3") and st[5] == B
            gk = pol.named_from_flat(grad)
            g64, _ = s3_emulated_grads(sd_now, rows, idx, torch.float64, HP)
            g32, _ = s3_emulated_grads(sd_now, rows, idx, torch.float32, HP)
            gdrop, _ = s3_emulated_grads(sd_now, rows, idx[:B - 16], torch.float64, HP)
            errs, errs_drop = _segment_errors(gk, g64, g32), _segment_errors(gdrop, g64, g32)
            record_property(f"grad_after_{max_norm}_{scale}", repr({"budget": max(budget_use(*v, K_S3, F_S3) for v in errs.values()),
                                                                    "drop_overshoot": max(budget_use(*v, K_S3, F_S3) for v in errs_drop.values()), "errs": errs}))
            bad = {key: v for key, v in errs.items() if v[0] > K_S3 * v[1] + F_S3 * v[2]}
            assert not bad, bad
            assert _rejects(errs_drop, K_S3, F_S3), ("the comparator does not see the last row tile dropped", errs_drop)
        after = pol.params.clone()
        _lib.check(_lib.lib().tma_policy_sync(_lib.ptr(pol.params), C.byref(pol.dims), _lib.stream_ptr()))
        assert torch.equal(after, pol.params), "the optimizer step left a derived copy out of date"


@pytest.mark.parametrize("D,H,A,cont", [(2500, 64, 3, False), (600, 1024, 2, True), (2100, 256, 4, False)])
def test_accepted_but_unrunnable_shapes_are_refused_by_every_entry_point(D, H, A, cont):
    """check_dims accepts these shapes (obs_dim <= 4096, hidden <= 1024), but one wave's LDS tile of the generic kernels does not fit:
    every entry point must return TMA_ERR_INVALID with a message before it launches anything."""
    from three_mlagents_amd import _lib
    from three_mlagents_amd.ppo import HipActorCriticPolicy

    L = _lib.lib()
    pol = HipActorCriticPolicy(D, A, cont, H, torch.device("cuda", 0), seed=1)
    n, T, N = 40, 4, 10
    dev = pol.params.device
    obs = torch.randn(n, D, device=dev)
    acts = torch.zeros((n, A) if cont else (n,), dtype=torch.float32 if cont else torch.int32, device=dev)
    vals, logp, rew = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    trunc = torch.ones(n, dtype=torch.uint8, device=dev)
    s = _lib.stream_ptr()
    calls = {
        "act": lambda: L.tma_policy_act(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), n, 1, 2, 0, 0, _lib.ptr(acts), _lib.ptr(vals), _lib.ptr(logp), s),
        "act_bootstrap": lambda: L.tma_policy_act_bootstrap(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), n, 1, 2, 0, _lib.ptr(acts), _lib.ptr(vals),
                                                            _lib.ptr(logp), _lib.ptr(obs), _lib.ptr(trunc), 0.99, _lib.ptr(rew), s),
        "values": lambda: L.tma_policy_values(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), n, _lib.ptr(vals), s),
        "bootstrap": lambda: L.tma_policy_bootstrap(_lib.ptr(pol.params), C.byref(pol.dims), _lib.ptr(obs), _lib.ptr(trunc), n, 0.99, _lib.ptr(rew), s),
    }
    for name, call in calls.items():
        assert call() == _lib.TMA_ERR_INVALID, name
        assert "LDS" in _lib.last_error(), (name, _lib.last_error())
        assert _last_dispatch()[0] == 0, name
    rv = _lib.Rollout(_lib.ptr(obs), _lib.ptr(acts), _lib.ptr(logp), _lib.ptr(vals), _lib.ptr(rew), T, N)
    mb = _lib.Minibatch(None, 1, 0, 0, n)
    hp = _lib.PPOHParams(0.2, 0.01, 0.5, 1)
    grad = torch.zeros(pol.n_trainable, device=dev)
    ws = torch.zeros(int(L.tma_ppo_workspace_bytes(C.byref(pol.dims))), dtype=torch.uint8, device=dev)
    rc = L.tma_ppo_minibatch_grad(_lib.ptr(pol.params), C.byref(pol.dims), C.byref(rv), C.byref(mb), C.byref(hp), _lib.ptr(grad), _lib.ptr(ws), s)
    assert rc == _lib.TMA_ERR_INVALID and "LDS" in _lib.last_error(), _lib.last_error()
    assert _last_dispatch()[1] == 0
    torch.cuda.synchronize()
    assert torch.isfinite(vals).all() and float(rew.abs().max()) == 0.0  # nothing ran
