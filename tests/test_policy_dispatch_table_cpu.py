"""The dispatch-record table of tests/test_policy_dispatch_gpu.py stays complete: every branch id include/tma.h declares has at least one
case that is meant to reach it (so a new specialisation cannot ship without a float64 reference test), and every case names ids that
exist; and the host-only query tma_debug_plan_dispatch -- the pure plan functions of csrc/tma_policy_plan.h behind every launch -- gives every
case the id the table expects and refuses what the real calls refuse.  Where one id stands for several compile-time variants the table is checked
one level down: every bf16 gradient leaf at every width and head, and every variant of the H = 64 image kernels (observation-width class, head
width, either kernel) together with every task shape that trains on them; the inputs of the H = 64 rows are checked from the references alone
(the comparator must see their last row tile go).  None of this touches a GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def _header_ids():
    text = open(os.path.join(ROOT, "include", "tma.h")).read()
    body = re.search(r"enum\s*\{\s*(TMA_DISPATCH_NONE.*?)\};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ids = {}
    for item in body.split(","):
        m = re.fullmatch(r"\s*TMA_DISPATCH_([A-Z0-9_]+)\s*=\s*(\d+)\s*", item)
        assert m, f"unparsed enum entry {item!r}: give every TMA_DISPATCH_ id an explicit value"
        ids[m.group(1)] = int(m.group(2))
    return ids


def test_every_dispatch_id_has_a_reference_case():
    import torch

    import test_policy_dispatch_gpu as t

    assert not torch.cuda.is_initialized()
    ids = _header_ids()
    assert ids == t.dispatch_ids()
    assert len(set(ids.values())) == len(ids), "two branch ids share a value"
    flag = ids["GRID_CAPPED"]
    assert all(v < flag for k, v in ids.items() if k != "GRID_CAPPED"), "the grid-capped flag must not overlap an id"
    covered, capped = set(), set()
    for entry, D, H, A, cont, B, ident in t.CASES:
        parts = ident.split("|")
        assert all(p in ids for p in parts), ident
        assert parts[0] not in ("NONE", "GRID_CAPPED") and parts[1:] in ([], ["GRID_CAPPED"]), ident
        covered.add(parts[0])
        if parts[1:]:
            capped.add(parts[0])
    missing = sorted(set(ids) - {"NONE", "GRID_CAPPED"} - covered)
    assert not missing, f"branch ids without a case in tests/test_policy_dispatch_gpu.py: {missing}"
    # the kernels that loop over a capped grid: the generic forward at 4 and 1 waves per block, a column-parallel forward, the generic gradient
    need = {"FWD_GENERIC_W4", "FWD_GENERIC_W1", "GRAD_GENERIC_W4"}
    assert need <= capped, sorted(need - capped)
    assert any(c.startswith("FWD_F32_") or c.startswith("FWD_BF16_") for c in capped)
    # every case a distinct test id
    case_ids = [t._case_id(c) for c in t.CASES]
    assert len(case_ids) == len(set(case_ids))


def _case_dims(entry, D, H, A, cont):
    from three_mlagents_amd import _lib

    mfma = 2 if entry.endswith("bf16x3") else (1 if entry.endswith("bf16") else 0)
    return _lib.PolicyDims(D, H, A, int(cont), mfma, -1)


def check_planned_cases(switch_entry=None):
    """tma_debug_plan_dispatch gives every CASES row its id (the table was verified on hardware through tma_debug_last_dispatch), a grid of at
    least one block and at most 160 KB of LDS; a bf16 gradient row the grid (n_pi + n_vf) and block of its leaf as well.  The rows of one
    SWITCH_ENTRIES entry alone when switch_entry names it: their switch is read once per process, so the caller is a child process with it set."""
    import torch

    import test_policy_dispatch_gpu as t

    n = 0
    for entry, D, H, A, cont, B, ident in t.CASES:
        if (entry != switch_entry) if switch_entry else (entry in t.SWITCH_ENTRIES):
            continue
        if entry.startswith("grad_nodz1"):
            os.environ["TMA_NO_DZ1_CACHE"] = "1"
        try:
            rc, got, grid, block, lds = t.planned(_case_dims(entry, D, H, A, cont), t._entry_which(entry), B)
        finally:
            os.environ.pop("TMA_NO_DZ1_CACHE", None)
        case = t._case_id((entry, D, H, A, cont, B, ident))
        assert rc == 0 and got == t.expected_value(ident), (case, rc, t._name(got))
        inner = ident in ("GRAD_H64_SMALL", "GRAD_H64", "GRAD_BF16X3")  # geometry picked by the family's own launcher: LDS -1
        assert grid >= 1 and block >= 64 and block % 64 == 0 and (lds == -1 if inner else 0 <= lds <= 160 * 1024), (case, grid, block, lds)
        if ident.startswith("GRAD_BF16_"):
            assert entry.endswith("_bf16") and block in (256, 512) and (grid, block) == t.bf_expected_geometry(ident, cont, B), (case, grid, block)
        n += 1
    rows = {"grad_nodefer": 3, "grad_nw4_bf16": 3, "grad_mt2_bf16": 1, "grad_nw8_bf16x3": 2}
    assert sorted(rows) == sorted(t.SWITCH_ENTRIES)
    assert n == (rows[switch_entry] if switch_entry else len(t.CASES) - sum(rows.values()))
    assert not torch.cuda.is_initialized()


def test_plan_query_gives_every_case_its_id():
    check_planned_cases()


def _planned_in_child(entry):
    import subprocess

    import test_policy_dispatch_gpu as t

    code = f"import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import test_policy_dispatch_table_cpu as m; m.check_planned_cases({entry!r})"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{t.SWITCH_ENTRIES[entry]: "1"}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])


def test_plan_query_gives_the_no_defer_cases_their_ids_in_a_child_process():
    _planned_in_child("grad_nodefer")


def test_plan_query_gives_the_bf16_four_wave_cases_their_ids_in_a_child_process():
    _planned_in_child("grad_nw4_bf16")


def test_plan_query_gives_the_bf16_32_row_group_case_its_id_in_a_child_process():
    _planned_in_child("grad_mt2_bf16")


def test_plan_query_gives_the_split_eight_wave_cases_their_ids_in_a_child_process():
    _planned_in_child("grad_nw8_bf16x3")


def test_every_bf16_gradient_leaf_has_a_case_at_every_width_and_head_it_takes():
    import test_policy_dispatch_gpu as t

    have = {(ident[len("GRAD_BF16_"):], H, cont) for entry, D, H, A, cont, B, ident in t.CASES if ident.startswith("GRAD_BF16_")}
    both, widths = (False, True), (128, 192, 256)
    want = {(leaf, H, c) for leaf in ("KT1_MT2", "KT2_MT2", "KS2_CACHED", "KS6_CACHED", "RUNTIME") for H in widths for c in both}
    want |= {(leaf, H, c) for leaf in ("KT1_MT4", "KT2_MT4") for H in (128, 256) for c in both}  # (H = 192 only has 32-row groups)
    want |= {("KT1_MT4_W8", 256, False)} | {(leaf, 256, True) for leaf in ("KS6_W8_CACHED", "KS6_W8_RECOMPUTE", "KS4_W8_CACHED", "KS4_W8_RECOMPUTE")}
    want |= {("KS2_RECOMPUTE", 256, False), ("KS6_RECOMPUTE", 256, False)}
    assert want <= have, sorted(want - have)
    # every bf16 gradient row is compared (the dropped-tile rejection included): none of them is a dispatch-only entry
    assert all(e.endswith("_bf16") for e, D, H, A, cont, B, ident in t.CASES if ident.startswith("GRAD_BF16_"))


def h64_grad_class(D, A, B):
    """The compile-time variant tma_launch_grad_h64 (csrc/tma_h64.hip) launches for a Discrete D x 64 x A policy and a minibatch of B samples,
    restated from its code: (kernel, DT, AT, KS1, padded columns).  Up to 128 row tiles of 16 the four-wave small kernel (one tile per wave, no
    compile-time head), beyond them the eight-wave persistent kernel; DT = D for 4 and 6 observations, 0 (runtime width) otherwise; AT = 5 on
    the eight-wave kernel at 4 x 64 x 5 alone.  KS1 = (D + 3) >> 2 layer-1 k-steps of four columns; the runtime-width kernels zero-pad the
    columns D .. 4 KS1 - 1, so KS1 and the padding belong to the class for DT = 0 only (None for the compile-time widths)."""
    assert 1 <= D <= 16 and 1 <= A <= 16 and B >= 241, (D, A, B)  # (the family: csrc/tma_mlp.h `fast`, plan_grad's tiles >= 16)
    kernel = "small" if -(-B // 16) <= 128 else "wave8"
    DT = D if D in (4, 6) else 0
    AT = 5 if (kernel == "wave8" and D == 4 and A == 5) else 0
    ks1 = (D + 3) >> 2
    return (kernel, DT, AT, ks1 if DT == 0 else None, 4 * ks1 - D if DT == 0 else None)


def head_row_class(A):
    """the head's rows in groups of four: A up to 4, 5 .. 8, 9 .. 12, 13 .. 16"""
    return (A + 3) >> 2


def test_every_h64_gradient_variant_has_a_float64_row_on_both_kernels():
    """GRAD_H64_SMALL and GRAD_H64 are one id each for every DT and AT, so test_every_dispatch_id_has_a_reference_case is satisfied by 4 x 64 x 5
    alone: this is the same check one level down, on the variant h64_grad_class derives for every f32 `grad` row of the family."""
    import torch

    import test_policy_dispatch_gpu as t

    rows = [c for c in t.CASES if c[0] == "grad" and c[6] in ("GRAD_H64_SMALL", "GRAD_H64")]
    for entry, D, H, A, cont, B, ident in rows:  # the restatement, the table and the plan agree on the kernel
        assert H == 64 and not cont and ident == {"small": "GRAD_H64_SMALL", "wave8": "GRAD_H64"}[h64_grad_class(D, A, B)[0]], (D, A, B, ident)
        rc, got = t.planned(_case_dims(entry, D, H, A, cont), "grad", B)[:2]
        assert rc == 0 and got == t.expected_value(ident), (D, A, B, t._name(got))
    classes = [h64_grad_class(D, A, B) for entry, D, H, A, cont, B, ident in rows]
    # every (kernel, DT, AT) some shape of the family reaches: every D and A at the first size of either kernel
    reachable = {h64_grad_class(D, A, B)[:3] for D in range(1, 17) for A in range(1, 17) for B in (241, 2049)}
    assert reachable == {("small", 4, 0), ("small", 6, 0), ("small", 0, 0), ("wave8", 4, 5), ("wave8", 4, 0), ("wave8", 6, 0), ("wave8", 0, 0)}
    have = {c[:3] for c in classes}
    assert reachable <= have, sorted(reachable - have)
    for kernel in ("small", "wave8"):
        on = [(c, A) for c, (entry, D, H, A, cont, B, ident) in zip(classes, rows) if c[0] == kernel]
        assert {1, 2, 3, 4} <= {c[3] for c, A in on}, kernel  # every KS1, at a runtime width
        assert {0, 1, 3} <= {c[4] for c, A in on}, kernel  # no padded column, one (Bicycle), three
        assert {1, 2, 3, 4} <= {head_row_class(A) for c, A in on}, kernel
        assert {(ks1, 3) for ks1 in (1, 2, 3, 4)} <= {(c[3], c[4]) for c, A in on}, kernel  # the most padding at every KS1
    assert not torch.cuda.is_initialized()


def _image_path_tasks():
    """(task, D, A) of every Discrete task with at most 16 observations and 16 actions, from the package's task and space tables"""
    from three_mlagents_amd.spaces import Discrete, task_spaces
    from three_mlagents_amd.tasks import ENGINE_TASKS

    out = []
    for task in ENGINE_TASKS.values():
        obs_space, act_space = task_spaces(task.kernel)
        if isinstance(act_space, Discrete) and obs_space.shape[0] <= 16 and act_space.n <= 16:
            out.append((task.id, obs_space.shape[0], act_space.n))
    return out


def test_every_task_that_trains_on_the_h64_path_has_its_shape_in_the_table():
    """Every task whose 64-wide policy runs the LDS-image kernels has, at its own (D, A), a float64 gradient row on the small kernel and on the
    eight-wave kernel, a forward row and an optimizer row."""
    import torch

    import test_policy_dispatch_gpu as t

    tasks = _image_path_tasks()
    assert tasks, "no task of the package's tables has a shape of the H = 64 image family"
    have = {(entry, D, A, ident) for entry, D, H, A, cont, B, ident in t.CASES if H == 64 and not cont}
    for name, D, A in tasks:
        for need in (("grad", D, A, "GRAD_H64_SMALL"), ("grad", D, A, "GRAD_H64"), ("fwd", D, A, "FWD_H64"), ("opt", D, A, "OPT_SCATTER_H64")):
            assert need in have, (name, need)
    assert not torch.cuda.is_initialized()


def _h64_class_grad_rows():
    import test_policy_dispatch_gpu as t

    return [pytest.param(*c, id=t._case_id(c)) for c in t.H64_CLASS_CASES if c[0].startswith("grad")]


@pytest.mark.parametrize("entry,D,H,A,cont,B,ident", _h64_class_grad_rows())
def test_comparator_sees_the_last_row_tile_of_every_h64_class_row_dropped(entry, D, H, A, cont, B, ident, record_property):
    """A condition on the rows' inputs, computed from grad_case_inputs and _grads alone, no kernel: the float64 gradient of the minibatch without
    its last row tile overshoots the K, F budget at least fourfold (the floor of tests/test_split3_ref_cpu.py), so the rejection each GPU row
    asserts has room.  A row that falls below moves by a tile; the constants stay."""
    import torch

    import test_policy_dispatch_gpu as t

    assert t.entry_dtype_kind(entry)[0] == "f32" and H == 64 and not cont
    sd = t.case_state_dict(D, H, A, cont)
    c = t.grad_case_inputs(entry, D, A, cont, B, sd)  # (_rollout asserts the clip margin)
    rows, idx, hp, drop = c["rows"], c["idx"], c["hp"], c["drop"]
    assert len(idx) == B and drop == (B % 16 or 16)
    g64, s64 = t._grads(sd, rows, idx, torch.float64, hp)
    g32, _ = t._grads(sd, rows, idx, torch.float32, hp)
    gdrop, _ = t._grads(sd, rows, idx[:B - drop], torch.float64, hp)
    assert 0.05 < s64["clip_fraction"] < 0.95  # both branches of the clipped surrogate
    errs_drop = t._segment_errors(gdrop, g64, g32)
    over = max(t.budget_use(*v, t.K, t.F) for v in errs_drop.values())
    record_property("drop_overshoot", over)
    print(f"{t._case_id((entry, D, H, A, cont, B, ident))}: drop of {drop} rows overshoots {over:.1f}-fold")
    assert t._rejects(errs_drop, t.K, t.F)
    assert over >= 4.0, (over, errs_drop)
    assert not torch.cuda.is_initialized()


def test_plan_query_refuses_what_the_real_calls_refuse():
    """the shapes test_accepted_but_unrunnable_shapes_are_refused_by_every_entry_point sends to the real calls, and mfma_dtype = 2 with a Box head"""
    import test_policy_dispatch_gpu as t
    from three_mlagents_amd import _lib

    for D, H, A, cont in [(2500, 64, 3, False), (600, 1024, 2, True), (2100, 256, 4, False)]:
        for which in ("fwd", "grad"):
            rc = t.planned(_case_dims(which, D, H, A, cont), which, 40)[0]
            assert rc == _lib.TMA_ERR_INVALID and "LDS" in _lib.last_error(), (D, H, which, rc, _lib.last_error())
    rc = t.planned(_case_dims("grad_bf16x3", 6, 256, 3, True), "grad", 4096)[0]
    assert rc == _lib.TMA_ERR_INVALID and "mfma_dtype 2" in _lib.last_error(), (rc, _lib.last_error())
    assert t.planned(_case_dims("fwd", 6, 256, 3, True), "fwd", 0)[0] == _lib.TMA_ERR_INVALID  # (the real calls refuse n < 1)
