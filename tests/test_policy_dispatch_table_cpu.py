"""The dispatch-record table of tests/test_policy_dispatch_gpu.py stays complete: every branch id include/tma.h declares has at least one
case that is meant to reach it (so a new specialisation cannot ship without a float64 reference test), and every case names ids that
exist; and the host-only query tma_debug_plan_dispatch -- the pure plan functions of csrc/tma_policy_plan.h behind every launch -- gives every
case the id the table expects and refuses what the real calls refuse.  None of this touches a GPU."""
import os
import re
import sys

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
