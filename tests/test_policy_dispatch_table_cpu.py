"""The dispatch-record table of tests/test_policy_dispatch_gpu.py stays complete: every branch id include/tma.h declares has at least one
case that is meant to reach it (so a new specialisation cannot ship without a float64 reference test), and every case names ids that
exist.  Importing the table touches no GPU."""
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
