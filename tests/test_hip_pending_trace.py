"""GPU: the bookkeeping of unstored rows (pymgrit_amd/csrc/pending_rows.h) against the record in tests/golden/pending_trace.json, made
by tests/golden/make_golden_pending_trace.py: every scripted call sequence of tests/pending_trace.py (its docstring says what they
are) leaves the same state of the four records behind every library call, and the same bytes in every slab behind a settle of
every level. Equality only, no case skipped. The record tests (test_hip_deferred_rows.py, test_hip_twin_rows.py,
test_hip_lagged_cpoints.py, test_hip_up2.py) say that the decisions are right; this one says that they have not moved."""
import pytest

import cases
import pending_trace as pt

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = cases.load_json("pending_trace.json")


def test_the_record_covers_every_case():
    assert sorted(GOLDEN["cases"]) == sorted(pt.case_id(c) for c in pt.CASES)


@pytest.mark.parametrize("case", pt.CASES, ids=pt.case_id)
def test_every_script_leaves_the_recorded_trace(case):
    assert torch.cuda.is_available()
    want, got = pt.unpack(GOLDEN, pt.case_id(case)), pt.run_case(case)
    print(f"{pt.case_id(case)}: {got['calls']} calls, {len(got['changes'])} changes, slabs {got['slabs']}")
    assert got["changes"] == want["changes"]
    assert (got["calls"], got["trace"]) == (want["calls"], want["trace"])
    assert pt.slabs_digest(got["slabs"]) == want["slabs"], f"recorded with '{GOLDEN['hipcc']}'"
