"""GPU: every case of tests/gemv_plan_cases.py as a real launch — teal_fused_gemv requests and the legacy entry points — reports
the return code, slab count and launch description recorded from the commit before the launch plan was gathered in one place
(tests/golden/gemv_plan_parent.json).  With tests/test_gemv_plan_host.py, which holds the host-only query to the same record,
this shows that the launch and the query share one plan; it is the only cover the legacy entries' geometry gets.  All data is
zeros (no activation survives a threshold of 0.5), so the whole table is a few hundred empty launches."""
import json
import os

import pytest

import gemv_plan_cases as C
from teal_amd import _lib, runtime

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemv_plan_parent.json")) as _f:
    RECORD = json.load(_f)


@pytest.fixture(scope="module")
def launched():
    runtime.init()
    L, D = _lib.load(), _lib.load_diag()
    assert L.teal_init() == RECORD["num_cu"], "the record is of an MI355X"
    try:
        return C.run_table(L, D)
    finally:
        C.set_switches(D, None)
        C._SHARED.clear()


def test_fused_launches_report_what_the_parent_reported(launched):
    got = launched[0]
    bad = [(k, got[k], want) for k, want in RECORD["fused"].items() if got.get(k) != want]
    assert len(got) == len(RECORD["fused"]) and not bad, f"{len(bad)} cases differ (id, launch, record): {bad[:8]}"


def test_legacy_entries_report_what_the_parent_reported(launched):
    got = launched[1]
    bad = [(k, got[k], want) for k, want in RECORD["legacy"].items() if got.get(k) != want]
    assert len(got) == len(RECORD["legacy"]) and not bad, f"{len(bad)} cases differ (id, launch, record): {bad[:8]}"


def test_the_query_answers_as_the_launch_on_this_device(launched):
    L = _lib.load()
    cu = L.teal_init()
    for c in C.FUSED:
        if not C.is_diag(c):
            assert list(C.call_plan(L, c, cu)) == launched[0][c["id"]], c["id"]
