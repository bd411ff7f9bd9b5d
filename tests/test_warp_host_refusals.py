"""Host-only: every refused call of the ten fused warp-photometric entry points returns the code and the e2e_last_error() text, and every
one of the nine size queries the value, that the build of the parent commit gave (tests/warp_host_refusals.json, recorded by
tests/warp_host_refusals.py from that commit and never from the code under test).  This pins the messages, the per-entry differences
and the ORDER of the checks (pairs of faults from two different checks) across a rewrite of the host side.

All non-NULL pointers are dummy integers: a refused call returns before any HIP call.  So that a regression can never hand one of them to
a kernel, the module skips itself where a GPU is present; there the test_refused_calls_leave_outputs_alone tests of the family's GPU
modules cover the same ground with real buffers."""
import json

import pytest
import torch

import warp_host_refusals as R

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: host-only machines only")


@pytest.fixture(scope="module")
def table():
    with open(R.TABLE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    return R.run()


def test_the_case_list_is_the_fixed_one(table):
    cases, queries = R.build_cases(), R.build_queries()
    assert len(R.ENTRIES) == 10 and len(R.QUERY_NAMES) == 9
    assert len(cases) == 424 and len({c for c, _, _ in cases}) == 424
    assert len(queries) == 3 * 21 + 6 * 84
    assert {e for _, e, _ in cases} == set(R.ENTRIES) and {q for q, _ in queries} == set(R.QUERY_NAMES)
    assert set(table["refusals"]) == {c for c, _, _ in cases} and len(table["queries"]) == len(queries)
    assert len(table["parent"]) == 40
    assert all(rc == R.E2E_ERR_ARG and msg for rc, msg in table["refusals"].values())          # the recorder's own condition


def test_refused_calls_answer_as_the_parent_did(table, got):
    wrong = {c: (r, table["refusals"][c]) for c, r in got["refusals"].items() if r != table["refusals"][c]}
    assert not wrong, f"{len(wrong)} refusals differ from the parent's (got, want): {dict(list(wrong.items())[:5])}"


def test_size_queries_answer_as_the_parent_did(table, got):
    wrong = {q: (v, table["queries"][q]) for q, v in got["queries"].items() if v != table["queries"][q]}
    assert not wrong, f"{len(wrong)} size queries differ from the parent's (got, want): {dict(list(wrong.items())[:5])}"
    assert got["queries"]["e2e_warp_photo_geo_bwd_intrinsics_workspace_bytes(2, 1, 9, 33)"] == 6112
    assert got["queries"]["e2e_warp_photo_geo_bwd_intrinsics_workspace_bytes(0, 1, 9, 33)"] == 0
