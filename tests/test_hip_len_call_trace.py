"""GPU: every length-aware entry of models.py (and its dense twin) launches the library entry points it launched when
tests/golden/len_call_trace.json was recorded (tools/record_len_call_trace.py), the same names in the same order.  The
cases are tests/len_trace_cases.py's; the host code between a public entry and the kernels may be rearranged, the launches
may not."""
import json
import os

import pytest

import len_trace_cases as C

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(__file__), "golden", "len_call_trace.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_holds_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(C.NAMES)
    assert all(GOLDEN[name] for name in C.NAMES)


@pytest.mark.parametrize("name", C.NAMES)
def test_entry_launches_what_it_launched(name, tmp_path, monkeypatch):
    from slu_hip import lib
    lib.require_gfx950()
    trace, _, _ = C.record(name, tmp_path, monkeypatch)
    want = GOLDEN[name]                               # a case the fixture lacks is a failure
    first = next((i for i, (a, b) in enumerate(zip(trace, want)) if a != b), min(len(trace), len(want)))
    assert trace == want, "%s: %d launches against %d recorded, first difference at %d: %r / %r" % (
        name, len(trace), len(want), first, trace[first:first + 3], want[first:first + 3])
