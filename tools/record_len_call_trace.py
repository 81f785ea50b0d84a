"""Writes tests/golden/len_call_trace.json: for every case of tests/len_trace_cases.py, the names of the library entry points
its call launched, in order (what slu_hip.lib.check was handed).  tests/test_hip_len_call_trace.py replays the cases and
compares.  Run it on an MI355X at the commit whose launch order is to be kept:

  python tools/record_len_call_trace.py [--out tests/golden/len_call_trace.json]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "end-to-end-slu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import pytest  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "len_call_trace.json"))
    args = ap.parse_args()
    import len_trace_cases as C
    from slu_hip import lib
    lib.require_gfx950()
    traces = {}
    for name in C.NAMES:
        with pytest.MonkeyPatch.context() as patch:
            traces[name], _, _ = C.record(name, tempfile.mkdtemp(), patch)
        print("%-40s %5d launches" % (name, len(traces[name])))
    with open(args.out, "w") as f:
        f.write("{\n%s\n}\n" % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(traces[k])) for k in sorted(traces)))


if __name__ == "__main__":
    main()
