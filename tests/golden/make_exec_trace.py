"""Golden fixture for the executor's call trace (tests/golden/exec_trace.json).

Test infrastructure only.  Runs every entry of tests/exec_trace.py's `runs()` -- the cora golden
streams with default options, each executor switch turned off alone, the MAX / MIN / MEAN pool
layers in both ORDERs, and the blocked-gate runs -- through the recording proxy over
tests/fake_ops.py, and writes the calls, byte / launch counts and matcher attributes it saw.
Regenerate only at a commit whose executor behaviour is the intended one: the file is what
tests/test_exec_trace_cpu.py holds later executors to.

Usage (from the repository root):  python tests/golden/make_exec_trace.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import exec_trace  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else exec_trace.FIXTURE
    doc = exec_trace.record_all(progress=lambda name: print(name, flush=True))
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
