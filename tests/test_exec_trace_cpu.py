"""The executor's call trace, reproduced exactly (tests/exec_trace.py; tests/golden/exec_trace.json).

Every run of the fixture -- the cora golden streams with default options (the ORDER C networks
BIDIR, GCNT and EDGEC among them), each executor switch turned off alone, the MAX / MIN / MEAN
pool layers in both ORDERs, the blocked-gate runs with gather_dtype None and bf16 -- is made again
through the recording proxy over tests/fake_ops.py.  The ops calls with the provenance, shape and
dtype of every tensor argument, the graph view and every scalar, then alg_bytes, launches,
gather_casts and the ten matcher attributes must come out as recorded: a refactor of the executor
changes no launch and no launch argument.
"""
import json

from . import exec_trace


def _first_difference(name, got, want):
    if got["matchers"] != want["matchers"]:
        m = next(k for k in exec_trace.MATCHERS if got["matchers"][k] != want["matchers"][k])
        return f"{name}: matcher attribute {m}: {got['matchers'][m]}, recorded {want['matchers'][m]}"
    for k, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        if a != b:
            return f"{name}: call {k}: {a}\n  recorded: {b}"
    if len(got["calls"]) != len(want["calls"]):
        k = min(len(got["calls"]), len(want["calls"]))
        return f"{name}: {len(got['calls'])} calls, recorded {len(want['calls'])}; first extra: {(got['calls'] + want['calls'])[k]}"
    return f"{name}: {got['summary']}, recorded {want['summary']}"


def test_every_recorded_run_is_reproduced():
    with open(exec_trace.FIXTURE) as f:
        doc = json.load(f)
    runs = exec_trace.runs()
    assert [name for name, _ in runs] == list(doc["runs"]), "the fixture's runs are not tests/exec_trace.py's"
    wrong = []
    for name, thunk in runs:
        got = thunk()
        want = exec_trace.resolve(doc, name)
        if got != want:
            wrong.append(_first_difference(name, got, want))
    assert not wrong, f"{len(wrong)} of {len(runs)} runs differ:\n" + "\n".join(wrong[:20])
