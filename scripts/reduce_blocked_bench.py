"""The column-blocked MAX gather against the row-chunked one, at the Flickr and Reddit shapes
(F = 128, x gathered by source), interleaved in one process:

  reduce_max          ops.reduce MAX, row-chunk plan 512 (gta_reduce, k_reduce)  -- the yardstick
  reduce_max_aa       the same call again (A/A): the run's own spread
  blocked_max_f32     ops.reduce_blocked MAX, fp32 table, BlockedPlan.auto_blocks(elem = 4)
  blocked_max_bf16    ops.reduce_blocked MAX, the table rounded to bf16, auto_blocks(elem = 2)
  agg_blocked_uw      ops.aggregate_blocked without weights, fp32 table, the fp32 plan: the sum twin

Before it times, the forms' values are compared once: blocked fp32 == row-chunked, blocked bf16 ==
row-chunked rounded to bf16.  Each round times every form once: a warm-up call, then `reps` calls
each between two HIP events; a form's figure for the round is the median of its calls, its final
figure the median over rounds.  The order of the forms alternates per round.  Prints one JSON line
per round and a summary line per shape.

Usage: python scripts/reduce_blocked_bench.py [--shapes flickr,reddit] [--rounds R] [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402

REPS = {"flickr": 100, "reddit": 8}
FORMS = ("reduce_max", "reduce_max_aa", "blocked_max_f32", "blocked_max_bf16", "agg_blocked_uw")
F = 128


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def bench(shape, rounds, dev, emit):
    g = G.dataset_graph(shape, device=dev)
    xf = torch.randn(g.n_rows, F, device=dev)
    xb = ops.pitched(xf.to(torch.bfloat16))
    B4, B2 = ops.BlockedPlan.auto_blocks(g, F, 4), ops.BlockedPlan.auto_blocks(g, F, 2)
    p4, p2 = g.blocked_plan(B4), g.blocked_plan(B2)
    y = torch.empty(g.n_rows, F, device=dev)
    calls = {
        "reduce_max": lambda: ops.reduce(g, xf, "MAX", "src", out=y, plan=512),
        "reduce_max_aa": lambda: ops.reduce(g, xf, "MAX", "src", out=y, plan=512),
        "blocked_max_f32": lambda: ops.reduce_blocked(g, xf, "MAX", out=y, plan=p4),
        "blocked_max_bf16": lambda: ops.reduce_blocked(g, xb, "MAX", out=y, plan=p2),
        "agg_blocked_uw": lambda: ops.aggregate_blocked(g, xf, None, out=y, plan=p4),
    }
    # the contract, once: every output is one of its inputs, and rounding commutes with the max
    base = ops.reduce(g, xf, "MAX", "src", plan=512)
    assert torch.equal(ops.reduce_blocked(g, xf, "MAX", plan=p4), base)
    assert torch.equal(ops.reduce_blocked(g, xb, "MAX", plan=p2), base.to(torch.bfloat16).float())
    del base
    stream = torch.cuda.current_stream(dev)
    reps = REPS.get(shape, 20)
    times = {k: [] for k in FORMS}
    for r in range(rounds):
        order = FORMS if r % 2 == 0 else FORMS[::-1]  # alternate the order: no form always runs after the same one
        for k in order:
            calls[k]()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for s, e in ev:
                s.record(stream)
                calls[k]()
                e.record(stream)
            torch.cuda.synchronize(dev)
            times[k].append(float(np.median([s.elapsed_time(e) for s, e in ev])))
        emit({"shape": shape, "round": r, "ms": {k: round(v[-1], 5) for k, v in times.items()}})
    med = {k: float(np.median(v)) for k, v in times.items()}
    aa = abs(med["reduce_max_aa"] - med["reduce_max"]) / med["reduce_max"]
    emit({"shape": shape, "rows": g.n_rows, "edges": g.nnz, "F": F, "blocks_f32": B4, "blocks_bf16": B2,
          "reps": reps, "rounds": rounds, "ms": {k: round(v, 5) for k, v in med.items()},
          "ms_rounds": {k: [round(t, 5) for t in v] for k, v in times.items()},
          "blocked_f32_over_reduce": round(med["blocked_max_f32"] / med["reduce_max"], 4),
          "blocked_bf16_over_reduce": round(med["blocked_max_bf16"] / med["reduce_max"], 4),
          "blocked_f32_over_agg_blocked": round(med["blocked_max_f32"] / med["agg_blocked_uw"], 4),
          "aa_spread": round(aa, 4),
          "faster_by_more_than_twice_aa": bool(med["blocked_max_f32"] < med["reduce_max"] * (1 - 2 * aa)),
          "round_spread": round((max(times["reduce_max"]) - min(times["reduce_max"])) / med["reduce_max"], 4)})


def main():
    if not torch.cuda.is_available():
        print("error: no HIP device: timings come from the GPU only", file=sys.stderr)
        return 2
    shapes = [s for s in _arg("--shapes", "flickr,reddit").split(",") if s]
    rounds, out = int(_arg("--rounds", 7)), _arg("--out", None)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for shape in shapes:
        bench(shape, rounds, torch.device("cuda", 0), emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
