"""bf16 against fp32 gathered tables in the column-blocked aggregate and the fused GAT attention
aggregate, at the Flickr and Reddit shapes (F = 128, 8 heads), interleaved in one process:

  w8_f32      aggregate_blocked, 8 head weights, fp32 table    -- the metric shape
  w8_f32_aa   the same call again (A/A): the run's own spread
  w8_bf16     the same plan and weights over the table rounded to bf16 (gta_aggregate_blocked_x)
  w8_bf16_b2  as w8_bf16 with the column blocks auto_blocks gives for 2-byte elements
  uw_f32 / uw_bf16    aggregate_blocked without weights
  att_f32 / att_bf16  gat_aggregate_blocked (normalised, exp-leaky-relu scores)
  chunk_bf16  ops.aggregate over the bf16 table with the 8 head weights: the row-chunked kernel a
              bf16 table took before the blocked kernels read bf16

Each round times every form once: a warm-up call, then `reps` calls each between two HIP events; a
form's figure for the round is the median of its calls, its final figure the median over rounds.  The
order of the forms alternates per round.  Prints one JSON line per round and a summary line per shape:
the medians, bf16 / fp32 per leg, and the A/A spread |w8_f32 - w8_f32_aa| / w8_f32.

Usage: python scripts/blocked_bf16_bench.py [--shapes flickr,reddit] [--rounds R] [--blocks B] [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402

REPS = {"flickr": 100, "reddit": 8}
FORMS = ("w8_f32", "w8_f32_aa", "w8_bf16", "w8_bf16_b2", "uw_f32", "uw_bf16", "att_f32", "att_bf16", "chunk_bf16")
F, H = 128, 8


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def bench(shape, rounds, blocks, dev, emit):
    g = G.dataset_graph(shape, device=dev)
    xf = torch.randn(g.n_rows, F, device=dev)
    xb = ops.pitched(xf.to(torch.bfloat16))
    w = torch.rand(g.nnz, H, device=dev)
    a, b = torch.randn(g.n_rows, H, device=dev), torch.randn(g.n_rows, H, device=dev)
    B4 = blocks or ops.BlockedPlan.auto_blocks(g, F, 4)
    B2 = blocks or ops.BlockedPlan.auto_blocks(g, F, 2)
    p4, p2 = g.blocked_plan(B4), g.blocked_plan(B2)
    y = torch.empty(g.n_rows, F, device=dev)
    calls = {
        "w8_f32": lambda: ops.aggregate_blocked(g, xf, w, out=y, plan=p4),
        "w8_f32_aa": lambda: ops.aggregate_blocked(g, xf, w, out=y, plan=p4),
        "w8_bf16": lambda: ops.aggregate_blocked(g, xb, w, out=y, plan=p4),
        "w8_bf16_b2": lambda: ops.aggregate_blocked(g, xb, w, out=y, plan=p2),
        "uw_f32": lambda: ops.aggregate_blocked(g, xf, None, out=y, plan=p4),
        "uw_bf16": lambda: ops.aggregate_blocked(g, xb, None, out=y, plan=p4),
        "att_f32": lambda: ops.gat_aggregate_blocked(g, xf, a, b, out=y, plan=p4),
        "att_bf16": lambda: ops.gat_aggregate_blocked(g, xb, a, b, out=y, plan=p4),
        "chunk_bf16": lambda: ops.aggregate(g, xb, "src", w, out=y, plan=512),
    }
    # the contract, once: the bf16 call is bitwise the fp32 call on the widened table
    twin = ops.aggregate_blocked(g, xb.float(), w, plan=p4)
    assert torch.equal(ops.aggregate_blocked(g, xb, w, plan=p4).view(torch.int32), twin.view(torch.int32))
    del twin
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
    emit({"shape": shape, "rows": g.n_rows, "edges": g.nnz, "F": F, "heads": H, "blocks_f32": B4, "blocks_bf16_b2": B2,
          "reps": reps, "rounds": rounds, "ms": {k: round(v, 5) for k, v in med.items()},
          "ms_rounds": {k: [round(t, 5) for t in v] for k, v in times.items()},
          "bf16_over_f32": {leg: round(med[leg + "_bf16"] / med[leg + "_f32"], 4) for leg in ("w8", "uw", "att")},
          "bf16_b2_over_f32": round(med["w8_bf16_b2"] / med["w8_f32"], 4),
          "blocked_bf16_over_chunk_bf16": round(med["w8_bf16"] / med["chunk_bf16"], 4),
          "aa_spread": round(abs(med["w8_f32_aa"] - med["w8_f32"]) / med["w8_f32"], 4),
          "round_spread": round((max(times["w8_f32"]) - min(times["w8_f32"])) / med["w8_f32"], 4)})


def main():
    if not torch.cuda.is_available():
        print("error: no HIP device: timings come from the GPU only", file=sys.stderr)
        return 2
    shapes = [s for s in _arg("--shapes", "flickr,reddit").split(",") if s]
    rounds, blocks, out = int(_arg("--rounds", 7)), int(_arg("--blocks", 0)), _arg("--out", None)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for shape in shapes:
        bench(shape, rounds, blocks, torch.device("cuda", 0), emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
