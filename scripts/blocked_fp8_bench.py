"""e4m3 against bf16 and fp32 gathered tables in the column-blocked aggregate and the fused GAT
attention aggregate, at the Flickr and Reddit shapes (F = 128, 8 heads), interleaved in one process:

  w8_f32 / w8_bf16 / w8_fp8    aggregate_blocked, 8 head weights -- the metric shape -- on fp32's plan
  w8_f32_aa                    the fp32 call again (A/A): the run's own spread
  w8_fp8_b1 / w8_fp8_b2        fp8 at the column blocks auto_blocks gives for 1-byte / 2-byte elements
  w8_fp8_lean / w8_fp8_b1_lean fp8 under seg_lean = 2: the lean kernel k_agg_q16f8 against the generic
                               quarter-wave form the calls above run, on fp32's plan and on fp8's own
  uw_f32 / uw_bf16 / uw_fp8 / uw_fp8_lean   aggregate_blocked without weights
  att_f32 / att_bf16 / att_fp8              gat_aggregate_blocked (normalised, exp-leaky-relu scores)

Each round times every form once: a warm-up call, then `reps` calls each between two HIP events; a
form's figure for the round is the median of its calls, its final figure the median over rounds.  The
order of the forms alternates per round.  Prints one JSON line per round and a summary line per shape:
the medians, the per-round values, fp8 / bf16 and fp8 / fp32 per leg, lean / generic, and the A/A
spread |w8_f32 - w8_f32_aa| / w8_f32.

Usage: python scripts/blocked_fp8_bench.py [--shapes flickr,reddit] [--rounds R] [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402

REPS = {"flickr": 100, "reddit": 8}
F, H = 128, 8


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def bench(shape, rounds, dev, emit):
    g = G.dataset_graph(shape, device=dev)
    xf = torch.randn(g.n_rows, F, device=dev)
    xb, x8 = ops.pitched(xf.to(torch.bfloat16)), ops.to_fp8(xf)
    w = torch.rand(g.nnz, H, device=dev)
    a, b = torch.randn(g.n_rows, H, device=dev), torch.randn(g.n_rows, H, device=dev)
    B4, B2, B1 = (ops.BlockedPlan.auto_blocks(g, F, e) for e in (4, 2, 1))
    p4, p2, p1 = g.blocked_plan(B4), g.blocked_plan(B2), g.blocked_plan(B1)
    y = torch.empty(g.n_rows, F, device=dev)

    def lean(fn):  # the call under seg_lean = 2
        def run():
            old = ops.get_debug("seg_lean")
            ops.set_debug("seg_lean", 2)
            try:
                fn()
            finally:
                ops.set_debug("seg_lean", old)
        return run

    calls = {}
    for tag, x in (("f32", xf), ("bf16", xb), ("fp8", x8)):
        calls["w8_" + tag] = lambda x=x: ops.aggregate_blocked(g, x, w, out=y, plan=p4)
        calls["uw_" + tag] = lambda x=x: ops.aggregate_blocked(g, x, None, out=y, plan=p4)
        calls["att_" + tag] = lambda x=x: ops.gat_aggregate_blocked(g, x, a, b, out=y, plan=p4)
    calls["w8_f32_aa"] = calls["w8_f32"]
    calls["w8_fp8_b1"] = lambda: ops.aggregate_blocked(g, x8, w, out=y, plan=p1)
    calls["w8_fp8_b2"] = lambda: ops.aggregate_blocked(g, x8, w, out=y, plan=p2)
    calls["w8_fp8_lean"] = lean(calls["w8_fp8"])
    calls["w8_fp8_b1_lean"] = lean(calls["w8_fp8_b1"])
    calls["uw_fp8_lean"] = lean(calls["uw_fp8"])
    forms = tuple(calls)
    # the contract, once: the fp8 call is bitwise the fp32 call on the widened table, generic and lean
    twin = ops.aggregate_blocked(g, x8.float(), w, plan=p4).view(torch.int32)
    assert torch.equal(ops.aggregate_blocked(g, x8, w, plan=p4).view(torch.int32), twin)
    calls["w8_fp8_lean"]()
    assert torch.equal(y.view(torch.int32), twin)
    del twin
    stream = torch.cuda.current_stream(dev)
    reps = REPS.get(shape, 20)
    times = {k: [] for k in forms}
    for r in range(rounds):
        for k in (forms if r % 2 == 0 else forms[::-1]):  # alternate the order
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
    emit({"shape": shape, "rows": g.n_rows, "edges": g.nnz, "F": F, "heads": H, "blocks": {"f32": B4, "bf16": B2, "fp8": B1},
          "reps": reps, "rounds": rounds, "ms": {k: round(v, 5) for k, v in med.items()},
          "ms_rounds": {k: [round(t, 5) for t in v] for k, v in times.items()},
          "fp8_over_bf16": {leg: round(med[leg + "_fp8"] / med[leg + "_bf16"], 4) for leg in ("w8", "uw", "att")},
          "fp8_over_f32": {leg: round(med[leg + "_fp8"] / med[leg + "_f32"], 4) for leg in ("w8", "uw", "att")},
          "lean_over_generic": {k: round(med[k + "_lean"] / med[k], 4) for k in ("w8_fp8", "w8_fp8_b1", "uw_fp8")},
          "aa_spread": round(abs(med["w8_f32_aa"] - med["w8_f32"]) / med["w8_f32"], 4)})


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
