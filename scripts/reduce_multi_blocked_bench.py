"""The column-blocked multi-reducer against the routes it would replace, at the Reddit shape
(232,965 rows, 114.6 M edges, F = 128; an fp32 and a bf16 table), SRC mode, interleaved in one process:

  multi1 / multi3 / multi5   ops.reduce_multi (row-chunked, plan 512) over ("STD",), ("MEAN", "MAX",
                             "MIN") and all five: the one launch Executor._eval_multi sends today
  separate                   ops.reduce_blocked MAX + MIN at BlockedPlan.auto_blocks and the
                             row-chunked ops.reduce_multi(("STD",)): today's route for such a pair
  mb1 / mb3 / mb5 @ B, R     ops.reduce_multi_blocked over the same reducer sets (P = 2, 4, 4 planes of
                             partials) at `blocks` B and `row_edges` R, item_edges 256; R = "d" is the
                             default plan of a request of B blocks (BlockedPlan.resolve)

Each round times every form once: a warm-up call, then `reps` calls each between two HIP events; a
form's figure for the round is the median of its calls, its final figure the median over rounds; the
order alternates per round.  Before the timing every blocked plan's outputs are compared with the
row-chunked launch's (MAX / MIN equal; the moments' largest difference is printed).  Prints one JSON
line per round and a summary per table type.

Usage: python scripts/reduce_multi_blocked_bench.py [--shape reddit] [--dtypes f32,bf16] [--rounds R]
           [--reps N] [--blocks 6,12,20] [--row-edges d,64,256] [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402

CHUNK, F = 512, 128
SETS = {"1": ("STD",), "3": ("MEAN", "MAX", "MIN"), "5": ops.MULTI_REDS}


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def forms(g, x, blocks, row_edges, dev):
    """{name: callable}, every output preallocated and every plan built before the timing."""
    ys = [torch.empty(g.n_rows, F, device=dev) for _ in range(5)]
    out = {}
    for tag, reds in SETS.items():
        out[f"multi{tag}"] = lambda reds=reds: ops.reduce_multi(g, x, reds, "src", outs=ys[:len(reds)], plan=CHUNK)
    B0 = max(4, ops.BlockedPlan.auto_blocks(g, F, x.element_size()))

    def separate():
        ops.reduce_blocked(g, x, "MAX", out=ys[0], blocks=B0)
        ops.reduce_blocked(g, x, "MIN", out=ys[1], blocks=B0)
        ops.reduce_multi(g, x, ("STD",), "src", outs=ys[2:3], plan=CHUNK)
    out["separate"] = separate
    plans = {(B, R): g.blocked_plan(B) if R == "d" else g.blocked_plan(B, 256, int(R)) for B in blocks for R in row_edges}
    # one slab buffer for every plan, sized for the largest: the bound is 2 KB per possible item at P = 4
    need = {(k, P): ops._L().gta_reduce_multi_blocked_workspace_bytes(g.n_rows, g.nnz, p.blocks, F, p.item_edges, which)
            for k, p in plans.items() for P, which in ((2, 16), (4, 31))}
    slab = torch.empty(max(need.values()), dtype=torch.uint8, device=dev)
    for (k, P), nb in need.items():
        plans[k]._ws[("multi", F, P)] = slab[:nb]
    for (B, R), plan in plans.items():
        for tag, reds in SETS.items():
            out[f"mb{tag}@{B},{R}"] = lambda reds=reds, plan=plan: ops.reduce_multi_blocked(
                g, x, reds, outs=ys[:len(reds)], plan=plan)
    return out


def bench(shape, dtype, rounds, reps, blocks, row_edges, dev, emit):
    g = G.dataset_graph(shape, device=dev)
    x = ops.pitched(torch.randn(g.n_rows, F, device=dev).to(dtype))
    fs = forms(g, x, blocks, row_edges, dev)
    names, stream = tuple(fs), torch.cuda.current_stream(dev)
    # the forms agree before anything is timed: every blocked plan's five outputs against the
    # row-chunked launch's -- MAX / MIN equal, the moments' largest absolute difference reported
    ref = [y.clone() for y in fs["multi5"]()]
    for k in names:
        if k.startswith("mb5@"):
            ys = fs[k]()
            assert torch.equal(ys[1], ref[1]) and torch.equal(ys[2], ref[2]), f"{k}: MAX / MIN differ from reduce_multi"
            emit({"shape": shape, "dtype": str(dtype), "form": k,
                  "max_abs_diff": {r: float((ys[i] - ref[i]).abs().max()) for i, r in enumerate(ops.MULTI_REDS) if i not in (1, 2)}})
    times = {k: [] for k in names}
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):  # no form always runs after the same one
            fs[k]()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for a, b in ev:
                a.record(stream)
                fs[k]()
                b.record(stream)
            torch.cuda.synchronize(dev)
            times[k].append(float(np.median([a.elapsed_time(b) for a, b in ev])))
        emit({"shape": shape, "dtype": str(dtype), "round": r, "ms": {k: round(v[-1], 4) for k, v in times.items()}})
    emit({"shape": shape, "dtype": str(dtype), "rows": g.n_rows, "edges": g.nnz, "F": F, "rounds": rounds, "reps": reps,
          "ms": {k: round(float(np.median(v)), 4) for k, v in times.items()},
          "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
          "items": {str(k): p.n_items for k, p in g._plans.items() if isinstance(k, tuple) and k[0] == "blocked"}})
    del x
    torch.cuda.empty_cache()


def main():
    if not torch.cuda.is_available():
        print("error: no HIP device: timings come from the GPU only", file=sys.stderr)
        return 2
    out, lines = _arg("--out", None), []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write("\n".join(lines) + "\n")

    blocks = [int(b) for b in _arg("--blocks", "6,12,20").split(",")]
    row_edges = _arg("--row-edges", "d,64,256").split(",")
    for name in _arg("--dtypes", "f32,bf16").split(","):
        bench(_arg("--shape", "reddit"), {"f32": torch.float32, "bf16": torch.bfloat16}[name], int(_arg("--rounds", 5)),
              int(_arg("--reps", 5)), blocks, row_edges, torch.device("cuda", 0), emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
