"""One whole-layer figure for the column-blocked MAX gather: a GraphSAGE-pool 128 -> 64 layer (the
gather MAX of a virtual scatter; tests/pool_layer.py builds its records) on the Reddit-sized graph,
one leg per process:

  chunked        Executor.reduce_blocked = False: the row-chunked gta_reduce
  blocked        the default: ops.reduce_blocked past the executor's size gate
  blocked_bf16   the same with gather_dtype = bf16 (one cast of the table, then 2-byte rows)

Prints one JSON line: the median and every one of `--forwards` event-timed eager forwards after a
warm-up forward.  Usage: python scripts/reduce_blocked_layer.py --leg LEG [--shape reddit] [--forwards 5]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import executor, graph as G, workloads  # noqa: E402
from tests import pool_layer  # noqa: E402


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    if not torch.cuda.is_available():
        print("error: no HIP device", file=sys.stderr)
        return 2
    leg, shape, forwards = _arg("--leg", "blocked"), _arg("--shape", "reddit"), int(_arg("--forwards", 5))
    dev = torch.device("cuda", 0)
    g = G.dataset_graph(shape, device=dev)
    recs, og, stream, sem = pool_layer.layer(g.n_rows, g.nnz, 128, "MAX")
    tensors = workloads.make_tensors(og, g, "GraphSAGE", seed=0)

    def forward():
        ex = executor.Executor(og, stream, g, tensors, sem, gather_dtype=torch.bfloat16 if leg == "blocked_bf16" else None)
        ex.reduce_blocked = leg != "chunked"
        ex.run()
        return ex

    ex = forward()
    torch.cuda.synchronize(dev)
    st = torch.cuda.current_stream(dev)
    ms = []
    for _ in range(forwards):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(st)
        forward()
        e.record(st)
        torch.cuda.synchronize(dev)
        ms.append(s.elapsed_time(e))
    blocked = [k for k in g._plans if isinstance(k, tuple) and k[0] == "blocked"]
    print(json.dumps({"leg": leg, "shape": shape, "rows": g.n_rows, "edges": g.nnz, "ms_median": round(float(np.median(ms)), 4),
                      "ms": [round(t, 4) for t in ms], "blocked_plans": blocked, "gather_casts": ex.gather_casts,
                      "launches": ex.launches}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
