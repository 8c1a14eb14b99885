"""gta_reduce MAX against the aggregate it is modelled on, at the Flickr and Reddit shapes (F = 128,
x_mode src, the same row-chunk plan for every form), interleaved in one process:

  reduce_max   gta_reduce(GTA_RED_MAX)                       -- k_reduce (+ k_reduce_combine)
  agg_generic  gta_aggregate, w NULL, knob agg_lean = 0      -- k_aggregate's generic form: the
               like-for-like yardstick (same bytes, same access pattern, fma instead of the compare)
  agg_generic2 the same call again (A/A): the run's own spread
  agg_lean     gta_aggregate, w NULL, knob agg_lean = 1      -- what a lean reduce form would still be worth

Each round times every form once: a warm-up call, then `reps` calls each between two HIP events; a
form's figure for the round is the median of its calls, its final figure the median over rounds.
Prints one JSON line per round and a summary line per shape: the raw medians, reduce_max / agg_generic,
and the A/A spread |agg_generic - agg_generic2| / agg_generic with the round-to-round spread beside it.

Usage: python scripts/reduce_bench.py [--shapes flickr,reddit] [--rounds R] [--chunk C] [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402

REPS = {"flickr": 100, "reddit": 8}
FORMS = ("reduce_max", "agg_generic", "agg_generic2", "agg_lean")


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _call(form, g, x, chunk):
    if form == "reduce_max":
        return ops.reduce(g, x, "MAX", "src", plan=chunk)
    ops.set_debug("agg_lean", 1 if form == "agg_lean" else 0)
    return ops.aggregate(g, x, "src", plan=chunk)


def bench(shape, rounds, chunk, dev, emit):
    g = G.dataset_graph(shape, device=dev)
    x = torch.randn(g.n_rows, 128, device=dev)
    stream = torch.cuda.current_stream(dev)
    reps = REPS.get(shape, 20)
    lean0 = ops.get_debug("agg_lean")
    times = {k: [] for k in FORMS}
    try:
        for r in range(rounds):
            order = FORMS if r % 2 == 0 else FORMS[::-1]  # alternate the order: no form always runs after the same one
            for k in order:
                _call(k, g, x, chunk)
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
                for a, b in ev:
                    a.record(stream)
                    _call(k, g, x, chunk)
                    b.record(stream)
                torch.cuda.synchronize(dev)
                times[k].append(float(np.median([a.elapsed_time(b) for a, b in ev])))
            emit({"shape": shape, "round": r, "ms": {k: round(v[-1], 5) for k, v in times.items()}})
    finally:
        ops.set_debug("agg_lean", lean0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    yard = med["agg_generic"]
    emit({"shape": shape, "rows": g.n_rows, "edges": g.nnz, "F": 128, "chunk": chunk, "split_rows": g.plan(chunk).splits,
          "reps": reps, "rounds": rounds, "ms": {k: round(v, 5) for k, v in med.items()},
          "ms_rounds": {k: [round(t, 5) for t in v] for k, v in times.items()},
          "reduce_over_generic": round(med["reduce_max"] / yard, 4),
          "lean_over_generic": round(med["agg_lean"] / yard, 4),
          "aa_spread": round(abs(med["agg_generic2"] - yard) / yard, 4),
          "round_spread": round((max(times["agg_generic"]) - min(times["agg_generic"])) / yard, 4)})


def main():
    if not torch.cuda.is_available():
        print("error: no HIP device: timings come from the GPU only", file=sys.stderr)
        return 2
    shapes = [s for s in _arg("--shapes", "flickr,reddit").split(",") if s]
    rounds, chunk, out = int(_arg("--rounds", 7)), int(_arg("--chunk", 512)), _arg("--out", None)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for shape in shapes:
        bench(shape, rounds, chunk, torch.device("cuda", 0), emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
