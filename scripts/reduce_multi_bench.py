"""One multi-reducer launch against the three calls it replaces, at the Flickr and Reddit shapes
(F = 128, row-chunk plan 512), in EDGE mode on an [E, 128] tensor (PNA's case) and in SRC mode,
interleaved in one process:

  three     ops.aggregate(row_scale = 1 / deg) + ops.reduce MAX + ops.reduce MIN: the yardstick, the
            three launches that give MEAN, MAX and MIN without gta_reduce_multi (timed as one span)
  three2    the same again (A/A): the run's own spread
  multi3    ops.reduce_multi(("MEAN", "MAX", "MIN"))
  multi5    ops.reduce_multi(("MEAN", "MAX", "MIN", "VAR", "STD"))
  blocked3  SRC mode only: the column-blocked calls, ops.aggregate_blocked(row_scale = 1 / deg) +
            ops.reduce_blocked MAX + MIN at BlockedPlan.auto_blocks -- what Executor.reduce_blocked
            runs for a table beyond L2, and what MULTI_MIN_BLOCKED weighs the one pass against

Each round times every form once: a warm-up call, then `reps` calls each between two HIP events; a
form's figure for the round is the median of its calls, its final figure the median over rounds; the
order of the forms alternates per round.  Prints one JSON line per round and a summary per leg.
--root DIR imports the package from another checkout (a build of the parent commit, which has the
yardstick's forms only), so the yardstick can be read on both builds in alternating processes;
--tag NAME labels the records of the run ("build").

Usage: python scripts/reduce_multi_bench.py [--shapes flickr,reddit] [--modes edge,src] [--rounds R]
                                            [--root DIR] [--tag NAME] [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


ROOT = os.path.abspath(_arg("--root", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402

REPS = {"flickr": 50, "reddit": 5}
CHUNK, F = 512, 128
RED3, RED5 = ("MEAN", "MAX", "MIN"), ("MEAN", "MAX", "MIN", "VAR", "STD")


def forms(g, x, mode, dev):
    """{name: callable} of the forms this build has, every output preallocated."""
    n = g.n_rows
    ys = [torch.empty(n, F, device=dev) for _ in range(5)]
    scale = 1.0 / g.degrees().to(torch.float32).clamp_min(1.0)

    def three():
        ops.aggregate(g, x, mode, None, row_scale=scale, out=ys[0], plan=CHUNK)
        ops.reduce(g, x, "MAX", mode, out=ys[1], plan=CHUNK)
        ops.reduce(g, x, "MIN", mode, out=ys[2], plan=CHUNK)

    out = {"three": three, "three2": three}
    if hasattr(ops, "reduce_multi"):
        out["multi3"] = lambda: ops.reduce_multi(g, x, RED3, mode, outs=ys[:3], plan=CHUNK)
        out["multi5"] = lambda: ops.reduce_multi(g, x, RED5, mode, outs=ys, plan=CHUNK)
    if mode == "src":
        B = ops.BlockedPlan.auto_blocks(g, F, 4)
        if B >= 4 and g.blocked_plan(B).sorted:
            def blocked3():
                ops.aggregate_blocked(g, x, None, row_scale=scale, out=ys[0], blocks=B)
                ops.reduce_blocked(g, x, "MAX", out=ys[1], blocks=B)
                ops.reduce_blocked(g, x, "MIN", out=ys[2], blocks=B)
            out["blocked3"] = blocked3
    return out


def bench(shape, mode, rounds, dev, emit):
    g = G.dataset_graph(shape, device=dev)
    x = torch.randn(g.nnz if mode == "edge" else g.n_rows, F, device=dev)
    fs = forms(g, x, mode, dev)
    names = tuple(fs)
    stream = torch.cuda.current_stream(dev)
    reps = REPS.get(shape, 20)
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
        emit({"shape": shape, "mode": mode, "round": r, "ms": {k: round(v[-1], 5) for k, v in times.items()}})
    med = {k: float(np.median(v)) for k, v in times.items()}
    yard = med["three"]
    rec = {"shape": shape, "mode": mode, "build": _arg("--tag", "this"), "rows": g.n_rows, "edges": g.nnz, "F": F, "chunk": CHUNK,
           "reps": reps, "rounds": rounds, "ms": {k: round(v, 5) for k, v in med.items()},
           "ms_rounds": {k: [round(t, 5) for t in v] for k, v in times.items()},
           "aa_spread": round(abs(med["three2"] - yard) / yard, 4),
           "yard_min_max_spread": round((max(times["three"] + times["three2"]) - min(times["three"] + times["three2"])) / yard, 4)}
    for k in names:
        if k not in ("three", "three2"):
            rec[f"{k}_over_three"] = round(med[k] / yard, 4)
    if "multi5" in med:
        rec["multi5_over_multi3"] = round(med["multi5"] / med["multi3"], 4)
    if "blocked3" in med and "multi3" in med:
        rec["multi3_over_blocked3"] = round(med["multi3"] / med["blocked3"], 4)
    emit(rec)
    del x
    torch.cuda.empty_cache()


def main():
    if not torch.cuda.is_available():
        print("error: no HIP device: timings come from the GPU only", file=sys.stderr)
        return 2
    shapes = [s for s in _arg("--shapes", "flickr,reddit").split(",") if s]
    modes = [m for m in _arg("--modes", "edge,src").split(",") if m]
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
        for mode in modes:
            bench(shape, mode, rounds, torch.device("cuda", 0), emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
