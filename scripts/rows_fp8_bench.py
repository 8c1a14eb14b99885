"""e4m3 rows against bf16 rows in the row-chunked aggregate at the gin-products shape (F = 100 on the
ogbn-products-shaped CSR of configs.py), interleaved in one process:

  uw_bf16 / w1_bf16 / self_bf16      the bf16 table at its 256-B line pitch (2 lines per row): unweighted,
                                     one weight per edge, and the self-term form writing a bf16 y
  uw_fp8 / w1_fp8 / self_fp8         the e4m3 table at a 128-B pitch (to_fp8(lines=True): 1 line per row)
  uw_fp8_p112 / w1_fp8_p112 / self_fp8_p112   the e4m3 table at to_fp8's default 112-B pitch (1.75 lines)
  uw_bf16_aa                         the bf16 call again (A/A): the run's own spread

Each round times every form once: a warm-up call, then `reps` calls each between two HIP events; a
form's figure for the round is the median of its calls, its final figure the median over rounds.  The
order of the forms alternates per round.  Prints one JSON line per round and a summary line: the
medians, the per-round values, fp8 / bf16 per leg and pitch, and the A/A spread.

Usage: python scripts/rows_fp8_bench.py [--shape products] [--rounds R] [--reps N] [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402

F = 100


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def bench(shape, rounds, reps, dev, emit):
    g = G.dataset_graph(shape, device=dev)
    xf = torch.randn(g.n_rows, F, device=dev)
    xb = ops.pitched(xf.to(torch.bfloat16))
    x8, x8p = ops.to_fp8(xf, lines=True), ops.to_fp8(xf)
    assert (xb.stride(0) * 2, x8.stride(0), x8p.stride(0)) == (256, 128, 112)
    w = torch.rand(g.nnz, 1, device=dev)
    s = torch.tensor([1.1], device=dev)
    y = torch.empty(g.n_rows, F, device=dev)
    yb = torch.empty(g.n_rows, 104, dtype=torch.bfloat16, device=dev)[:, :F]
    plan = g.plan(512)
    plan = plan if plan.splits else None
    calls = {}
    for tag, x in (("bf16", xb), ("fp8", x8), ("fp8_p112", x8p)):
        calls["uw_" + tag] = lambda x=x: ops.aggregate(g, x, "src", None, out=y, plan=plan)
        calls["w1_" + tag] = lambda x=x: ops.aggregate(g, x, "src", w, out=y, plan=plan)
        calls["self_" + tag] = lambda x=x: ops.aggregate(g, x, "src", None, out=yb, plan=plan, self_term=(xb, s),
                                                         out_dtype=torch.bfloat16)
    calls["uw_bf16_aa"] = calls["uw_bf16"]
    forms = tuple(calls)
    stream = torch.cuda.current_stream(dev)
    times = {k: [] for k in forms}
    for r in range(rounds):
        for k in (forms if r % 2 == 0 else forms[::-1]):  # alternate the order
            calls[k]()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for a, b in ev:
                a.record(stream)
                calls[k]()
                b.record(stream)
            torch.cuda.synchronize(dev)
            times[k].append(float(np.median([a.elapsed_time(b) for a, b in ev])))
        emit({"shape": shape, "round": r, "ms": {k: round(v[-1], 5) for k, v in times.items()}})
    med = {k: float(np.median(v)) for k, v in times.items()}
    emit({"shape": shape, "rows": g.n_rows, "edges": g.nnz, "F": F, "reps": reps, "rounds": rounds,
          "pitch_bytes": {"bf16": 256, "fp8": 128, "fp8_p112": 112},
          "ms": {k: round(v, 5) for k, v in med.items()},
          "ms_rounds": {k: [round(t, 5) for t in v] for k, v in times.items()},
          "fp8_over_bf16": {leg: round(med[leg + "_fp8"] / med[leg + "_bf16"], 4) for leg in ("uw", "w1", "self")},
          "fp8_p112_over_bf16": {leg: round(med[leg + "_fp8_p112"] / med[leg + "_bf16"], 4) for leg in ("uw", "w1", "self")},
          "aa_spread": round(abs(med["uw_bf16_aa"] - med["uw_bf16"]) / med["uw_bf16"], 4)})


def main():
    if not torch.cuda.is_available():
        print("error: no HIP device: timings come from the GPU only", file=sys.stderr)
        return 2
    rounds, reps, out = int(_arg("--rounds", 5)), int(_arg("--reps", 8)), _arg("--out", None)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write("\n".join(lines) + "\n")

    bench(_arg("--shape", "products"), rounds, reps, torch.device("cuda", 0), emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
