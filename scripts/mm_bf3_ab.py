"""A/B of the fp32 UPDATE against its bf16x3 precision on the layer shapes, in one process:
ops.update_mm (default knobs: gta_update_mm_t on the layer shapes, its split-K form on Cora's) beside ops.update_mm(precision="bf16x3"),
interleaved rounds, HIP-event medians, x and out rotated over enough copies that no call finds its
operands in L2 / the Infinity Cache.  Accuracy: max |d| / sum|x||w| of both against an fp64 product of
the first rows.  Prints one JSON line per shape, and appends it to --out.

Usage: python scripts/mm_bf3_ab.py [--rounds R] [--out FILE] [M,K,N ...]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import ops  # noqa: E402

# GAT-8 Flickr x W, Reddit x W, Reddit hidden, PNA-Flickr's edge GEMM [E, 500] x [500, 128], GCN Cora
SHAPES = [(89250, 500, 128), (232965, 602, 128), (232965, 128, 128), (899756, 500, 128), (2708, 1433, 128)]
CHECK_ROWS = 4096


def timed(fn, reps):
    s = torch.cuda.current_stream()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (a, b) in enumerate(ev):
        a.record(s)
        fn(i)
        b.record(s)
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    args = sys.argv[1:]
    rounds, out_path = 3, None
    for flag in ("--rounds", "--out"):
        if flag in args:
            i = args.index(flag)
            if flag == "--rounds":
                rounds = int(args[i + 1])
            else:
                out_path = args[i + 1]
            del args[i:i + 2]
    shapes = [tuple(int(v) for v in a.split(",")) for a in args] or SHAPES
    dev = torch.device("cuda", 0)
    for M, K, N in shapes:
        g = torch.Generator(device="cpu").manual_seed(M + K + N)
        x0 = torch.randn(M, K, generator=g)
        w = (torch.randn(K, N, generator=g) / K ** 0.5).to(dev)
        copies = int(min(6, max(2, -(-(1 << 30) // (M * K * 4)))))
        xs = [x0.to(dev) for _ in range(copies)]
        outs = [torch.empty(M, N, device=dev) for _ in range(copies)]
        runs = {"f32": lambda i: ops.update_mm(xs[i % copies], w, out=outs[i % copies]),
                "bf16x3": lambda i: ops.update_mm(xs[i % copies], w, out=outs[i % copies], precision="bf16x3")}
        ms = {k: [] for k in runs}
        err = {}
        n = min(M, CHECK_ROWS)
        x64, w64 = xs[0][:n].double(), w.double()
        ref, scale = x64 @ w64, x64.abs() @ w64.abs()
        for name, run in runs.items():
            run(0)
            err[name] = float(((outs[0][:n].double() - ref).abs() / scale).max())
        for _ in range(rounds):
            for name, run in runs.items():
                run(0)
                ms[name].append(timed(run, 12))
        rec = {"M": M, "K": K, "N": N, "x_copies": copies}
        for name in runs:
            t = float(np.median(ms[name]))
            rec[name] = {"ms": round(t, 4), "TFs": round(2 * M * K * N / t / 1e9, 1), "all_ms": [round(v, 4) for v in ms[name]],
                         "max_err_over_sum_abs": err[name]}
        rec["speedup"] = round(rec["f32"]["ms"] / rec["bf16x3"]["ms"], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(line + "\n")
        del xs, outs, x0, w, x64, w64, ref, scale
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
