"""gin-products with the e4m3 row gather (--gather-dtype fp8 + fp8_rows) against fp64 evaluated from
the UNROUNDED fp32 inputs, per op on the special rows plus 256 random ones: max|d| / max|ref| and
max|d| / sum|terms| (oracle.sampled.gin_unrounded_errors), beside the default bf16 run's figures.
A reported figure: e4m3 is unscaled, so inputs below 2^-10 flush to 0.

Usage: python scripts/rows_fp8_accuracy.py [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import configs, workloads  # noqa: E402
from oracle.sampled import SampledChecker, gin_unrounded_errors  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    layers, g, tensors = configs.build("gin-products", dev)
    lay, t = layers[0], tensors[0]
    t32 = workloads.make_tensors(lay.opgraph, g, "GIN", seed=0)
    ip, ix = g.numpy()
    out = {}
    for tag, (gdt, rows) in {"bf16": (None, False), "fp8_rows": (torch.float8_e4m3fn, True)}.items():
        lay.gather_dtype, lay.fp8_rows = gdt, rows
        res, ex = lay.run(t)
        chk = SampledChecker(ex, ip, ix)
        sp = np.concatenate(list(chk.special_rows().values()))
        rows_ = np.unique(np.concatenate([sp, np.random.default_rng(3).choice(g.n_rows, 256, replace=False)]))
        errs = gin_unrounded_errors(chk, t32, rows_)
        out[tag] = {"gather_casts": ex.gather_casts,
                    "per_op": {str(k): {"max_d_over_max_ref": a, "max_d_over_sum_terms": b, "n": n} for k, (a, b, n) in errs.items()}}
    line = json.dumps(out)
    print(line, flush=True)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
