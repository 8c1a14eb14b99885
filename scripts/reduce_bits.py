"""Result bits of the row reducers (gta_reduce, gta_reduce_multi), one sha256 per case:
python scripts/reduce_bits.py [--root DIR] [--out FILE]

Run in two builds (the parent's checkout and this tree) the two listings must be identical: the
check that a change to k_reduce / k_reduce_multi, their combine kernels or their dispatch moved no
result bit -- the moments' sums depend on which edge lands in which slot of a form, so they show a
moved slot or a reordered addition.  Each line is `<case> <sha256 over the raw bytes of the outputs>`.
--root DIR imports the package from another checkout (a build of the parent commit).

Graph: tests/test_gpu_reduce.py's, rebuilt here from its seed (300 rows, empty rows, a one-edge row,
rows of exactly 64 and 65 edges, one row of 700 edges: 11 items at chunk 64, 2 at chunk 512).
Cases: F in {3, 36, 64, 100, 128, 256, 300, 602, 1024} (VW 1 / 2 / 4, 4 .. 64 lanes per edge, 1 / 2 / 4
pieces per lane, the 16-B bf16 pieces with and without the clamped last one) x operand {edge, src,
dst} fp32 and {src, dst} bf16.  Each at plan 64 (many split rows) with gta_reduce MAX / MIN / ADD and
reduce_multi {MEAN, MAX, MIN} (one tensor per output) and all five (strided column blocks of one
[N, 5F] table); without a plan with MAX and the two multi sets; the fp32 edge and src tables at plan
512 too (one split row).  At F = 100 and 128 the other 29 non-empty subsets (src, fp32 and bf16).
The agg_vw knob at 1 and 2 (0 is the default); at F = 128 an odd ldx (the scalar form); at F = 100
and 128 a table with NaN, +-inf and +-0 planted as tests/test_gpu_reduce.py::test_special_values
plants them.  Some 620 lines: not the full cross product, but every kernel instantiation class the
two entry points reach on these shapes, with and without split rows."""
import contextlib
import hashlib
import itertools
import os
import sys

import numpy as np
import torch


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


ROOT = os.path.abspath(_arg("--root", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402

N, HEAVY, R64, R65 = 300, 150, 10, 11
EMPTY = (0, 37, 120, 201, 250)
WIDTHS = (3, 36, 64, 100, 128, 256, 300, 602, 1024)
PLANS = (None, 64, 512)
ALL5 = ops.MULTI_REDS
RED3 = ("MEAN", "MAX", "MIN")
SUBSETS = [s for r in range(1, 6) for s in itertools.combinations(ALL5, r)]


def graph_np():
    rng = np.random.default_rng(7)
    deg = rng.multinomial(5170, np.full(N, 1.0 / N))
    deg[list(EMPTY)] = 0
    deg[HEAVY], deg[R64], deg[R65], deg[-1] = 700, 64, 65, 1
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = rng.integers(0, N, int(ip[-1])).astype(np.int32)
    return ip, ix


@contextlib.contextmanager
def knob(key, value):
    old = ops.get_debug(key)
    try:
        ops.set_debug(key, value)
        yield
    finally:
        ops.set_debug(key, old)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    if not torch.cuda.is_available():
        print("error: no HIP device", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    out = _arg("--out", None)
    ip, ix = graph_np()
    g = G.from_numpy(ip, ix, device=dev)
    E = len(ix)
    lines = []

    def emit(case, *tensors):
        torch.cuda.synchronize(dev)
        lines.append(f"{case} {digest(*tensors)}")

    def multi(tag, x, mode, plan, reds):
        if len(reds) == 5:  # the outputs as column blocks of one table: row stride 5F
            table = torch.full((N, 5 * x.shape[1]), 7.0, device=dev)
            ops.reduce_multi(g, x, reds, mode, out=table, plan=plan)
            emit(f"{tag} multi {'+'.join(reds)} table", table)
        else:
            emit(f"{tag} multi {'+'.join(reds)}", *ops.reduce_multi(g, x, reds, mode, plan=plan))

    def every(tag, x, mode, plan, reds=("MAX", "MIN", "ADD"), subsets=(RED3, ALL5)):
        for red in reds:
            emit(f"{tag} {red}", ops.reduce(g, x, red, mode, plan=plan))
        for s in subsets:
            multi(tag, x, mode, plan, s)

    for F in WIDTHS:
        rng = np.random.default_rng(1000 + F)
        xn = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32)).to(dev)
        xe = torch.from_numpy(rng.standard_normal((E, F)).astype(np.float32)).to(dev)
        xb = xn.to(torch.bfloat16)
        # every operand with many split rows and with none; plan 512 (one split row) on the fp32 tables
        for name, x, mode in (("edge fp32", xe, "edge"), ("src fp32", xn, "src"), ("dst fp32", xn, "dst"),
                              ("src bf16", xb, "src"), ("dst bf16", xb, "dst")):
            every(f"F={F} {name} plan=64", x, mode, 64)
            every(f"F={F} {name} plan=None", x, mode, None, reds=("MAX",))
        for name, x, mode in (("edge fp32", xe, "edge"), ("src fp32", xn, "src")):
            every(f"F={F} {name} plan=512", x, mode, 512, reds=("MAX",), subsets=(ALL5,))
        if F in (100, 128):  # the other 29 subsets: which outputs are stored, moments with or without extrema
            rest = [s for s in SUBSETS if s not in (RED3, ALL5)]
            every(f"F={F} src fp32 plan=64", xn, "src", 64, reds=(), subsets=rest)
            every(f"F={F} src bf16 plan=64", xb, "src", 64, reds=(), subsets=rest)
        for vw in (1, 2):
            with knob("agg_vw", vw):
                every(f"F={F} src fp32 plan=64 agg_vw={vw}", xn, "src", 64, reds=("MAX",))
                if F in (100, 128):
                    every(f"F={F} src bf16 plan=64 agg_vw={vw}", xb, "src", 64, reds=("MAX",))
        if F == 128:  # an odd leading dimension: the scalar form
            for name, t, mode in (("src", xn, "src"), ("edge", xe, "edge")):
                wide = torch.full((t.shape[0], F + 1), float("nan"), device=dev)
                wide[:, :F] = t
                every(f"F={F} {name} fp32 ldx=F+1 plan=64", wide[:, :F], mode, 64)
        if F in (100, 128):  # special values, through the edge tensor and through an index
            v = xe.clone()
            v[int(ip[HEAVY]) + 130, 5] = float("nan")  # the third item of the heavy row at chunk 64
            v[int(ip[-1]) - 1, F - 1] = float("nan")   # the last row's only edge
            v[int(ip[R64]):int(ip[R64 + 1])] = float("-inf")
            v[int(ip[R65]):int(ip[R65 + 1])] = float("inf")
            v[int(ip[R65 + 1]):int(ip[R65 + 2]), ::2] = 0.0
            v[int(ip[R65 + 1]):int(ip[R65 + 2]):2, ::2] = -0.0
            xs = xn.clone()
            xs[17, 5] = float("nan")
            xs[18], xs[19] = float("inf"), float("-inf")
            xs[20, ::2], xs[21, ::2] = 0.0, -0.0
            for plan in PLANS:
                every(f"F={F} special edge plan={plan}", v, "edge", plan, subsets=(ALL5,))
            every(f"F={F} special src plan=64", xs, "src", 64, subsets=(ALL5,))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
