"""Result bits of every column-blocked entry point, one sha256 per case: python scripts/blocked_bits.py [--out FILE]

Run in two builds (the parent's checkout and this tree) the two listings must be identical: the
check that a change to the blocked item kernels or their dispatch moved no result bit.  Each line is
`<case> <sha256 over the raw bytes of y>` (and of sums for the GAT aggregate).

Graphs: tests/test_gpu_reduce_blocked.py's g900 (900 rows, 30,000 edges) and empty (300 rows with empty
rows, a 3-edge and a 1,500-edge row), rebuilt here from the same seeds.  Cases: F in {64, 128, 256} x
{fp32, bf16} x blocks {1, 5} x item_edges {7, 256}; the sum unweighted, with [E, 1] and with [E, 8]
weights; the GAT aggregate (exp-leaky-relu and exp scores) unshifted and shifted; MAX and MIN.  At
F = 128, where the knobs select other kernels: seg_lean / att_lean 1 and 0, seg_alpha1 1 and 0, seg_pf 0
and 1."""
import contextlib
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402

HEAVY, SHORT = 5, 6  # rows of the "empty" graph: 1,500 edges / 3 edges
H = 8


def graphs():
    ip9, ix9 = G.synthetic(900, 30000, seed=11).numpy()
    rng = np.random.default_rng(4)
    deg = np.diff(ip9)[:300].copy()
    deg[[0, 17, 18, 299]] = 0
    deg[HEAVY], deg[SHORT] = 1500, 3
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = np.concatenate([np.sort(rng.integers(0, 300, d)) for d in deg]).astype(np.int32)
    own = {int(ix[ip[HEAVY] + e]): HEAVY for e in (16, 600)}  # as the test: three sources gathered by one row only
    own[int(ix[ip[SHORT] + 1])] = SHORT
    spare = next(s for s in range(300) if s not in own)
    for r in range(300):
        seg = ix[ip[r]:ip[r + 1]]
        for s, owner in own.items():
            if r != owner:
                seg[seg == s] = spare
        seg.sort()
    return {"g900": (ip9, ix9), "empty": (ip, ix)}


@contextlib.contextmanager
def knobs(**kv):
    old = {k: ops.get_debug(k) for k in kv}
    try:
        for k, v in kv.items():
            ops.set_debug(k, v)
        yield
    finally:
        for k, v in old.items():
            ops.set_debug(k, v)


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
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []

    def emit(case, *tensors):
        torch.cuda.synchronize(dev)
        lines.append(f"{case} {digest(*tensors)}")

    for name, (ip, ix) in graphs().items():
        g = G.from_numpy(ip, ix, device=dev)
        rng = np.random.default_rng(7)
        w1 = torch.from_numpy(rng.random((g.nnz, 1)).astype(np.float32)).to(dev)
        w8 = torch.from_numpy(rng.random((g.nnz, H)).astype(np.float32)).to(dev)
        a = torch.from_numpy(rng.standard_normal((g.n_rows, H)).astype(np.float32)).to(dev)
        b = torch.from_numpy(rng.standard_normal((g.n_rows, H)).astype(np.float32)).to(dev)
        shifts = {sf: ops.softmax_shift(g, a, b, sf) for sf in ("EXP_LEAKY_RELU", "EXP")}
        for F in (64, 128, 256):
            xf = torch.from_numpy(np.random.default_rng(1000 + F).standard_normal((g.n_rows, F)).astype(np.float32)).to(dev)
            for bf in (False, True):
                x = ops.pitched(xf.to(torch.bfloat16)) if bf else xf
                for blocks in (1, 5):
                    for item_edges in (7, 256):
                        plan = g.blocked_plan(blocks, item_edges)
                        base = f"{name} F={F} {'bf16' if bf else 'fp32'} B={blocks} items={item_edges}"
                        for lean in ((1, 0) if F == 128 else (1,)):
                            tag = f"{base} lean={lean}"
                            with knobs(seg_lean=lean, att_lean=lean):
                                emit(f"{tag} sum", ops.aggregate_blocked(g, x, None, plan=plan))
                                emit(f"{tag} sum_w1", ops.aggregate_blocked(g, x, w1, plan=plan))
                                for a1 in ((1, 0) if F == 128 and lean else (1,)):
                                    for pf in ((0, 1) if F == 128 and lean and a1 else (0,)):
                                        with knobs(seg_alpha1=a1, seg_pf=pf):
                                            emit(f"{tag} sum_w8 alpha1={a1} pf={pf}", ops.aggregate_blocked(g, x, w8, plan=plan))
                                for sf in ("EXP_LEAKY_RELU", "EXP"):
                                    emit(f"{tag} gat {sf}", *ops.gat_aggregate_blocked(g, x, a, b, sf=sf, want_sums=True, plan=plan))
                                    emit(f"{tag} gat {sf} shifted", *ops.gat_aggregate_blocked(
                                        g, x, a, b, sf=sf, want_sums=True, plan=plan, shift=shifts[sf]))
                                for red in ("MAX", "MIN"):
                                    emit(f"{tag} {red}", ops.reduce_blocked(g, x, red, plan=plan))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
