"""A/B: ops.aggregate_edge_mm against update_mm + aggregate_expr at Flickr PNA's shape, interleaved."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops

dev = torch.device("cuda:0")
n, E, K, N = 89250, 899756, 500, 128
g = G.synthetic(n, E, device=dev)
E = g.nnz
gen = torch.Generator().manual_seed(1)
ef = torch.randn(E, K, generator=gen).to(dev)
w = (torch.randn(K, N, generator=gen) / K ** 0.5).to(dev)
p, q = torch.randn(n, N, generator=gen).to(dev), torch.randn(n, N, generator=gen).to(dev)

def pair():
    m = ops.update_mm(ef, w, m=E)
    return ops.aggregate_expr(g, 2, [(p, "src"), (q, "dst"), (m, "edge")], ["ADD", "ADD"], [None, "RELU"], swap=True, plan=512)

def gemm():
    return ops.update_mm(ef, w, m=E)

def fused():
    return ops.aggregate_edge_mm(g, ef, w, p, q, "RELU")

def fused_bare():  # no p, no q, no SF: the ring GEMM, the tile and the walk over LDS alone
    return ops.aggregate_edge_mm(g, ef, w)

def gemm_ring1():  # the unfused GEMM forced onto k_mm_ring at 64-row groups: k_emm_gather's mainloop with a tile store
    ops.set_debug("mm_wave", 0)
    ops.set_debug("mm_ring_fr", 1)
    try:
        return ops.update_mm(ef, w, m=E)
    finally:
        ops.set_debug("mm_wave", 1)
        ops.set_debug("mm_ring_fr", 0)

def timed(fn, reps=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps

ya, yb = pair(), fused()
torch.cuda.synchronize()
d = (ya - yb).abs().max().item()
print(f"n={n} E={E} K={K} N={N}  max |pair - fused| = {d:.3e}  max |y| = {ya.abs().max().item():.3e}", flush=True)
for fn in (pair, gemm, fused, fused_bare, gemm_ring1):
    timed(fn, 3)
for r in range(5):
    print(f"rep {r}: pair {timed(pair):.4f} ms   gemm alone {timed(gemm):.4f} ms   fused {timed(fused):.4f} ms   "
          f"fused, no p / q / SF {timed(fused_bare):.4f} ms   gemm on k_mm_ring FR=1 {timed(gemm_ring1):.4f} ms", flush=True)
