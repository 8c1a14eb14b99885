"""Kernel time of the edge-wise / node-wise element kernels and the unfused GAT softmax at a
Flickr-shaped size (89,250 nodes, 899,756 edges): python scripts/edge_probe.py [--reps N]

One launch of each kernel between two HIP events, the median (and min, max) of N back-to-back eager
launches after three warm-up calls; one JSON line per leg.  Legs: apply_edge at Fo 8
(k_apply_edge_pack), 100 (k_apply_edge_cols<1>), 128 and 256 (k_apply_edge_flat<2>, <4>, and with
APPLY_EDGE_FLAT off k_apply_edge_cols<2>, <4>); apply_node at F 128 with apply_node_vec 0 / 1
(k_apply_node, k_apply_node4); edge_softmax at H 8 with esm_lane 0 / 1 and normalize on / off
(k_edge_softmax<8>, k_edge_softmax_v<8, 4>); softmax_shift at H 8 (k_softmax_shift<8>).  For an A/B run
it in the two builds alternately and compare the medians against the other build's own spread."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(s)
        fn()
        b.record(s)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"event_ms": round(ms[reps // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    dev = torch.device("cuda", 0)
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    g = G.dataset_graph("flickr", seed=0, device=dev)
    gen = torch.Generator(device="cpu").manual_seed(5)

    def randn(rows, F):
        return torch.randn(rows, F, generator=gen).to(dev)

    def leg(name, fn, **knobs):
        old = {k: ops.get_debug(k) for k in knobs}
        for k, v in knobs.items():
            ops.set_debug(k, v)
        try:
            rec = {"leg": name, "N": g.n_rows, "E": g.nnz, **timed(fn, reps)}
        finally:
            for k, v in old.items():
                ops.set_debug(k, v)
        print(json.dumps(rec), flush=True)

    old_flat = ops.APPLY_EDGE_FLAT
    try:
        for Fo, flat in ((8, False), (100, False), (128, True), (128, False), (256, True), (256, False)):
            a, b, out = randn(g.n_cols, Fo), randn(g.n_rows, Fo), torch.empty(g.nnz, Fo, device=dev)
            ops.APPLY_EDGE_FLAT = flat
            leg(f"apply_edge Fo={Fo} {'flat' if flat else 'sweep'}",
                lambda: ops.apply_edge(g, "ADD", "RELU", a, "src", b, "dst", out=out))
            del a, b, out
    finally:
        ops.APPLY_EDGE_FLAT = old_flat
    a, b, out = randn(g.n_rows, 128), randn(g.n_rows, 128), torch.empty(g.n_rows, 128, device=dev)
    for vec in (0, 1):
        leg(f"apply_node F=128 vec={vec}", lambda: ops.apply_node("ADD", "RELU", a, b, out=out), apply_node_vec=vec)
    H = 8
    a, b = randn(g.n_rows, H), randn(g.n_cols, H)
    out, sums = torch.empty(g.nnz, H, device=dev), torch.empty(g.n_rows, H, device=dev)
    for lane in (0, 1):
        for normalize in (True, False):
            leg(f"edge_softmax H={H} esm_lane={lane} normalize={int(normalize)}",
                lambda: ops.edge_softmax(g, a, b, normalize=normalize, out=out, sums=sums), esm_lane=lane)
    shift = torch.empty(g.n_rows, H, device=dev)
    leg(f"softmax_shift H={H}", lambda: ops.softmax_shift(g, a, b, out=shift))


if __name__ == "__main__":
    main()
