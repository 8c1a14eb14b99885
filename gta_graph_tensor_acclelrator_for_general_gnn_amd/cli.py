"""Command line in the shape of the reference's start.py (code/start.py:13-62, vTCAD/code/start.py):
compile every layer, generate its instruction stream, then run it -- here on the GPU, with the
reference's modelled latency and traffic for the same stream printed beside the measured time.

  python -m gta_graph_tensor_acclelrator_for_general_gnn_amd --dataset cora --network GCN

start.py's flags keep their names and meaning (--dataset, --network, --isReorder, --isSinput,
--isPingpang).  Two differences, both deliberate:
  - start.py declares its flags type=bool, so any non-empty value, "False" included, turns one on;
    here "False" / "0" / "no" turn it off.
  - start.py reads the op graphs the reference committed under Network/ (GAT: layer1-3, every other
    network: one 'alllayer' file).  This tool generates each layer's op graph itself
    (frontend.gen_ops, genGraphOP's three layers) on a synthetic graph of the dataset's shape
    (graph.SHAPES; no dataset files here) and runs each layer on fresh seeded tensors, as the
    reference simulates each layer on its own.
Printed as start.py prints them (:35-62): the phase lines, 'Latency:' (modelled cycles - 1) / 1e9 s
(the cycle model runs at Python speed, so by default only up to --model-edges edges), the modelled
DRAM bytes in MB, the 'Test Name:' line; then the measured device time per layer and in total.
The layers run through the libgta kernels only: no HIP device is an error, not a CPU run.
"""
import argparse
import json
import sys

import torch

from . import compiler, executor, frontend, graph as G, pipeline, tiles, workloads

FEATURES = {"cora": 1433, "citeseer": 3703, "pubmed": 500, "flickr": 500, "reddit": 602,
            "products": 100}  # genGraphOP.py:178-195 (cora / pubmed / citeseer / reddit); configs.py (flickr / products)


def _flag(v):
    s = str(v).strip().lower()
    if s in ("1", "true", "yes", "y", "on"):
        return True
    if s in ("0", "false", "no", "n", "off", ""):
        return False
    raise argparse.ArgumentTypeError(f"not a boolean: {v!r}")


def _aggregator(v):
    """--aggregator: one name of frontend.AGGREGATORS, or a comma list (PNA) as a tuple."""
    names = [s.strip().upper() for s in str(v).split(",")]
    if len(names) == 1:
        if names[0] not in frontend.AGGREGATORS:
            raise argparse.ArgumentTypeError(f"{v!r}: one of {', '.join(frontend.AGGREGATORS)}, or a comma list for PNA")
        return names[0]
    if len(set(names)) != len(names) or any(n not in frontend.MULTI_AGGREGATORS for n in names):
        raise argparse.ArgumentTypeError(f"{v!r}: a comma list holds distinct names of "
                                         f"{', '.join(frontend.MULTI_AGGREGATORS)}")
    return tuple(names)


def parser():
    p = argparse.ArgumentParser(prog="python -m gta_graph_tensor_acclelrator_for_general_gnn_amd",
                                description="compile -> instruction stream -> GPU execution (start.py's flow)")
    p.add_argument("--dataset", required=True, choices=sorted(G.SHAPES), help="dataset shape (graph.SHAPES)")
    p.add_argument("--network", required=True, choices=["GCN", "GAT", "SGC", "GraphSAGE", "GIN", "DGN", "PNA"])
    p.add_argument("--isReorder", type=_flag, default=False, help="the reordered (trans) op graph")
    p.add_argument("--isSinput", type=_flag, default=False, help="modelled with the streaming-input option")
    p.add_argument("--isPingpang", type=_flag, default=False, help="fusion search with ping-pong buffers")
    p.add_argument("--layers", default="1,2,3", help="genGraphOP layers to run (default 1,2,3)")
    p.add_argument("--feature", type=int, default=None, help="input width (default: the dataset's)")
    p.add_argument("--heads", type=int, default=16, help="attention heads (GAT)")
    p.add_argument("--aggregator", default="ADD", type=_aggregator, metavar="{" + ",".join(frontend.AGGREGATORS) + "}",
                   help="reduce function of the message gathers (their COMP_TYPE); GAT takes ADD only.  PNA also "
                        "takes a comma list, e.g. MEAN,MAX,MIN,STD: every aggregator over the same messages, one launch")
    p.add_argument("--stable-softmax", action="store_true",
                   help="overflow-safe attention softmax: exp(score - row max) (GAT; off: the unshifted kernels)")
    p.add_argument("--gather-dtype", choices=["f32", "bf16"], default="f32",
                   help="storage type of the node tables the column-blocked aggregates gather (bf16: rounded "
                        "once, sums in fp32; f32: as they are)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--reps", type=int, default=3, help="runs per layer; the fastest is reported")
    p.add_argument("--model-edges", type=int, default=1 << 20,
                   help="run the cycle model when the graph has at most this many edges")
    p.add_argument("--json", action="store_true", help="also print one JSON line with every number")
    return p


def run(args, device, log=print):
    """The three phases of start.py on `device`; returns the summary dict."""
    feature = args.feature or FEATURES[args.dataset]
    layer_ids = [int(v) for v in str(args.layers).split(",") if v.strip()]
    if not layer_ids or any(L not in (1, 2, 3) for L in layer_ids):
        raise ValueError(f"--layers: genGraphOP defines layers 1, 2 and 3 (got {args.layers!r})")
    g = G.dataset_graph(args.dataset, seed=args.seed, device=device)
    log("Starting compilation...")
    layers = []
    meta = tiles.metadata(g, start=64, end=min(g.n_rows, 4096))  # what pipeline.Layer computes by default
    for L in layer_ids:
        records = frontend.gen_ops(args.network, L, g.n_rows, g.nnz, feature, args.isReorder, args.heads,
                                   getattr(args, "aggregator", "ADD"))
        # (a tuple aggregator's graph: no search, pipeline.Layer takes its default partition)
        cands = [] if isinstance(getattr(args, "aggregator", "ADD"), tuple) else \
            compiler.search(records, g.n_rows, *meta, pingpang=args.isPingpang, sinput=args.isSinput)
        kw = dict(reorder=args.isReorder, heads=args.heads, metadata=meta, pingpang=args.isPingpang,
                  sinput=args.isSinput, aggregator=getattr(args, "aggregator", "ADD"),
                  stable_softmax=getattr(args, "stable_softmax", False))
        if getattr(args, "gather_dtype", "f32") == "bf16":
            kw["gather_dtype"] = torch.bfloat16
        lay = None
        for k, (op_array, tile_size_list) in enumerate(c[:2] for c in cands):
            try:
                lay = pipeline.Layer(args.network, L, g, feature, op_array=op_array, tile_size_list=tile_size_list, **kw)
                break
            except TypeError as e:
                # the reference's interpret() raises on some partitions its search ranks first
                # (lowering.py restates it, code/interpreter.py:165-194); take the next candidate
                log(f"  layer{L}: candidate {k} does not lower ({e}); trying the next")
        if lay is None:  # no candidate (or none lowers): Layer's default partition
            lay = pipeline.Layer(args.network, L, g, feature, **kw)
        layers.append(lay)
    log("Compilation Done\n")
    log("Generating instructions...")
    for lay in layers:  # lowered in Layer (lowering.lower); report what interpret() would have written
        log(f"  layer{lay.layer}: {len(lay.op_array)} fused blocks, "
            f"{sum(len(b) for b in lay.stream_records)} instructions")
    log("Inst Generated\n")
    log("Starting simulation...")
    model = "full" if g.nnz <= args.model_edges else "rw"
    cycle, rw, per_layer = 0, 0, []
    for k, lay in enumerate(layers):
        tensors = workloads.make_tensors(lay.opgraph, g, args.network, seed=args.seed + k)
        best = None
        for _ in range(max(1, args.reps)):
            res, _ = lay.run(tensors)
            best = res.elapsed_s if best is None else min(best, res.elapsed_s)
        try:
            executor.attach_model(res, lay.stream_records, lay.tile_size_list, g, model, args.isSinput, args.dataset)
        except RuntimeError as e:  # costmodel raises where simulate()'s cycle loop would never end
            log(f"  layer{lay.layer}: no modelled latency ({e}); traffic only")
            model = "rw"
            executor.attach_model(res, lay.stream_records, lay.tile_size_list, g, model, args.isSinput, args.dataset)
        rw += res.model_rw
        if res.model_cycles is not None:
            cycle += res.model_cycles
        per_layer.append({"layer": lay.layer, "measured_ms": best * 1e3, "model_rw": res.model_rw,
                          "model_cycles": res.model_cycles, "blocks": lay.op_array,
                          "tiles": lay.tile_size_list})
    log("Simulation Done\n")
    name = f"{args.dataset}-{args.network}-{'Reorder' if args.isReorder else 'Original'}"
    if model == "full":
        log(f"Latency: {(cycle - 1) / 10 ** 9} s")
    elif g.nnz > args.model_edges:
        log(f"Latency: (cycle model skipped: {g.nnz} edges > --model-edges {args.model_edges})")
    else:
        log("Latency: (no modelled latency: the cycle model does not terminate on a layer's stream)")
    log(f"总访存量: {rw / 10 ** 6} MB")
    log(f"Test Name: {name}")
    for r in per_layer:
        log(f"Measured layer{r['layer']}: {r['measured_ms']:.4f} ms on {device}")
    total_ms = sum(r["measured_ms"] for r in per_layer)
    log(f"Measured total: {total_ms:.4f} ms")
    return {"test_name": name, "N": g.n_rows, "E": g.nnz, "feature": feature,
            "model_cycles": cycle if model == "full" else None, "model_rw": rw,
            "measured_ms": total_ms, "layers": per_layer}


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if isinstance(args.aggregator, tuple) and args.network != "PNA":
        p.error(f"--aggregator {','.join(args.aggregator)}: a comma list is PNA's (several aggregators of the same "
                f"messages); {args.network} takes one name")
    if not torch.cuda.is_available():
        print("error: no HIP device: the layers run on libgta's kernels only", file=sys.stderr)
        return 2
    out = run(args, torch.device("cuda", torch.cuda.current_device()))
    if args.json:
        print(json.dumps(out, default=str))
    return 0
