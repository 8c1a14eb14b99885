"""A GraphSAGE-pool layer whose gather reads a virtual scatter (tests, and scripts/reduce_blocked_layer.py).

frontend.gen_ops(..., aggregator=) rewrites only the gathers' COMP_TYPE, so in every network's op
graph an applyedge MUL by an edge weight still sits between the scatter and the gather, and the
executor reduces that [E, F] product in EDGE mode: no stock layer hands
_eval_reduce a virtual scatter.  GraphSAGE-pool as published has no edge weight -- the max over the
neighbours' rows -- which is GraphSAGE's layer with that MUL dropped:

    0 scatter C(x) -> 1 gather `agg` -> 2 MM;  3 MM(x);  4 ADD(2, 3);  5 SF

These records are what the column-blocked reducers' executor tests run.
"""
import copy

from gta_graph_tensor_acclelrator_for_general_gnn_amd import frontend, ir, lowering
from gta_graph_tensor_acclelrator_for_general_gnn_amd.semantics import Semantics


def records(n, e, feature, agg, layer=2):
    recs = copy.deepcopy(frontend.gen_ops("GraphSAGE", layer, n, e, feature, False, aggregator=agg))
    assert [(r["TYPE"], r["COMP_TYPE"]) for r in recs[:3]] == [("scatter", "NONE"), ("applyedge", "MUL"), ("gather", agg)]
    mul_out = recs[1]["OUTPUT"]["output_list"]
    new = lambda i: i if i < 1 else i - 1  # noqa: E731
    out = []
    for r in recs:
        if r["OP_NO"] == 1:
            continue
        ins = [0 if i == 1 else new(i) for i in r["INPUT"]["input_g_list"]]
        outs = [new(j) for o in r["OUTPUT"]["output_list"] for j in (mul_out if o == 1 else [o])]
        r["INPUT"]["input_g_list"], r["OUTPUT"]["output_list"], r["OP_NO"] = ins, outs, new(r["OP_NO"])
        out.append(r)
    return out


def layer(n, e, feature, agg, tile=64):
    """-> (records, OpGraph, Stream, Semantics) with the scatter and the gather in one block."""
    recs = records(n, e, feature, agg)
    op_array = [[0, 1]] + [[i] for i in range(2, len(recs))]
    stream = ir.Stream(lowering.lower(recs, n, op_array, [[tile, 1]] * len(op_array)))
    return recs, ir.OpGraph(recs), stream, Semantics()
