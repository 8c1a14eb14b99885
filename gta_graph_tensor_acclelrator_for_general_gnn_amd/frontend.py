"""Op-graph front end: GNN layer -> op-graph records (the op_template of the IR).

Restates vTCAD/GraphOP/genGraphOP.py:27-154 (gen_yaml) as data: each network is a
table of op rows with symbolic sizes, expanded per layer.  Pinned byte-for-byte
against the reference's YAML for all 7 networks x 3 layers x original/trans
(tests/test_frontend.py).  Sizes are bytes of fp32 features, as in the reference:
  fin  = [0, F, 128, 64, 16][layer]   input width      (genGraphOP.py:31)
  fout = [0, 128, 64, 16][layer]      output width     (genGraphOP.py:32)
  fh   = 16 (weight_size[3])          attention width; `heads` overrides it
The reference's quirks are part of the data (GAT row 2 carries OP_NO 1; GCN-trans
ops 1/2 list themselves as outputs; PNA-trans ops 0/1 list themselves as inputs;
GAT-original op 10 lists input 7).
"""
import yaml

# row: (op_no, comp, type, order, fnum, inputs, g_num, nong, wsize, in_sizes, outputs, onum, osize)
#   fnum/onum: "N"/"E" symbols; wsize/in_sizes/osize: products of fin/fout/fh (bytes = 4 * product)
_N, _E = "N", "E"


def _r(no, comp, kind, order, fnum, ins, g, nong, w, isz, outs, onum, osz):
    return (no, comp, kind, order, fnum, ins, g, nong, w, isz, outs, onum, osz)


_AGG_IN = ("fin",)
TABLE = {
    ("GCN", False): [
        _r(0, "NONE", "scatter", "C", [_N], [], 1, 0, None, ["fin"], [1], _E, "fin"),
        _r(1, "MUL", "applyedge", "R", [_E, _E], [0, -1], 2, 0, None, ["fin", "fin"], [2], _E, "fin"),
        _r(2, "ADD", "gather", "R", [_E], [1], 1, 0, None, ["fin"], [3], _N, "fin"),
        _r(3, "MM", "applynode", "R", [_N], [2], 1, 1, "fin*fout", ["fin"], [], _N, "fout"),
    ],
    ("GCN", True): [
        _r(0, "MM", "applynode", "R", [_N], [], 1, 1, "fin*fout", ["fin"], [1], _N, "fout"),
        _r(1, "NONE", "scatter", "C", [_N], [0], 1, 0, None, ["fout"], [1], _E, "fout"),
        _r(2, "MUL", "applyedge", "R", [_E], [1, -1], 2, 0, None, ["fout", "fout"], [2], _E, "fout"),
        _r(3, "ADD", "gather", "R", [_E], [2], 1, 0, None, ["fout"], [], _N, "fout"),
    ],
    ("GAT", False): [
        _r(0, "MM", "applynode", "R", [_N], [], 1, 1, "fout*fin", ["fin"], [1, 2, 3], _N, "fout"),
        _r(1, "MM", "applynode", "R", [_N], [0], 1, 1, "fout*fh", ["fout"], [4], _N, "fh"),
        _r(1, "MM", "applynode", "R", [_N], [0], 1, 1, "fout*fh", ["fout"], [5], _N, "fh"),
        _r(3, "NONE", "scatter", "C", [_N], [0], 1, 0, None, ["fout"], [11], _E, "fout"),
        _r(4, "NONE", "scatter", "R", [_N], [1], 1, 0, None, ["fh"], [6], _E, "fh"),
        _r(5, "NONE", "scatter", "C", [_N], [2], 1, 0, None, ["fh"], [6], _E, "fh"),
        _r(6, "ADD", "applyedge", "R", [_E, _E], [4, 5], 2, 0, None, ["fh", "fh"], [7], _E, "fh"),
        _r(7, "SF", "applyedge", "R", [_E], [6], 1, 0, None, ["fh"], [8, 9], _E, "fh"),
        _r(8, "ADD", "gather", "R", [_E], [7], 1, 0, None, ["fh"], [10], _N, "fh"),
        _r(9, "MUL", "applyedge", "R", [_E, _E], [7, 10], 2, 0, None, ["fh", "fh"], [11], _E, "fh"),
        _r(10, "NONE", "scatter", "R", [_N], [7], 1, 0, None, ["fh"], [9], _E, "fh"),
        _r(11, "MUL", "applyedge", "R", [_E, _E], [3, 9], 2, 0, None, ["fout", "fh"], [12], _E, "fout"),
        _r(12, "ADD", "gather", "R", [_E], [11], 1, 0, None, ["fout"], [13], _N, "fout"),
        _r(13, "SF", "applynode", "R", [_N], [12], 1, 0, None, ["fout"], [], _N, "fout"),
    ],
    ("GAT", True): [
        _r(0, "MM", "applynode", "R", [_N], [], 1, 1, "fout*fin", ["fin"], [1, 2, 3], _N, "fout"),
        _r(1, "MM", "applynode", "R", [_N], [0], 1, 1, "fout*fh", ["fout"], [4], _N, "fh"),
        _r(1, "MM", "applynode", "R", [_N], [0], 1, 1, "fout*fh", ["fout"], [5], _N, "fh"),
        _r(3, "NONE", "scatter", "C", [_N], [0], 1, 0, None, ["fout"], [11], _E, "fout"),
        _r(4, "NONE", "scatter", "R", [_N], [1], 1, 0, None, ["fh"], [6], _E, "fh"),
        _r(5, "NONE", "scatter", "C", [_N], [2], 1, 0, None, ["fh"], [6], _E, "fh"),
        _r(6, "ADD", "applyedge", "R", [_E, _E], [4, 5], 2, 0, None, ["fh", "fh"], [7], _E, "fh"),
        _r(7, "MUL", "applyedge", "R", [_E, _E], [3, 8], 2, 0, None, ["fout", "fh"], [10], _E, "fout"),
        _r(8, "SF", "applyedge", "R", [_E], [6], 1, 0, None, ["fh"], [9], _E, "fh"),
        _r(9, "ADD", "gather", "R", [_E], [8], 1, 0, None, ["fh"], [11], _N, "fh"),
        _r(10, "ADD", "gather", "R", [_E], [7], 1, 0, None, ["fout"], [11], _N, "fout"),
        _r(11, "MUL", "applynode", "R", [_N, _N], [9, 10], 2, 0, None, ["fh", "fout"], [12], _N, "fout"),
        _r(12, "SF", "applynode", "R", [_N], [11], 1, 0, None, ["fout"], [], _N, "fout"),
    ],
    "SGC": [
        _r(0, "NONE", "scatter", "C", [_N], [], 1, 0, None, ["fin"], [1], _E, "fin"),
        _r(1, "MUL", "applyedge", "R", [_E, _E], [0, -1], 2, 0, None, ["fin", "fin"], [2], _E, "fin"),
        _r(2, "ADD", "gather", "R", [_E], [1], 1, 0, None, ["fin"], [3], _N, "fin"),
        _r(3, "NONE", "scatter", "C", [_N], [2], 1, 0, None, ["fin"], [4], _E, "fin"),
        _r(4, "MUL", "applyedge", "R", [_E, _E], [3, -1], 2, 0, None, ["fin", "fin"], [5], _E, "fin"),
        _r(5, "ADD", "gather", "R", [_E], [4], 1, 0, None, ["fin"], [6], _N, "fin"),
        _r(6, "MM", "applynode", "R", [_N], [5], 1, 1, "fin*fout", ["fin"], [], _N, "fout"),
    ],
    "GraphSAGE": [
        _r(0, "NONE", "scatter", "C", [_N], [], 1, 0, None, ["fin"], [1], _E, "fin"),
        _r(1, "MUL", "applyedge", "R", [_E, _E], [0, -1], 2, 0, None, ["fin", "fin"], [2], _E, "fin"),
        _r(2, "ADD", "gather", "R", [_E], [1], 1, 0, None, ["fin"], [3], _N, "fin"),
        _r(3, "MM", "applynode", "R", [_N], [2], 1, 1, "fin*fout", ["fin"], [5], _N, "fout"),
        _r(4, "MM", "applynode", "R", [_N], [], 1, 1, "fin*fout", ["fin"], [5], _N, "fout"),
        _r(5, "ADD", "applynode", "R", [_N, _N], [3, 4], 2, 0, None, ["fout", "fout"], [6], _N, "fout"),
        _r(6, "SF", "applynode", "R", [_N], [5], 1, 0, None, ["fout"], [], _N, "fout"),
    ],
    "GIN": [
        _r(0, "NONE", "scatter", "C", [_N], [], 1, 0, None, ["fin"], [1], _E, "fin"),
        _r(1, "MUL", "applyedge", "R", [_E, _E], [0, -1], 2, 0, None, ["fin", "fin"], [2], _E, "fin"),
        _r(2, "ADD", "gather", "R", [_E], [1], 1, 0, None, ["fin"], [3], _N, "fin"),
        _r(3, "MUL", "applynode", "R", [_N, _N], [-1, -1], 2, 0, None, ["fin", "1"], [4], _N, "fin"),
        _r(4, "ADD", "applynode", "R", [_N, _N], [2, 3], 2, 0, None, ["fin", "fin"], [5], _N, "fin"),
        _r(5, "MM", "applynode", "R", [_N], [4], 1, 1, "fin*fout", ["fin"], [6], _N, "fout"),
        _r(6, "SF", "applynode", "R", [_N], [5], 1, 0, None, ["fout"], [7], _N, "fout"),
        _r(7, "MM", "applynode", "R", [_N], [6], 1, 1, "fout*fout", ["fout"], [8], _N, "fout"),
        _r(8, "SF", "applynode", "R", [_N], [7], 1, 0, None, ["fout"], [], _N, "fout"),
    ],
    "DGN": [
        _r(0, "NONE", "scatter", "C", [_N], [], 1, 0, None, ["fin"], [2], _E, "fin"),
        _r(1, "NONE", "scatter", "R", [_N], [], 1, 0, None, ["fin"], [2], _E, "fin"),
        _r(2, "ADD", "applyedge", "R", [_E, _E], [0, 1], 2, 0, None, ["fin", "fin"], [3], _E, "fin"),
        _r(3, "MM", "applyedge", "R", [_E], [2], 1, 1, "fin*fout", ["fin"], [7], _E, "fout"),
        _r(4, "NONE", "scatter", "C", [_N], [], 1, 0, None, ["fout"], [6], _E, "fout"),
        _r(5, "NONE", "scatter", "R", [_N], [], 1, 0, None, ["fout"], [6], _E, "fout"),
        _r(6, "ADD", "applyedge", "R", [_E, _E], [4, 5], 2, 0, None, ["fout", "fout"], [7], _E, "fout"),
        _r(7, "ADD", "applyedge", "R", [_E, _E], [3, 6], 2, 0, None, ["fout", "fout"], [8], _E, "fout"),
        _r(8, "ADD", "gather", "R", [_E], [7], 1, 0, None, ["fout"], [9], _N, "fout"),
        _r(9, "MUL", "applynode", "R", [_N], [8], 1, 0, None, ["fout"], [10], _N, "fout"),
        _r(10, "SF", "applynode", "R", [_N], [9], 1, 0, None, ["fout"], [], _N, "fout"),
    ],
    ("PNA", False): [
        _r(0, "NONE", "scatter", "C", [_N], [], 1, 0, None, ["fin"], [3], _E, "fin"),
        _r(1, "NONE", "scatter", "R", [_N], [], 1, 0, None, ["fin"], [4], _E, "fin"),
        _r(2, "MM", "applyedge", "R", [_E], [], 1, 1, "fin*fout", ["fin"], [6], _E, "fout"),
        _r(3, "MM", "applyedge", "R", [_E], [0], 1, 1, "fin*fout", ["fin"], [5], _E, "fout"),
        _r(4, "MM", "applyedge", "R", [_E], [1], 1, 1, "fin*fout", ["fin"], [5], _E, "fout"),
        _r(5, "ADD", "applyedge", "R", [_E, _E], [3, 4], 2, 0, None, ["fout", "fout"], [6], _E, "fout"),
        _r(6, "ADD", "applyedge", "R", [_E, _E], [2, 5], 2, 0, None, ["fout", "fout"], [7], _E, "fout"),
        _r(7, "SF", "applyedge", "R", [_E], [6], 1, 0, None, ["fout"], [8], _E, "fout"),
        _r(8, "ADD", "gather", "R", [_E], [7], 1, 0, None, ["fout"], [9], _N, "fout"),
        _r(9, "MUL", "applynode", "R", [_N], [8], 1, 0, None, ["fout"], [10], _N, "fout"),
        _r(10, "MM", "applynode", "R", [_N], [9], 1, 1, "fout*fout", ["fout"], [], _N, "fout"),
    ],
    ("PNA", True): [
        _r(0, "MM", "applynode", "R", [_N], [0], 1, 1, "fin*fout", ["fin"], [3], _N, "fout"),
        _r(1, "MM", "applynode", "R", [_N], [1], 1, 1, "fin*fout", ["fin"], [4], _N, "fout"),
        _r(2, "MM", "applyedge", "R", [_E], [], 1, 1, "fin*fout", ["fin"], [6], _E, "fout"),
        _r(3, "NONE", "scatter", "C", [_N], [], 1, 0, None, ["fout"], [5], _E, "fout"),
        _r(4, "NONE", "scatter", "R", [_N], [], 1, 0, None, ["fout"], [5], _E, "fout"),
        _r(5, "ADD", "applyedge", "R", [_E, _E], [3, 4], 2, 0, None, ["fout", "fout"], [6], _E, "fout"),
        _r(6, "ADD", "applyedge", "R", [_E, _E], [2, 5], 2, 0, None, ["fout", "fout"], [7], _E, "fout"),
        _r(7, "SF", "applyedge", "R", [_E], [6], 1, 0, None, ["fout"], [8], _E, "fout"),
        _r(8, "ADD", "gather", "R", [_E], [7], 1, 0, None, ["fout"], [9], _N, "fout"),
        _r(9, "MUL", "applynode", "R", [_N], [8], 1, 0, None, ["fout"], [10], _N, "fout"),
        _r(10, "MM", "applynode", "R", [_N], [9], 1, 1, "fout*fout", ["fout"], [], _N, "fout"),
    ],
}
NETWORKS = ["GCN", "GAT", "SGC", "GraphSAGE", "GIN", "DGN", "PNA"]


def _size(sym, env):
    v = 1
    for part in sym.split("*"):
        v *= env[part] if part in env else int(part)
    return v * 4


# COMP_TYPE values of a message gather (ADD: genGraphOP's; VAR / STD: the population variance and
# sqrt(VAR + eps) of the messages, PNA's fourth aggregator)
AGGREGATORS = ("ADD", "MAX", "MIN", "MEAN", "VAR", "STD")
MULTI_AGGREGATORS = ("MEAN", "MAX", "MIN", "VAR", "STD")  # what a tuple aggregator (PNA) may hold

_PNA_GATHER, _PNA_TAIL = 8, (9, 10)  # PNA's message gather and its tail (the scaler MUL, the MM) in both tables


def pna_clones(k):
    """{op of the expanded PNA graph: the op of TABLE's PNA it is a copy of} for a tuple aggregator
    of k members: gathers 8 .. 7+k (of op 8), scaler MULs 8+k .. 7+2k (of op 9), MMs 8+2k .. 7+3k
    (of op 10).  The k-1 ADDs that sum the MM outputs (8+3k ..) are new ops, copies of none."""
    out = {}
    for j in range(k):
        out[8 + j], out[8 + k + j], out[8 + 2 * k + j] = 8, 9, 10
    return out


def _pna_rows(rows, aggs):
    """PNA's rows with the message gather (op 8) as one sibling gather of op 7 per aggregator, each
    with its own clone of the tail (MUL op 9, MM op 10), the MM outputs summed by a chain of
    applynode ADDs: concat(a_1 .. a_K) W = sum_k a_k W_k, written with the ops the ISA has (it has
    no concat).  New ops are numbered consecutively after op 7 (pna_clones)."""
    k = len(aggs)
    head = [r for r in rows if r[0] < _PNA_GATHER]
    g8, m9, m10 = (next(r for r in rows if r[0] == i) for i in (_PNA_GATHER,) + _PNA_TAIL)
    G, M, W, A = 8, 8 + k, 8 + 2 * k, 8 + 3 * k  # first gather, MUL, MM and ADD
    out = [r if r[0] != 7 else r[:10] + ([G + j for j in range(k)],) + r[11:] for r in head]

    def clone(r, no, ins, outs, comp=None):
        return (no, comp or r[1], r[2], r[3], r[4], ins, r[6], r[7], r[8], r[9], outs, r[11], r[12])

    out += [clone(g8, G + j, [7], [M + j], comp=aggs[j]) for j in range(k)]
    out += [clone(m9, M + j, [G + j], [W + j]) for j in range(k)]
    # MM j feeds ADD max(j - 1, 0): the chain's first ADD sums MMs 0 and 1, each later one adds the next MM
    out += [clone(m10, W + j, [M + j], [A + max(j - 1, 0)]) for j in range(k)]
    for j in range(k - 1):
        ins = [W, W + 1] if j == 0 else [A + j - 1, W + j + 1]
        out.append(_r(A + j, "ADD", "applynode", "R", [_N, _N], ins, 2, 0, None, ["fout", "fout"],
                      [] if j == k - 2 else [A + j + 1], _N, "fout"))
    return out


def gen_ops(network, layer, node_num, edge_num, feature, reorder=False, heads=16, aggregator="ADD"):
    """Op-graph records for one layer (what gen_yaml writes, genGraphOP.py:27-154).

    aggregator: the reduce function of the network's message gathers -- the gather op's COMP_TYPE
    (the ISA gather carries it as a field: COMPUTE mul: add, template/ISA_defination.yaml:58-61).
    "ADD" is genGraphOP's output unchanged; "MAX" / "MIN" / "MEAN" / "VAR" / "STD" rewrite the
    COMP_TYPE of every gather of the layer (both hops of SGC) and nothing else: GraphSAGE-pool's
    max, PNA's max / min / mean / std, GCN- and SAGE-mean.  GAT's gathers are its softmax sums, not
    a message reducer: any other aggregator than ADD raises ValueError.
    A tuple or list (PNA only, e.g. ("MEAN", "MAX", "MIN", "STD"): distinct names of
    MULTI_AGGREGATORS, at least two) applies every member to the same messages: op 8 becomes one
    sibling gather of op 7 per member, each with its own scaler MUL and MM, summed by an ADD chain
    (_pna_rows; pna_clones names what each new op copies)."""
    key = (network, bool(reorder))
    rows = TABLE.get(key, TABLE.get(network))
    if rows is None:
        raise ValueError(f"no such network {network}")
    if isinstance(aggregator, (tuple, list)):
        aggs = tuple(aggregator)
        if network != "PNA":
            raise ValueError(f"a tuple aggregator is PNA's (several aggregators of the same messages); {network} takes one name")
        if len(aggs) < 2 or len(set(aggs)) != len(aggs) or any(a not in MULTI_AGGREGATORS for a in aggs):
            raise ValueError(f"a tuple aggregator holds two or more distinct names of {MULTI_AGGREGATORS} (got {aggs!r})")
        rows, aggregator = _pna_rows(rows, aggs), "ADD"  # (the gathers carry their COMP_TYPE already)
    if aggregator not in AGGREGATORS:
        raise ValueError(f"aggregator must be one of {AGGREGATORS} (got {aggregator!r})")
    if aggregator != "ADD" and network == "GAT":
        raise ValueError("GAT's gathers are the sums of its edge softmax: it takes no aggregator but ADD")
    env = {"fin": [0, feature, 128, 64, 16][layer], "fout": [0, 128, 64, 16][layer], "fh": heads}
    count = {_N: node_num, _E: edge_num}
    out = []
    for no, comp, kind, order, fnum, ins, g, nong, w, isz, outs, onum, osz in rows:
        if kind == "gather" and comp == "ADD":
            comp = aggregator
        out.append({
            "OP_NO": no, "COMP_TYPE": comp, "TYPE": kind, "ORDER": order,
            "INPUT": {"input_g_list": list(ins), "input_g_num": g, "input_nong_num": nong, "input_nong_list": [],
                      "input_size": [] if w is None else [_size(w, env)],
                      "feature_number": [count[f] for f in fnum],
                      "size_per_feature": [_size(s, env) for s in isz]},
            "OUTPUT": {"output_list": list(outs), "output_number": count[onum], "size_per_feature": _size(osz, env)},
        })
    return out


def gen_yaml(path, node_num, edge_num, size_per_feature, network, layer, isReorder, heads=16, aggregator="ADD"):
    """Same call and output as genGraphOP.gen_yaml (+ optional attention width `heads` and message
    `aggregator`, see gen_ops)."""
    import os
    data = gen_ops(network, layer, node_num, edge_num, size_per_feature, isReorder, heads, aggregator)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        yaml.safe_dump(data, f)
    return path


def dumps(records):
    return yaml.safe_dump(records)
