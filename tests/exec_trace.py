"""TEST-ONLY recording proxy over tests/fake_ops.py: the executor's call trace, as data.

`Recorder` stands where the executor looks up `ops`.  Every function the executor calls through it
is logged as one signature string -- the name, then each argument by parameter name (one left at,
or passed as, the parameter's default object is not listed: the same launch either way):
  * a tensor by provenance, with shape and dtype: `t:<key>` (shares storage with that entry of the
    run's `tensors` dict), `r<k>` (with result k of this run's calls; `r<k>.<j>` for a tuple
    result), else `new`; `+<offset>` when it starts inside that storage (a column view);
  * a graph as `csr` (the layer's own) or `csc:<kind>` (a view of ops.csc of it);
  * scalars, strings, dtypes and None as they are; lists and tuples element-wise.
Results and operands are kept alive for the run, so an address is never reused under a label.
`ops.csc` itself launches nothing and is a cached lookup: it is passed through unlogged (its views
show up as graph arguments).  After a run, `summary` adds alg_bytes, launches and gather_casts.

`runs()` lists every run of tests/golden/exec_trace.json; tests/golden/make_exec_trace.py writes
that file and tests/test_exec_trace_cpu.py requires it to be reproduced exactly.
"""
import contextlib
import copy
import inspect
import json
import os
import types

import numpy as np
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import executor, graph as G, ir, lowering, ops, pipeline, tiles, workloads
from gta_graph_tensor_acclelrator_for_general_gnn_amd.semantics import Semantics

from . import fake_ops, pool_layer, reduce_ref
from .conftest import GOLDEN, load_manifest

FIXTURE = os.path.join(GOLDEN, "exec_trace.json")
MATCHERS = ("consumers", "softmax", "attn", "reorder", "two_hop", "pushdown", "gacc", "gacc_t", "expr", "expr_nodes")
SWITCHES = ("fuse_softmax", "fuse_attention", "mm_first", "gather_acc", "edge_expr", "node_mm", "mm_pushdown",
            "sibling_mm", "fuse_sf", "fuse_mlp", "elide_scatter_stores")
_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.int64: "i64", torch.float64: "f64"}


class Recorder:
    def __init__(self, base, graph, tensors):
        self.base, self.graph, self.calls = base, graph, []
        self._labels, self._keep = {}, []
        for key, t in tensors.items():
            self._labels.setdefault(t.untyped_storage().data_ptr(), f"t:{key}")
            self._keep.append(t)

    def _arg(self, a):
        if isinstance(a, torch.Tensor):
            self._keep.append(a)
            where = self._labels.get(a.untyped_storage().data_ptr(), "new")
            off = f"+{a.storage_offset()}" if a.storage_offset() else ""
            return f"{where}{off}[{'x'.join(map(str, a.shape))},{_DT.get(a.dtype, a.dtype)}]"
        if isinstance(a, G.Graph):
            if a is self.graph:
                return "csr"
            c = self.base.csc(self.graph)
            return next((f"csc:{k}" for k in ("edge", "dst", "src") if c.view(k) is a), "graph?")
        if isinstance(a, (list, tuple)):
            return "(" + ",".join(self._arg(x) for x in a) + ")"
        if isinstance(a, torch.dtype):
            return _DT.get(a, str(a))
        return repr(a)

    def _result(self, k, r):
        for j, t in enumerate(r if isinstance(r, tuple) else (r,)):
            if isinstance(t, torch.Tensor):
                self._keep.append(t)
                self._labels.setdefault(t.untyped_storage().data_ptr(), f"r{k}.{j}" if isinstance(r, tuple) else f"r{k}")

    def __getattr__(self, name):
        fn = getattr(self.base, name)
        if not isinstance(fn, types.FunctionType) or name == "csc":
            return fn
        params = inspect.signature(fn)

        def call(*args, **kw):
            k = len(self.calls)
            bound = params.bind(*args, **kw)
            sig = [f"{n}={self._arg(v)}" for n, v in bound.arguments.items()
                   if isinstance(v, torch.Tensor) or v is not params.parameters[n].default]
            self.calls.append(f"{name}({', '.join(sig)})")
            r = fn(*args, **kw)
            self._result(k, r)
            return r
        return call


def canon(v):
    """A matcher attribute as one compact JSON string (tuples as lists, sets sorted, int keys as text)."""
    def c(x):
        if isinstance(x, dict):
            return {str(k): c(y) for k, y in sorted(x.items())}
        if isinstance(x, (set, frozenset)):
            return sorted(x)
        return [c(y) for y in x] if isinstance(x, (list, tuple)) else x
    return json.dumps(c(v), separators=(",", ":"))


@contextlib.contextmanager
def patched(mod, **names):
    missing = object()
    old = {n: getattr(mod, n, missing) for n in names}
    for n, v in names.items():
        setattr(mod, n, v)
    try:
        yield
    finally:
        for n, v in old.items():
            delattr(mod, n) if v is missing else setattr(mod, n, v)


@contextlib.contextmanager
def blocked_stand_ins():
    """fake_ops with numpy reduce / reduce_blocked / aggregate_blocked and the real plan's shape rules,
    as tests/test_reduce_blocked_cpu.py's `stand_ins` fixture opens the blocked gate."""
    def _red(graph, x, red, mode):
        ip, ix = graph.numpy()
        y = reduce_ref.reduce_csr(ip, ix, x.detach().cpu().float().numpy(), red, mode)
        return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))

    def reduce(graph, x, red="MAX", x_mode="src", out=None, plan=None):
        return _red(graph, x, red, x_mode)

    def reduce_blocked(graph, x, red="MAX", out=None, plan=None, blocks=32):
        return _red(graph, x, red, "src")

    def aggregate_blocked(graph, x, w=None, row_scale=None, out=None, accumulate=False, plan=None, blocks=32):
        return fake_ops.aggregate(graph, x.float(), "src", w, row_scale, out, accumulate)

    def pitched(t):
        return t

    class Plan:
        DTYPES = ops.BlockedPlan.DTYPES
        supports = staticmethod(ops.BlockedPlan.supports)
        supports_att = staticmethod(ops.BlockedPlan.supports_att)
        auto_blocks = staticmethod(lambda graph, F, elem=4: 1)

    def blocked_plan(self, blocks=32, item_edges=None, row_edges=None):
        return types.SimpleNamespace(sorted=fake_ops.blocked_ready(self, blocks), blocks=blocks)

    with patched(fake_ops, reduce=reduce, reduce_blocked=reduce_blocked, aggregate_blocked=aggregate_blocked,
                 pitched=pitched, BlockedPlan=Plan), patched(G.Graph, blocked_plan=blocked_plan):
        yield


def record(og, stream, g, tensors, sem, setup=None, **kw):
    """One executor run through a Recorder -> {"calls": [...], "summary": ..., "matchers": {...}}."""
    rec = Recorder(fake_ops, g, tensors)
    with patched(executor, ops=rec):
        ex = executor.Executor(og, stream, g, tensors, sem, plan_chunk=0, **kw)
        for name, value in (setup or {}).items():
            assert hasattr(ex, name), name
            setattr(ex, name, value)
        ex.run()
        for i in range(len(og)):  # every op's value, fused-away ones included (recomputed on demand)
            ex.tensor_of(i)
    return {"calls": rec.calls,
            "summary": f"alg_bytes={ex.alg_bytes} launches={ex.launches} gather_casts={ex.gather_casts}",
            "matchers": {m: canon(getattr(ex, m)) for m in MATCHERS}}


def _cora():
    z = np.load(os.path.join(GOLDEN, "cora_graph.npz"))
    return G.from_numpy(z["indptr"], z["indices"])


def _stream_run(g, idx, rec, setup=None):
    sem = Semantics.for_network(rec["network"], rec["reorder"])
    og = ir.OpGraph.load(os.path.join(GOLDEN, "ops", rec["op_yaml"]), sem.inputs)
    st = ir.Stream.load(os.path.join(GOLDEN, "streams", rec["file"]))
    return record(og, st, g, workloads.make_tensors(og, g, rec["network"], seed=idx), sem, setup)


N, E, FEATURE, BLOCKS = 60, 400, 128, 5
GATE = {"blocked_min_table_bytes": 0, "blocked_blocks": BLOCKS}


def _pool(agg, order, setup=None, **kw):
    recs = pool_layer.records(N, E, FEATURE, agg)
    recs[1]["ORDER"] = order
    op_array = [[0, 1]] + [[i] for i in range(2, len(recs))]
    stream = ir.Stream(lowering.lower(recs, N, op_array, [[64, 1]] * len(op_array)))
    og, g = ir.OpGraph(recs), G.synthetic(N, E)
    return record(og, stream, g, workloads.make_tensors(og, g, "GraphSAGE", seed=3), Semantics(), setup, **kw)


def _pair(comp, scatter_order, order, setup=None, **kw):
    """scatter -> gather `comp`, nothing else: each operand kind of each direction on its own."""
    recs = copy.deepcopy(pool_layer.records(N, E, FEATURE, "MAX" if comp == "ADD" else comp)[:2])
    recs[0]["ORDER"], recs[0]["OUTPUT"]["output_list"] = scatter_order, [1]
    recs[1].update(ORDER=order, COMP_TYPE=comp)
    recs[1]["OUTPUT"]["output_list"] = []
    stream = ir.Stream(lowering.lower(recs, N, [[0, 1]], [[64, 1]]))
    x = torch.randn(N, FEATURE, generator=torch.Generator().manual_seed(5))
    return record(ir.OpGraph(recs), stream, G.synthetic(N, E), {"x": x}, Semantics(), setup, **kw)


def _gcn(setup=None, **kw):
    g = G.synthetic(N, E)
    with patched(tiles, ops=fake_ops):
        lay = pipeline.Layer("GCN", 2, g, FEATURE)
    return record(lay.opgraph, lay.stream, g, workloads.make_tensors(lay.opgraph, g, "GCN", seed=3), lay.sem, setup, **kw)


def runs():
    """-> [(name, thunk)]: every run of the fixture, in file order.  A switch run is named
    `<stream>/<switch>=off`; it is recorded on the first cora stream of every (network, reorder)."""
    out = []
    g = _cora()
    streams = [s for s in load_manifest()["streams"] if "file" in s and s["dataset"] == "cora"]
    first = set()
    for idx, rec in enumerate(streams):
        name = rec["file"][:-5]
        out.append((name, lambda idx=idx, rec=rec: _stream_run(g, idx, rec)))
        if (rec["network"], rec["reorder"]) in first:
            continue
        first.add((rec["network"], rec["reorder"]))
        for sw in SWITCHES:
            setup = {sw: False}
            if sw == "fuse_attention":
                setup["attention_blocks"] = 2
                out.append((f"{name}/attention_blocks=2", lambda idx=idx, rec=rec: _stream_run(g, idx, rec, {"attention_blocks": 2})))
            out.append((f"{name}/{sw}=off", lambda idx=idx, rec=rec, setup=setup: _stream_run(g, idx, rec, setup)))

    def gated(fn, *a, setup=GATE, **kw):
        def thunk():
            with blocked_stand_ins():
                return fn(*a, setup=setup, **kw)
        return thunk
    for agg in executor.REDUCERS:  # the default gate: these small tables stay row-chunked
        for order in "RC":
            out.append((f"pool-{agg}-{order}", gated(_pool, agg, order, setup=None)))
    for dt, tag in ((None, "f32"), (torch.bfloat16, "bf16")):
        for agg in executor.REDUCERS:
            for order in "RC":
                out.append((f"blocked-{tag}/pool-{agg}-{order}", gated(_pool, agg, order, gather_dtype=dt)))
            for so in "RC":
                for order in "RC":
                    out.append((f"blocked-{tag}/scatter{so}-{agg}-{order}", gated(_pair, agg, so, order, gather_dtype=dt)))
        for so in "RC":
            for order in "RC":
                out.append((f"blocked-{tag}/scatter{so}-ADD-{order}", gated(_pair, "ADD", so, order, gather_dtype=dt)))
        out.append((f"blocked-{tag}/GCN", gated(_gcn, gather_dtype=dt)))
    return out


def record_all(progress=None):
    """The fixture's content.  Distinct call signatures are stored once ("calls") and a run lists their
    indices; matcher attributes once per distinct value set ("graphs"); a switch run whose record
    equals its stream's default run as "=<that run>".  `resolve` undoes all three."""
    doc = {"calls": [], "graphs": [], "runs": {}}
    index = {}
    for name, thunk in runs():
        r = thunk()
        if r["matchers"] not in doc["graphs"]:
            doc["graphs"].append(r["matchers"])
        r["matchers"] = doc["graphs"].index(r["matchers"])
        for c in r["calls"]:
            if c not in index:
                index[c] = len(doc["calls"])
                doc["calls"].append(c)
        r["calls"] = [index[c] for c in r["calls"]]
        base = name.split("/")[0]
        doc["runs"][name] = f"={base}" if "/" in name and doc["runs"].get(base) == r else r
        if progress:
            progress(name)
    return doc


def resolve(doc, name):
    """Run `name` of a fixture document as `record` returns it."""
    r = doc["runs"][name]
    if isinstance(r, str):
        r = doc["runs"][r[1:]]
    return {"calls": [doc["calls"][k] for k in r["calls"]], "summary": r["summary"], "matchers": doc["graphs"][r["matchers"]]}
