"""The moment reducers VAR / STD and the multi-reducer launch without a GPU: gta_reduce_multi's
argument checks through ctypes, the front end's new names and PNA's tuple aggregator, lowering of
the expanded graph, the sibling-gather matcher, the executor's routing (tests/fake_ops.py plus numpy
stand-ins attached here, against tests/moments_ref.py), the CLI's parsing, the distributed refusal,
and the fp32 emulation that shows the cancellation test of tests/test_gpu_moments.py tells the
shifted form from the naive one."""
import ctypes
import types

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import (_build, _lib, cli, executor, frontend, graph as G, ir,
                                                              lowering, ops, pipeline, rewrites, tiles, workloads)
from gta_graph_tensor_acclelrator_for_general_gnn_amd.semantics import Semantics
from oracle import opgraph_ref

from . import fake_ops, moments_ref, reduce_ref

N, E, FEATURE = 200, 1500, 96
PNA4 = ("MEAN", "MAX", "MIN", "STD")


# ------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    if _build.needs_build():
        _build.build(verbose=False)
    return _lib.load()


def test_header_declares_and_library_exports_reduce_multi(lib):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(_build.HDR), "gta.h")).read()
    decl = re.search(r"int gta_reduce_multi\(([^;]*)\);", hdr)
    assert decl, "include/gta.h does not declare gta_reduce_multi"
    assert len(lib.gta_reduce_multi.argtypes) == len(decl.group(1).split(",")) == 17
    for name, bit in (("MEAN", 1), ("MAX", 2), ("MIN", 4), ("VAR", 8), ("STD", 16)):
        assert re.search(rf"GTA_MR_{name} = {bit}\b", hdr) and getattr(_lib, f"MR_{name}") == bit
    assert "gta_reduce_multi" in _lib.SIGNATURES and "reduce_multi" in ops.reduce_multi.__doc__


def test_gta_reduce_multi_argument_checks_need_no_device(lib):
    """Every refusal comes before any device work: the pointers are NULL or host memory."""
    assert lib.gta_abi_version() == 15 == _lib.ABI_VERSION
    old = (None, None, 10, 10, _lib.IDX_SRC, None, 4, 4, _lib.GTA_F32, None, 4, None, 0, None, None)
    assert lib.gta_reduce(3, *old) == _lib.ERR_ARG  # the single reducer's enum did not grow

    host = (ctypes.c_float * 64)()
    ys1 = (ctypes.c_void_p * 5)(*([ctypes.addressof(host)] * 5))
    ld1 = (ctypes.c_int64 * 5)(*([4] * 5))

    def call(which=_lib.MR_MEAN | _lib.MR_STD, x_mode=_lib.IDX_SRC, x_dtype=_lib.GTA_F32, ys=ys1, ldys=ld1, n_rows=10):
        return lib.gta_reduce_multi(which, None, None, n_rows, 10, x_mode, None, 4, 4, x_dtype, ys, ldys, 1e-5, None, 0,
                                    None, None)

    for which in (0, 32, 64 | _lib.MR_MAX, -1):
        assert call(which=which) == _lib.ERR_ARG and b"reduce_multi" in lib.gta_last_error(), which
    assert call(x_mode=7) == _lib.ERR_ARG and b"x_mode" in lib.gta_last_error()
    assert call(x_dtype=5) == _lib.ERR_ARG and b"x_dtype" in lib.gta_last_error()
    assert call(x_mode=_lib.IDX_EDGE, x_dtype=_lib.GTA_BF16) == _lib.ERR_UNSUPPORTED and b"bf16" in lib.gta_last_error()
    assert call(ys=None) == _lib.ERR_ARG and b"reduce_multi" in lib.gta_last_error()
    assert call(ldys=None) == _lib.ERR_ARG
    null2 = (ctypes.c_void_p * 2)(ctypes.addressof(host), None)  # the second requested output is NULL
    assert call(ys=null2) == _lib.ERR_ARG and b"output" in lib.gta_last_error()
    short = (ctypes.c_int64 * 2)(4, 3)  # row stride < F
    assert call(ldys=short) == _lib.ERR_ARG
    assert call() == _lib.ERR_ARG  # indptr / x NULL: after the outputs were accepted, still before any launch
    assert call(n_rows=0) == _lib.OK  # nothing to do


def test_ops_reduce_multi_refusals():
    g = G.synthetic(20, 60, seed=0)
    x = torch.zeros(20, 4)
    with pytest.raises(_lib.GTAError):
        ops.reduce_multi(g, x, ("MEAN", "STD"))  # CPU tensors: no CPU path
    for reds in ((), ("MEAN", "MEAN"), ("SUM",), ("ADD", "MAX"), ("MAX", "max")):
        with pytest.raises(ValueError, match="reds"):
            ops.reduce_multi(g, x, reds)
    with pytest.raises(ValueError, match="x_mode"):
        ops.reduce_multi(g, x, ("MAX",), x_mode="col")
    assert ops.reduce_multi_planes(("MAX",)) == 2 and ops.reduce_multi_planes(("VAR",)) == 2
    assert ops.reduce_multi_planes(ops.MULTI_REDS) == 4 and ops.reduce_multi_planes(("MIN", "MEAN")) == 4


# ------------------------------------------------------------------------------------ front end
def test_aggregators_gain_var_and_std():
    assert frontend.AGGREGATORS == ("ADD", "MAX", "MIN", "MEAN", "VAR", "STD")
    assert lowering.UNIT_OF["VAR"] == lowering.UNIT_OF["STD"] == "VEC_ALU"
    for network in frontend.NETWORKS:
        for reorder in (False, True):
            base = frontend.gen_ops(network, 2, 2708, 10556, 1433, reorder)
            assert frontend.dumps(frontend.gen_ops(network, 2, 2708, 10556, 1433, reorder, aggregator="ADD")) \
                == frontend.dumps(base)  # the default output is byte-identical
            for agg in ("VAR", "STD"):
                if network == "GAT":
                    with pytest.raises(ValueError, match="GAT"):
                        frontend.gen_ops(network, 2, 2708, 10556, 1433, reorder, aggregator=agg)
                    continue
                recs = frontend.gen_ops(network, 2, 2708, 10556, 1433, reorder, aggregator=agg)
                assert len(recs) == len(base)
                for r, b in zip(recs, base):
                    if b["TYPE"] == "gather":
                        assert b["COMP_TYPE"] == "ADD" and r["COMP_TYPE"] == agg
                        assert {k: v for k, v in r.items() if k != "COMP_TYPE"} == \
                            {k: v for k, v in b.items() if k != "COMP_TYPE"}
                    else:
                        assert r == b
    with pytest.raises(ValueError, match="aggregator"):
        frontend.gen_ops("PNA", 1, 10, 20, 8, aggregator="SUM")


def test_tuple_aggregator_is_pna_only_and_checked():
    for network in frontend.NETWORKS:
        if network != "PNA":
            with pytest.raises(ValueError, match="PNA"):
                frontend.gen_ops(network, 2, 100, 500, 32, aggregator=PNA4)
    for bad in (("MEAN",), ("MEAN", "MEAN"), ("MEAN", "ADD"), ("MAX", "SUM"), ()):
        with pytest.raises(ValueError, match="tuple aggregator"):
            frontend.gen_ops("PNA", 2, 100, 500, 32, aggregator=bad)
    assert frontend.gen_ops("PNA", 2, 100, 500, 32, aggregator=list(PNA4)) == \
        frontend.gen_ops("PNA", 2, 100, 500, 32, aggregator=PNA4)


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("aggs", [PNA4, ("MAX", "VAR"), ("MEAN", "MAX", "MIN", "VAR", "STD")])
def test_tuple_aggregator_expands_the_gather_and_its_tail(aggs, reorder):
    n, e, K = 300, 2000, len(aggs)
    base = frontend.gen_ops("PNA", 2, n, e, 50, reorder)
    recs = frontend.gen_ops("PNA", 2, n, e, 50, reorder, aggregator=aggs)
    assert len(recs) == 8 + 3 * K + (K - 1) and [r["OP_NO"] for r in recs] == list(range(len(recs)))
    assert recs[:7] == base[:7]
    G0, M0, W0, A0 = 8, 8 + K, 8 + 2 * K, 8 + 3 * K
    assert recs[7]["OUTPUT"]["output_list"] == list(range(G0, G0 + K))
    assert {k: v for k, v in recs[7].items() if k != "OUTPUT"} == {k: v for k, v in base[7].items() if k != "OUTPUT"}
    for j, agg in enumerate(aggs):
        g, m, w = recs[G0 + j], recs[M0 + j], recs[W0 + j]
        assert (g["TYPE"], g["COMP_TYPE"], g["ORDER"]) == ("gather", agg, base[8]["ORDER"])
        assert g["INPUT"] == base[8]["INPUT"] and g["OUTPUT"]["output_list"] == [M0 + j]
        assert (m["TYPE"], m["COMP_TYPE"]) == ("applynode", "MUL") and m["INPUT"]["input_g_list"] == [G0 + j]
        assert m["OUTPUT"]["output_list"] == [W0 + j]
        assert (w["TYPE"], w["COMP_TYPE"]) == ("applynode", "MM") and w["INPUT"]["input_g_list"] == [M0 + j]
        assert w["INPUT"]["input_size"] == base[10]["INPUT"]["input_size"]
        for new, old in ((g, base[8]), (m, base[9]), (w, base[10])):  # the sizes are the original's
            assert new["OUTPUT"]["size_per_feature"] == old["OUTPUT"]["size_per_feature"]
            assert new["OUTPUT"]["output_number"] == old["OUTPUT"]["output_number"]
            assert new["INPUT"]["size_per_feature"] == old["INPUT"]["size_per_feature"]
    adds = recs[A0:]
    assert all((a["TYPE"], a["COMP_TYPE"], a["INPUT"]["input_g_num"]) == ("applynode", "ADD", 2) for a in adds)
    assert adds[-1]["OUTPUT"]["output_list"] == [] and [r["OP_NO"] for r in recs if not r["OUTPUT"]["output_list"]] == [A0 + K - 2]
    # the records are one consistent graph: every edge is listed at both of its ends, and the
    # oracle's reader orders it
    for i, r in enumerate(recs[7:], 7):
        for o in r["OUTPUT"]["output_list"]:
            assert i in recs[o]["INPUT"]["input_g_list"], (i, o)
        if i > 7:
            for p in r["INPUT"]["input_g_list"]:
                assert i in recs[p]["OUTPUT"]["output_list"], (p, i)
    order = opgraph_ref.topo(recs, None)
    assert sorted(order) == list(range(len(recs)))
    flow = opgraph_ref.dataflow(recs, None)
    assert [flow[G0 + j][0] for j in range(K)] == [("op", 7)] * K
    assert frontend.pna_clones(K) == {**{G0 + j: 8 for j in range(K)}, **{M0 + j: 9 for j in range(K)},
                                      **{W0 + j: 10 for j in range(K)}}
    # the clones resolve as their originals: PNA's SF (op 7) stays, nothing past it has an entry
    sem = Semantics.for_network("PNA", reorder, clones=frontend.pna_clones(K))
    plain = Semantics.for_network("PNA", reorder)
    assert sem.sf == plain.sf and sem.bin == plain.bin and sem.inputs == plain.inputs
    moved = Semantics.for_network("GAT", False, clones={20: 9, 21: 13})  # a table with entries to move
    assert moved.bin == {9: "DIV", 20: "DIV"} and moved.sf == {7: "EXP_LEAKY_RELU", 13: "ELU", 21: "ELU"}


@pytest.mark.parametrize("reorder", [False, True])
def test_expanded_graph_lowers(reorder):
    n, e = 300, 2000
    recs = frontend.gen_ops("PNA", 2, n, e, 50, reorder, aggregator=PNA4)
    og = ir.OpGraph(recs, None)
    blocks = [[i] for i in range(len(recs))]
    stream = lowering.lower(recs, n, blocks, [[64, 1] for _ in blocks])
    insts = [i for b in stream for i in b]
    for agg in PNA4:
        hit = [i for i in insts if f"COMP_{agg}" in i["TYPE"]]
        assert hit and all(i["Hardware_Unit"] == "VEC_ALU" for i in hit), agg
    assert len(ir.Stream(stream).blocks) == len(blocks) and len(og) == len(recs)


# ------------------------------------------------------------------------------ sibling matcher
def _gather(no, comp, src, order="R", outs=()):
    return {"OP_NO": no, "COMP_TYPE": comp, "TYPE": "gather", "ORDER": order,
            "INPUT": {"input_g_list": [src], "input_g_num": 1, "input_nong_num": 0, "input_nong_list": [],
                      "input_size": [], "feature_number": [40], "size_per_feature": [64]},
            "OUTPUT": {"output_list": list(outs), "output_number": 10, "size_per_feature": 64}}


def _edge_graph(gathers):
    """scatter C (op 0) -> applyedge SF (op 1) -> the given gathers (ops 2 ..)."""
    base = frontend.gen_ops("PNA", 3, 10, 40, 16)
    sc = dict(base[0], OUTPUT=dict(base[0]["OUTPUT"], output_list=[1]))
    sf = dict(base[7], OP_NO=1, INPUT=dict(base[7]["INPUT"], input_g_list=[0]),
              OUTPUT=dict(base[7]["OUTPUT"], output_list=[2 + j for j in range(len(gathers))]))
    return ir.OpGraph([sc, sf] + [_gather(2 + j, comp, src, order) for j, (comp, src, order) in enumerate(gathers)], None)


def test_sibling_gathers_matcher():
    sib = rewrites.sibling_gathers
    assert sib(_edge_graph([("MEAN", 1, "R"), ("MAX", 1, "R"), ("STD", 1, "R")])) == [(2, 3, 4)]
    assert sib(_edge_graph([("MIN", 1, "C"), ("VAR", 1, "C")])) == [(2, 3)]
    assert sib(_edge_graph([("MAX", 1, "R")])) == []                                  # one gather is no group
    assert sib(_edge_graph([("MAX", 1, "R"), ("MIN", 1, "C")])) == []                 # two ORDERs
    assert sib(_edge_graph([("MAX", 1, "R"), ("ADD", 1, "R")])) == []                 # the sum has its own fusions
    assert sib(_edge_graph([("MAX", 1, "R"), ("MIN", 1, "R"), ("ADD", 1, "R")])) == []
    assert sib(_edge_graph([("MAX", 1, "R"), ("MAX", 1, "R")])) == []                 # one launch, distinct outputs
    assert sib(_edge_graph([("MAX", 1, "R"), ("MIN", 0, "R")])) == []                 # two producers
    assert sib(_edge_graph([("MAX", 1, "R"), ("MIN", 1, "R"), ("MEAN", 1, "C"), ("STD", 1, "C")])) == [(4, 5), (2, 3)] \
        or sib(_edge_graph([("MAX", 1, "R"), ("MIN", 1, "R"), ("MEAN", 1, "C"), ("STD", 1, "C")])) == [(2, 3), (4, 5)]
    for network in frontend.NETWORKS:  # no op graph that exists today has sibling gathers
        for reorder in (False, True):
            for agg in ("ADD", "MAX", "STD"):
                if network == "GAT" and agg != "ADD":
                    continue
                recs = frontend.gen_ops(network, 2, 100, 500, 32, reorder, aggregator=agg)
                sem = Semantics.for_network(network, reorder)
                assert sib(ir.OpGraph(recs, sem.inputs)) == []
    og = ir.OpGraph(frontend.gen_ops("PNA", 2, 100, 500, 32, aggregator=PNA4), None)
    assert sib(og) == [(8, 9, 10, 11)]


# ------------------------------------------------------------------------------- executor routing
@pytest.fixture
def stand_ins(monkeypatch):
    """fake_ops over the executor's and the tile counter's ops, with numpy `reduce` and
    `reduce_multi` attached; every gather-shaped call is logged."""
    calls = []

    def reduce(graph, x, red="MAX", x_mode="src", out=None, plan=None):
        calls.append(("reduce", (red,), x_mode))
        ip, ix = graph.numpy()
        y = reduce_ref.reduce_csr(ip, ix, x.detach().cpu().float().numpy(), red, x_mode)
        return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))

    def reduce_multi(graph, x, reds, x_mode="src", outs=None, out=None, plan=None, std_eps=1e-5):
        calls.append(("reduce_multi", tuple(reds), x_mode))
        ip, ix = graph.numpy()
        xn = x.detach().cpu().double().numpy()
        mom = moments_ref.moments_csr(ip, ix, xn, x_mode, std_eps)
        res = []
        for r in reds:
            y = mom[r][0] if r in mom else reduce_ref.reduce_csr(ip, ix, xn, r, x_mode)
            res.append(torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)))
        return tuple(res)

    real_aggregate = fake_ops.aggregate

    def aggregate(graph, x, x_mode="src", w=None, row_scale=None, *a, **kw):
        if row_scale is not None and w is None:
            calls.append(("aggregate", ("MEAN",), x_mode))
        return real_aggregate(graph, x, x_mode, w, row_scale, *a, **kw)

    monkeypatch.setattr(fake_ops, "reduce", reduce, raising=False)
    monkeypatch.setattr(fake_ops, "reduce_multi", reduce_multi, raising=False)
    monkeypatch.setattr(fake_ops, "aggregate", aggregate)
    for mod in (executor, tiles):
        monkeypatch.setattr(mod, "ops", fake_ops)
    return calls


def _layer(network, g, agg, reorder=False):
    for k in range(16):  # the first candidate partition that lowers (as cli.run steps over the others)
        try:
            return pipeline.Layer(network, 2, g, FEATURE, reorder=reorder, aggregator=agg, candidate=k)
        except TypeError:
            continue
    raise AssertionError(f"no candidate of {network} lowers")


def _check(lay, ex, tensors, g):
    ip, ix = g.numpy()
    ref = moments_ref.layer_ref(lay.records, lay.sem, ip, ix, {k: v.double().numpy() for k, v in tensors.items()},
                                lay.sem.inputs)
    for i in range(len(lay.opgraph)):
        got = ex.tensor_of(i).detach().cpu().double().numpy()
        _, exp, ab = ref[i]
        assert got.shape == exp.shape, (i, got.shape, exp.shape)
        err, bound = np.abs(got - exp), 1e-5 * ab + 1e-6
        assert np.all(err <= bound), f"op {i}: max err {err.max():.3e}, excess {(err - bound).max():.3e}"
    return ref


@pytest.mark.parametrize("network,agg,reorder", [("GraphSAGE", "STD", False), ("PNA", "VAR", False),
                                                 ("PNA", "STD", True), ("GIN", "VAR", False)])
def test_executor_routes_a_single_moment_gather(stand_ins, network, agg, reorder):
    g = G.synthetic(N, E)
    lay = _layer(network, g, agg, reorder)
    tensors = workloads.make_tensors(lay.opgraph, g, network, seed=3)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0)
    ex.run()
    assert [c[:2] for c in stand_ins if c[0] != "aggregate"] == [("reduce_multi", (agg,))]
    assert not ex.siblings and executor.REDUCERS == ("MAX", "MIN", "MEAN") and executor.MOMENTS == ("VAR", "STD")
    ref = _check(lay, ex, tensors, g)
    # the reference's value is numpy's own population variance of each row's messages
    gather = next(op.idx for op in lay.opgraph.ops if op.type == "gather")
    ip = g.numpy()[0]
    xe = ref[lay.opgraph.inputs[gather][0].op][1]
    xe = np.broadcast_to(xe, (g.nnz, xe.shape[1]))
    var = np.stack([xe[ip[i]:ip[i + 1]].var(0) if ip[i + 1] > ip[i] else np.zeros(xe.shape[1]) for i in range(g.n_rows)])
    want = var if agg == "VAR" else np.where((np.diff(ip) > 0)[:, None], np.sqrt(var + 1e-5), 0)
    assert np.allclose(ref[gather][1], want, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("reorder", [False, True])
def test_executor_fills_sibling_gathers_with_one_launch(stand_ins, reorder):
    g = G.synthetic(N, E)
    lay = pipeline.Layer("PNA", 2, g, FEATURE, reorder=reorder, aggregator=PNA4)
    assert lay.candidates == [] and "search" in pipeline.Layer.__init__.__doc__  # no fusion search for a tuple
    tensors = workloads.make_tensors(lay.opgraph, g, "PNA", seed=5)
    for j in range(4):  # PNA's scalers: one per aggregator, addressed per op index
        tensors[f"ext:{12 + j}:1"] = torch.full((1, 1), 0.5 + 0.25 * j)
    assert {f"w:{16 + j}" for j in range(4)} <= set(tensors)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0)
    assert ex.multi_reduce and ex.siblings == {i: (8, 9, 10, 11) for i in (8, 9, 10, 11)}
    ex.trace = True
    ex.run()
    gathers = [c for c in stand_ins if c[0] in ("reduce", "reduce_multi", "aggregate")]
    assert gathers == [("reduce_multi", PNA4, "edge")], gathers
    by_op = {e["args"]["op"]: e["args"] for e in ex.trace_events}
    assert [by_op[i]["launches"] for i in (8, 9, 10, 11)] == [1, 0, 0, 0]
    n, F = g.n_rows, 64
    assert by_op[8]["alg_bytes"] == g.nnz * 4 * F + n * (8 + 4 * F) + 3 * n * 4 * F  # one read, four outputs
    _check(lay, ex, tensors, g)
    one = {i: ex.tensor_of(i).clone() for i in range(len(lay.opgraph))}

    del stand_ins[:]
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0, multi_reduce=False)
    ex.run()
    gathers = [c[:2] for c in stand_ins if c[0] in ("reduce", "reduce_multi", "aggregate")]
    assert gathers == [("aggregate", ("MEAN",)), ("reduce", ("MAX",)), ("reduce", ("MIN",)), ("reduce_multi", ("STD",))]
    _check(lay, ex, tensors, g)
    for i in (9, 10):
        assert torch.equal(ex.tensor_of(i), one[i])


def test_a_blocked_pair_stays_blocked_and_a_triple_takes_the_one_pass(stand_ins, monkeypatch):
    """Where every member of a group would pass the column-blocked gate on its own, the one
    row-chunked launch runs only from MULTI_MIN_BLOCKED members."""
    assert executor.MULTI_MIN_BLOCKED == 3
    g = G.synthetic(N, E)
    lay = pipeline.Layer("PNA", 2, g, FEATURE, aggregator=("MAX", "MIN"))
    ex = executor.Executor(lay.opgraph, lay.stream, g, {}, lay.sem, plan_chunk=0)
    t = torch.zeros(N, 64)
    scat = executor.Scat(t, "src")
    monkeypatch.setattr(ex, "_blocked_blocks", lambda *a, **k: 4)
    assert ex._would_block("MAX", scat, t, g, False) and not ex._would_block("STD", scat, t, g, False)
    assert not ex._would_block("MEAN", scat, t, g, False)  # MEAN goes blocked under gather_dtype bf16 only
    assert not ex._would_block("MAX", executor.EdgeT(t), t, g, False)
    assert not ex._multi_wanted((8, 9), scat, t, g, False)       # MAX, MIN: both blocked -> two blocked passes
    assert ex._multi_wanted((8, 9), executor.EdgeT(t), t, g, False)  # an edge tensor is never blocked
    assert ex._multi_wanted((8, 9, 10), scat, t, g, False)
    monkeypatch.setattr(ex, "_blocked_blocks", lambda *a, **k: 0)
    assert ex._multi_wanted((8, 9), scat, t, g, False)


# ----------------------------------------------------------------------------------- distributed
@pytest.mark.parametrize("agg", ["VAR", "STD", PNA4])
def test_partial_row_shards_refuse_the_moments(stand_ins, agg):
    g = G.synthetic(N, E)
    net = "PNA" if isinstance(agg, tuple) else "GraphSAGE"
    lay = pipeline.Layer(net, 2, g, FEATURE, aggregator=agg)
    tensors = workloads.make_tensors(lay.opgraph, g, net, seed=1)
    dist = types.SimpleNamespace(local_rows=False, n_local=g.n_rows, s=types.SimpleNamespace(world=2), src_fill=None,
                                 gather_rows=lambda x: x, reduce_rows=lambda y: y, reduce_cols=lambda y: y,
                                 replicated=lambda key: None)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0, dist=dist)
    gather = next(op for op in lay.opgraph.ops if op.type == "gather")
    with pytest.raises(NotImplementedError, match=rf"op {gather.idx}: gather {gather.comp}"):
        ex.run()


# ------------------------------------------------------------------------------------------- CLI
def test_cli_parses_the_new_names_and_a_comma_list(capsys):
    p = cli.parser()
    base = ["--dataset", "cora", "--network", "PNA"]
    assert p.parse_args(base).aggregator == "ADD"
    assert p.parse_args(base + ["--aggregator", "STD"]).aggregator == "STD"
    assert p.parse_args(base + ["--aggregator", "VAR"]).aggregator == "VAR"
    assert p.parse_args(base + ["--aggregator", "MEAN,MAX,MIN,STD"]).aggregator == PNA4
    for bad in ("SUM", "MEAN,SUM", "MAX,MAX", "ADD,MAX"):
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--aggregator", bad])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:  # a comma list is PNA's: a clear error before any device work
        cli.main(["--dataset", "cora", "--network", "GraphSAGE", "--aggregator", "MEAN,MAX"])
    assert e.value.code == 2 and "PNA" in capsys.readouterr().err


def test_cli_run_compiles_and_runs_a_tuple_aggregator(stand_ins):
    """cli.run on the stand-ins (traffic model only): no fusion search for the comma list, the
    default partition, one reduce_multi launch for the four gathers of the layer."""
    args = cli.parser().parse_args(["--dataset", "cora", "--network", "PNA", "--aggregator", "MEAN,MAX,MIN,STD",
                                    "--layers", "3", "--feature", "32", "--reps", "1", "--model-edges", "0"])
    out = cli.run(args, torch.device("cpu"), log=lambda *a: None)
    assert [c[:2] for c in stand_ins if c[0] in ("reduce", "reduce_multi")] == [("reduce_multi", PNA4)]
    assert len(out["layers"]) == 1 and out["layers"][0]["blocks"][0] == [7, 8] and out["model_rw"] > 0


# --------------------------------------------------------------------- the cancellation test (b)
def test_the_cancellation_data_tells_the_shifted_form_from_the_naive_one():
    """x = 1000 + N(0, 1) in fp32 on the GPU tests' graph: the shifted form, emulated in fp32 edge by
    edge, stays inside the bound at every element; the naive E[x^2] - E[x]^2 leaves it on most
    rows (its error is about 1e6 * 2^-24 * a few, against a bound of about 1e-5)."""
    from .test_gpu_moments import cancel_values, graph_np
    ip, ix = graph_np()
    xe = cancel_values(16)[1]
    ref = moments_ref.moments_csr(ip, ix, xe.astype(np.float64), "edge")
    deg = np.diff(ip)
    for shifted in (True, False):
        mean, var, std = moments_ref.emulate_f32(ip, xe, shifted=shifted)
        ok = {}
        for name, got in (("MEAN", mean), ("VAR", var), ("STD", std)):
            exp, bound = ref[name]
            ok[name] = np.abs(got.astype(np.float64) - exp) <= bound
        if shifted:
            assert all(o.all() for o in ok.values()), {k: int((~o).sum()) for k, o in ok.items()}
        else:
            rows = deg > 1  # (a single value has no variance to lose)
            bad_rows = (~ok["VAR"]).any(1)[rows].mean()
            assert bad_rows > 0.5 and (~ok["STD"]).any(1)[rows].mean() > 0.5, bad_rows
