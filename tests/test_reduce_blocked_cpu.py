"""Column-blocked MAX / MIN gather (gta_reduce_blocked) without a GPU: the ABI's declaration, export
and argument checks, ops.reduce_blocked's host-side refusals, and the executor's routing through
tests/fake_ops.py with numpy stand-ins for the blocked ops attached here.
"""
import os
import re
import types

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import (_build, _lib, executor, frontend, graph as G, ir, lowering,
                                                              ops, pipeline, tiles, workloads)
from gta_graph_tensor_acclelrator_for_general_gnn_amd.semantics import Semantics

from . import fake_ops, pool_layer, reduce_ref

N, E, FEATURE = 60, 400, 128
BLOCKS = 5


# ------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    if _build.needs_build():
        _build.build(verbose=False)
    return _lib.load()


def test_header_declares_and_library_exports_reduce_blocked(lib):
    with open(_build.HDR) as f:
        hdr = f.read()
    decl = re.search(r"int gta_reduce_blocked\(([^;]*)\);", hdr)
    assert decl, "include/gta.h does not declare gta_reduce_blocked"
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).replace("\n", " ").split(",")]
    assert names == ["red", "indptr", "indices", "n_rows", "n_cols", "nnz", "x", "ldx", "F", "x_dtype", "y", "ldy",
                     "plan", "blocks", "item_edges", "workspace", "stream"]
    assert "#define GTA_ABI_VERSION 15" in hdr and lib.gta_abi_version() == 15 == _lib.ABI_VERSION
    assert hasattr(lib, "gta_reduce_blocked")
    assert len(lib.gta_reduce_blocked.argtypes) == len(names)


def test_gta_reduce_blocked_argument_checks_need_no_device(lib):
    """Every argument error is found before any memory is touched: the pointers here are NULL or
    point nowhere, and there is no device."""
    junk = 0x1000  # never dereferenced

    def call(red=_lib.RED_MAX, indptr=junk, n_rows=10, x=junk, x_dtype=_lib.GTA_F32, y=junk, plan=junk, blocks=4,
             item_edges=256, ws=junk, nnz=10):
        return lib.gta_reduce_blocked(red, indptr, junk, n_rows, 10, nnz, x, 128, 128, x_dtype, y, 128, plan, blocks,
                                      item_edges, ws, None)

    for red in (3, -1, 99):
        assert call(red=red) == _lib.ERR_ARG and b"reduce_blocked" in lib.gta_last_error()
    for dt in (2, 5, -1):
        assert call(x_dtype=dt) == _lib.ERR_ARG and b"x_dtype" in lib.gta_last_error()
    for blocks in (0, 64, -3):
        assert call(blocks=blocks) == _lib.ERR_ARG and b"reduce_blocked" in lib.gta_last_error()
    assert call(item_edges=0) == _lib.ERR_ARG
    assert call(plan=None) == _lib.ERR_ARG and b"reduce_blocked" in lib.gta_last_error()
    assert call(indptr=None) == _lib.ERR_ARG
    assert call(y=None) == _lib.ERR_ARG
    assert call(x=None) == _lib.ERR_ARG and call(ws=None) == _lib.ERR_ARG  # needed when nnz > 0
    for red in (_lib.RED_ADD, _lib.RED_MAX, _lib.RED_MIN):
        assert call(red=red, n_rows=0, plan=None) == _lib.OK  # no rows: nothing to do
        assert call(red=red, plan=None) == _lib.ERR_ARG


def test_ops_reduce_blocked_refuses_cpu_tensors_and_bad_names():
    g = G.synthetic(20, 60, seed=0)
    with pytest.raises(_lib.GTAError, match="no CPU path"):
        ops.reduce_blocked(g, torch.zeros(20, 128), "MAX")
    fake = types.SimpleNamespace(indptr=types.SimpleNamespace(is_cuda=True))
    x = types.SimpleNamespace(is_cuda=True)
    with pytest.raises(ValueError, match="red must be one of"):
        ops.reduce_blocked(fake, x, "SUM")
    with pytest.raises(ValueError, match="red must be one of"):
        ops.reduce_blocked(fake, x, "MEAN")
    assert "reduce_blocked" in ops.__doc__ and "gta_reduce_blocked" in ops.__doc__


# ------------------------------------------------------------------------------- executor routing
@pytest.fixture
def stand_ins(monkeypatch):
    """fake_ops over the executor's ops, with numpy stand-ins for reduce, reduce_blocked and
    aggregate_blocked that record their calls, and a BlockedPlan whose shape rules are the real
    ones (the gate itself is then the executor's: size, auto_blocks, the sorted plan)."""
    calls = []

    def _red(graph, x, red, mode):
        ip, ix = graph.numpy()
        y = reduce_ref.reduce_csr(ip, ix, x.detach().cpu().float().numpy(), red, mode)
        return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))

    def reduce(graph, x, red="MAX", x_mode="src", out=None, plan=None):
        assert red in ("MAX", "MIN") and out is None
        calls.append(("reduce", red, x_mode, graph, x, None))
        return _red(graph, x, red, x_mode)

    def reduce_blocked(graph, x, red="MAX", out=None, plan=None, blocks=32):
        assert red in ("MAX", "MIN") and out is None and plan is None
        calls.append(("reduce_blocked", red, "src", graph, x, blocks))
        return _red(graph, x, red, "src")

    def aggregate_blocked(graph, x, w=None, row_scale=None, out=None, accumulate=False, plan=None, blocks=32):
        calls.append(("aggregate_blocked", "MEAN" if row_scale is not None else "ADD", "src", graph, x, blocks))
        return fake_ops.aggregate(graph, x.float(), "src", w, row_scale, out, accumulate)

    class Plan:
        DTYPES = ops.BlockedPlan.DTYPES
        supports = staticmethod(ops.BlockedPlan.supports)
        supports_att = staticmethod(ops.BlockedPlan.supports_att)
        auto_blocks = staticmethod(lambda graph, F, elem=4: 1)  # a small table: below the 4-block minimum

    monkeypatch.setattr(fake_ops, "reduce", reduce, raising=False)
    monkeypatch.setattr(fake_ops, "reduce_blocked", reduce_blocked, raising=False)
    monkeypatch.setattr(fake_ops, "aggregate_blocked", aggregate_blocked, raising=False)
    monkeypatch.setattr(fake_ops, "pitched", lambda t: t, raising=False)
    monkeypatch.setattr(fake_ops, "BlockedPlan", Plan)
    monkeypatch.setattr(G.Graph, "blocked_plan", lambda self, blocks=32, item_edges=None, row_edges=None:
                        types.SimpleNamespace(sorted=fake_ops.blocked_ready(self, blocks), blocks=blocks))
    for mod in (executor, tiles):
        monkeypatch.setattr(mod, "ops", fake_ops)
    return calls


def _layer(network, g, agg, reorder=False):
    for k in range(16):  # the first candidate partition that lowers
        try:
            return pipeline.Layer(network, 2, g, FEATURE, reorder=reorder, aggregator=agg, candidate=k)
        except TypeError:
            continue
    raise AssertionError(f"no candidate of {network} lowers")


def _executor(network, agg, reorder=False, gate=True, **kw):
    """network "pool": GraphSAGE's layer 2 without the edge-weight MUL (tests/pool_layer.py), the
    layer whose gather reads a virtual scatter; any other name: the stock layer."""
    g = G.synthetic(N, E)
    if network == "pool":
        recs, og, stream, sem = pool_layer.layer(N, E, FEATURE, agg)
        lay = types.SimpleNamespace(records=recs, opgraph=og, stream=stream, sem=sem)
    else:
        lay = _layer(network, g, agg, reorder)
    tensors = workloads.make_tensors(lay.opgraph, g, "GraphSAGE" if network == "pool" else network, seed=3)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0, **kw)
    if gate:
        ex.blocked_min_table_bytes, ex.blocked_blocks = 0, BLOCKS
    return lay, ex, tensors, g


def _gather_calls(calls):
    return [c for c in calls if c[0] in ("reduce", "reduce_blocked", "aggregate_blocked")]


def test_switch_defaults_on(stand_ins):
    lay = pipeline.Layer("GraphSAGE", 2, G.synthetic(N, E), FEATURE)
    assert executor.Executor(lay.opgraph, lay.stream, None, {}, lay.sem).reduce_blocked is True


@pytest.mark.parametrize("agg", ["MAX", "MIN"])
def test_max_gather_of_a_source_scatter_above_the_gate_goes_blocked(stand_ins, agg):
    lay, ex, tensors, g = _executor("pool", agg)
    ex.run()
    (name, red, mode, graph, x, blocks), = _gather_calls(stand_ins)
    assert (name, red, blocks) == ("reduce_blocked", agg, BLOCKS) and graph is g
    assert x is tensors["x"] and x.shape[1] == FEATURE  # the node table itself: no [E, F] tensor, no cast
    gather = next(op.idx for op in lay.opgraph.ops if op.type == "gather")
    ip, ix = g.numpy()
    assert np.array_equal(ex.tensor_of(gather).numpy(), reduce_ref.reduce_csr(ip, ix, x.numpy(), agg, "src"))
    assert ex.gather_casts == 0


def test_below_the_gate_or_switched_off_it_stays_row_chunked(stand_ins):
    # the default gate: a 30 KB table is far below blocked_min_table_bytes, and auto_blocks gives 1
    lay, ex, tensors, g = _executor("pool", "MAX", gate=False)
    ex.run()
    assert [c[:3] for c in _gather_calls(stand_ins)] == [("reduce", "MAX", "src")]
    # the size passes but auto_blocks stays below the 4-block minimum
    del stand_ins[:]
    lay, ex, tensors, g = _executor("pool", "MAX", gate=False)
    ex.blocked_min_table_bytes = 0
    ex.run()
    assert [c[:3] for c in _gather_calls(stand_ins)] == [("reduce", "MAX", "src")]
    # the switch
    del stand_ins[:]
    lay, ex, tensors, g = _executor("pool", "MAX")
    ex.reduce_blocked = False
    ex.run()
    assert [c[:3] for c in _gather_calls(stand_ins)] == [("reduce", "MAX", "src")]
    # blocked_blocks 0 = never
    del stand_ins[:]
    lay, ex, tensors, g = _executor("pool", "MAX")
    ex.blocked_blocks = 0
    ex.run()
    assert [c[:3] for c in _gather_calls(stand_ins)] == [("reduce", "MAX", "src")]


def test_an_unsupported_width_stays_row_chunked(stand_ins):
    g = G.synthetic(N, E)
    x = torch.randn(N, 24, generator=torch.Generator().manual_seed(5))
    og, stream = _scatter_gather(g, "R", 24)
    ex = executor.Executor(og, stream, g, {"x": x}, Semantics(), plan_chunk=0)
    ex.blocked_min_table_bytes, ex.blocked_blocks = 0, BLOCKS
    ex.run()
    assert [c[:3] for c in _gather_calls(stand_ins)] == [("reduce", "MAX", "src")]


def test_an_edge_tensor_operand_keeps_the_current_route(stand_ins):
    """PNA's gather reduces an applyedge tree: an [E, F] tensor in EDGE mode, never the blocked form.
    So does every stock layer: its gather reads the Deferred applyedge MUL by the edge weight."""
    lay, ex, tensors, g = _executor("PNA", "MAX", reorder=True)
    ex.run()
    got = _gather_calls(stand_ins)
    assert [c[0] for c in got] == ["reduce"] and got[0][2] == "edge"
    del stand_ins[:]
    lay, ex, tensors, g = _executor("GraphSAGE", "MAX", gather_dtype=torch.bfloat16)
    ex.run()
    got = _gather_calls(stand_ins)
    assert [c[0] for c in got] == ["reduce"] and got[0][2] == "edge" and ex.gather_casts == 0


def _scatter_gather(g, order, F, comp="MAX", scatter_order=None):
    """scatter -> gather `comp`: a two-op graph (GCN's records with the MUL and the MM dropped)."""
    recs = frontend.gen_ops("GCN", 2, N, E, F, True)[1:]
    recs = [dict(r, OP_NO=k) for k, r in enumerate(recs)]
    recs = [recs[0], dict(recs[2], COMP_TYPE=comp, ORDER=order)]
    recs[0] = dict(recs[0], INPUT=dict(recs[0]["INPUT"], input_g_list=[]), OUTPUT=dict(recs[0]["OUTPUT"], output_list=[1]))
    if scatter_order is not None:
        recs[0] = dict(recs[0], ORDER=scatter_order)
    recs[1] = dict(recs[1], OP_NO=1, INPUT=dict(recs[1]["INPUT"], input_g_list=[0]))
    return ir.OpGraph(recs), ir.Stream(lowering.lower(recs, N, [[0, 1]], [[64, 1]]))


def test_order_c_of_a_scatter_r_goes_blocked_over_the_transposed_view(stand_ins):
    g = G.synthetic(N, E)
    ip, ix = g.numpy()
    x = torch.randn(N, FEATURE, generator=torch.Generator().manual_seed(5))
    # scatter R (mode dst) reduced to the source nodes: the transposed aggregate's view
    og, stream = _scatter_gather(g, "C", FEATURE, scatter_order="R")
    ex = executor.Executor(og, stream, g, {"x": x}, Semantics(), plan_chunk=0)
    ex.blocked_min_table_bytes, ex.blocked_blocks = 0, BLOCKS
    y = ex.run()[1].numpy()
    (name, red, mode, graph, xt, blocks), = _gather_calls(stand_ins)
    assert name == "reduce_blocked" and blocks == BLOCKS and xt is x
    assert graph is fake_ops.csc(g).view("dst")
    assert np.array_equal(y, reduce_ref.reduce_csc(ip, ix, N, x.numpy(), "MAX", "dst"))
    # scatter C reduced to the source nodes gathers column j's own row: not a source gather, row-chunked
    del stand_ins[:]
    og, stream = _scatter_gather(g, "C", FEATURE)
    ex = executor.Executor(og, stream, g, {"x": x}, Semantics(), plan_chunk=0)
    ex.blocked_min_table_bytes, ex.blocked_blocks = 0, BLOCKS
    ex.run()
    assert [c[0] for c in _gather_calls(stand_ins)] == ["reduce"]
    # scatter R reduced to the destination (mode dst, ORDER R): row-chunked as today
    del stand_ins[:]
    og, stream = _scatter_gather(g, "R", FEATURE, scatter_order="R")
    ex = executor.Executor(og, stream, g, {"x": x}, Semantics(), plan_chunk=0)
    ex.blocked_min_table_bytes, ex.blocked_blocks = 0, BLOCKS
    ex.run()
    assert [c[:3] for c in _gather_calls(stand_ins)] == [("reduce", "MAX", "dst")]


def test_gather_dtype_bf16_casts_once_and_counts_two_byte_rows(stand_ins):
    lay, ex, tensors, g = _executor("pool", "MAX", gather_dtype=torch.bfloat16)
    ex.run()
    (name, red, mode, graph, x, blocks), = _gather_calls(stand_ins)
    assert name == "reduce_blocked" and x.dtype == torch.bfloat16 and ex.gather_casts == 1
    assert torch.equal(x, tensors["x"].to(torch.bfloat16))
    lay, ex0, _, _ = _executor("pool", "MAX")
    ex0.run()
    # 2 B fewer per gathered element, plus the cast pass (read 4 B, write 2 B per element)
    assert ex.alg_bytes == ex0.alg_bytes - g.nnz * FEATURE * 2 + g.n_rows * FEATURE * 6
    # the size gate sees 2-byte elements
    del stand_ins[:]
    lay, ex, tensors, g = _executor("pool", "MAX", gather_dtype=torch.bfloat16)
    ex.blocked_min_table_bytes = N * FEATURE * 2 + 1
    ex.run()
    assert [c[0] for c in _gather_calls(stand_ins)] == ["reduce"] and ex.gather_casts == 0
    del stand_ins[:]
    lay, ex, tensors, g = _executor("pool", "MAX", gather_dtype=torch.bfloat16)
    ex.blocked_min_table_bytes = N * FEATURE * 2
    ex.run()
    assert [c[0] for c in _gather_calls(stand_ins)] == ["reduce_blocked"]


def test_mean_goes_blocked_only_under_gather_dtype_bf16(stand_ins):
    lay, ex, tensors, g = _executor("pool", "MEAN")
    ex.run()
    assert _gather_calls(stand_ins) == []  # ops.aggregate with row_scale, as today
    lay, ex, tensors, g = _executor("pool", "MEAN", gather_dtype=torch.bfloat16)
    ex.run()
    (name, red, mode, graph, x, blocks), = _gather_calls(stand_ins)
    assert (name, red, blocks) == ("aggregate_blocked", "MEAN", BLOCKS) and x.dtype == torch.bfloat16
    assert ex.gather_casts == 1
    gather = next(op.idx for op in lay.opgraph.ops if op.type == "gather")
    ip, ix = g.numpy()
    ref = reduce_ref.reduce_csr(ip, ix, x.float().numpy().astype(np.float64), "MEAN", "src")
    assert np.allclose(ex.tensor_of(gather).numpy(), ref, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("agg", ["MAX", "MEAN"])
def test_the_shard_refusal_still_comes_first(stand_ins, agg):
    g = G.synthetic(N, E)
    lay = pipeline.Layer("GraphSAGE", 2, g, FEATURE, aggregator=agg)
    tensors = workloads.make_tensors(lay.opgraph, g, "GraphSAGE", seed=1)
    dist = types.SimpleNamespace(local_rows=False, n_local=g.n_rows, s=types.SimpleNamespace(world=2), src_fill=None,
                                 gather_rows=lambda x: x, reduce_rows=lambda y: y, reduce_cols=lambda y: y,
                                 replicated=lambda key: None)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0, dist=dist,
                           gather_dtype=torch.bfloat16)
    ex.blocked_min_table_bytes, ex.blocked_blocks = 0, BLOCKS
    gather = next(op.idx for op in lay.opgraph.ops if op.type == "gather")
    with pytest.raises(NotImplementedError, match=rf"op {gather}: gather {agg}"):
        ex.run()
    assert _gather_calls(stand_ins) == []
