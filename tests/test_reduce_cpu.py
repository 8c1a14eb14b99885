"""The gather reducers MAX / MIN / MEAN without a GPU: front end, lowering and model side, the
executor's routing (through tests/fake_ops.py plus a numpy `reduce` stand-in attached here, against
tests/reduce_ref.py), gta_reduce's argument checks through ctypes, and the distributed refusal."""
import types

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import (_build, _lib, executor, frontend, graph as G, pipeline,
                                                              tiles, workloads)

from . import fake_ops, reduce_ref

N, E, FEATURE = 200, 1500, 96


# ------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("network", frontend.NETWORKS)
def test_gen_ops_default_is_byte_identical_and_max_rewrites_only_the_gathers(network, reorder):
    for layer in (1, 2, 3):
        base = frontend.gen_ops(network, layer, 2708, 10556, 1433, reorder)
        assert frontend.dumps(frontend.gen_ops(network, layer, 2708, 10556, 1433, reorder, aggregator="ADD")) \
            == frontend.dumps(base)
        if network == "GAT":
            for agg in ("MAX", "MIN", "MEAN"):
                with pytest.raises(ValueError, match="GAT"):
                    frontend.gen_ops(network, layer, 2708, 10556, 1433, reorder, aggregator=agg)
            continue
        for agg in ("MAX", "MIN", "MEAN"):
            recs = frontend.gen_ops(network, layer, 2708, 10556, 1433, reorder, aggregator=agg)
            gathers = [i for i, r in enumerate(base) if r["TYPE"] == "gather"]
            assert len(gathers) == (2 if network == "SGC" else 1)
            assert len(recs) == len(base)
            for i, (r, b) in enumerate(zip(recs, base)):
                if i in gathers:
                    assert b["COMP_TYPE"] == "ADD" and r["COMP_TYPE"] == agg
                    assert {k: v for k, v in r.items() if k != "COMP_TYPE"} == {k: v for k, v in b.items()
                                                                                if k != "COMP_TYPE"}
                else:
                    assert r == b
    with pytest.raises(ValueError, match="aggregator"):
        frontend.gen_ops(network, 1, 10, 20, 8, reorder, aggregator="SUM")


def _small_graph():
    return G.synthetic(N, E)


@pytest.fixture
def stand_ins(monkeypatch):
    """fake_ops over the executor's and the tile counter's ops, with a numpy `reduce` attached."""
    calls = []

    def reduce(graph, x, red="MAX", x_mode="src", out=None, plan=None):
        assert red in ("MAX", "MIN") and out is None
        calls.append((red, x_mode, graph))
        ip, ix = graph.numpy()
        y = reduce_ref.reduce_csr(ip, ix, x.detach().cpu().float().numpy(), red, x_mode)
        return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))

    monkeypatch.setattr(fake_ops, "reduce", reduce, raising=False)
    for mod in (executor, tiles):
        monkeypatch.setattr(mod, "ops", fake_ops)
    return calls


@pytest.mark.parametrize("network", ["GraphSAGE", "GIN", "PNA"])
def test_max_layer_lowers_and_models(stand_ins, network):
    g = _small_graph()
    lay = pipeline.Layer(network, 2, g, FEATURE, aggregator="MAX")
    insts = [i for b in lay.stream_records for i in b]
    maxes = [i for i in insts if "COMP_MAX" in i["TYPE"]]
    assert maxes and all(i["Hardware_Unit"] == "VEC_ALU" for i in maxes)
    assert not any("COMP_ADD" in i["TYPE"] and "gather" in i["ID"] for i in insts)
    res = executor.ExecResult({}, {}, 0.0, 0, 0)
    executor.attach_model(res, lay.stream_records, lay.tile_size_list, g, model="inst")
    assert res.model_insts and np.isfinite(res.model_rw) and res.model_rw > 0
    assert all(np.isfinite(r["busy"]) and np.isfinite(r["rw_bytes"]) for r in res.model_insts)


# ------------------------------------------------------------------------------- executor routing
def _layer(network, layer, g, agg, reorder=False):
    """The first candidate partition that lowers (the reference's interpret() raises on some that
    its search ranks first, whatever the aggregator: cli.run steps over them the same way)."""
    for k in range(16):
        try:
            return pipeline.Layer(network, layer, g, FEATURE, reorder=reorder, aggregator=agg, candidate=k)
        except TypeError:
            continue
    raise AssertionError(f"no candidate of {network} lowers")


def _run(network, agg, reorder=False, layer=2, seed=3):
    g = _small_graph()
    lay = _layer(network, layer, g, agg, reorder)
    tensors = workloads.make_tensors(lay.opgraph, g, network, seed=seed)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0)
    outs = ex.run()
    ip, ix = g.numpy()
    ref = reduce_ref.layer_ref(lay.records, lay.sem, ip, ix, {k: v.double().numpy() for k, v in tensors.items()},
                               lay.sem.inputs)
    assert set(outs) == {op.idx for op in lay.opgraph.ops if not op.out_list}
    for i in range(len(lay.opgraph)):
        got = ex.tensor_of(i).detach().cpu().double().numpy()
        _, exp, ab = ref[i]
        assert got.shape == exp.shape, (i, got.shape, exp.shape)
        err = np.abs(got - exp)
        bound = 1e-5 * ab + 1e-6  # the project's bound (tests/test_gpu_ops.py); the max itself adds no error
        assert np.all(err <= bound), f"{network}-{agg} op {i}: max err {err.max():.3e}, excess {(err - bound).max():.3e}"
    return lay, ex


def _differs_from_sum(lay, ex):
    """The gathers' values are not the sums the parent commit computed for them."""
    g = ex.graph
    ip, ix = g.numpy()
    for op in lay.opgraph.ops:
        if op.type == "gather":
            src = lay.opgraph.inputs[op.idx][0].op
            xe = ex.tensor_of(src).double().numpy()
            summed = reduce_ref.segment(ix if op.order == "C" else reduce_ref.rows_of(ip), xe, g.n_rows, "ADD")
            assert not np.allclose(ex.tensor_of(op.idx).double().numpy(), summed, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("network,agg,reorder", [("GraphSAGE", "MAX", False), ("GIN", "MIN", False),
                                                 ("GraphSAGE", "MEAN", False), ("PNA", "MAX", True)])
def test_executor_routes_reducers(stand_ins, network, agg, reorder):
    self_terms = fake_ops.SELF_TERM_CALLS[0]
    lay, ex = _run(network, agg, reorder)
    assert [r["COMP_TYPE"] for r in lay.records if r["TYPE"] == "gather"] == [agg]
    # none of the rewrites that rely on a sum: MM-first, the GIN self-term accumulate, the expression gather
    assert not ex.reorder and not ex.gacc and not ex.expr and not ex.two_hop
    assert fake_ops.SELF_TERM_CALLS[0] == self_terms
    assert len(stand_ins) == (0 if agg == "MEAN" else 1)
    if agg != "MEAN":
        assert stand_ins[0][0] == agg
    _differs_from_sum(lay, ex)


def test_sgc_max_runs_both_hops_without_the_two_hop_rewrite(stand_ins):
    lay, ex = _run("SGC", "MAX")
    assert [r["COMP_TYPE"] for r in lay.records if r["TYPE"] == "gather"] == ["MAX", "MAX"]
    assert ex.two_hop == {} and ex.reorder == {}
    assert [c[0] for c in stand_ins] == ["MAX", "MAX"]
    _differs_from_sum(lay, ex)
    sum_lay = pipeline.Layer("SGC", 2, _small_graph(), FEATURE)  # the sum still takes the rewrite
    assert executor.Executor(sum_lay.opgraph, sum_lay.stream, None, {}, sum_lay.sem).two_hop


def test_dgn_max_materialises_the_tree(stand_ins):
    before = fake_ops.EXPR_CALLS[0]
    lay, ex = _run("DGN", "MAX")
    assert fake_ops.EXPR_CALLS[0] == before and ex.expr == {} and not ex.expr_nodes
    assert [(c[0], c[1]) for c in stand_ins] == [("MAX", "edge")]  # the applyedge tree as an [E, F] tensor
    sum_lay = pipeline.Layer("DGN", 2, _small_graph(), FEATURE)
    assert executor.Executor(sum_lay.opgraph, sum_lay.stream, None, {}, sum_lay.sem).expr


def test_virtual_scatter_is_reduced_by_index_in_both_directions(stand_ins):
    """scatter -> gather MAX: ORDER R reads the node table by index (no [E, F] tensor); ORDER C
    runs over the CSC view; a sum-only matcher never sees either."""
    g = _small_graph()
    ip, ix = g.numpy()
    x = torch.randn(N, 24, generator=torch.Generator().manual_seed(5))
    for order, mode_seen in (("R", "src"), ("C", "src")):
        recs = frontend.gen_ops("GCN", 2, N, E, 24, True)[1:]  # scatter C -> MUL -> gather, MM dropped
        recs = [dict(r, OP_NO=k) for k, r in enumerate(recs)]
        recs = [recs[0], dict(recs[2], COMP_TYPE="MAX", ORDER=order)]
        recs[0] = dict(recs[0], INPUT=dict(recs[0]["INPUT"], input_g_list=[]),
                       OUTPUT=dict(recs[0]["OUTPUT"], output_list=[1]))
        recs[1] = dict(recs[1], OP_NO=1, INPUT=dict(recs[1]["INPUT"], input_g_list=[0]))
        from gta_graph_tensor_acclelrator_for_general_gnn_amd import ir, lowering
        from gta_graph_tensor_acclelrator_for_general_gnn_amd.semantics import Semantics
        og = ir.OpGraph(recs)
        stream = ir.Stream(lowering.lower(recs, N, [[0, 1]], [[64, 1]]))
        del stand_ins[:]
        ex = executor.Executor(og, stream, g, {"x": x}, Semantics(), plan_chunk=0)
        y = ex.run()[1].numpy()
        xs = x.numpy()
        exp = reduce_ref.reduce_csr(ip, ix, xs, "MAX", "src") if order == "R" else \
            reduce_ref.reduce_csc(ip, ix, N, xs, "MAX", "src")
        assert np.array_equal(y, exp)
        assert len(stand_ins) == 1 and stand_ins[0][1] == mode_seen
        assert (stand_ins[0][2] is g) == (order == "R")


# ------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    if _build.needs_build():
        _build.build(verbose=False)
    return _lib.load()


def test_gta_reduce_argument_checks_need_no_device(lib):
    assert lib.gta_abi_version() == 15 == _lib.ABI_VERSION
    args = (None, None, 10, 10, _lib.IDX_SRC, None, 4, 4, _lib.GTA_F32, None, 4, None, 0, None, None)
    for red in (3, -1, 99):
        assert lib.gta_reduce(red, *args) == _lib.ERR_ARG
        assert b"reduce" in lib.gta_last_error()
    bad_mode = (None, None, 10, 10, 7, None, 4, 4, _lib.GTA_F32, None, 4, None, 0, None, None)
    assert lib.gta_reduce(_lib.RED_MAX, *bad_mode) == _lib.ERR_ARG and b"reduce" in lib.gta_last_error()
    bad_dtype = (None, None, 10, 10, _lib.IDX_SRC, None, 4, 4, 5, None, 4, None, 0, None, None)
    assert lib.gta_reduce(_lib.RED_MIN, *bad_dtype) == _lib.ERR_ARG and b"reduce" in lib.gta_last_error()
    bf_edge = (None, None, 10, 10, _lib.IDX_EDGE, None, 4, 4, _lib.GTA_BF16, None, 4, None, 0, None, None)
    assert lib.gta_reduce(_lib.RED_MAX, *bf_edge) == _lib.ERR_UNSUPPORTED and b"reduce" in lib.gta_last_error()
    assert lib.gta_reduce(_lib.RED_MAX, *args) == _lib.ERR_ARG and b"reduce" in lib.gta_last_error()  # NULL pointers
    assert lib.gta_reduce(_lib.RED_ADD, *args) < 0 and b"reduce" in lib.gta_last_error()  # forwarded to the sum


def test_ops_reduce_refuses_cpu_tensors_and_bad_names():
    from gta_graph_tensor_acclelrator_for_general_gnn_amd import ops
    g = G.synthetic(20, 60, seed=0)
    with pytest.raises(_lib.GTAError):
        ops.reduce(g, torch.zeros(20, 4), "MAX")


# ----------------------------------------------------------------------------------- distributed
@pytest.mark.parametrize("agg", ["MAX", "MIN", "MEAN"])
def test_partial_row_shards_refuse_the_reducers(stand_ins, agg):
    """A column shard's gathers are partial sums over its source columns, summed across ranks:
    partial maxima / means cannot be; the executor names the op instead of summing them."""
    g = _small_graph()
    lay = pipeline.Layer("GraphSAGE", 2, g, FEATURE, aggregator=agg)
    tensors = workloads.make_tensors(lay.opgraph, g, "GraphSAGE", seed=1)
    dist = types.SimpleNamespace(local_rows=False, n_local=g.n_rows, s=types.SimpleNamespace(world=2), src_fill=None,
                                 gather_rows=lambda x: x, reduce_rows=lambda y: y, reduce_cols=lambda y: y,
                                 replicated=lambda key: None)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0, dist=dist)
    gather = next(op.idx for op in lay.opgraph.ops if op.type == "gather")
    with pytest.raises(NotImplementedError, match=rf"op {gather}: gather {agg}"):
        ex.run()
    # whole rows on the rank (a row shard, or a world of one): unchanged
    dist.local_rows = True
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0, dist=dist)
    ex.run()
