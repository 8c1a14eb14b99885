"""e4m3 (GTA_FP8) gathered tables in the column-blocked aggregates: every code widens exactly, and an
fp8 call is bitwise the fp32 call on the widened table (gta.h)."""
import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, executor, graph as G, ops, pipeline, workloads
from oracle import isa_ref

from .test_gpu_blocked_bf16 import (_att_pair, _blocked_plans, _dev_graph, _executor, _gat_layer, _golden, _graphs,
                                    _knobs, _memo, _raw_att, _raw_plain, _same_bits, _scores, _weights, cora)  # noqa: F401
from .test_gpu_ops import _check

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn
NAMES = ("g900", "g5", "empty")


def _table8(name, F, dev):
    """The e4m3 table of a graph on the device and its fp32 widening (made on the CPU: the definition)."""
    def make():
        n = len(_graphs()[name][0]) - 1
        x8 = ops.to_fp8(torch.randn(n, F, generator=torch.Generator().manual_seed(8000 + F)) * 40)
        return x8.to(dev), x8.float().to(dev)
    return _memo(("x8", name, F), make)


def _ref8(name, F, heads, dev):
    def make():
        ip, ix = _graphs()[name]
        x = _table8(name, F, dev)[1].cpu().numpy().astype(np.float64)
        w = _weights(name, heads, dev)
        w = None if w is None else w.cpu().numpy().astype(np.float64)
        return isa_ref.aggregate(ip, ix, x, "src", w), isa_ref.aggregate_abs(ip, ix, x, "src", w)
    return _memo(("ref8", name, F, heads), make)


@pytest.mark.parametrize("F", [64, 128, 256])
def test_all_256_codes_widen_exactly(dev, F):
    """Every byte value at every column (so at every lane and byte position), one edge per row: the
    aggregate is the gathered row of x8.cpu().float() -- denormals and the two NaN codes included."""
    n = 256
    codes = ((torch.arange(n).view(n, 1) + torch.arange(F).view(1, F)) % 256).to(torch.uint8)
    x8 = codes.view(FP8)
    src = np.random.default_rng(3).permutation(n).astype(np.int32)
    g = G.from_numpy(np.arange(n + 1, dtype=np.int64), src, device=dev)
    want = x8.float().numpy()[src]
    for lean in (2, 0):  # the lean F = 128 kernel (opt-in) and the generic forms
        with _knobs(seg_lean=lean):
            y = ops.aggregate_blocked(g, x8.to(dev), None, blocks=2).cpu().numpy()
        assert np.array_equal(y, want, equal_nan=True), f"F={F} seg_lean={lean}"


PLAIN = [(128, 0), (128, 8), (128, 1), (128, 4), (64, 0), (64, 4), (256, 16)]


@pytest.mark.parametrize("item_edges", [7, 256])
@pytest.mark.parametrize("blocks", [1, 5])
@pytest.mark.parametrize("F,heads", PLAIN)
def test_plain_bitwise_twin(dev, F, heads, blocks, item_edges):
    """aggregate_blocked(x8) == aggregate_blocked(x8.float()) bit for bit, once against the fp64 oracle
    of the widened table; (128, 0 / 1 / 8) again under seg_lean = 0 and 2: generic == lean (k_agg_q16f8)."""
    for name in NAMES:
        g = _dev_graph(name, dev)
        x8, xf = _table8(name, F, dev)
        w = _weights(name, heads, dev)
        plan = g.blocked_plan(blocks, item_edges)
        what = f"fp8 plain {name} F={F} heads={heads} B={blocks} items={item_edges}"
        y8 = ops.aggregate_blocked(g, x8, w, plan=plan)
        _same_bits(y8, ops.aggregate_blocked(g, xf, w, plan=plan), what)
        _check(y8, *_ref8(name, F, heads, dev), what)
        if F == 128 and heads in (0, 1, 8):
            for lean in (0, 2):
                with _knobs(seg_lean=lean):
                    _same_bits(ops.aggregate_blocked(g, x8, w, plan=plan), y8, what + f" seg_lean={lean}")


@pytest.mark.parametrize("blocks,item_edges", [(1, 7), (5, 7), (1, 256), (5, 256)])
@pytest.mark.parametrize("F,H", [(128, 8), (64, 4), (256, 16)])
def test_attention_bitwise_twin(dev, F, H, blocks, item_edges):
    """gat_aggregate_blocked(x8) == gat_aggregate_blocked(x8.float()), y and sums, shifted and unshifted."""
    for name in NAMES:
        g = _dev_graph(name, dev)
        x8, xf = _table8(name, F, dev)
        a, b = _scores(name, H, dev)
        plan = g.blocked_plan(blocks, item_edges)
        for sh in (None, ops.softmax_shift(g, a, b, "EXP_LEAKY_RELU")):
            _att_pair(g, x8, xf, a, b, plan, f"fp8 att {name} F={F} H={H} B={blocks} items={item_edges} "
                      f"shifted={sh is not None}", shift=sh)


def test_refusals(dev):
    g = _dev_graph("g900", dev)
    F = 128
    x8, _ = _table8("g900", F, dev)
    a, b = _scores("g900", 8, dev)
    plan = g.blocked_plan(4, 256)
    y = torch.zeros(g.n_rows, F, device=dev)
    odd = torch.zeros(g.n_cols, F + 8, dtype=torch.uint8, device=dev).view(FP8)[:, :F]  # ldx % 16 != 0
    off = torch.zeros(g.n_cols * F + 16, dtype=torch.uint8, device=dev).view(FP8)[8:8 + g.n_cols * F].view(g.n_cols, F)
    assert off.data_ptr() % 16 == 8
    for bad, ld in ((odd, F + 8), (off, F)):
        with pytest.raises(ValueError, match="16-B aligned rows"):
            ops.aggregate_blocked(g, bad, None, plan=plan)
        with pytest.raises(ValueError, match="16-B aligned rows"):
            ops.gat_aggregate_blocked(g, bad, a, b, plan=plan)
        assert _raw_plain(g, bad.data_ptr(), ld, F, _lib.GTA_FP8, y, plan, dev) == _lib.ERR_UNSUPPORTED
        assert _raw_att(g, bad.data_ptr(), ld, F, _lib.GTA_FP8, a, b, y, plan, dev) == _lib.ERR_UNSUPPORTED
    # heads that do not fit the quarter-wave lanes: 32 heads of 4 columns, a lane holds 8
    w32 = torch.rand(g.nnz, 32, device=dev)
    with pytest.raises(ValueError, match="unsupported"):
        ops.aggregate_blocked(g, x8, w32, plan=plan)
    assert _lib.load().gta_aggregate_blocked_x(g.indptr.data_ptr(), g.indices.data_ptr(), g.n_rows, g.n_cols, g.nnz, x8.data_ptr(),
                                     F, F, _lib.GTA_FP8, w32.data_ptr(), 32, 32, None, y.data_ptr(), F, 0,
                                     plan.buf.data_ptr(), plan.blocks, plan.item_edges, plan.workspace(F).data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(y.any()), "a refused call wrote y"
    with pytest.raises(ValueError):  # the reducers take no fp8
        ops.reduce_blocked(g, x8, "MAX", plan=plan)


def test_executor_gcn_layer2_bitwise(golden_dir, manifest, cora, dev):
    """GCN layer 2 on an input already representable in e4m3: one cast, outputs bitwise the default run's."""
    og, st, sem = _golden(golden_dir, manifest, "GCN", 2)
    ip, ix = cora
    gd = G.from_numpy(ip, ix, device=dev)
    tensors = {k: v.to(dev) for k, v in workloads.make_tensors(og, G.from_numpy(ip, ix), "GCN", seed=2).items()}
    tensors["x"] = ops.to_fp8(tensors["x"]).float()
    outs = {}
    for gdt in (None, FP8):
        ex = _executor(og, st, gd, tensors, sem, gather_dtype=gdt)
        ex.mm_first = False
        outs[gdt] = {k: v.clone() for k, v in ex.run().items()}
        assert ex.gather_casts == (0 if gdt is None else 1) and _blocked_plans(gd)
    (src, _, cast), = ex._gather_cache.values()
    assert src is tensors["x"] and cast.dtype == FP8
    for k in outs[None]:
        _same_bits(outs[None][k], outs[FP8][k], f"GCN layer 2 output {k}")


def test_executor_auto_graph_keeps_the_option_apart(cora, dev):
    """run_stream: the replayed HIP graph equals the eager run; the option is part of the graph's key."""
    gd, lay, tensors = _gat_layer(dev, cora)
    executor.clear_auto_graphs()
    try:
        eager = {}
        for gdt in (None, FP8):
            res = executor.Executor(lay.opgraph, lay.stream, gd, tensors, lay.sem, gather_dtype=gdt).run()
            eager[gdt] = res[sorted(res)[-1]].clone()
        assert not torch.equal(eager[None], eager[FP8])
        for rep in range(3):  # call 1 eager, call 2 captures, call 3 replays; the two options interleaved
            for gdt in (None, FP8):
                res, ex = executor.run_stream(lay.opgraph, lay.stream, gd, tensors, lay.sem, gather_dtype=gdt)
                _same_bits(res.outputs[sorted(res.outputs)[-1]], eager[gdt], f"run_stream call {rep + 1} {gdt}")
        assert len(executor._AUTO) == 2 and all(e.run is not None for e in executor._AUTO.values())
        lay2 = pipeline.Layer("GAT", 1, gd, 1433, heads=8, op_array=lay.op_array, tile_size_list=lay.tile_size_list,
                              gather_dtype=FP8)
        res, ex = lay2.run(tensors)
        assert ex.gather_dtype == FP8
        _same_bits(res.outputs[sorted(res.outputs)[-1]], eager[FP8], "Layer.run")
    finally:
        executor.clear_auto_graphs()
