"""Degree-class column blocks: the blocked plan numbers its items class by class.

A row's class is its merge factor m = merge_of(deg, B, row_edges) (light rows merge m = 2^k
neighbouring fine blocks).  With the knob seg_class_major (default 1) the rows of one class run
together, m = 1 first, and a class's items are numbered merged-block-major over its own
ceil(B / m) merged blocks; with 0 all rows are one class numbered fine-block-major (the order of
every earlier plan).  Partial grouping and each row's item list depend on (fine blocks, item_edges,
row_edges) alone, so the item order may not change a bit of any result.

The structure tests decode the device plan and compare it with a numpy restatement of the rules.
"""
import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, graph as G, ops
from oracle import isa_ref

from . import prep_ref
from .test_gpu_footprint import CAP, Arena, _graph_in, _knobs, _ok, _p, _st
from .test_gpu_ops import _check

gpu = pytest.mark.gpu


def _merge_of(deg, B, row_edges):
    m = 1
    while row_edges and deg and m < B and deg * m < row_edges * B:
        m *= 2
    return m


_GRAPH = {}


def _items_graph(n=600, e=15000):
    """test_blocked_plan_items' graph: rows of 4,000 and 700 edges, two empty rows (made once)."""
    if n not in _GRAPH:
        ip, _ = G.synthetic(n, e, seed=11, device="cpu").numpy()
        deg = np.diff(ip).copy()
        deg[3], deg[4] = 4000, 700
        deg[[10, 11]] = 0
        _GRAPH[n] = _csr_of(deg, n)
    return _GRAPH[n]


def _csr_of(deg, n_cols, seed=0):
    rng = np.random.default_rng(seed)
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = np.concatenate([np.sort(rng.integers(0, n_cols, d)) for d in deg] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ip, ix


def _decode(plan, n_rows):
    """(hdr, items [n_items, 3] = beg, row, len, row_ptr, row_items) of a device plan."""
    return prep_ref.decode_blocked(plan.buf, n_rows, plan.blocks)


def _check_plan(plan, ip, ix, n_cols, blocks, item_edges, row_edges, class_major):
    """Every rule of the plan on the decoded device plan (tests/prep_ref.py, vectorised)."""
    prep_ref.check_blocked(_decode(plan, len(ip) - 1), ip, ix, n_cols, blocks, item_edges, row_edges, class_major,
                           n_items=plan.n_items)


@gpu
@pytest.mark.parametrize("class_major", [1, 0])
@pytest.mark.parametrize("item_edges", [7, 256])
@pytest.mark.parametrize("row_edges", [0, 16, 40])
@pytest.mark.parametrize("blocks", [1, 5, 16, 63])
def test_plan_structure(dev, blocks, row_edges, item_edges, class_major):
    n = 600
    ip, ix = _items_graph(n)
    g = G.from_numpy(ip, ix, device=dev)
    with _knobs(seg_class_major=class_major):
        plan = ops.BlockedPlan(g, blocks, item_edges, row_edges)
    assert (plan.blocks, plan.item_edges, plan.row_edges) == (blocks, item_edges, row_edges)
    _check_plan(plan, ip, ix, n, blocks, item_edges, row_edges, class_major)


def _degenerate(name):
    """(deg, n_cols, blocks, row_edges)"""
    rng = np.random.default_rng(5)
    if name == "all_light":     # every row lighter than row_edges: all rows collapse to one block
        return rng.integers(0, 12, 300), 300, 16, 12
    if name == "empty_class":   # m in {1, 4, 16}: the classes m = 2 and m = 8 have no rows
        return np.repeat([400, 100, 1, 0], [20, 30, 40, 3]), 500, 16, 16
    if name == "few_rows":      # n_rows < blocks
        return np.array([90, 0, 3, 700, 17]), 400, 63, 16
    if name == "one_row":
        return np.array([33]), 64, 20, 16
    raise KeyError(name)


@gpu
@pytest.mark.parametrize("class_major", [1, 0])
@pytest.mark.parametrize("name", ["all_light", "empty_class", "few_rows", "one_row"])
def test_plan_degenerate(dev, name, class_major):
    deg, n_cols, blocks, row_edges = _degenerate(name)
    ip, ix = _csr_of(deg, n_cols, seed=1)
    g = G.from_numpy(ip, ix, device=dev, n_cols=n_cols)
    for item_edges in (5, 256):
        with _knobs(seg_class_major=class_major):
            plan = ops.BlockedPlan(g, blocks, item_edges, row_edges)
        _check_plan(plan, ip, ix, n_cols, blocks, item_edges, row_edges, class_major)
        if name == "all_light" and item_edges == 256:
            assert plan.n_items == int((deg > 0).sum())  # one item per non-empty row
    F = 128
    rng = np.random.default_rng(2)
    x = rng.standard_normal((n_cols, F)).astype(np.float32)
    w = rng.random((len(ix), 8)).astype(np.float32)
    y = ops.aggregate_blocked(g, torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev), plan=plan)
    _check(y, isa_ref.aggregate(ip, ix, x, "src", w), isa_ref.aggregate_abs(ip, ix, x, "src", w), f"degenerate {name}")


_BIT = {}


def _bitwise_inputs(dev):
    """One lognormal graph with rows in every class at (blocks 24, row_edges 16), and its two plans."""
    if not _BIT:
        n, e, B, ie, re_ = 1500, 60000, 24, 32, 16
        g = G.synthetic(n, e, seed=7, device=dev)
        plans = {}
        for cm in (0, 1):
            with _knobs(seg_class_major=cm):
                plans[cm] = ops.BlockedPlan(g, B, ie, re_)
        ip, _ = g.numpy()
        ms = {_merge_of(int(d), B, re_) for d in np.diff(ip)}
        assert len(ms) >= 4, ms
        _, it0, _, _ = _decode(plans[0], n)
        _, it1, _, _ = _decode(plans[1], n)
        assert plans[0].n_items == plans[1].n_items and not np.array_equal(it0, it1), "the two orders do not differ"
        rng = np.random.default_rng(3)
        _BIT.update(g=g, plans=plans, rng_x={F: torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)).to(dev)
                                             for F in (64, 128, 256)},
                    w=torch.from_numpy(rng.random((g.nnz, 8)).astype(np.float32)).to(dev),
                    a=torch.from_numpy(rng.standard_normal((n, 8)).astype(np.float32)).to(dev),
                    b=torch.from_numpy(rng.standard_normal((n, 8)).astype(np.float32)).to(dev))
    return _BIT


@gpu
@pytest.mark.parametrize("F", [64, 128, 256])
@pytest.mark.parametrize("op", ["agg_w8", "agg", "agg_w8_bf16", "agg_bf16", "gat_sums", "max"])
def test_item_order_changes_no_bit(dev, op, F):
    d = _bitwise_inputs(dev)
    g, x, w = d["g"], d["rng_x"][F], d["w"]
    if "bf16" in op:
        x = x.to(torch.bfloat16)
    outs = []
    for cm in (0, 1):
        plan = d["plans"][cm]
        if op.startswith("agg"):
            outs.append((ops.aggregate_blocked(g, x, w if "w8" in op else None, plan=plan),))
        elif op == "gat_sums":
            outs.append(ops.gat_aggregate_blocked(g, x, d["a"], d["b"], want_sums=True, plan=plan))
        else:
            outs.append((ops.reduce_blocked(g, x, "MAX", plan=plan),))
    for t0, t1 in zip(*outs):
        assert bool(torch.isfinite(t0).all()) and float(t0.abs().max()) > 0
        assert torch.equal(t0, t1), f"{op} F={F}: class-major and block-major items differ"


@gpu
def test_default_plan_oracle(dev):
    """The default plan of a blocks = 8 request on a lognormal graph of 3,000 rows / 300 k edges,
    with the default mapping reaching it (seg_fine_min 1) at 1.6 x fine blocks and row_edges 16 --
    several classes populated -- and with the knobs as they are, against the fp64 oracle."""
    n, e, F = 3000, 300000, 128
    g = G.synthetic(n, e, seed=4, device=dev)
    ip, ix = g.numpy()
    rng = np.random.default_rng(9)
    x = rng.standard_normal((n, F)).astype(np.float32)
    w = rng.random((len(ix), 8)).astype(np.float32)
    ref, ab = isa_ref.aggregate(ip, ix, x, "src", w), isa_ref.aggregate_abs(ip, ix, x, "src", w)
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    with _knobs(seg_fine_min=1, seg_fine_pct=160, seg_row_edges=16):
        plan = g.blocked_plan(8)
        assert (plan.requested, plan.blocks, plan.item_edges, plan.row_edges) == (8, 13, ops.BlockedPlan.ITEM_EDGES, 16)
        assert len({_merge_of(int(d), 13, 16) for d in np.diff(ip)}) >= 3
        _check_plan(plan, ip, ix, n, 13, ops.BlockedPlan.ITEM_EDGES, 16, ops.get_debug("seg_class_major"))
        _check(ops.aggregate_blocked(g, xd, wd, blocks=8), ref, ab, "default plan, 13 fine blocks, row_edges 16")
    assert g.blocked_plan(8) is not plan                       # another mapping, another cache entry
    assert g.blocked_plan(8, plan.item_edges, 16).blocks == 8  # named: exactly what was asked for
    _check(ops.aggregate_blocked(g, xd, wd, blocks=8), ref, ab, "default plan, default knobs")
    fine, ie, re_ = ops.BlockedPlan.resolve(20)
    p20 = g.blocked_plan(20)
    assert (p20.requested, p20.blocks, p20.item_edges, p20.row_edges) == (20, fine, ie, re_)
    _check_plan(p20, ip, ix, n, fine, ie, re_, ops.get_debug("seg_class_major"))
    _check(ops.aggregate_blocked(g, xd, wd, blocks=20), ref, ab, "default plan of a 20-block request")


@gpu
@pytest.mark.parametrize("variant", ["classes_b63", "all_light", "few_rows", "block_major"])
def test_plan_variants_exact_buffers(dev, variant):
    """The class-major plan variants build and run inside buffers of exactly plan_bytes /
    workspace_bytes, canaries on both sides (tests/test_gpu_footprint.py's arena)."""
    L = _lib.load()
    F, H, ie = 128, 8, 16
    if variant in ("classes_b63", "block_major"):
        deg, nc, B, re_ = np.repeat([900, 260, 70, 20, 3, 0], [3, 10, 30, 60, 90, 4]), 700, 63, 16
    else:
        deg, nc, B, re_ = _degenerate(variant)
    ip, ix = _csr_of(deg, nc, seed=6)
    n, nnz = len(deg), len(ix)
    rng = np.random.default_rng(8)
    x = rng.standard_normal((nc, F)).astype(np.float32)
    w = rng.random((nnz, H)).astype(np.float32)
    a, b = rng.standard_normal((n, H)).astype(np.float32), rng.standard_normal((nc, H)).astype(np.float32)
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, nc, "a")
    pb = int(L.gta_aggregate_blocked_plan_bytes(n, nnz, B, ie))
    wsb = int(L.gta_aggregate_blocked_workspace_bytes(n, nnz, B, F, ie))
    wsb2 = int(L.gta_gat_aggregate_blocked_workspace_bytes(n, nnz, B, F, H, ie))
    plan, ws, ws2 = ar.raw("plan", pb), ar.raw("slabs", wsb), ar.raw("slabs_att", wsb2)
    xt, wt = ar.table("x", x, "a"), ar.table("w", w, "a")
    at, bt = ar.table("a_dst", a, "a"), ar.table("b_src", b, "a")
    y, y2, y3, sums = ar.out("y", n, F, "a"), ar.out("y_att", n, F, "a"), ar.out("y_max", n, F, "a"), ar.mat("sums", n, H)
    what = f"class plan {variant}"
    build = (_p(g.indptr), _p(g.indices), n, nc, nnz, B, ie, re_, _p(plan))
    with _knobs(seg_class_major=0 if variant == "block_major" else 1):
        ar.seal()
        assert L.gta_aggregate_blocked_plan_build(*build, pb - 1, _st(dev)) == _lib.ERR_ARG
        ar.check([], what + " one byte short")
        assert L.gta_aggregate_blocked_plan_build(*build, pb, _st(dev)) == 0, L.gta_last_error()
        ar.check([plan], what + " build")
    hdr = plan[:128].view(torch.int64).cpu()
    assert int(hdr[3]) == 0 and 0 < int(hdr[4]) <= int(hdr[6])
    gi = (_p(g.indptr), _p(g.indices), n, nc, nnz)
    ar.seal()
    assert L.gta_aggregate_blocked(*gi, _p(xt), xt.stride(0), F, _p(wt), wt.stride(0), H, None, _p(y), y.stride(0), 0,
                                   _p(plan), B, ie, _p(ws), _st(dev)) == 0, L.gta_last_error()
    ar.check([ws, y], what + " aggregate_blocked")
    _ok(y, isa_ref.aggregate(ip, ix, x, "src", w), isa_ref.aggregate_abs(ip, ix, x, "src", w), what + " aggregate_blocked")
    ar.seal()
    assert L.gta_gat_aggregate_blocked(*gi, _p(xt), xt.stride(0), F, _p(at), at.stride(0), _p(bt), bt.stride(0), H,
                                       _lib.SF["EXP_LEAKY_RELU"], 1, 0, _p(y2), y2.stride(0), _p(sums), _p(plan), B, ie,
                                       _p(ws2), _st(dev)) == 0, L.gta_last_error()
    ar.check([ws2, y2, sums], what + " gat_aggregate_blocked")
    _, rsum = isa_ref.gat_aggregate(ip, ix, x.astype(np.float64), a.astype(np.float64), b.astype(np.float64),
                                    "EXP_LEAKY_RELU", True)
    _ok(sums, rsum, rsum, what + " gat sums")
    ar.seal()
    assert L.gta_reduce_blocked(ops._REDS["MAX"], *gi, _p(xt), xt.stride(0), F, _lib.GTA_F32, _p(y3), y3.stride(0),
                                _p(plan), B, ie, _p(ws), _st(dev)) == 0, L.gta_last_error()
    ar.check([ws, y3], what + " reduce_blocked")
    want = np.zeros((n, F), np.float32)
    for r in range(n):
        if ip[r + 1] > ip[r]:
            want[r] = x[ix[ip[r]:ip[r + 1]]].max(axis=0)
    assert np.array_equal(y3.cpu().numpy(), want), what + " reduce_blocked MAX"
