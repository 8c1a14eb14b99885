"""Column-blocked multi-reducer (gta_reduce_multi_blocked, ops.reduce_multi_blocked) on the GPU.

MAX / MIN are compared by value (NaN matching NaN) with tests/reduce_ref.py: they have no tolerance.
MEAN / VAR / STD are compared with tests/moments_ref.py inside the project's bound 1e-5 * sum|terms|
+ 1e-6 about the first-edge shift.  A fully sequential fp32 walk of a 1,500-edge row stays at 0.29
of that bound (moments_ref.emulate_f32, N(0,1) and 1000 + N(0,1), F = 64), and the blocked grouping
sums fewer terms per chain.  The graphs are tests/test_gpu_reduce_blocked.py's "empty" and "g5".
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, executor, graph as G, ir, lowering, ops, workloads
from gta_graph_tensor_acclelrator_for_general_gnn_amd.semantics import Semantics

from . import moments_ref, pool_layer, reduce_ref
from .test_gpu_footprint import Arena, _csr, _graph_in  # names only: no test function
from .test_gpu_moments import _check_ops, _within
from .test_gpu_reduce_blocked import (E_EX, HEAVY, N_EX, NAN_EDGES, SHORT, _dev_graph, _gated, _graphs, _knobs, _memo, _pool, _same,
                                      _table)

pytestmark = pytest.mark.gpu

ALL = ops.MULTI_REDS
MOM = ("MEAN", "VAR", "STD")
EPS = 1e-5


def _refs(name, x, key):
    """({MEAN | VAR | STD: (value, bound)}, {MAX | MIN: value}) of the fp32 table x, once per key."""
    def make():
        ip, ix = _graphs()[name]
        xn = x.cpu().numpy()
        return (moments_ref.moments_csr(ip, ix, xn.astype(np.float64), "src", EPS),
                {r: reduce_ref.reduce_csr(ip, ix, xn, r, "src") for r in ("MAX", "MIN")})
    return _memo(("mrb", name, key), make)


def _check(ys, refs, empty, what):
    mom, ext = refs
    for red, y in zip(ALL, ys):
        if red in mom:
            print(f"{what} {red}: max err / bound {_within(y, mom, red, what):.3f}")
        else:
            _same(y, ext[red], f"{what} {red}")
        assert not bool(y[empty].any()), f"{what} {red}: a row without edges is not 0"


@pytest.mark.parametrize("item_edges", [7, 256])
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_sweep(dev, F, bf, item_edges):
    for lean in ((1, 0) if F == 128 else (1,)):
        with _knobs(seg_lean=lean):
            for name in ("empty", "g5"):
                g = _dev_graph(name, dev)
                plan = g.blocked_plan(4, item_edges)
                empty = torch.from_numpy(np.flatnonzero(np.diff(_graphs()[name][0]) == 0)).to(dev)
                x, xb, xw = _table(name, F, "mixed", dev)
                what = f"{name} F={F} bf16={bf} items={item_edges} seg_lean={lean}"
                ys = ops.reduce_multi_blocked(g, xb if bf else x, ALL, plan=plan)
                _check(ys, _refs(name, xw if bf else x, (F, bf)), empty, what)
                for t in (xb, xw) if bf else (x,):  # a second call; bf16: the fp32 call on the widened table too
                    again = ops.reduce_multi_blocked(g, t, ALL, plan=plan)
                    assert all(torch.equal(a, b) for a, b in zip(ys, again)), f"{what}: the {t.dtype} call differs"


def test_subsets_and_strided_outputs(dev):
    F, g = 128, _dev_graph("empty", dev)
    x, plan = _table("empty", F, "mixed", dev)[0], g.blocked_plan(4, 7)
    full = dict(zip(ALL, ops.reduce_multi_blocked(g, x, ALL, plan=plan)))
    for reds in [(r,) for r in ALL] + [MOM, ("MIN", "MAX"), ("STD", "MAX", "MEAN")]:
        for red, y in zip(reds, ops.reduce_multi_blocked(g, x, reds, plan=plan)):
            assert torch.equal(y, full[red]), f"{red} of {reds} differs from the full call"
    table = torch.full((g.n_rows, 5 * F + 4), 7.0, device=dev)
    ys = ops.reduce_multi_blocked(g, x, ALL, out=table[:, :5 * F], plan=plan)
    for k, red in enumerate(ALL):
        assert ys[k].data_ptr() == table[:, k * F:].data_ptr() and torch.equal(ys[k], full[red]), red
    assert bool((table[:, 5 * F:] == 7.0).all())
    odd = torch.full((g.n_rows, F + 1), 7.0, device=dev)  # rows not aligned to F / 64 floats: element stores
    y, = ops.reduce_multi_blocked(g, x, ("VAR",), outs=(odd[:, 1:],), plan=plan)
    assert torch.equal(y, full["VAR"]) and bool((odd[:, 0] == 7.0).all())


@pytest.mark.parametrize("F", [64, 128])
def test_cancellation(dev, F):
    g = _dev_graph("empty", dev)
    x = 1000 + _table("empty", F, "mixed", dev)[0]
    ys = dict(zip(ALL, ops.reduce_multi_blocked(g, x, ALL, plan=g.blocked_plan(4, 7))))
    for red in ("VAR", "STD"):
        print(f"cancellation F={F} {red}: max err / bound {_within(ys[red], _refs('empty', x, (F, 'cancel'))[0], red, 'cancel'):.3f}")


@pytest.mark.parametrize("item_edges", [7, 256])
def test_special_values(dev, item_edges):
    F, g = 128, _dev_graph("empty", dev)
    ip, ix = _graphs()["empty"]
    plan = g.blocked_plan(4, item_edges)
    base = _table("empty", F, "mixed", dev)[0]
    src, col = int(ix[ip[HEAVY] + NAN_EDGES[item_edges]]), 3
    want = np.zeros((g.n_rows, F), bool)
    want[HEAVY, col] = True
    for v in (float("nan"), float("inf")):
        x = base.clone()
        x[src, col] = v
        for red, y in zip(ALL, ops.reduce_multi_blocked(g, x, ALL, plan=plan)):
            if red in MOM or v != v:
                assert np.array_equal(torch.isnan(y).cpu().numpy(), want), f"{v} {red}: NaN elsewhere than ({HEAVY}, {col})"
            else:
                assert torch.equal(y, ops.reduce(g, x, red, "src")), f"inf {red} differs from ops.reduce"
    x = base.clone()
    x[torch.from_numpy(ix[ip[SHORT]:ip[SHORT + 1]].astype(np.int64)).to(dev)] = base[7]
    mean, _, _, var, std = ops.reduce_multi_blocked(g, x, ALL, plan=plan)
    assert not bool(var[SHORT].any()) and torch.equal(mean[SHORT], base[7])
    assert torch.equal(std[SHORT], torch.full((F,), EPS, device=dev).sqrt())


def test_edges_of_the_contract(dev):
    n, F, L = 37, 128, _lib.load()
    g0 = G.from_numpy(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), device=dev)
    plan, st = g0.blocked_plan(2), torch.cuda.current_stream(dev).cuda_stream
    ys = [torch.full((n, F), 7.0, device=dev) for _ in ALL]
    ptrs, lds = (ctypes.c_void_p * 5)(*(y.data_ptr() for y in ys)), (ctypes.c_int64 * 5)(*([F] * 5))

    def raw(which, width):
        return L.gta_reduce_multi_blocked(which, g0.indptr.data_ptr(), None, n, n, 0, None, 0, width, _lib.GTA_F32, ptrs, lds,
                                          EPS, plan.buf.data_ptr(), plan.blocks, plan.item_edges, None, st)
    assert raw(0, F) == _lib.ERR_ARG and raw(64, F) == _lib.ERR_ARG
    assert raw(31, 100) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize(dev)
    assert all(bool((y == 7.0).all()) for y in ys), "a refused call wrote an output"
    assert raw(31, F) == _lib.OK, L.gta_last_error()
    assert not any(bool(y.any()) for y in ys)
    g, x = _dev_graph("g5", dev), _table("g5", F, "mixed", dev)[0]
    with pytest.raises(ValueError, match="reds"):
        ops.reduce_multi_blocked(g, x, ("MAX", "SUM"), blocks=2)
    ip, ix = (a.copy() for a in _graphs()["g5"])
    ix[ip[2]], ix[ip[2] + 1] = 4, 0  # row 2 no longer sorted
    with pytest.raises(ValueError, match="sorted"):
        ops.reduce_multi_blocked(G.from_numpy(ip, ix, device=dev), x, ALL, blocks=2)


@pytest.mark.parametrize("F", [64, 128])
def test_guard_bands(dev, F):
    """Every tensor a view of one NaN-poisoned arena, plan and workspace of exactly their *_bytes:
    only the five outputs and the workspace change, and the results are finite and the reference's."""
    L = _lib.load()
    n, blocks, ie = 130, 5, 7
    ip, ix = _csr(n, 3000, 2, sort=True)
    nnz = len(ix)
    x = np.random.default_rng(900 + F).standard_normal((n, F)).astype(np.float32)
    ar = Arena(dev, 8 << 20)
    g = _graph_in(ar, ip, ix, n, "a")
    xt = ar.table("x", x, "a")
    ys = [ar.out(f"y{k}", n, F, "a") for k in range(5)]
    ptrs, lds = (ctypes.c_void_p * 5)(*(y.data_ptr() for y in ys)), (ctypes.c_int64 * 5)(*(y.stride(0) for y in ys))
    pb = int(L.gta_aggregate_blocked_plan_bytes(n, nnz, blocks, ie))
    wsb = int(L.gta_reduce_multi_blocked_workspace_bytes(n, nnz, blocks, F, ie, 31))
    assert wsb == 4 * int(L.gta_aggregate_blocked_workspace_bytes(n, nnz, blocks, F, ie))
    plan, ws = ar.raw("plan", pb), ar.raw("slabs", wsb)
    st = torch.cuda.current_stream(dev).cuda_stream
    ar.seal()
    assert L.gta_aggregate_blocked_plan_build(g.indptr.data_ptr(), g.indices.data_ptr(), n, n, nnz, blocks, ie, 0,
                                              plan.data_ptr(), pb, st) == 0, L.gta_last_error()
    ar.check([plan], "plan build")
    ar.seal()
    rc = L.gta_reduce_multi_blocked(31, g.indptr.data_ptr(), g.indices.data_ptr(), n, n, nnz, xt.data_ptr(), xt.stride(0), F,
                                    _lib.GTA_F32, ptrs, lds, EPS, plan.data_ptr(), blocks, ie, ws.data_ptr(), st)
    assert rc == 0, L.gta_last_error()
    ar.check([ws] + ys, f"reduce_multi_blocked guard F={F}")
    assert all(np.isfinite(y.cpu().numpy()).all() for y in ys), "poison was read and used"
    mom = moments_ref.moments_csr(ip, ix, x.astype(np.float64), "src", EPS)
    for red, y in zip(ALL, ys):
        if red in MOM:
            _within(y, mom, red, "guard")
        else:
            _same(y, reduce_ref.reduce_csr(ip, ix, x, red, "src"), f"guard {red}")


@pytest.mark.parametrize("agg", ["STD", "VAR"])
def test_executor_single_moment_gather(dev, monkeypatch, agg):
    """GraphSAGE-pool layer 2 with the size gate open: under multi_reduce_blocked exactly one
    ops.reduce_multi_blocked call and no reduce_multi, every op within the bound of the fp64 walk;
    with the flag off the one row-chunked reduce_multi call."""
    g, recs, og, stream, sem, tensors = _pool(dev, agg)
    ip, ix = g.numpy()
    ref = moments_ref.layer_ref(recs, sem, ip, ix, {k: v.double().cpu().numpy() for k, v in tensors.items()}, sem.inputs)
    calls = []
    for name in ("reduce_multi", "reduce_multi_blocked"):
        monkeypatch.setattr(ops, name, lambda *a, _f=getattr(ops, name), _n=name, **kw: calls.append(_n) or _f(*a, **kw))
    _gated(monkeypatch)
    for on, want in ((True, ["reduce_multi_blocked"]), (False, ["reduce_multi"])):
        del calls[:]
        ex = executor.Executor(og, stream, g, tensors, sem, multi_reduce_blocked=on)
        ex.run()
        assert calls == want, calls
        _check_ops(ex, ref, range(len(og)), f"pool-{agg} multi_reduce_blocked={on}")


@pytest.mark.parametrize("reds", [("MAX", "STD"), ("MEAN", "MAX", "MIN", "STD")], ids=["pair", "four"])
def test_executor_sibling_group(dev, monkeypatch, reds):
    """The pool layer with its gather repeated (distinct COMP_TYPEs over the one scatter, one op per
    block): a sibling group of a virtual scatter.  Under multi_reduce_blocked the group takes exactly
    one ops.reduce_multi_blocked call whatever its size and no other gather launch; with the flag off
    the one row-chunked reduce_multi call.  Every op within the bound of the fp64 walk."""
    g = G.synthetic(N_EX, E_EX, seed=2, device=dev)
    recs = pool_layer.records(N_EX, g.nnz, 128, reds[0])
    for comp in reds[1:]:
        r = copy.deepcopy(recs[1])
        r["COMP_TYPE"], r["OP_NO"], r["OUTPUT"]["output_list"] = comp, len(recs), []
        recs[0]["OUTPUT"]["output_list"].append(r["OP_NO"])
        recs.append(r)
    og, sem = ir.OpGraph(recs), Semantics()
    stream = ir.Stream(lowering.lower(recs, N_EX, [[i] for i in range(len(recs))], [[64, 1]] * len(recs)))
    tensors = workloads.make_tensors(og, g, "GraphSAGE", seed=4)
    ip, ix = g.numpy()
    ref = moments_ref.layer_ref(recs, sem, ip, ix, {k: v.double().cpu().numpy() for k, v in tensors.items()}, sem.inputs)
    calls = []
    for name in ("reduce_multi", "reduce_multi_blocked", "reduce", "reduce_blocked", "aggregate", "aggregate_blocked"):
        monkeypatch.setattr(ops, name, lambda *a, _f=getattr(ops, name), _n=name, **kw: calls.append(_n) or _f(*a, **kw))
    _gated(monkeypatch)
    for on, want in ((True, ["reduce_multi_blocked"]), (False, ["reduce_multi"])):
        del calls[:]
        ex = executor.Executor(og, stream, g, tensors, sem, multi_reduce_blocked=on)
        ex.run()
        assert calls == want, calls
        _check_ops(ex, ref, range(len(og)), f"group {reds} multi_reduce_blocked={on}")
