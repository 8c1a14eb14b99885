"""Column-blocked MAX / MIN gather (gta_reduce_blocked, ops.reduce_blocked) on the GPU.

Apart from the sign of a zero every output of a MAX / MIN is bitwise one of its inputs, so the
blocked form must give exactly the row-chunked form's value for any plan, block count or item
length: every comparison is by value with NaN matching NaN and has no tolerance.  The reference is
tests/reduce_ref.py.  The sizes are the smallest at which these kernels can go wrong: items that
split a row (item_edges 7), full unmasked steps (256), two items of unequal length per wave, an
item count that is no multiple of the items per wave, empty rows, a 3-edge and a 1,500-edge row.

Executor: in every stock op graph an applyedge MUL by an edge weight sits between the scatter and
the gather, so a stock layer's reducer reads an [E, F] edge tensor and keeps the row-chunked route
(checked below on GraphSAGE and PNA).  The blocked route is exercised on GraphSAGE's layer 2
without that MUL (tests/pool_layer.py: GraphSAGE-pool, the gather of a virtual scatter).
"""
import contextlib

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, executor, graph as G, ops, pipeline, workloads

from . import pool_layer, reduce_ref
from .test_gpu_footprint import Arena, _csr, _graph_in  # names only: no test function

pytestmark = pytest.mark.gpu

_MEMO = {}
HEAVY, SHORT = 5, 6  # rows of the "empty" graph: 1,500 edges / 3 edges
NAN_EDGES = {7: 16, 256: 600}  # item_edges -> an edge of the heavy row inside its third item (7 / 250 edges each)


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


@contextlib.contextmanager
def _knobs(**kv):
    old = {k: ops.get_debug(k) for k in kv}
    try:
        for k, v in kv.items():
            ops.set_debug(k, v)
        yield
    finally:
        for k, v in old.items():
            ops.set_debug(k, v)


def _graphs():
    """tests/test_gpu_blocked_bf16.py's three graphs, columns sorted per row.  In "empty" the
    sources of three chosen edges (one in the heavy row's third item at item_edges 7, one at 256, the
    middle edge of the 3-edge row) are gathered by no other row, so a value planted there shows in
    exactly one row."""
    def make():
        out = {}
        for name, (n, e) in {"g900": (900, 30000), "g5": (5, 2000)}.items():
            ip, ix = G.synthetic(n, e, seed=11).numpy()
            assert all(np.all(np.diff(ix[ip[r]:ip[r + 1]]) >= 0) for r in range(n))
            out[name] = (ip, ix)
        rng = np.random.default_rng(4)
        deg = np.diff(out["g900"][0])[:300].copy()
        deg[[0, 17, 18, 299]] = 0
        deg[HEAVY], deg[SHORT] = 1500, 3
        ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        ix = np.concatenate([np.sort(rng.integers(0, 300, d)) for d in deg]).astype(np.int32)
        own = {int(ix[ip[HEAVY] + e]): HEAVY for e in NAN_EDGES.values()}
        own[int(ix[ip[SHORT] + 1])] = SHORT
        assert len(own) == 3
        spare = next(s for s in range(300) if s not in own)
        for r in range(300):
            seg = ix[ip[r]:ip[r + 1]]
            for s, owner in own.items():
                if r != owner:
                    seg[seg == s] = spare
            seg.sort()
        out["empty"] = (ip, ix)
        return out
    return _memo("graphs", make)


def _dev_graph(name, dev):
    return _memo(("dg", name), lambda: G.from_numpy(*_graphs()[name], device=dev))


def _table(name, F, kind, dev):
    """(fp32 table, bf16 table, the bf16 table widened), on the device: kind "neg" = -1 - |N(0,1)|
    (a 0 identity shows as a wrong maximum at once), "mixed" = N(0,1).  No zeros, no NaN."""
    def make():
        n = len(_graphs()[name][0]) - 1
        rng = np.random.default_rng(1000 + F + (0 if kind == "neg" else 1))
        x = rng.standard_normal((n, F))
        if kind == "neg":
            x = -1 - np.abs(x)
        x = torch.from_numpy(x.astype(np.float32)).to(dev)
        xb = x.to(torch.bfloat16)
        assert not bool((x == 0).any()) and not bool((xb.float() == 0).any())
        return x, xb, xb.float()
    return _memo(("x", name, F, kind), make)


def _ref(name, F, kind, bf, red, dev):
    def make():
        ip, ix = _graphs()[name]
        x, _, xw = _table(name, F, kind, dev)
        return reduce_ref.reduce_csr(ip, ix, (xw if bf else x).cpu().numpy(), red, "src")
    return _memo(("ref", name, F, kind, bf, red), make)


def _row_chunked(name, F, kind, bf, red, dev):
    def make():
        x, xb, _ = _table(name, F, kind, dev)
        return ops.reduce(_dev_graph(name, dev), xb if bf else x, red, "src")
    return _memo(("rc", name, F, kind, bf, red), make)


def _same(y, ref, what):
    got = y.detach().cpu().numpy()
    ref = np.asarray(ref)
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}"


# ---------------------------------------------------------------------------------------------
# 1. sweep
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("item_edges", [7, 256])
@pytest.mark.parametrize("blocks", [1, 5])
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_sweep(dev, F, bf, blocks, item_edges):
    """Quarter-wave forms (F = 64 / 256), the lean half-wave form and, under seg_lean 0, the generic
    half-wave form (F = 128); MAX and MIN; both value kinds; the three graphs.  Equal to the reference
    on the table as gathered, and torch.equal to the row-chunked ops.reduce."""
    for lean in ((1, 0) if F == 128 else (1,)):
        with _knobs(seg_lean=lean):
            for name in ("g900", "g5", "empty"):
                g = _dev_graph(name, dev)
                plan = g.blocked_plan(blocks, item_edges)
                for kind in ("neg", "mixed"):
                    x, xb, _ = _table(name, F, kind, dev)
                    for red in ("MAX", "MIN"):
                        what = f"{name} F={F} bf16={bf} {red} {kind} B={blocks} items={item_edges} seg_lean={lean}"
                        y = ops.reduce_blocked(g, xb if bf else x, red, plan=plan)
                        _same(y, _ref(name, F, kind, bf, red, dev), what)
                        assert torch.equal(y, _row_chunked(name, F, kind, bf, red, dev)), what + ": differs from ops.reduce"
    assert ops.get_debug("seg_lean") == 1


# ---------------------------------------------------------------------------------------------
# 2. RNE rounding to bf16 is monotone: it commutes with the max
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [64, 128, 256])
def test_bf16_commutes_with_the_reducer(dev, F):
    for name in ("g900", "empty"):
        g = _dev_graph(name, dev)
        for kind in ("neg", "mixed"):
            x, xb, _ = _table(name, F, kind, dev)
            for red in ("MAX", "MIN"):
                y = ops.reduce_blocked(g, xb, red, plan=g.blocked_plan(5, 7))
                exp = _row_chunked(name, F, kind, False, red, dev).to(torch.bfloat16).float()
                _same(y, exp.cpu().numpy(), f"bf16 commutes {name} F={F} {kind} {red}")


# ---------------------------------------------------------------------------------------------
# 3. special values
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_special_values(dev, F, bf):
    ip, ix = _graphs()["empty"]
    g = _dev_graph("empty", dev)
    n = g.n_rows
    empty = np.flatnonzero(np.diff(ip) == 0)
    assert set(empty) >= {0, 17, 18, 299}
    base = _table("empty", F, "mixed", dev)[1 if bf else 0]
    for ie, edge in NAN_EDGES.items():
        for blocks in (1, 5):
            plan = g.blocked_plan(blocks, ie)
            # a NaN lands at exactly its (row, column): inside the heavy row's third item, and in the 3-edge row
            for row, src, col in ((HEAVY, int(ix[ip[HEAVY] + edge]), 3), (SHORT, int(ix[ip[SHORT] + 1]), F - 1)):
                x = base.clone()
                x[src, col] = float("nan")
                for red in ("MAX", "MIN"):
                    y = ops.reduce_blocked(g, x, red, plan=plan)
                    nan = torch.isnan(y).cpu().numpy()
                    want = np.zeros((n, F), bool)
                    want[row, col] = True
                    what = f"NaN F={F} bf16={bf} {red} items={ie} B={blocks} row={row}"
                    assert np.array_equal(nan, want), f"{what}: NaN at {np.argwhere(nan).tolist()[:5]}"
                    _same(y, reduce_ref.reduce_csr(ip, ix, x.float().cpu().numpy(), red, "src"), what)
            # a row whose every source value is the identity's value keeps it; rows without edges get 0
            for red, v in (("MAX", float("-inf")), ("MIN", float("inf"))):
                x = base.clone()
                x[torch.from_numpy(ix[ip[SHORT]:ip[SHORT + 1]].astype(np.int64)).to(dev)] = v
                y = ops.reduce_blocked(g, x, red, plan=plan)
                what = f"inf row F={F} bf16={bf} {red} items={ie} B={blocks}"
                assert bool((y[SHORT] == v).all()), what
                assert not bool(y[torch.from_numpy(empty).to(dev)].any()), what + ": an empty row is not 0"
                _same(y, reduce_ref.reduce_csr(ip, ix, x.float().cpu().numpy(), red, "src"), what)


SPECIAL = {3: 0x7FC0, 4: 0x7FC5, 10: 0x7F80, 20: 0xFF80, 40: 0x0001, 41: 0x8001, 50: 0x007F, 51: 0xFFC1}  # row -> bf16 bits


@pytest.mark.parametrize("F", [64, 128, 256])
def test_bf16_bit_patterns_come_back(dev, F):
    """NaN (with payload), +-inf and bf16 denormals gathered alone come back as the same fp32 bits."""
    xb = _table("g900", F, "mixed", dev)[1].clone()
    bits = xb.view(torch.int16)
    for r, v in SPECIAL.items():
        bits[r, :] = v - 0x10000 if v >= 0x8000 else v
    xw = xb.float()
    for r, v in SPECIAL.items():
        one = G.from_numpy(np.array([0, 1], dtype=np.int64), np.array([r], dtype=np.int32), device=dev, n_cols=xb.shape[0])
        for red in ("MAX", "MIN"):
            y = ops.reduce_blocked(one, xb, red, blocks=1)
            got, exp = y.view(torch.int32), xw[r:r + 1].contiguous().view(torch.int32)
            assert torch.equal(got, exp), f"bf16 bits {v:#06x} F={F} {red}: came back as {int(got[0, 0]) & 0xffffffff:#010x}"
            assert int(exp[0, 0]) & 0xffffffff == v << 16


# ---------------------------------------------------------------------------------------------
# 4. views and refusals
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_pitched_view(dev, F, bf):
    """ldx = F + 8: a view into a wider table whose other columns are NaN."""
    g = _dev_graph("g900", dev)
    x = _table("g900", F, "neg", dev)[1 if bf else 0]
    wide = torch.full((g.n_cols, F + 8), float("nan"), dtype=x.dtype, device=dev)
    wide[:, :F] = x
    view = wide[:, :F]
    assert view.stride(0) == F + 8
    for blocks, ie in ((1, 256), (5, 7)):
        for red in ("MAX", "MIN"):
            y = ops.reduce_blocked(g, view, red, plan=g.blocked_plan(blocks, ie))
            _same(y, _ref("g900", F, "neg", bf, red, dev), f"pitched F={F} bf16={bf} {red} B={blocks}")


def _raw(g, xptr, ldx, F, dt, y, plan, dev, red=_lib.RED_MAX):
    return _lib.load().gta_reduce_blocked(red, g.indptr.data_ptr(), g.indices.data_ptr(), g.n_rows, g.n_cols, g.nnz, xptr,
                                          ldx, F, dt, y.data_ptr(), y.stride(0), plan.buf.data_ptr(), plan.blocks,
                                          plan.item_edges, plan.workspace(F).data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream)


def test_add_and_refusals(dev):
    F = 128
    g = _dev_graph("g900", dev)
    x, xb, _ = _table("g900", F, "mixed", dev)
    plan = g.blocked_plan(5, 7)
    for t in (x, xb):
        y = ops.reduce_blocked(g, t, "ADD", plan=plan)
        assert torch.equal(y.view(torch.int32), ops.aggregate_blocked(g, t, None, plan=plan).view(torch.int32)), "ADD"
    with pytest.raises(ValueError, match="red"):
        ops.reduce_blocked(g, x, "SUM", plan=plan)
    with pytest.raises(ValueError, match="unsupported F=96"):
        ops.reduce_blocked(g, torch.zeros(g.n_cols, 96, device=dev), "MAX", plan=plan)
    with pytest.raises(ValueError, match="unsupported dtype"):
        ops.reduce_blocked(g, x.to(torch.float16), "MAX", plan=plan)
    wide = torch.zeros(g.n_cols, F + 4, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="16-B aligned rows"):
        ops.reduce_blocked(g, wide[:, :F], "MAX", plan=plan)  # bf16 with ldx % 8 != 0
    ip, ix = (a.copy() for a in _graphs()["g5"])
    ix[ip[2]], ix[ip[2] + 1] = 4, 0  # row 2 (400 edges) no longer sorted
    unsorted = G.from_numpy(ip, ix, device=dev)
    with pytest.raises(ValueError, match="sorted"):
        ops.reduce_blocked(unsorted, _table("g5", F, "mixed", dev)[0], "MAX", blocks=2)
    # the raw ABI: a misaligned table is refused (there is no one-item-per-wave twin) and y is not written
    y = torch.zeros(g.n_rows, F, device=dev)
    L = _lib.load()
    for t, dt, off in ((x, _lib.GTA_F32, 4), (xb, _lib.GTA_BF16, 8), (xb, _lib.GTA_BF16, 2)):
        assert _raw(g, t.data_ptr() + off, F, F, dt, y, plan, dev) == _lib.ERR_UNSUPPORTED
        assert b"reduce_blocked" in L.gta_last_error()
    assert _raw(g, x.data_ptr(), F + 2, F, _lib.GTA_F32, y, plan, dev) == _lib.ERR_UNSUPPORTED  # ldx % 4 != 0
    torch.cuda.synchronize(dev)
    assert not bool(y.any()), "a refused call wrote y"
    assert _raw(g, x.data_ptr(), F, F, _lib.GTA_F32, y, plan, dev) == _lib.OK
    assert torch.equal(y, _row_chunked("g900", F, "mixed", False, "MAX", dev))


# ---------------------------------------------------------------------------------------------
# 5. guard bands
# ---------------------------------------------------------------------------------------------

N_GB, E_GB = 130, 3000


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_guard_bands(dev, F, lay, bf):
    """Every tensor a view of one NaN-poisoned arena, plan and workspace of exactly their *_bytes:
    only rows x width of y and the workspace change, and the result is finite and the reference's.
    Layout a has 16-B rows (bf16: 8 padding elements).  Layouts b and c do not (odd pitch; 8-B base):
    the call is refused with GTA_ERR_UNSUPPORTED and writes nothing."""
    L = _lib.load()
    ip, ix = _csr(N_GB, E_GB, 2, sort=True)
    n, nnz = N_GB, len(ix)
    rng = np.random.default_rng(700 + F)
    x = (-1 - np.abs(rng.standard_normal((n, F)))).astype(np.float32)
    ar = Arena(dev, 8 << 20)
    g = _graph_in(ar, ip, ix, n, lay)
    xt = ar.table("x", x, "a8" if bf and lay == "a" else lay, dtype=torch.bfloat16 if bf else torch.float32)
    xw = xt.float().cpu().numpy()
    y = ar.out("y", n, F, "a")
    st = torch.cuda.current_stream(dev).cuda_stream
    for blocks, ie in ((1, 64), (5, 7)):
        pb = int(L.gta_aggregate_blocked_plan_bytes(n, nnz, blocks, ie))
        wsb = int(L.gta_aggregate_blocked_workspace_bytes(n, nnz, blocks, F, ie))
        plan, ws = ar.raw(f"plan{blocks}", pb), ar.raw(f"slabs{blocks}", wsb)
        ar.seal()
        assert L.gta_aggregate_blocked_plan_build(g.indptr.data_ptr(), g.indices.data_ptr(), n, n, nnz, blocks, ie, 0,
                                                  plan.data_ptr(), pb, st) == 0, L.gta_last_error()
        ar.check([plan], "plan build")
        for red, code in (("MAX", _lib.RED_MAX), ("MIN", _lib.RED_MIN)):
            for lean in ((1, 0) if F == 128 else (1,)):
                what = f"reduce_blocked guard F={F} lay={lay} bf16={bf} {red} B={blocks} items={ie} seg_lean={lean}"
                ar.repoison("y")
                ar.seal()
                with _knobs(seg_lean=lean):
                    rc = L.gta_reduce_blocked(code, g.indptr.data_ptr(), g.indices.data_ptr(), n, n, nnz, xt.data_ptr(),
                                              xt.stride(0), F, _lib.GTA_BF16 if bf else _lib.GTA_F32, y.data_ptr(),
                                              y.stride(0), plan.data_ptr(), blocks, ie, ws.data_ptr(), st)
                if lay != "a":
                    assert rc == _lib.ERR_UNSUPPORTED, what
                    ar.check([], what + " (refused)")
                    continue
                assert rc == 0, L.gta_last_error()
                ar.check([ws, y], what)
                got = y.cpu().numpy()
                assert np.isfinite(got).all(), f"{what}: poison was read and used"
                _same(y, reduce_ref.reduce_csr(ip, ix, xw, red, "src"), what)


# ---------------------------------------------------------------------------------------------
# 6. no edges, 7. direction C
# ---------------------------------------------------------------------------------------------

def test_no_edges_writes_zeros_and_never_reads_x(dev):
    n, F = 37, 128
    g = G.from_numpy(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), device=dev)
    for dt in (torch.float32, torch.bfloat16):
        x = torch.full((n, F), float("nan"), dtype=dt, device=dev)
        for red in ("MAX", "MIN", "ADD"):
            y = ops.reduce_blocked(g, x, red, out=torch.full((n, F), 7.0, device=dev), blocks=2)
            assert y.shape == (n, F) and not bool(y.any()), (dt, red)
    y = torch.full((n, F), 7.0, device=dev)
    plan = g.blocked_plan(2)
    L = _lib.load()
    assert L.gta_reduce_blocked(_lib.RED_MAX, g.indptr.data_ptr(), None, n, n, 0, None, 0, F, _lib.GTA_F32, y.data_ptr(), F,
                                plan.buf.data_ptr(), 2, plan.item_edges, None,
                                torch.cuda.current_stream(dev).cuda_stream) == _lib.OK, L.gta_last_error()
    assert not bool(y.any())


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", [64, 128])
def test_direction_c(dev, F, bf):
    """The reduce to the SOURCE nodes over the transposed aggregate's view."""
    ip, ix = _graphs()["g900"]
    g = _dev_graph("g900", dev)
    x, xb, xw = _table("g900", F, "neg", dev)
    view = ops.csc(g).view("dst")
    for red in ("MAX", "MIN"):
        ref = reduce_ref.reduce_csc(ip, ix, g.n_cols, (xw if bf else x).cpu().numpy(), red, "dst")
        for blocks, ie in ((1, 256), (5, 7)):
            y = ops.reduce_blocked(view, xb if bf else x, red, plan=view.blocked_plan(blocks, ie))
            _same(y, ref, f"direction C F={F} bf16={bf} {red} B={blocks}")


# ---------------------------------------------------------------------------------------------
# 8. executor
# ---------------------------------------------------------------------------------------------

N_EX, E_EX = 500, 5000


def _blocked_plans(g):
    return [k for k in g._plans if isinstance(k, tuple) and k[0] == "blocked"]


_EXECUTOR = executor.Executor


def _gated(monkeypatch, **attrs):
    """executor.Executor with the size gate lowered (and attrs set), for every Executor the module
    builds -- run_stream's eager run, the capture's warm-up and the captured run alike."""
    class Gated(_EXECUTOR):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.blocked_min_table_bytes, self.blocked_blocks = 0, 4
            for k, v in attrs.items():
                setattr(self, k, v)

    monkeypatch.setattr(executor, "Executor", Gated)


def _pool(dev, agg):
    g = G.synthetic(N_EX, E_EX, seed=2, device=dev)
    recs, og, stream, sem = pool_layer.layer(N_EX, g.nnz, 128, agg)
    tensors = workloads.make_tensors(og, g, "GraphSAGE", seed=4)
    return g, recs, og, stream, sem, tensors


def _gather_of(og):
    return next(op.idx for op in og.ops if op.type == "gather")


def test_executor_pool_layer_max(dev, monkeypatch):
    """GraphSAGE-pool layer 2 (128 -> 64), MAX: a blocked plan is built, every op's tensor is
    torch.equal to the run with reduce_blocked = False and within tests/test_gpu_reduce.py's bound of
    reduce_ref.layer_ref, and two further calls replay the captured graph with equal outputs."""
    g, recs, og, stream, sem, tensors = _pool(dev, "MAX")
    ip, ix = g.numpy()
    assert all(np.all(np.diff(ix[ip[r]:ip[r + 1]]) >= 0) for r in range(N_EX))
    ref = reduce_ref.layer_ref(recs, sem, ip, ix, {k: v.double().cpu().numpy() for k, v in tensors.items()}, sem.inputs)
    _gated(monkeypatch, reduce_blocked=False)
    ex0 = executor.Executor(og, stream, g, tensors, sem)
    ex0.run()
    assert not _blocked_plans(g)
    off = {i: ex0.tensor_of(i).clone() for i in range(len(og))}
    _gated(monkeypatch)
    executor.clear_auto_graphs()
    try:
        res, ex = executor.run_stream(og, stream, g, tensors, sem)
        assert ex.reduce_blocked and _blocked_plans(g) == [("blocked", 4, ops.BlockedPlan.ITEM_EDGES, ops.BlockedPlan.ROW_EDGES)]
        first = {i: t.clone() for i, t in res.outputs.items()}
        for i in range(len(og)):
            t = ex.tensor_of(i)
            assert torch.equal(t, off[i]), f"op {i} differs from the run with reduce_blocked = False"
            got = t.double().cpu().numpy()
            _, exp, ab = ref[i]
            err, bound = np.abs(got - exp), 1e-5 * ab + 1e-6
            print(f"pool-MAX op {i}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
            assert np.all(err <= bound), f"op {i}: max err {err.max():.3e}, excess {(err - bound).max():.3e}"
        for _ in range(2):  # the second call captures the stream as a HIP graph, the third replays it
            res2, _ = executor.run_stream(og, stream, g, tensors, sem)
            for i, t in first.items():
                assert torch.equal(res2.outputs[i], t), f"replayed output {i} differs"
        ents = [e for e in executor._AUTO.values() if e.refs[0] is og]
        assert ents and all(e.run is not None and not e.failed for e in ents), "the layer was not captured and replayed"
    finally:
        executor.clear_auto_graphs()


def test_executor_pool_layer_max_bf16(dev, monkeypatch):
    """The same layer with gather_dtype = bf16: exactly one cast, and the gather's value is the
    default gather's value rounded to bf16 (rounding commutes with the max)."""
    g, recs, og, stream, sem, tensors = _pool(dev, "MAX")
    _gated(monkeypatch)
    gather = _gather_of(og)
    ex0 = executor.Executor(og, stream, g, tensors, sem)
    ex0.run()
    ex = executor.Executor(og, stream, g, tensors, sem, gather_dtype=torch.bfloat16)
    ex.run()
    assert ex0.gather_casts == 0 and ex.gather_casts == 1
    (src, ver, cast), = ex._gather_cache.values()
    assert src is tensors["x"] and cast.dtype == torch.bfloat16
    _same(ex.tensor_of(gather), ex0.tensor_of(gather).to(torch.bfloat16).float().cpu().numpy(), "bf16 gather")
    assert ex.alg_bytes == ex0.alg_bytes - g.nnz * 128 * 2 + g.n_rows * 128 * 6


def test_executor_pool_layer_mean(dev, monkeypatch):
    """MEAN moves to the blocked aggregate only under gather_dtype = bf16: then the gather is bitwise
    ops.aggregate_blocked of the widened cast table with row_scale = 1 / deg at the same blocks; with
    the option off the route and the bits are the row-chunked aggregate's."""
    g, recs, og, stream, sem, tensors = _pool(dev, "MEAN")
    _gated(monkeypatch)
    gather = _gather_of(og)
    x = tensors["x"]
    scale = executor._mean_scale(g)
    ex0 = executor.Executor(og, stream, g, tensors, sem)
    ex0.run()
    assert not _blocked_plans(g) and ex0.gather_casts == 0
    today = ops.aggregate(g, x, "src", None, row_scale=scale, plan=512)
    assert torch.equal(ex0.tensor_of(gather).view(torch.int32), today.view(torch.int32))
    ex = executor.Executor(og, stream, g, tensors, sem, gather_dtype=torch.bfloat16)
    ex.run()
    assert _blocked_plans(g) and ex.gather_casts == 1
    exp = ops.aggregate_blocked(g, x.to(torch.bfloat16).float(), None, row_scale=scale, blocks=4)
    assert torch.equal(ex.tensor_of(gather).view(torch.int32), exp.view(torch.int32))


def _stock_layer(network, g, agg, reorder):
    for k in range(16):  # the first candidate partition that lowers
        try:
            return pipeline.Layer(network, 2, g, 128, reorder=reorder, aggregator=agg, candidate=k)
        except TypeError:
            continue
    raise AssertionError(f"no candidate of {network} lowers")


@pytest.mark.parametrize("network,agg,reorder", [("PNA", "MIN", True), ("GraphSAGE", "MAX", False)])
def test_executor_stock_layers_keep_their_route(dev, monkeypatch, network, agg, reorder):
    """A tree operand (PNA) or the edge-weight product (GraphSAGE) is an [E, F] tensor: the outputs
    equal the parent route's and no blocked plan is built for the reducer."""
    g = G.synthetic(N_EX, E_EX, seed=2, device=dev)
    lay = _stock_layer(network, g, agg, reorder)
    tensors = workloads.make_tensors(lay.opgraph, g, network, seed=4)
    outs, plans = {}, {}
    for on in (False, True):
        _gated(monkeypatch, reduce_blocked=on)
        ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem)
        assert ex.reduce_blocked is on
        outs[on] = {i: t.clone() for i, t in ex.run().items()}
        plans[on] = sorted(_blocked_plans(g))
    assert plans[True] == plans[False]
    assert set(outs[True]) == set(outs[False])
    for i in outs[False]:
        assert torch.equal(outs[True][i], outs[False][i]), f"{network}-{agg} output {i}"
