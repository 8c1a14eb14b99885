"""gta_reduce (the gather's MAX / MIN) and the executor's MAX / MIN / MEAN gathers on the GPU.

The graph carries the cases at which k_reduce can go wrong: 300 rows, ~6,000 edges, one row of 700
edges (11 items at chunk 64), 5 empty rows (row 0 among them), a last row with one edge, rows of
exactly 64 and 65 edges.  The first value set is all negative (-1 - |N(0,1)|): a 0 identity, or a
`valid ? t : 0` kept from the sum, shows at once; the second has mixed signs.  A max returns one of
its inputs, so every comparison with tests/reduce_ref.py is by value (`==`), without a tolerance.
"""
import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, executor, graph as G, ops, pipeline, workloads

from . import reduce_ref
from .test_gpu_footprint import CAP, Arena, LAYOUTS, _csr, _graph_in  # names only: no test function

gpu = pytest.mark.gpu

N, HEAVY, R64, R65 = 300, 150, 10, 11
EMPTY = (0, 37, 120, 201, 250)
WIDTHS = [1, 3, 16, 64, 100, 128, 256, 260, 602]  # 260: two vectors per lane (NV 2)
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _graph_np():
    def make():
        rng = np.random.default_rng(7)
        deg = rng.multinomial(5170, np.full(N, 1.0 / N))
        deg[list(EMPTY)] = 0
        deg[HEAVY], deg[R64], deg[R65], deg[-1] = 700, 64, 65, 1
        ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        ix = rng.integers(0, N, int(ip[-1])).astype(np.int32)
        return ip, ix
    return _memo("graph", make)


def _graph(dev):
    ip, ix = _graph_np()
    return _memo(("graph", str(dev)), lambda: G.from_numpy(ip, ix, device=dev))


def _values(F, kind):
    """(x [N, F], xe [E, F]) float32: kind 'neg' = -1 - |N(0,1)|, 'mixed' = N(0,1)."""
    def make():
        ip, ix = _graph_np()
        rng = np.random.default_rng(1000 + F + (0 if kind == "neg" else 1))
        x, xe = rng.standard_normal((N, F)), rng.standard_normal((len(ix), F))
        if kind == "neg":
            x, xe = -1 - np.abs(x), -1 - np.abs(xe)
        return x.astype(np.float32), xe.astype(np.float32)
    return _memo(("values", F, kind), make)


def _ref(F, kind, red, mode):
    def make():
        ip, ix = _graph_np()
        x, xe = _values(F, kind)
        return reduce_ref.reduce_csr(ip, ix, xe if mode == "edge" else x, red, mode)
    return _memo(("ref", F, kind, red, mode), make)


def _same(y, ref, what):
    got = y.detach().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}"


def test_the_graph_has_its_cases():
    ip, _ = _graph_np()
    deg = np.diff(ip)
    assert len(deg) == N and 5500 <= ip[-1] <= 6500
    assert deg[HEAVY] == 700 and deg[R64] == 64 and deg[R65] == 65 and deg[-1] == 1
    assert deg[0] == 0 and (deg == 0).sum() == 5


@gpu
@pytest.mark.parametrize("F", WIDTHS)
def test_widths_and_modes(dev, F):
    g = _graph(dev)
    ip, _ = _graph_np()
    deg = np.diff(ip)
    for kind in ("neg", "mixed"):
        x, xe = _values(F, kind)
        xd, xed = torch.from_numpy(x).to(dev), torch.from_numpy(xe).to(dev)
        for red in ("MAX", "MIN"):
            for mode in ("src", "dst", "edge"):
                for plan in (None, 64):
                    y = ops.reduce(g, xed if mode == "edge" else xd, red, mode, plan=plan)
                    _same(y, _ref(F, kind, red, mode), f"reduce F={F} {kind} {red} {mode} plan={plan}")
                    if mode == "dst":  # every edge of row i reads x[i]
                        assert np.array_equal(y.cpu().numpy(), np.where(deg[:, None] > 0, x, np.float32(0)))


@gpu
def test_odd_leading_dimension_takes_the_scalar_form(dev):
    F = 128
    g = _graph(dev)
    x, xe = _values(F, "neg")
    xb = torch.full((N, F + 1), float("nan"), device=dev)
    xb[:, :F] = torch.from_numpy(x).to(dev)
    xeb = torch.full((len(xe), F + 1), float("nan"), device=dev)
    xeb[:, :F] = torch.from_numpy(xe).to(dev)
    yb = torch.full((N, F + 1), 7.0, device=dev)
    for red in ("MAX", "MIN"):
        for mode, t in (("src", xb[:, :F]), ("edge", xeb[:, :F])):
            assert t.stride(0) == F + 1
            y = ops.reduce(g, t, red, mode, out=yb[:, :F], plan=64)
            _same(y, _ref(F, "neg", red, mode), f"ldx = F + 1 {red} {mode}")
            assert bool((yb[:, F] == 7.0).all())


@gpu
@pytest.mark.parametrize("F", [100, 128])
def test_bf16_rows(dev, F):
    """bf16 node rows are widened exactly: the 16-B piece form (the last lane's piece of F = 100
    clamped inside the row) and the 8-B form give the maxima of the widened values."""
    g = _graph(dev)
    ip, ix = _graph_np()
    for kind in ("neg", "mixed"):
        xb = torch.from_numpy(_values(F, kind)[0]).to(torch.bfloat16)
        wide = xb.float().numpy()
        xd = xb.to(dev)
        for red in ("MAX", "MIN"):
            ref = reduce_ref.reduce_csr(ip, ix, wide, red, "src")
            old = ops.get_debug("agg_bf16_vw8")
            try:
                for vw8 in (old, 0):
                    ops.set_debug("agg_bf16_vw8", vw8)
                    for plan in (None, 64):
                        _same(ops.reduce(g, xd, red, "src", plan=plan), ref, f"bf16 F={F} {kind} {red} vw8={vw8} plan={plan}")
            finally:
                ops.set_debug("agg_bf16_vw8", old)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.reduce(g, torch.zeros(g.nnz, F, dtype=torch.bfloat16, device=dev), "MAX", "edge")


@gpu
@pytest.mark.parametrize("F", [100, 128, 602])
def test_plan_invariance(dev, F):
    g = _graph(dev)
    ip, _ = _graph_np()
    deg = np.diff(ip)
    p64 = g.plan(64)
    assert p64.splits == 2 and p64.n_items() == int(np.where(deg <= 64, 1, -(-deg // 64)).sum())
    assert -(-700 // 64) == 11 and g.plan(512).splits == 1
    x, xe = _values(F, "mixed")
    xd, xed = torch.from_numpy(x).to(dev), torch.from_numpy(xe).to(dev)
    for red in ("MAX", "MIN"):
        for mode in ("src", "edge"):
            t = xed if mode == "edge" else xd
            ys = [ops.reduce(g, t, red, mode, plan=p) for p in (None, 64, 512, p64)]
            assert all(torch.equal(ys[0], y) for y in ys[1:]), f"F={F} {red} {mode}"
    old = ops.get_debug("agg_vw")
    try:  # the vector width does not change the value either
        ys = []
        for vw in (0, 1):
            ops.set_debug("agg_vw", vw)
            ys.append(ops.reduce(g, xd, "MAX", "src", plan=64))
        assert torch.equal(ys[0], ys[1])
    finally:
        ops.set_debug("agg_vw", old)


@gpu
@pytest.mark.parametrize("F", [100, 128])
def test_special_values(dev, F):
    """NaN propagates to exactly its (row, column); an all -inf row gives -inf under MAX (+inf under
    MIN for an all +inf row): the empty-row 0 is decided by the degree, not by the identity."""
    g = _graph(dev)
    ip, ix = _graph_np()
    xe = _values(F, "neg")[1].copy()
    c1, c2 = 5, F - 1
    e_heavy = int(ip[HEAVY]) + 130           # the third item of the heavy row at chunk 64
    e_last = int(ip[-1]) - 1                 # the last row's only edge
    assert ip[N - 1] == e_last
    xe[e_heavy, c1] = np.nan
    xe[e_last, c2] = np.nan
    for red, inf in (("MAX", -np.inf), ("MIN", np.inf)):
        v = xe.copy()
        v[ip[R64]:ip[R64 + 1]] = inf
        ref = reduce_ref.reduce_csr(ip, ix, v, red, "edge")
        want_nan = np.zeros((N, F), bool)
        want_nan[HEAVY, c1] = want_nan[N - 1, c2] = True
        assert np.array_equal(np.isnan(ref), want_nan) and np.all(ref[R64] == inf) and np.all(ref[list(EMPTY)] == 0)
        vd = torch.from_numpy(v).to(dev)
        for plan in (None, 64, 512):
            y = ops.reduce(g, vd, red, "edge", plan=plan)
            got = y.cpu().numpy()
            assert np.array_equal(np.isnan(got), want_nan), f"{red} plan={plan}: NaN at {np.argwhere(np.isnan(got))[:4]}"
            _same(y, ref, f"special values {red} plan={plan}")
            assert np.all(got[R64] == inf) and np.all(got[list(EMPTY)] == 0)
    # through an index too: a NaN node row reaches every row that has an edge from it, nothing else
    x = _values(F, "mixed")[0].copy()
    x[17, c1] = np.nan
    ref = reduce_ref.reduce_csr(ip, ix, x, "MAX", "src")
    rows = np.unique(reduce_ref.rows_of(ip)[ix == 17])
    assert len(rows) and np.array_equal(np.argwhere(np.isnan(ref)), np.stack([rows, np.full_like(rows, c1)], 1))
    _same(ops.reduce(g, torch.from_numpy(x).to(dev), "MAX", "src", plan=64), ref, "NaN node row")


@gpu
def test_empty_graph_and_sum(dev):
    """nnz == 0: an all-zero y, x and indices never read; red ADD is the unweighted aggregate."""
    F = 100
    g0 = G.from_numpy(np.zeros(8, np.int64), np.zeros(0, np.int32), device=dev, n_cols=7)
    y = torch.full((7, F), float("nan"), device=dev)
    L = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    for red in (_lib.RED_MAX, _lib.RED_MIN):
        y.fill_(float("nan"))
        assert L.gta_reduce(red, g0.indptr.data_ptr(), None, 7, 0, _lib.IDX_SRC, None, F, F, _lib.GTA_F32,
                            y.data_ptr(), F, None, 0, None, st) == 0, L.gta_last_error()
        assert bool((y == 0).all())
    g = _graph(dev)
    xd = torch.from_numpy(_values(F, "mixed")[0]).to(dev)
    assert torch.equal(ops.reduce(g, xd, "ADD", "src", plan=64), ops.aggregate(g, xd, "src", plan=64))
    with pytest.raises(ValueError, match="red"):
        ops.reduce(g, xd, "SUM")


@gpu
@pytest.mark.parametrize("F", [16, 128])
def test_direction_c(dev, F):
    """The reduce to the SOURCE nodes: the same kernels over the CSC views."""
    g = _graph(dev)
    ip, ix = _graph_np()
    x, xe = _values(F, "neg")
    xd, xed = torch.from_numpy(x).to(dev), torch.from_numpy(xe).to(dev)
    c = ops.csc(g)
    for red in ("MAX", "MIN"):
        for kind, t, tn in (("edge", xed, xe), ("dst", xd, x), ("src", xd, x)):
            ref = reduce_ref.reduce_csc(ip, ix, N, tn, red, kind)
            for plan in (None, 64):
                _same(ops.reduce(c.view(kind), t, red, "src", plan=plan), ref, f"direction C {red} {kind} plan={plan}")


# ---------------------------------------------------------------------------------- guard bands
N_GB, E_GB = 130, 3000


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("F", [64, 100, 128])
def test_guard_bands(dev, F, lay):
    """Every tensor a view of one NaN-poisoned arena, plan and workspace of exactly *_bytes: only
    rows x width of y (and the workspace) change, and the result is finite and the reference's."""
    assert lay in LAYOUTS
    L = _lib.load()
    chunk = 64
    ip, ix = _csr(N_GB, E_GB, 1)
    n, nnz = len(ip) - 1, len(ix)
    rng = np.random.default_rng(300 + F)
    x = (-1 - np.abs(rng.standard_normal((n, F)))).astype(np.float32)
    xe = (-1 - np.abs(rng.standard_normal((nnz, F)))).astype(np.float32)
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, n, lay)
    pb, wsb = int(L.gta_aggregate_plan_bytes(n, nnz, chunk)), int(L.gta_aggregate_workspace_bytes(n, nnz, chunk, F))
    plan, ws = ar.raw("plan", pb), ar.raw("workspace", wsb)
    xt, xet = ar.table("x", x, lay), ar.table("xe", xe, lay)
    y = ar.out("y", n, F, lay)
    st = torch.cuda.current_stream(dev).cuda_stream
    ar.seal()
    assert L.gta_aggregate_plan_build(g.indptr.data_ptr(), n, nnz, chunk, plan.data_ptr(), pb, st) == 0, L.gta_last_error()
    ar.check([plan], "plan build")
    assert int(plan[8:16].view(torch.int64).item()) >= 1  # the 700-edge row is split
    for red, code in (("MAX", _lib.RED_MAX), ("MIN", _lib.RED_MIN)):
        for mode, t, tn in (("src", xt, x), ("edge", xet, xe), ("dst", xt, x)):
            for use_plan in (False, True):
                what = f"reduce guard F={F} lay={lay} {red} {mode} plan={use_plan}"
                ar.repoison("y")
                ar.repoison("workspace")
                ar.seal()
                rc = L.gta_reduce(code, g.indptr.data_ptr(), g.indices.data_ptr(), n, nnz, ops._MODES[mode], t.data_ptr(),
                                  t.stride(0), F, _lib.GTA_F32, y.data_ptr(), y.stride(0),
                                  plan.data_ptr() if use_plan else None, chunk if use_plan else 0,
                                  ws.data_ptr() if use_plan else None, st)
                assert rc == 0, L.gta_last_error()
                ar.check([ws, y] if use_plan else [y], what)
                got = y.cpu().numpy()
                assert np.isfinite(got).all(), f"{what}: poison was read and used"
                _same(y, reduce_ref.reduce_csr(ip, ix, tn, red, mode), what)


# ------------------------------------------------------------------------------------- executor
def _layer(network, g, agg, reorder):
    for k in range(16):  # the first candidate partition that lowers (as cli.run steps over the others)
        try:
            return pipeline.Layer(network, 2, g, 128, reorder=reorder, aggregator=agg, candidate=k)
        except TypeError:
            continue
    raise AssertionError(f"no candidate of {network} lowers")


@gpu
@pytest.mark.parametrize("network,agg,reorder", [("GraphSAGE", "MAX", False), ("PNA", "MIN", True),
                                                 ("GraphSAGE", "MEAN", False)])
def test_executor_layers(dev, network, agg, reorder):
    """A layer-2 (128 -> 64) layer with the reducer against the fp64 reference, within the project's
    bound |d| <= 1e-5 * sum|terms| + 1e-6 (tests/test_gpu_ops.py), sum|terms| taken through the MM
    that follows (the max itself is exact; a MEAN's summed terms are divided by the degree); then
    the replay of the captured HIP graph gives the same tensors."""
    g = G.synthetic(500, 5000, seed=2, device=dev)
    lay = _layer(network, g, agg, reorder)
    assert [r["COMP_TYPE"] for r in lay.records if r["TYPE"] == "gather"] == [agg]
    tensors = workloads.make_tensors(lay.opgraph, g, network, seed=4)
    ip, ix = g.numpy()
    ref = reduce_ref.layer_ref(lay.records, lay.sem, ip, ix, {k: v.double().cpu().numpy() for k, v in tensors.items()},
                               lay.sem.inputs)
    res, ex = lay.run(tensors)
    first = {i: t.clone() for i, t in res.outputs.items()}
    assert set(first) == {op.idx for op in lay.opgraph.ops if not op.out_list}
    gather = next(op.idx for op in lay.opgraph.ops if op.type == "gather")
    for i, t in list(first.items()) + [(gather, ex.tensor_of(gather))]:
        got = t.double().cpu().numpy()
        _, exp, ab = ref[i]
        err, bound = np.abs(got - exp), 1e-5 * ab + 1e-6
        print(f"{network}-{agg} op {i}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
        assert np.all(err <= bound), f"{network}-{agg} op {i}: max err {err.max():.3e}, excess {(err - bound).max():.3e}"
    for _ in range(2):  # the second call captures the stream as a HIP graph and replays it
        res2, _ = lay.run(tensors)
        for i, t in first.items():
            assert torch.equal(res2.outputs[i], t), f"replayed output {i} differs"
    ents = [e for e in executor._AUTO.values() if e.refs[0] is lay.opgraph]
    assert ents and all(e.run is not None and not e.failed for e in ents), "the layer was not captured and replayed"
