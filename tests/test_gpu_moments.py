"""gta_reduce_multi (MEAN / MAX / MIN / VAR / STD in one pass) and the executor's VAR / STD and
sibling gathers on the GPU.

The graph is tests/test_gpu_reduce.py's recipe, restated: 300 rows, ~5.9 k edges, one row of 700
edges (11 items at chunk 64, 2 at 512), 5 empty rows (row 0 among them), a last row with one edge,
rows of exactly 64 and 65 edges (at chunk 64 the second is split, the first is not).  MAX / MIN are
compared with ops.reduce by value; the moments with tests/moments_ref.py's fp64 two-pass values,
within the project's bound 1e-5 * sum|terms| + 1e-6 applied to the shifted form (moments_ref's
module text)."""
import itertools

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, executor, graph as G, ops, pipeline, workloads

from . import moments_ref, reduce_ref
from .test_gpu_footprint import CAP, Arena, LAYOUTS, _csr, _graph_in  # names only: no test function

gpu = pytest.mark.gpu

N, HEAVY, R64, R65 = 300, 150, 10, 11
EMPTY = (0, 37, 120, 201, 250)
WIDTHS = [1, 3, 16, 64, 100, 128, 256, 260, 602]
PLANS = (None, 64, 512)
ALL = ("MEAN", "MAX", "MIN", "VAR", "STD")
PNA4 = ("MEAN", "MAX", "MIN", "STD")
EPS = 1e-5
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def graph_np():
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
    ip, ix = graph_np()
    return _memo(("graph", str(dev)), lambda: G.from_numpy(ip, ix, device=dev))


def values(F):
    """(x [N, F], xe [E, F]) float32 ~ N(0, 1)."""
    def make():
        ip, ix = graph_np()
        rng = np.random.default_rng(2000 + F)
        return rng.standard_normal((N, F)).astype(np.float32), rng.standard_normal((len(ix), F)).astype(np.float32)
    return _memo(("values", F), make)


def cancel_values(F):
    """(x, xe) float32 = 1000 + N(0, 1): |mean| = 1000 std, where E[x^2] - E[x]^2 has no digit left in fp32."""
    def make():
        ip, ix = graph_np()
        rng = np.random.default_rng(3000 + F)
        return ((1000 + rng.standard_normal((N, F))).astype(np.float32),
                (1000 + rng.standard_normal((len(ix), F))).astype(np.float32))
    return _memo(("cancel", F), make)


def _ref(key, t, mode):
    """{"MEAN" | "VAR" | "STD": (fp64 value, bound)} of the float32 operand t, computed once per key."""
    ip, ix = graph_np()
    return _memo(("ref", key, mode), lambda: moments_ref.moments_csr(ip, ix, t.astype(np.float64), mode, EPS))


def _within(y, ref, red, what):
    got = y.detach().cpu().numpy()
    exp, bound = ref[red]
    assert got.dtype == np.float32 and got.shape == exp.shape, what
    err = np.abs(got.astype(np.float64) - exp)
    bad = ~(err <= bound)  # (a NaN fails)
    assert not bad.any(), (f"{what} {red}: {int(bad.sum())} of {bad.size} outside the bound, first at "
                           f"{tuple(np.argwhere(bad)[0])}: err {err[bad][0]:.3e} bound {bound[bad][0]:.3e}")
    return float((err / bound).max())


def _check_all(ys, reds, ref, g, t, mode, plan, what):
    """ys (in reds order): MAX / MIN torch.equal to ops.reduce, the moments within their bounds,
    rows without edges exactly 0."""
    for red, y in zip(reds, ys):
        if red in ("MAX", "MIN"):
            assert torch.equal(y, ops.reduce(g, t, red, mode, plan=plan)), f"{what} {red} differs from ops.reduce"
        else:
            _within(y, ref, red, what)
        assert bool((y[list(EMPTY)] == 0).all()), f"{what} {red}: a row without edges is not 0"


def test_the_graph_has_its_cases():
    ip, _ = graph_np()
    deg = np.diff(ip)
    assert len(deg) == N and 5500 <= ip[-1] <= 6500
    assert deg[HEAVY] == 700 and deg[R64] == 64 and deg[R65] == 65 and deg[-1] == 1
    assert deg[0] == 0 and (deg == 0).sum() == 5


# ------------------------------------------------------------------------------ (a) widths, modes
@gpu
@pytest.mark.parametrize("F", WIDTHS)
def test_widths_and_modes(dev, F):
    g = _graph(dev)
    assert g.plan(64).splits == 2 and g.plan(512).splits == 1
    x, xe = values(F)
    xd, xed = torch.from_numpy(x).to(dev), torch.from_numpy(xe).to(dev)
    for mode in ("src", "dst", "edge"):
        tn, t = (xe, xed) if mode == "edge" else (x, xd)
        ref = _ref(("values", F), tn, mode)
        for plan in PLANS:
            ys = ops.reduce_multi(g, t, ALL, mode, plan=plan)
            assert len(ys) == 5 and all(y.shape == (N, F) and y.dtype == torch.float32 for y in ys)
            _check_all(ys, ALL, ref, g, t, mode, plan, f"reduce_multi F={F} {mode} plan={plan}")


@gpu
@pytest.mark.parametrize("F", [100, 128])
def test_every_one_and_two_member_subset(dev, F):
    """The three kernel specialisations (moments, extrema, both) and the order of the outputs."""
    g = _graph(dev)
    x, xe = values(F)
    xd, xed = torch.from_numpy(x).to(dev), torch.from_numpy(xe).to(dev)
    subsets = [(a,) for a in ALL] + list(itertools.permutations(ALL, 2))
    assert len(subsets) == 25
    for mode, tn, t in (("src", x, xd), ("edge", xe, xed)):
        ref = _ref(("values", F), tn, mode)
        for plan in (None, 64):
            full = dict(zip(ALL, ops.reduce_multi(g, t, ALL, mode, plan=plan)))
            for reds in subsets:
                ys = ops.reduce_multi(g, t, reds, mode, plan=plan)
                assert len(ys) == len(reds)
                _check_all(ys, reds, ref, g, t, mode, plan, f"subset {reds} F={F} {mode} plan={plan}")
                for red, y in zip(reds, ys):  # the same arithmetic whatever else the launch fills
                    assert torch.equal(y, full[red]), f"subset {reds} F={F} {mode} plan={plan}: {red} differs from the full call"


# ------------------------------------------------------------------------------ (b) cancellation
@gpu
@pytest.mark.parametrize("F", [128, 100])
def test_cancellation(dev, F):
    """x = 1000 + N(0, 1): the shifted sums keep VAR and STD inside the bound (the naive form does
    not: tests/test_moments_cpu.py shows it on this data)."""
    g = _graph(dev)
    x, xe = cancel_values(F)
    xd, xed = torch.from_numpy(x).to(dev), torch.from_numpy(xe).to(dev)
    for mode, tn, t in (("src", x, xd), ("edge", xe, xed)):
        ref = _ref(("cancel", F), tn, mode)
        assert 0.5 < np.median(ref["VAR"][0][np.diff(graph_np()[0]) > 8]) < 2 and np.all(ref["VAR"][1] < 1e-3)
        for plan in PLANS:
            ys = dict(zip(ALL, ops.reduce_multi(g, t, ALL, mode, plan=plan)))
            for red in ("MEAN", "VAR", "STD"):
                worst = _within(ys[red], ref, red, f"cancellation F={F} {mode} plan={plan}")
                print(f"cancellation F={F} {mode} plan={plan} {red}: max err / bound {worst:.3f}")


# --------------------------------------------------------------------------------------- (c) bf16
@gpu
@pytest.mark.parametrize("F", [36, 100, 128])
def test_bf16_tables(dev, F):
    """bf16 node rows are widened exactly: bitwise the fp32 call on x.float() (F = 36 and 100: the
    last 16-B piece of the extrema's bf16 form is clamped inside the row)."""
    g = _graph(dev)
    xb = torch.from_numpy(values(F)[0]).to(torch.bfloat16).to(dev)
    wide = xb.float()
    old = ops.get_debug("agg_bf16_vw8")
    try:
        for vw8 in (old, 0):
            ops.set_debug("agg_bf16_vw8", vw8)
            for mode in ("src", "dst"):
                for plan in (None, 64):
                    for reds in (ALL, ("MAX", "MIN"), ("STD",)):
                        got = ops.reduce_multi(g, xb, reds, mode, plan=plan)
                        want = ops.reduce_multi(g, wide, reds, mode, plan=plan)
                        for red, a, b in zip(reds, got, want):
                            assert torch.equal(a, b), f"bf16 F={F} {mode} plan={plan} vw8={vw8} {reds}: {red} differs"
    finally:
        ops.set_debug("agg_bf16_vw8", old)
    ref = _memo(("bf16ref", F), lambda: moments_ref.moments_csr(*graph_np(), wide.cpu().numpy().astype(np.float64), "src", EPS))
    _check_all(ops.reduce_multi(g, xb, ALL, "src", plan=64), ALL, ref, g, xb, "src", 64, f"bf16 F={F}")
    with pytest.raises(TypeError, match="bfloat16"):
        ops.reduce_multi(g, torch.zeros(g.nnz, F, dtype=torch.bfloat16, device=dev), ALL, "edge")
    L = _lib.load()
    ys = (torch.empty(N, F, device=dev),)
    arr, lds = (np.array([ys[0].data_ptr()], np.uint64), np.array([F], np.int64))
    rc = L.gta_reduce_multi(_lib.MR_STD, g.indptr.data_ptr(), g.indices.data_ptr(), N, g.nnz, _lib.IDX_EDGE,
                            xb.data_ptr(), F, F, _lib.GTA_BF16, arr.ctypes.data, lds.ctypes.data, EPS, None, 0, None,
                            torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _lib.ERR_UNSUPPORTED


# -------------------------------------------------------------------------------- (d) determinism
@gpu
@pytest.mark.parametrize("F", [100, 128, 602])
def test_determinism_and_plans(dev, F):
    g = _graph(dev)
    x, xe = values(F)
    xd, xed = torch.from_numpy(x).to(dev), torch.from_numpy(xe).to(dev)
    for mode, tn, t in (("src", x, xd), ("edge", xe, xed)):
        ref = _ref(("values", F), tn, mode)
        by_plan = {}
        for plan in PLANS + (g.plan(64),):
            a = ops.reduce_multi(g, t, ALL, mode, plan=plan)
            b = ops.reduce_multi(g, t, ALL, mode, plan=plan)
            assert all(torch.equal(u, v) for u, v in zip(a, b)), f"F={F} {mode} plan={plan}: two calls differ"
            by_plan[plan] = dict(zip(ALL, a))
        for plan in (64, 512):
            for red in ("MAX", "MIN"):
                assert torch.equal(by_plan[plan][red], by_plan[None][red]), f"F={F} {mode} {red} plan={plan}"
            for red in ("MEAN", "VAR", "STD"):  # the split rows' sums are grouped by item: within the bound
                _within(by_plan[plan][red], ref, red, f"F={F} {mode} plan={plan}")
                rows = [i for i in range(N) if i not in (HEAVY,) + ((R65,) if plan == 64 else ())]
                assert torch.equal(by_plan[plan][red][rows], by_plan[None][red][rows]), "a row in one item moved"
        assert all(torch.equal(by_plan[64][r], by_plan[g.plan(64)][r]) for r in ALL)


# ----------------------------------------------------------------------------- (e) special values
@gpu
@pytest.mark.parametrize("F", [100, 128])
def test_special_values(dev, F):
    g = _graph(dev)
    ip, ix = graph_np()
    xe = values(F)[1].copy()
    c1, c2 = 5, F - 1
    e_heavy = int(ip[HEAVY]) + 130           # the third item of the heavy row at chunk 64
    e_last = int(ip[-1]) - 1                 # the last row's only edge
    assert ip[N - 1] == e_last
    xe[e_heavy, c1] = np.nan
    xe[ip[R64]:ip[R64 + 1]] = np.linspace(-3, 900, F).astype(np.float32)  # a row of identical values per column
    want_nan = np.zeros((N, F), bool)
    want_nan[HEAVY, c1] = True
    last = xe[e_last].copy()
    xed = torch.from_numpy(xe).to(dev)
    sqrt_eps = np.sqrt(np.float32(EPS), dtype=np.float32)
    assert sqrt_eps == np.float32(np.sqrt(np.float64(np.float32(EPS))))  # sqrt(eps) rounded to fp32
    for plan in PLANS:
        ys = dict(zip(ALL, ops.reduce_multi(g, xed, ALL, "edge", plan=plan, std_eps=EPS)))
        for red, y in ys.items():
            got = y.cpu().numpy()
            assert np.array_equal(np.isnan(got), want_nan), f"{red} plan={plan}: NaN at {np.argwhere(np.isnan(got))[:4]}"
            assert np.isfinite(got[~want_nan]).all()
        assert bool((ys["VAR"][R64] == 0).all()), "a row of identical values has VAR exactly 0"
        assert np.array_equal(ys["STD"][R64].cpu().numpy(), np.full(F, sqrt_eps, np.float32))
        assert np.array_equal(ys["MEAN"][R64].cpu().numpy(), xe[ip[R64]])
        assert np.array_equal(ys["MEAN"][N - 1].cpu().numpy().view(np.uint32), last.view(np.uint32)), "degree 1: MEAN is the value"
        assert bool((ys["VAR"][N - 1] == 0).all()) and bool((ys["MAX"][N - 1] == ys["MIN"][N - 1]).all())
    # through an index: a NaN node row reaches every row that has an edge from it, in all five, nothing else
    x = values(F)[0].copy()
    x[17, c2] = np.nan
    rows = np.unique(reduce_ref.rows_of(ip)[ix == 17])
    want = np.zeros((N, F), bool)
    want[rows, c2] = True
    for y in ops.reduce_multi(g, torch.from_numpy(x).to(dev), ALL, "src", plan=64):
        assert np.array_equal(np.isnan(y.cpu().numpy()), want)
    # +-inf: the moment outputs of its (row, column) are NaN, MAX / MIN follow ops.reduce
    v = values(F)[1].copy()
    v[e_heavy, c1], v[int(ip[R65]) + 3, c2] = np.inf, -np.inf
    vd = torch.from_numpy(v).to(dev)
    want = np.zeros((N, F), bool)
    want[HEAVY, c1] = want[R65, c2] = True
    for plan in (None, 64):
        ys = dict(zip(ALL, ops.reduce_multi(g, vd, ALL, "edge", plan=plan)))
        for red in ("MEAN", "VAR", "STD"):
            assert np.array_equal(np.isnan(ys[red].cpu().numpy()), want), f"inf {red} plan={plan}"
        for red in ("MAX", "MIN"):
            assert torch.equal(ys[red], ops.reduce(g, vd, red, "edge", plan=plan))


@gpu
def test_empty_graph_and_refusals(dev):
    """nnz == 0: every output all zero, x and indices never read; the Python refusals."""
    F = 100
    g0 = G.from_numpy(np.zeros(8, np.int64), np.zeros(0, np.int32), device=dev, n_cols=7)
    y = torch.full((7, 5 * F), float("nan"), device=dev)
    ptrs = np.array([y.data_ptr() + 4 * k * F for k in range(5)], np.uint64)
    lds = np.full(5, 5 * F, np.int64)
    L = _lib.load()
    rc = L.gta_reduce_multi(31, g0.indptr.data_ptr(), None, 7, 0, _lib.IDX_SRC, None, F, F, _lib.GTA_F32,
                            ptrs.ctypes.data, lds.ctypes.data, EPS, None, 0, None, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, L.gta_last_error()
    assert bool((y == 0).all())
    g = _graph(dev)
    xd = torch.from_numpy(values(F)[0]).to(dev)
    with pytest.raises(ValueError, match="reds"):
        ops.reduce_multi(g, xd, ("MEAN", "MEAN"))
    with pytest.raises(ValueError, match="reds"):
        ops.reduce_multi(g, xd, ("SUM",))
    with pytest.raises(ValueError, match="out"):
        ops.reduce_multi(g, xd, ALL, out=torch.empty(N, 4 * F, device=dev))
    with pytest.raises(_lib.GTAError):
        ops.reduce_multi(g, xd.cpu(), ALL)


# -------------------------------------------------------------------------- (f) strided outputs
@gpu
@pytest.mark.parametrize("F", [3, 100, 128])
def test_strided_outputs(dev, F):
    """One [N, 5F] table (PNA's concatenation) and padded views, each output with its own row
    stride: columns beyond a block keep the sentinel.  Strides that keep the plain call's vector
    width give its bits (the edge slots depend on F and the alignment only); odd strides take the
    scalar form, whose moments are checked against the reference."""
    g = _graph(dev)
    x, _ = values(F)
    xd = torch.from_numpy(x).to(dev)
    ref = _ref(("values", F), x, "src")
    for plan in (None, 64):
        plain = ops.reduce_multi(g, xd, ALL, "src", plan=plan)
        spare = 4 if F % 4 == 0 else 2
        table = torch.full((N, 5 * F + spare), 7.0, device=dev)
        views = ops.reduce_multi(g, xd, ALL, "src", out=table[:, :5 * F], plan=plan)
        for k, (v, p) in enumerate(zip(views, plain)):
            assert v.data_ptr() == table.data_ptr() + 4 * k * F and v.stride(0) == 5 * F + spare
            assert torch.equal(v, p) and torch.equal(table[:, k * F:(k + 1) * F], p)
        assert bool((table[:, 5 * F:] == 7.0).all())
        for step in (4, 1):  # each output its own stride: aligned as the plain outputs are, then odd
            pads = [torch.full((N, F + step * (k + 1)), 7.0, device=dev) for k in range(5)]
            outs = ops.reduce_multi(g, xd, ALL, "src", outs=[p[:, :F] for p in pads], plan=plan)
            _check_all(outs, ALL, ref, g, xd, "src", plan, f"padded outputs F={F} step={step} plan={plan}")
            for k, (o, p) in enumerate(zip(outs, plain)):
                assert o.data_ptr() == pads[k].data_ptr() and o.stride(0) == F + step * (k + 1)
                assert torch.equal(o, p) or (step == 1 and ALL[k] not in ("MAX", "MIN")), f"output {k} step={step}"
                assert bool((pads[k][:, F:] == 7.0).all()), f"output {k}: a column beyond its block changed"
        rev = ops.reduce_multi(g, xd, ALL[::-1], "src", plan=plan)  # reds order, not bit order
        assert all(torch.equal(a, b) for a, b in zip(rev, plain[::-1]))


N_GB, E_GB = 130, 3000


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("F", [64, 100, 128])
def test_guard_bands(dev, F, lay):
    """Every tensor a view of one NaN-poisoned arena, plan and workspace of exactly *_bytes (the
    workspace: P * F = 4 F columns): only rows x width of the five outputs (and the workspace)
    change, and the results are finite and the reference's."""
    assert lay in LAYOUTS
    L = _lib.load()
    chunk = 64
    ip, ix = _csr(N_GB, E_GB, 1)
    n, nnz = len(ip) - 1, len(ix)
    rng = np.random.default_rng(400 + F)
    x = rng.standard_normal((n, F)).astype(np.float32)
    xe = rng.standard_normal((nnz, F)).astype(np.float32)
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, n, lay)
    pb = int(L.gta_aggregate_plan_bytes(n, nnz, chunk))
    wsb = int(L.gta_aggregate_workspace_bytes(n, nnz, chunk, ops.reduce_multi_planes(ALL) * F))
    assert wsb == 4 * int(L.gta_aggregate_workspace_bytes(n, nnz, chunk, F))
    plan, ws = ar.raw("plan", pb), ar.raw("workspace", wsb)
    xt, xet = ar.table("x", x, lay), ar.table("xe", xe, lay)
    ys = [ar.out(f"y{k}", n, F, lay) for k in range(5)]
    ptrs = np.array([y.data_ptr() for y in ys], np.uint64)
    lds = np.array([y.stride(0) for y in ys], np.int64)
    st = torch.cuda.current_stream(dev).cuda_stream
    ar.seal()
    assert L.gta_aggregate_plan_build(g.indptr.data_ptr(), n, nnz, chunk, plan.data_ptr(), pb, st) == 0, L.gta_last_error()
    ar.check([plan], "plan build")
    assert int(plan[8:16].view(torch.int64).item()) >= 1  # the 700-edge row is split
    for mode, t, tn in (("src", xt, x), ("edge", xet, xe), ("dst", xt, x)):
        ref = moments_ref.moments_csr(ip, ix, tn.astype(np.float64), mode, EPS)
        for use_plan in (False, True):
            what = f"reduce_multi guard F={F} lay={lay} {mode} plan={use_plan}"
            for k in range(5):
                ar.repoison(f"y{k}")
            ar.repoison("workspace")
            ar.seal()
            rc = L.gta_reduce_multi(31, g.indptr.data_ptr(), g.indices.data_ptr(), n, nnz, ops._MODES[mode], t.data_ptr(),
                                    t.stride(0), F, _lib.GTA_F32, ptrs.ctypes.data, lds.ctypes.data, EPS,
                                    plan.data_ptr() if use_plan else None, chunk if use_plan else 0,
                                    ws.data_ptr() if use_plan else None, st)
            assert rc == 0, L.gta_last_error()
            ar.check(([ws] if use_plan else []) + ys, what)
            for red, y in zip(ALL, ys):
                got = y.cpu().numpy()
                assert np.isfinite(got).all(), f"{what} {red}: poison was read and used"
                if red in ("MAX", "MIN"):
                    assert np.array_equal(got, reduce_ref.reduce_csr(ip, ix, tn, red, mode)), f"{what} {red}"
                else:
                    _within(y, ref, red, what)


# ------------------------------------------------------------------------------- (g) direction C
@gpu
@pytest.mark.parametrize("F", [16, 128])
def test_direction_c(dev, F):
    """The reducers to the SOURCE nodes: the same kernels over the CSC views."""
    g = _graph(dev)
    ip, ix = graph_np()
    x, xe = values(F)
    xd, xed = torch.from_numpy(x).to(dev), torch.from_numpy(xe).to(dev)
    c = ops.csc(g)
    for kind, t, tn in (("edge", xed, xe), ("dst", xd, x), ("src", xd, x)):
        ref = moments_ref.moments_csc(ip, ix, N, tn.astype(np.float64), kind, EPS)
        for plan in (None, 64):
            ys = ops.reduce_multi(c.view(kind), t, ALL, "src", plan=plan)
            for red, y in zip(ALL, ys):
                what = f"direction C {kind} F={F} plan={plan}"
                if red in ("MAX", "MIN"):
                    assert torch.equal(y, ops.reduce(c.view(kind), t, red, "src", plan=plan)), f"{what} {red}"
                    assert np.array_equal(y.cpu().numpy(), reduce_ref.reduce_csc(ip, ix, N, tn, red, kind)), f"{what} {red}"
                else:
                    _within(y, ref, red, what)


# ------------------------------------------------------------------------------------- executor
def _layer(network, g, agg, reorder):
    for k in range(16):  # the first candidate partition that lowers (as cli.run steps over the others)
        try:
            return pipeline.Layer(network, 2, g, 128, reorder=reorder, aggregator=agg, candidate=k)
        except TypeError:
            continue
    raise AssertionError(f"no candidate of {network} lowers")


def _layer_ref(lay, g, tensors):
    ip, ix = g.numpy()
    return moments_ref.layer_ref(lay.records, lay.sem, ip, ix, {k: v.double().cpu().numpy() for k, v in tensors.items()},
                                 lay.sem.inputs)


def _check_ops(ex, ref, idxs, what):
    for i in idxs:
        got = ex.tensor_of(i).double().cpu().numpy()
        _, exp, ab = ref[i]
        err, bound = np.abs(got - exp), 1e-5 * ab + 1e-6
        print(f"{what} op {i}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
        assert np.all(err <= bound), f"{what} op {i}: max err {err.max():.3e}, excess {(err - bound).max():.3e}"


@gpu
@pytest.mark.parametrize("network,agg,reorder", [("GraphSAGE", "STD", False), ("GraphSAGE", "VAR", False),
                                                 ("PNA", "STD", True), ("PNA", "VAR", False)])
def test_executor_single_moment_gather(dev, network, agg, reorder):
    """(h) A layer-2 (128 -> 64) layer on a Cora-sized graph whose gather is VAR / STD: every op
    against the fp64 walk, within the project's bound carried through the ops that follow."""
    g = _memo(("cora", str(dev)), lambda: G.synthetic(2708, 10556, seed=2, device=dev))
    lay = _layer(network, g, agg, reorder)
    assert [r["COMP_TYPE"] for r in lay.records if r["TYPE"] == "gather"] == [agg]
    tensors = workloads.make_tensors(lay.opgraph, g, network, seed=4)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem)
    outs = ex.run()
    assert set(outs) == {op.idx for op in lay.opgraph.ops if not op.out_list}
    _check_ops(ex, _layer_ref(lay, g, tensors), range(len(lay.opgraph)), f"{network}-{agg}")


class _Spy:
    """Counts the gather-shaped launches the executor makes through ops."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("reduce_multi", "reduce", "aggregate", "reduce_blocked", "aggregate_blocked"):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def call(*a, **kw):
            self.calls.append((name, tuple(a[2]) if name == "reduce_multi" else (a[2] if name.startswith("reduce") else None)))
            return fn(*a, **kw)
        return call


def _pna4(dev, reorder):
    g = _memo(("cora", str(dev)), lambda: G.synthetic(2708, 10556, seed=2, device=dev))
    lay = pipeline.Layer("PNA", 2, g, 128, reorder=reorder, aggregator=PNA4)
    tensors = workloads.make_tensors(lay.opgraph, g, "PNA", seed=6)
    for j in range(4):  # PNA's scalers, one per aggregator
        tensors[f"ext:{12 + j}:1"] = torch.full((1, 1), 0.5 + 0.25 * j, device=dev)
    return g, lay, tensors


@gpu
@pytest.mark.parametrize("reorder", [False, True])
def test_executor_tuple_aggregator_one_launch(dev, reorder, monkeypatch):
    """(i) PNA with ("MEAN", "MAX", "MIN", "STD"): the four sibling gathers come from exactly one
    gta_reduce_multi launch (k_reduce_multi) and no gta_reduce / gta_aggregate gather; with
    multi_reduce=False from four launches, MAX / MIN equal and the rest within the bound; every op,
    the layer's output among them, within the propagated bound of the fp64 walk."""
    g, lay, tensors = _pna4(dev, reorder)
    assert [r["COMP_TYPE"] for r in lay.records if r["TYPE"] == "gather"] == list(PNA4)
    ref = _layer_ref(lay, g, tensors)
    spy = _Spy(monkeypatch)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem)
    ex.trace = True
    outs = ex.run()
    assert spy.calls == [("reduce_multi", PNA4)], spy.calls
    by_op = {e["args"]["op"]: e["args"]["launches"] for e in ex.trace_events}
    assert [by_op[i] for i in (8, 9, 10, 11)] == [1, 0, 0, 0]
    assert set(outs) == {22}
    _check_ops(ex, ref, range(len(lay.opgraph)), f"PNA4 reorder={reorder} one launch")
    one = {i: ex.tensor_of(i).clone() for i in (8, 9, 10, 11, 22)}

    del spy.calls[:]
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, multi_reduce=False)
    ex.run()
    assert spy.calls == [("aggregate", None), ("reduce", "MAX"), ("reduce", "MIN"), ("reduce_multi", ("STD",))], spy.calls
    _check_ops(ex, ref, range(len(lay.opgraph)), f"PNA4 reorder={reorder} four launches")
    assert torch.equal(ex.tensor_of(9), one[9]) and torch.equal(ex.tensor_of(10), one[10])
    assert torch.equal(ex.tensor_of(11), one[11])  # STD: the same kernel arithmetic with one member


@gpu
def test_executor_tuple_aggregator_replays_as_a_hip_graph(dev):
    """(j) The same layer through Layer.run: the second call captures the stream as a HIP graph (the
    host arrays of gta_reduce_multi are read during the call, nothing in it syncs) and replays it."""
    g, lay, tensors = _pna4(dev, False)
    res, ex = lay.run(tensors)
    first = {i: t.clone() for i, t in res.outputs.items()}
    _check_ops(ex, _layer_ref(lay, g, tensors), [22], "PNA4 Layer.run")
    for _ in range(2):
        res2, _ = lay.run(tensors)
        for i, t in first.items():
            assert torch.equal(res2.outputs[i], t), f"replayed output {i} differs"
    ents = [e for e in executor._AUTO.values() if e.refs[0] is lay.opgraph]
    assert ents and all(e.run is not None and not e.failed for e in ents), "the layer was not captured and replayed"
