"""The grid walk of the weighted 8-head lean blocked aggregate (k_agg_h32<..., GR>, knob seg_grid).

The walk puts an item's 8-edge steps and 32-edge index chunks on the global edge grid instead of at
the item's first edge and masks the edges of its first and last windows that belong to other items.
Lane by lane the edge order and the fma chain are those of the A1 form, so the yardstick everywhere is
bitwise equality with the same call under seg_grid = 0 (compared as int32 bit patterns where a NaN is
expected), and once the fp64 oracle at the bench's bound.  Shapes: F = 128, 8 heads, n_cols = 640.
"""
import contextlib

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops
from oracle import isa_ref

pytestmark = pytest.mark.gpu

F, H, N_COLS = 128, 8, 640
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 39, 40, 41, 63, 64, 65, 72)
LONG = (257, 300, 513)
ROWS_PLAN = (1, 256, 0)  # blocks, item_edges, row_edges: items are rows (cut into parts beyond 256 edges)

_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


@contextlib.contextmanager
def _grid(v):
    old = ops.get_debug("seg_grid")
    try:
        ops.set_debug("seg_grid", v)
        yield
    finally:
        ops.set_debug("seg_grid", old)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _csr():
    """(indptr, indices, starts): for every residue rho of 32 and every L of LENGTHS a filler row that
    brings nnz to rho (mod 32) and then a row of L edges; three long rows; a last row that leaves
    nnz % 8 != 0.  starts[(rho, L)] = the row of that pair."""
    def make():
        deg, starts, nnz = [], {}, 0
        for rho in range(32):
            for L in LENGTHS:
                fill = (rho - nnz) % 32
                deg.append(fill)
                nnz += fill
                starts[(rho, L)] = len(deg)
                deg.append(L)
                nnz += L
        for L in LONG:
            deg.append(L)
            nnz += L
        last = 5 if (nnz + 5) % 8 else 6
        deg.append(last)
        nnz += last
        ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        rng = np.random.default_rng(32)
        ix = np.concatenate([np.sort(rng.integers(0, N_COLS, d)) for d in deg]).astype(np.int32)
        return ip, ix, starts
    return _memo("csr", make)


def _inputs(dev):
    """(graph, x fp32 with bf16-exact values, x bf16, alpha) on the device."""
    def make():
        ip, ix, _ = _csr()
        gen = torch.Generator().manual_seed(128)
        xb = torch.randn(N_COLS, F, generator=gen).to(torch.bfloat16).to(dev)
        w = (torch.rand(len(ix), H, generator=gen) - 0.25).to(dev)
        return G.from_numpy(ip, ix, device=dev, n_cols=N_COLS), xb.float(), xb, w
    return _memo("inputs", make)


def _both(g, x, w, plan_args):
    """(y under seg_grid = 1, y under seg_grid = 0) of the same call."""
    ys = []
    for v in (1, 0):
        with _grid(v):
            ys.append(ops.aggregate_blocked(g, x, w, plan=g.blocked_plan(*plan_args)))
    assert ops.get_debug("seg_grid") == 1
    return ys


def _rows_pair(dev, bf):
    def make():
        g, xf, xb, w = _inputs(dev)
        return _both(g, xb if bf else xf, w, ROWS_PLAN)
    return _memo(("rows", bf), make)


def test_graph_has_every_phase():
    ip, ix, starts = _csr()
    assert ip[-1] == len(ix) and ip[-1] % 32 and ip[-1] % 8
    for (rho, L), r in starts.items():
        assert ip[r] % 32 == rho and ip[r + 1] - ip[r] == L
    assert set(int(b) % 32 for b in ip[:-1]) == set(range(32))
    assert 1300 < len(ip) - 1 < 1400 and 25000 < len(ix) < 35000


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_every_phase_and_short_length(dev, bf):
    """Items are rows: every start residue of 32 with every short length, long rows cut into parts,
    a ragged end of the tensors."""
    y1, y0 = _rows_pair(dev, bf)
    assert torch.isfinite(y0).all()
    assert torch.equal(y1, y0), f"{int((_bits(y1) != _bits(y0)).sum())} elements differ"


def test_bf16_is_the_fp32_twin(dev):
    assert torch.equal(_rows_pair(dev, True)[0], _rows_pair(dev, False)[0])


@pytest.mark.parametrize("item_edges", [7, 256])
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_many_short_items(dev, bf, item_edges):
    g, xf, xb, w = _inputs(dev)
    y1, y0 = _both(g, xb if bf else xf, w, (5, item_edges))
    assert torch.equal(y1, y0), f"{int((_bits(y1) != _bits(y0)).sum())} elements differ"


@pytest.mark.parametrize("plan_args", [ROWS_PLAN, (5, 7)], ids=["rows", "items7"])
def test_foreign_edges_stay_out(dev, plan_args):
    """A row whose alpha is NaN and one whose alpha is +Inf, both inside windows shared with their
    neighbours: no other row sees them."""
    ip, _, starts = _csr()
    g, xf, _, w = _inputs(dev)
    r_nan, r_inf = starts[(13, 9)], starts[(22, 3)]
    wp = w.clone()
    wp[ip[r_nan]:ip[r_nan + 1]] = float("nan")
    wp[ip[r_inf]:ip[r_inf + 1]] = float("inf")
    y1, y0 = _both(g, xf, wp, plan_args)
    assert not bool((_bits(y1) != _bits(y0)).any())
    clean = torch.ones(g.n_rows, dtype=torch.bool, device=dev)
    clean[[r_nan, r_inf]] = False
    assert torch.isfinite(y1[clean]).all()
    assert not torch.isfinite(y1[~clean]).any()
    if plan_args == ROWS_PLAN:  # and the clean rows are what they are without the poison
        assert torch.equal(y1[clean], _rows_pair(dev, False)[0][clean])


@pytest.mark.parametrize("lead,aligned", [(32, True), (1, False)], ids=["aligned", "offset32B"])
def test_ends_of_the_tensors(dev, lead, aligned):
    """alpha and indices as views inside larger poisoned buffers: nothing outside them is used.  lead
    edges of poison in front: 32 keeps both views 128-B aligned (the grid form), 1 puts alpha 32 B off
    (the A1 form runs instead)."""
    ip, ix, _ = _csr()
    g0, xf, _, w = _inputs(dev)
    nnz = len(ix)
    xbig = torch.full((N_COLS + 8, F), float("nan"), device=dev)
    xbig[:N_COLS] = xf
    wbuf = torch.full((lead + nnz + 64, H), float("nan"), device=dev)
    wbuf[lead:lead + nnz] = w
    wv = wbuf[lead:lead + nnz]
    il = 32 if aligned else 8  # int32 entries: 128 B or 32 B
    ibuf = torch.full((il + nnz + 64,), N_COLS + 3, dtype=torch.int32, device=dev)  # a NaN row of xbig, outside the graph
    ibuf[il:il + nnz] = g0.indices
    iv = ibuf[il:il + nnz]
    assert (wv.data_ptr() % 128 == 0) == aligned and (iv.data_ptr() % 128 == 0) == aligned
    assert wv.data_ptr() % 32 == 0 and iv.data_ptr() % 32 == 0
    g = G.Graph(g0.indptr, iv, n_cols=N_COLS)
    assert g.indices.data_ptr() == iv.data_ptr() and g.nnz == nnz
    for plan_args in (ROWS_PLAN, (5, 7)):
        y1, y0 = _both(g, xbig[:N_COLS], wv, plan_args)
        assert torch.isfinite(y1).all(), "poison from outside the views reached y"
        assert torch.equal(y1, y0)
        if plan_args == ROWS_PLAN:
            assert torch.equal(y1, _rows_pair(dev, False)[0])


@pytest.mark.parametrize("plan_args", [ROWS_PLAN, (5,)], ids=["rows", "default5"])
def test_row_chunks(dev, plan_args):
    """The bench's form: a row range of the graph over the whole indices and alpha, into y[a:b]."""
    g, xf, _, w = _inputs(dev)
    cuts = [0, 401, 977, g.n_rows]
    for a, b in zip(cuts[:-1], cuts[1:]):
        gg = G.Graph(g.indptr[a:b + 1], g.indices, n_cols=N_COLS)
        ys = []
        for v in (1, 0):
            y = torch.full((g.n_rows, F), float("nan"), device=dev)
            with _grid(v):
                ops.aggregate_blocked(gg, xf, w, out=y[a:b], plan=gg.blocked_plan(*plan_args))
            assert torch.isnan(y[:a]).all() and torch.isnan(y[b:]).all(), "rows outside the chunk were written"
            ys.append(y[a:b])
        assert torch.equal(ys[0], ys[1]), f"rows [{a}, {b})"
        if plan_args == ROWS_PLAN:
            assert torch.equal(ys[0], _rows_pair(dev, False)[0][a:b])


def test_against_the_oracle(dev):
    ip, ix, _ = _csr()
    _, xf, _, w = _inputs(dev)
    x64, w64 = xf.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
    ref = isa_ref.aggregate(ip, ix, x64, "src", w64)
    bound = 1e-5 * isa_ref.aggregate_abs(ip, ix, x64, "src", w64) + 1e-6
    err = np.abs(_rows_pair(dev, False)[0].cpu().numpy().astype(np.float64) - ref)
    print("grid walk vs oracle: max err / bound =", float((err / bound).max()))
    assert (err <= bound).all(), f"{int((err > bound).sum())} elements past the bound, worst {float((err / bound).max()):.3f}"
