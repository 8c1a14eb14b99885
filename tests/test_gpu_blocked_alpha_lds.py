"""The grid walk with its weights staged in LDS a chunk ahead (k_agg_h32<..., GR, AL>, knob seg_alpha_lds).

Same weights, per-lane edge order and fma chain as the grid walk, so the yardstick is bitwise equality
(torch.equal; int32 bit patterns where a NaN is expected) of the same call under seg_alpha_lds = 1 and
= 0.  What can go wrong is the staging: a lane slot of the wrong edge, a buffer read before it landed
or after it was refilled, a neighbour's or a stale weight entering a sum, a byte of alpha outside the
tensor read.  Shapes: F = 128, 8 heads, n_cols = 640, ~33 k edges.
"""
import contextlib

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops

pytestmark = pytest.mark.gpu

F, H, N_COLS = 128, 8, 640
LENGTHS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256)
LONG = (600, 777)  # rows cut into 256-edge items: >= 3 chunks each, so both LDS buffers are refilled
ROWS_PLAN = (1, 256, 0)  # blocks, item_edges, row_edges: items are rows (cut into parts beyond 256 edges)

_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


@contextlib.contextmanager
def _alpha_lds(v):
    old = ops.get_debug("seg_alpha_lds")
    try:
        ops.set_debug("seg_alpha_lds", v)
        yield
    finally:
        ops.set_debug("seg_alpha_lds", old)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _csr():
    """(indptr, indices, starts): for every residue rho of 32 and every L of LENGTHS a filler row that
    brings nnz to rho (mod 32) and then a row of L edges; the LONG rows; a last row that ends at nnz
    with nnz % 8 != 0.  starts[(rho, L)] = the row of that pair."""
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
        rng = np.random.default_rng(950)
        ix = np.concatenate([np.sort(rng.integers(0, N_COLS, d)) for d in deg]).astype(np.int32)
        return ip, ix, starts
    return _memo("csr", make)


def _inputs(dev):
    """(graph, x fp32 with bf16-exact values, x bf16, alpha [nnz, 8] with nothing after it)."""
    def make():
        ip, ix, _ = _csr()
        gen = torch.Generator().manual_seed(128)
        xb = torch.randn(N_COLS, F, generator=gen).to(torch.bfloat16).to(dev)
        w = (torch.rand(len(ix), H, generator=gen) - 0.25).to(dev)
        return G.from_numpy(ip, ix, device=dev, n_cols=N_COLS), xb.float(), xb, w
    return _memo("inputs", make)


def _both(g, x, w, plan_args):
    """(y under seg_alpha_lds = 1, y under seg_alpha_lds = 0) of the same call."""
    default = ops.get_debug("seg_alpha_lds")
    ys = []
    for v in (1, 0):
        with _alpha_lds(v):
            ys.append(ops.aggregate_blocked(g, x, w, plan=g.blocked_plan(*plan_args)))
    assert ops.get_debug("seg_alpha_lds") == default
    return ys


def _rows_pair(dev, bf):
    def make():
        g, xf, xb, w = _inputs(dev)
        return _both(g, xb if bf else xf, w, ROWS_PLAN)
    return _memo(("rows", bf), make)


def _same(y1, y0):
    assert not bool((_bits(y1) != _bits(y0)).any()), f"{int((_bits(y1) != _bits(y0)).sum())} elements differ"


def test_graph_has_every_case():
    ip, ix, starts = _csr()
    assert ip[-1] == len(ix) and ip[-1] % 8
    assert len(starts) == 32 * len(LENGTHS)
    for (rho, L), r in starts.items():
        assert ip[r] % 32 == rho and ip[r + 1] - ip[r] == L
    assert all(L > 2 * 256 + 32 for L in LONG)
    assert len(ip) - 1 < 800 and len(ix) < 100_000


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_every_residue_and_length(dev, bf):
    """Items are rows: every start residue of 32 with every length, rows cut into several 256-edge
    items, the last item ending exactly at nnz with no alpha after it."""
    y1, y0 = _rows_pair(dev, bf)
    assert torch.isfinite(y0).all()
    assert torch.equal(y1, y0), f"{int((_bits(y1) != _bits(y0)).sum())} elements differ"


def test_bf16_is_the_fp32_twin(dev):
    assert torch.equal(_rows_pair(dev, True)[0], _rows_pair(dev, False)[0])


@pytest.mark.parametrize("item_edges", [7, 256])
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_column_blocks(dev, bf, item_edges):
    """Five column blocks: many short items that start and end anywhere on the grid."""
    g, xf, xb, w = _inputs(dev)
    y1, y0 = _both(g, xb if bf else xf, w, (5, item_edges))
    assert torch.equal(y1, y0), f"{int((_bits(y1) != _bits(y0)).sum())} elements differ"


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_unequal_pair_and_idle_half_wave(dev, bf):
    """A handful of items: a 70-edge item shares its wave with a short one (which idles through two
    chunks of the long one's staging), and with an odd item count the last wave has a lane group past
    n_items, which the kernel holds as an empty item.  The row without edges is written as zeros."""
    _, xf, xb, _ = _inputs(dev)
    odd = 0
    for deg in ([70, 0, 5, 3], [70, 0, 5, 3, 2]):  # one of the two item counts is odd
        ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        rng = np.random.default_rng(3)
        ix = np.concatenate([np.sort(rng.integers(0, N_COLS, d)) for d in deg]).astype(np.int32)
        g = G.from_numpy(ip, ix, device=dev, n_cols=N_COLS)
        w = (torch.rand(len(ix), H, generator=torch.Generator().manual_seed(4)) - 0.25).to(dev)
        odd += g.blocked_plan(*ROWS_PLAN).n_items % 2
        y1, y0 = _both(g, xb if bf else xf, w, ROWS_PLAN)
        assert torch.equal(y1, y0)
        rows = torch.tensor([d > 0 for d in deg], device=dev)
        assert not y1[~rows].any() and y1[rows].any(dim=1).all()
    assert odd == 1


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("plan_args", [ROWS_PLAN, (5, 7)], ids=["rows", "items7"])
def test_neighbours_stay_out(dev, plan_args, bf):
    """NaN, +Inf and -Inf in alpha at the edges immediately before and after rows, inside the 16-B
    pieces, windows and chunks those rows stage: no other row's sum sees them."""
    ip, _, starts = _csr()
    g, xf, xb, w = _inputs(dev)
    poisoned = {starts[(13, 9)]: float("nan"), starts[(22, 1)]: float("inf"), starts[(31, 33)]: float("-inf"),
                starts[(0, 256)]: float("nan"), starts[(5, 7)]: float("inf")}
    wp = w.clone()
    for r, v in poisoned.items():
        wp[ip[r]:ip[r + 1]] = v
    y1, y0 = _both(g, xb if bf else xf, wp, plan_args)
    _same(y1, y0)
    clean = torch.ones(g.n_rows, dtype=torch.bool, device=dev)
    clean[list(poisoned)] = False
    assert torch.isfinite(y1[clean]).all()
    assert not torch.isfinite(y1[~clean]).any()
    if plan_args == ROWS_PLAN:  # and the clean rows are what they are without the poison
        assert torch.equal(y1[clean], _rows_pair(dev, bf)[0][clean])


def test_poison_around_the_tensors(dev):
    """alpha and indices as 128-B aligned views inside larger poisoned buffers, the last item ending at
    the view's last edge: nothing outside the views is staged or used."""
    ip, ix, _ = _csr()
    g0, xf, _, w = _inputs(dev)
    nnz = len(ix)
    xbig = torch.full((N_COLS + 8, F), float("nan"), device=dev)
    xbig[:N_COLS] = xf
    wbuf = torch.full((32 + nnz + 64, H), float("nan"), device=dev)
    wbuf[32:32 + nnz] = w
    wv = wbuf[32:32 + nnz]
    ibuf = torch.full((32 + nnz + 64,), N_COLS + 3, dtype=torch.int32, device=dev)  # a NaN row of xbig
    ibuf[32:32 + nnz] = g0.indices
    iv = ibuf[32:32 + nnz]
    assert wv.data_ptr() % 128 == 0 and iv.data_ptr() % 128 == 0
    g = G.Graph(g0.indptr, iv, n_cols=N_COLS)
    assert g.indices.data_ptr() == iv.data_ptr() and g.nnz == nnz
    for plan_args in (ROWS_PLAN, (5, 7)):
        y1, y0 = _both(g, xbig[:N_COLS], wv, plan_args)
        assert torch.isfinite(y1).all(), "poison from outside the views reached y"
        assert torch.equal(y1, y0)
        if plan_args == ROWS_PLAN:
            assert torch.equal(y1, _rows_pair(dev, False)[0])


@pytest.mark.parametrize("case", ["ldw16", "offset32B"])
def test_refused_cases_keep_their_path(dev, case):
    """ldw != 8, or an alpha base off the 128-B grid: the grid walk refuses, the knob changes nothing
    and the result is the default's."""
    g, xf, _, w = _inputs(dev)
    nnz = g.nnz
    if case == "ldw16":
        wide = torch.full((nnz, 2 * H), float("nan"), device=dev)
        wide[:, :H] = w
        wv = wide[:, :H]
        assert wv.stride(0) == 2 * H
    else:
        wbuf = torch.full((1 + nnz + 64, H), float("nan"), device=dev)
        wbuf[1:1 + nnz] = w
        wv = wbuf[1:1 + nnz]
        assert wv.data_ptr() % 128 == 32
    y1, y0 = _both(g, xf, wv, ROWS_PLAN)
    assert torch.equal(y1, y0)
    assert torch.equal(y1, _rows_pair(dev, False)[1])


def test_row_chunks(dev):
    """The bench's form: a row range of the graph over the whole indices and alpha, into y[a:b]."""
    g, xf, _, w = _inputs(dev)
    cuts = [0, 301, g.n_rows]
    for a, b in zip(cuts[:-1], cuts[1:]):
        gg = G.Graph(g.indptr[a:b + 1], g.indices, n_cols=N_COLS)
        ys = []
        for v in (1, 0):
            y = torch.full((g.n_rows, F), float("nan"), device=dev)
            with _alpha_lds(v):
                ops.aggregate_blocked(gg, xf, w, out=y[a:b], plan=gg.blocked_plan(*ROWS_PLAN))
            assert torch.isnan(y[:a]).all() and torch.isnan(y[b:]).all(), "rows outside the chunk were written"
            ys.append(y[a:b])
        assert torch.equal(ys[0], ys[1]), f"rows [{a}, {b})"
        assert torch.equal(ys[0], _rows_pair(dev, False)[0][a:b])
