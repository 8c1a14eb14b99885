"""Graph preprocessing past one scan tile: the CSC build, the blocked plan and the row-chunk plan at
the smallest sizes where their multi-workgroup paths differ from the single-tile form, compared
exactly with the numpy references of tests/prep_ref.py.

Thresholds of csrc/gta_kernels.hip crossed here:
  scan_excl<int64_t> over row_ptr, tiled above 16,384 rows         test_blocked_plan_past_one_tile
  scan_excl<int32_t> over the radix histogram [256][ceil(nnz / 4096)], tiled from 262,145 edges
                                                                     test_csc_build_past_one_tile
  scan_excl tile doubling above 4,096 x 16,384 = 67,108,864 counts  test_blocked_plan_tile_doubling
  4 radix passes from 2^24 + 1 columns                               test_csc_build_past_one_tile[4_passes]
  k_plan_scan's thread partition at 1,023 / 1,024 / 1,025 rows       test_row_plan_decoded

In every test the structure check runs before any kernel consumes the plan or the view, and a failed
check ends the test: a wrong plan fails as an assertion, never as a GPU fault.
"""
import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops

from . import prep_ref
from .test_gpu_footprint import _knobs
from .test_gpu_ops import _check

pytestmark = pytest.mark.gpu

_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _degrees(n_rows, nnz, seed, heavy=5000):
    """nnz edges over n_rows rows: one heavy row (more than a radix tile and than any item), about
    a tenth of the rows empty, the rest spread at random."""
    rng = np.random.default_rng(seed)
    heavy = min(heavy, nnz)
    live = np.flatnonzero(rng.random(n_rows) >= 0.1)
    deg = np.bincount(rng.choice(live, nnz - heavy), minlength=n_rows)
    deg[live[len(live) // 2]] += heavy
    assert deg.sum() == nnz and (deg == 0).any() and deg.max() > 4096
    return deg


# ---- CSC build ----------------------------------------------------------------------------------
_CSC_ROWS = 20000
_CSC = {  # name: (nnz, n_cols, indices)
    "nb64_last_single_tile": (262144, 3000, "random"),
    "nb65_second_tile_of_256": (262145, 3000, "random"),
    "2_passes": (1000003, 70000, "random"),
    "3_passes": (1000003, (1 << 20) + 3, "random"),
    "4_passes": (1000003, (1 << 24) + 3, "random"),
    "all_equal_one_col": (262145, 1, "zero"),
    "all_equal_last_col": (262145, 70000, "last"),
    "ascending": (262145, 70000, "ascending"),
    "descending": (262145, 70000, "descending"),
}
_CSC_GATHER = ("nb65_second_tile_of_256", "2_passes")


def _csc_graph(name):
    nnz, n_cols, kind = _CSC[name]
    deg = _degrees(_CSC_ROWS, nnz, seed=len(name))
    if kind == "random":
        return prep_ref.random_csr(deg, n_cols, seed=nnz % 97) + (n_cols,)
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    if kind == "zero":
        ix = np.zeros(nnz, np.int32)
    elif kind == "last":
        ix = np.full(nnz, n_cols - 1, np.int32)
    else:  # sorted over the whole edge array
        ix = np.sort(np.random.default_rng(7).integers(0, n_cols, nnz)).astype(np.int32)
        if kind == "descending":
            ix = ix[::-1].copy()
    return ip, ix, n_cols


@pytest.mark.parametrize("name", list(_CSC))
def test_csc_build_past_one_tile(dev, name):
    """gta_csc_build == the stable argsort by source column, bit-exact (perm, colptr, rows), and a
    second build equal to the first; then (two graphs) gather C through the checked view."""
    ip, ix, n_cols = _csc_graph(name)
    g = G.from_numpy(ip, ix, device=dev, n_cols=n_cols)
    c = g.csc()
    perm, colptr, rows = prep_ref.csc(ip, ix, n_cols)
    assert np.array_equal(c.colptr.cpu().numpy(), colptr), f"{name}: colptr"
    got = c.perm.cpu().numpy()
    bad = np.flatnonzero(got != perm)
    assert len(bad) == 0, f"{name}: perm differs at {len(bad)} positions, first {int(bad[0])} (radix tile {int(bad[0]) // 4096})"
    assert np.array_equal(c.rows.cpu().numpy(), rows), f"{name}: rows"
    c2 = ops.CSC(g)  # a pure function of the graph
    assert torch.equal(c.perm, c2.perm) and torch.equal(c.colptr, c2.colptr) and torch.equal(c.rows, c2.rows), \
        f"{name}: a second build differs"
    if name not in _CSC_GATHER:
        return
    F = 4
    xe = np.random.default_rng(1).standard_normal((len(ix), F)).astype(np.float32)
    xd = torch.from_numpy(xe).to(dev)
    y = ops.gather_add(g, xd, direction="C")  # g.csc() is the view checked above
    ref, ab = np.zeros((n_cols, F)), np.zeros((n_cols, F))
    np.add.at(ref, ix.astype(np.int64), xe.astype(np.float64))
    np.add.at(ab, ix.astype(np.int64), np.abs(xe.astype(np.float64)))
    _check(y, ref, ab, f"gather C {name}")
    assert torch.equal(y, ops.gather_add(g, xd, direction="C")), f"{name}: gather C is not reproducible"


# ---- blocked plan -------------------------------------------------------------------------------
def _blocked_graph(n):
    def make():
        deg = np.random.default_rng(n).integers(0, 6, n)  # empty rows among them
        deg[n // 3], deg[n - 2] = 5000, 700
        return prep_ref.random_csr(deg, n, seed=n + 1)
    return _memo(("blocked", n), make)


_BLOCKED = [  # (n_rows, blocks, row_edges, item_edges, class_major): every value once at each size
    (16384, 1, 0, 7, 1), (16384, 1, 16, 256, 0), (16384, 1, 16, 7, 1),      # both scans: exactly one tile
    (16385, 1, 0, 7, 1), (16385, 1, 16, 256, 0), (16385, 1, 16, 7, 1),      # a second tile of one element
    (16385, 5, 0, 7, 1), (16385, 5, 16, 256, 0), (16385, 5, 16, 7, 1),
    (40000, 63, 0, 7, 1), (40000, 63, 16, 256, 0), (40000, 63, 16, 7, 1),
]
_BLOCKED_RUN = ((16385, 5), (40000, 63))


def _agg_inputs(n, dev):
    """x, w and the fp64 aggregate of the graph of n rows at F = 64, H = 8 (made once, shared)."""
    def make():
        ip, ix = _blocked_graph(n)
        rng = np.random.default_rng(3)
        x = rng.standard_normal((n, 64)).astype(np.float32)
        w = rng.random((len(ix), 8)).astype(np.float32)
        ref, ab = prep_ref.aggregate_rows(ip, ix, x, w)
        return torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev), ref, ab
    return _memo(("agg", n), make)


@pytest.mark.parametrize("n,blocks,row_edges,item_edges,class_major", _BLOCKED)
def test_blocked_plan_past_one_tile(dev, n, blocks, row_edges, item_edges, class_major):
    ip, ix = _blocked_graph(n)
    g = G.from_numpy(ip, ix, device=dev)
    with _knobs(seg_class_major=class_major):
        plan = ops.BlockedPlan(g, blocks, item_edges, row_edges)
    assert ops.BlockedPlan.supports(64, 8)
    prep_ref.check_blocked(prep_ref.decode_blocked(plan.buf, n, blocks), ip, ix, n, blocks, item_edges, row_edges,
                           class_major, n_items=plan.n_items)
    if (n, blocks) not in _BLOCKED_RUN:
        return
    xd, wd, ref, ab = _agg_inputs(n, dev)
    y = ops.aggregate_blocked(g, xd, wd, plan=plan)
    _check(y, ref, ab, f"blocked aggregate n={n} B={blocks} re={row_edges} ie={item_edges} cm={class_major}")
    assert torch.equal(y, ops.aggregate_blocked(g, xd, wd, plan=plan)), "the blocked aggregate is not reproducible"


# ---- tile doubling: n_rows * blocks past 4,096 tiles of 16,384 ------------------------------------
_DBL_ROWS, _DBL_COLS, _DBL_BLOCKS, _DBL_HEAVY = 1070000, 200003, 63, (5000, 700, 300)


def _doubling_graph():
    def make():
        deg = np.random.default_rng(11).integers(0, 3, _DBL_ROWS)
        at = np.array([_DBL_ROWS // 4, _DBL_ROWS // 2, _DBL_ROWS - 7])
        deg[at] = _DBL_HEAVY
        ip, ix = prep_ref.random_csr(deg, _DBL_COLS, seed=12)
        rng = np.random.default_rng(13)
        rows = np.concatenate([at, [0, _DBL_ROWS - 1], rng.choice(_DBL_ROWS, 250, replace=False)])
        x = rng.standard_normal((_DBL_COLS, 64)).astype(np.float32)
        ref, ab = prep_ref.aggregate_rows(ip, ix, x, None, rows)  # visits only those rows
        return ip, ix, rows, x, ref, ab
    return _memo("doubling", make)


@pytest.mark.parametrize("row_edges", [0, 16])
def test_blocked_plan_tile_doubling(dev, row_edges):
    """n_rows * blocks = 67,410,000 counts: more than kScanMaxTiles tiles of kScanTile, so scan_excl
    doubles its tile (32,768 counts, 2,058 tiles)."""
    assert _DBL_ROWS * _DBL_BLOCKS > 4096 * 16384
    ip, ix, rows, x, ref, ab = _doubling_graph()
    g = G.from_numpy(ip, ix, device=dev, n_cols=_DBL_COLS)
    plan = ops.BlockedPlan(g, _DBL_BLOCKS, 256, row_edges)
    prep_ref.check_blocked(prep_ref.decode_blocked(plan.buf, _DBL_ROWS, _DBL_BLOCKS), ip, ix, _DBL_COLS, _DBL_BLOCKS,
                           256, row_edges, ops.get_debug("seg_class_major"), n_items=plan.n_items)
    y = ops.aggregate_blocked(g, torch.from_numpy(x).to(dev), None, plan=plan)
    _check(y[torch.from_numpy(rows).to(dev)], ref, ab, f"blocked aggregate past the tile doubling, row_edges {row_edges}")


# ---- row-chunk plan -----------------------------------------------------------------------------
def _row_plan_degrees(n, chunk):
    """Degrees 0..3 with an empty row, rows of exactly chunk, chunk + 1 and 40 chunks, and a split
    last row (a one-row graph: that split row alone)."""
    deg = np.random.default_rng(n).integers(0, 4, n)
    if n >= 5:
        deg[0], deg[n // 3], deg[n // 2], deg[2 * n // 3] = 0, chunk, chunk + 1, 40 * chunk
    deg[n - 1] = 2 * chunk + 5
    return deg


@pytest.mark.parametrize("chunk", [64, 512])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049, 20000])
def test_row_plan_decoded(dev, n, chunk):
    deg = _row_plan_degrees(n, chunk)
    ip, ix = prep_ref.random_csr(deg, n, seed=chunk, sort_cols=False)
    g = G.from_numpy(ip, ix, device=dev)
    p = ops.AggregatePlan(g, chunk)
    prep_ref.check_row_plan(prep_ref.decode_row_plan(p.buf, n, len(ix), chunk), ip, chunk)
    chunks = np.where(deg <= chunk, 1, -(-deg // chunk))
    assert p.n_items() == int(chunks.sum()) and p.n_split() == int((deg > chunk).sum()) == (3 if n >= 5 else 1)
    if n != 20000:
        return
    F = 16
    x = np.random.default_rng(5).standard_normal((n, F)).astype(np.float32)
    y = ops.aggregate(g, torch.from_numpy(x).to(dev), "src", None, plan=p)  # the plan checked above
    ref, ab = prep_ref.aggregate_rows(ip, ix, x)
    _check(y, ref, ab, f"aggregate through the row-chunk plan, chunk {chunk}")
