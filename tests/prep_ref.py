"""Vectorised numpy restatements of the graph preprocessing builders (no torch, no GPU).

The builders of csrc/gta_kernels.hip produce integer tables -- the row-chunk plan
(gta_aggregate_plan_build), the blocked plan (gta_aggregate_blocked_plan_build) and the CSC view
(gta_csc_build) -- so every comparison here is exact.  The references never allocate an
[n_rows, blocks] array: they work on one key per edge, so they scale to the sizes at which the
device scans leave their single-tile form (tests/test_gpu_prep_scale.py).

decode_* read a plan buffer by the layouts of the .hip file (BlockedView, PlanView); a device
buffer is sliced on the device and only the needed parts are copied.  check_* raise AssertionError
with a message naming what broke; tests/test_prep_ref_cpu.py proves that they reject corrupted plans.
"""
import numpy as np


def _r16(b):
    return (int(b) + 15) // 16 * 16


def _ceil_div(a, b):
    return -(-a // b)


def random_csr(deg, n_cols, seed=0, sort_cols=True):
    """(indptr int64, indices int32) of a CSR with the given degrees and uniform random columns,
    sorted inside each row (duplicates stay); built without a per-row loop."""
    deg = np.asarray(deg, np.int64)
    rng = np.random.default_rng(seed)
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n_cols, int(ip[-1]))
    if sort_cols:
        row = np.repeat(np.arange(len(deg), dtype=np.int64), deg)
        col = col[np.lexsort((col, row))]
    return ip, col.astype(np.int32)


# ---- blocked plan: the rules of the comment block above `struct BlockedView` ----------------------
def merge_of(deg, B, row_edges):
    """Fine blocks per merged block of every row: the smallest m = 2^k with deg * m >= row_edges * B,
    capped at the first m >= B; 1 for an empty row or row_edges 0."""
    deg = np.asarray(deg, np.int64)
    m = np.ones(len(deg), np.int64)
    if not row_edges:
        return m
    while True:
        grow = (deg > 0) & (m < B) & (deg * m < row_edges * B)
        if not grow.any():
            return m
        m = np.where(grow, m * 2, m)


def segments(ip, ix, n_cols, blocks, row_edges):
    """The non-empty (row, merged block) segments: (row, merged block, first edge, edges), in
    (row, merged block) order, from one key per edge."""
    ip, ix = np.asarray(ip, np.int64), np.asarray(ix, np.int64)
    n = len(ip) - 1
    deg = np.diff(ip)
    bsize = _ceil_div(int(n_cols), int(blocks))
    m = merge_of(deg, blocks, row_edges)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    key = row * 64 + (ix // bsize) // m[row]
    ukey, first, count = np.unique(key, return_index=True, return_counts=True)
    return ukey // 64, ukey % 64, first.astype(np.int64), count.astype(np.int64)


def items_per_row(ip, ix, n_cols, blocks, item_edges, row_edges):
    """Items of every row: the sum over its non-empty merged blocks of ceil(edges / item_edges)."""
    n = len(ip) - 1
    srow, _, _, count = segments(ip, ix, n_cols, blocks, row_edges)
    # float64 weights: exact, a row's count is far below 2^53
    return np.bincount(srow, weights=_ceil_div(count, int(item_edges)), minlength=n).astype(np.int64)


def blocked_plan(ip, ix, n_cols, blocks, item_edges, row_edges, class_major):
    """A valid decoded plan (items [n_items, 3] = beg, row, len; row_ptr; row_items) of a graph whose
    rows have sorted columns.  A segment of L edges is cut into p = ceil(L / item_edges) parts of
    floor(L / p) or ceil(L / p) edges (the device's parts are ceil(L / p) long and the last one
    shorter: the checker takes either); item ids are (class, merged block)-major -- not
    class-major: one class, a merged block at its first fine block -- and longest first inside a
    group with the length capped at 256; orders the kernel leaves free are the stable ones."""
    ip = np.asarray(ip, np.int64)
    n = len(ip) - 1
    m = merge_of(np.diff(ip), blocks, row_edges)
    srow, smb, sfirst, slen = segments(ip, ix, n_cols, blocks, row_edges)
    parts = _ceil_div(slen, int(item_edges))
    base, extra = slen // parts, slen % parts  # the first `extra` parts hold one edge more
    seg = np.repeat(np.arange(len(srow)), parts)
    j = np.arange(int(parts.sum()), dtype=np.int64) - np.repeat(np.cumsum(parts) - parts, parts)
    beg = sfirst[seg] + j * base[seg] + np.minimum(j, extra[seg])
    ln = base[seg] + (j < extra[seg])
    row, mb = srow[seg], smb[seg]
    cls = np.log2(m[row]).astype(np.int64) if class_major else np.zeros(len(row), np.int64)
    group = cls * 64 + (mb if class_major else mb * m[row])
    order = np.lexsort((256 - np.minimum(ln, 256), group))  # stable: ties keep (row, block, part) order
    items = np.stack([beg[order], row[order], ln[order]], axis=1)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int64)
    row_items = np.argsort(items[:, 0], kind="stable").astype(np.int64)  # edge order = (row, block, part)
    return items, row_ptr, row_items


def blocked_header(ip, n_cols, blocks, item_edges, row_edges, class_major, n_items):
    """The 16 int64 header words of a sorted graph's plan, as gta_aggregate_blocked_plan_build writes
    them (the row_items byte offset, word 7, is a layout detail: 0 here)."""
    n, nnz = len(ip) - 1, int(ip[-1])
    mi = min(n * blocks, nnz) + nnz // item_edges
    hdr = np.zeros(16, np.int64)
    hdr[:10] = [blocks, _ceil_div(int(n_cols), blocks), n, 0, n_items, item_edges, mi, 0, row_edges, class_major]
    return hdr


def _take(buf, off, nbytes):
    """nbytes of a plan buffer from byte off, as a numpy uint8 array (a device tensor is sliced on
    the device, so only this part is copied)."""
    part = buf[off:off + nbytes]
    return part.cpu().numpy() if hasattr(part, "cpu") else np.asarray(part)


def decode_blocked(buf, n_rows, blocks):
    """(hdr, items [n_items, 3] = beg, row, len, row_ptr, row_items) of a blocked plan buffer."""
    hdr = _take(buf, 0, 128).view(np.int64).copy()
    B, mi, n_items, ri_off = int(hdr[0]), int(hdr[6]), int(hdr[4]), int(hdr[7])
    assert int(hdr[2]) == n_rows and B == blocks, "plan header: rows or blocks are not the graph's"
    assert 0 <= n_items <= mi, f"plan header: n_items {n_items} outside [0, max_items {mi}]"
    # the layout of csrc/gta_kernels.hip (BlockedView): the fixed part ends where the items begin
    off = 128 + _r16(n_rows * 4) + _r16(n_rows * (B + 1) * 4) + _r16(2 * 256 * 4) + _r16(256 * 4)
    row_ptr = _take(buf, off, (n_rows + 1) * 8).view(np.int64).copy()
    off += _r16((n_rows + 1) * 8) + _r16(n_rows * B * 4) + _r16(4097 * 8) + _r16(2 * 128 * 257 * 4)
    assert off == ri_off - _r16(mi * 16), "plan layout: the item array does not follow the fixed part"
    it = _take(buf, off, n_items * 16).view(np.int32).reshape(n_items, 4)
    beg = it[:, :2].copy().view(np.int64)[:, 0]
    items = np.stack([beg, it[:, 2].astype(np.int64), it[:, 3].astype(np.int64)], axis=1)
    row_items = _take(buf, ri_off, n_items * 4).view(np.int32).astype(np.int64)
    return hdr, items, row_ptr, row_items


def check_blocked(decoded, ip, ix, n_cols, blocks, item_edges, row_edges, class_major, n_items=None):
    """Every rule of the blocked plan on a decoded plan (decode_blocked's tuple); n_items: the count
    the plan object reports, when there is one."""
    hdr, items, row_ptr, row_items = decoded
    ip, ix = np.asarray(ip, np.int64), np.asarray(ix, np.int64)
    n = len(ip) - 1
    deg = np.diff(ip)
    bsize = _ceil_div(int(n_cols), int(blocks))
    assert int(hdr[3]) == 0 and int(hdr[5]) == item_edges and int(hdr[8]) == row_edges and int(hdr[9]) == class_major, \
        "plan header: unsorted flag, item_edges, row_edges or class_major"
    m_of = merge_of(deg, blocks, row_edges)
    want_rows = items_per_row(ip, ix, n_cols, blocks, item_edges, row_edges)
    if n_items is None:
        n_items = int(hdr[4])
    assert n_items == int(hdr[4]) == int(want_rows.sum()) <= int(hdr[6]), \
        f"n_items: plan {n_items}, header {int(hdr[4])}, rules {int(want_rows.sum())}, max_items {int(hdr[6])}"
    assert len(items) == len(row_items) == n_items and len(row_ptr) == n + 1, "decoded arrays: wrong lengths"
    got_rows = np.diff(row_ptr)
    if not (np.array_equal(got_rows, want_rows) and row_ptr[0] == 0):
        bad = np.flatnonzero(got_rows != want_rows)
        where = f"first at row {int(bad[0])}: {int(got_rows[bad[0]])} for {int(want_rows[bad[0]])}" if len(bad) else "row_ptr[0]"
        raise AssertionError(f"row_ptr is not the scan of the items per row ({len(bad)} rows differ, {where})")
    beg, row, ln = items[:, 0], items[:, 1], items[:, 2]
    if len(items) == 0:
        return
    # every edge in exactly one item, inside its row, inside one merged block of its row
    assert (ln >= 1).all() and (ln <= item_edges).all(), "an item's length is outside [1, item_edges]"
    assert (row >= 0).all() and (row < n).all(), "an item's row is outside the graph"
    assert (beg >= ip[row]).all() and (beg + ln <= ip[row + 1]).all(), "an item lies outside its row"
    cover = np.bincount(beg, minlength=len(ix) + 1) - np.bincount(beg + ln, minlength=len(ix) + 1)
    assert (np.cumsum(cover)[:len(ix)] == 1).all(), "an edge in no item, or in two"
    m = m_of[row]
    mb = ix[beg] // bsize // m
    assert np.array_equal(mb, ix[beg + ln - 1] // bsize // m), "an item spans two merged blocks"
    # ascending item id: the (class, merged block) key never decreases (not class-major: the first
    # fine block of the merged block), and inside a key the capped lengths never increase
    cls = np.log2(m).astype(np.int64) if class_major else np.zeros(len(m), np.int64)
    key = cls * 64 + (mb if class_major else mb * m)
    assert (np.diff(key) >= 0).all(), "item ids are not (class, merged block)-major"
    same = np.diff(key) == 0
    assert (np.diff(np.minimum(ln, 256))[same] <= 0).all(), "a group's items are not longest first"
    # each row's list: its own items in (block, part) order -- columns are sorted, so edge order
    assert np.array_equal(np.sort(row_items), np.arange(len(items))), "row_items is not a permutation of the item ids"
    lrow = np.repeat(np.arange(n), want_rows)
    assert np.array_equal(row[row_items], lrow), "a row's list holds another row's item"
    first = np.zeros(len(items), bool)
    first[row_ptr[:-1][want_rows > 0]] = True
    lb, ll = beg[row_items], ln[row_items]
    assert np.array_equal(lb[first], ip[:-1][want_rows > 0]), "a row's list does not start at the row's first edge"
    assert np.array_equal(lb[1:][~first[1:]], (lb + ll)[:-1][~first[1:]]), "a row's list is not in (block, part) order"


# ---- row-chunk plan (gta_aggregate_plan_build) --------------------------------------------------
SPLIT_BIT = np.int64(1) << 31


def row_plan(ip, chunk):
    """(item_row, item_beg, item_end, splits) of the row-chunk plan: a row of deg edges is
    1 if deg <= chunk else ceil(deg / chunk) items of chunk edges (the last one shorter; an empty row
    one empty item), in row order; item_row (int64 here) carries bit 31 when the row is split;
    splits [n_split, 3] = (row, first item, count), sorted by row."""
    ip = np.asarray(ip, np.int64)
    n = len(ip) - 1
    deg = np.diff(ip)
    chunks = np.where(deg <= chunk, 1, _ceil_div(deg, int(chunk)))
    offs = np.cumsum(chunks) - chunks
    row = np.repeat(np.arange(n, dtype=np.int64), chunks)
    j = np.arange(int(chunks.sum()), dtype=np.int64) - offs[row]
    item_beg = ip[row] + j * chunk
    item_end = np.minimum(item_beg + chunk, ip[row + 1])
    item_row = row | np.where(chunks[row] > 1, SPLIT_BIT, 0)
    split = np.flatnonzero(chunks > 1)
    return item_row, item_beg, item_end, np.stack([split, offs[split], chunks[split]], axis=1).astype(np.int64)


def decode_row_plan(buf, n_rows, nnz, chunk):
    """(hdr [4] = n_items, n_split, chunk, n_rows; item_row; item_beg; item_end; splits [n_split, 3]) of
    a row-chunk plan buffer, by plan_view's layout with max_items = n_rows + ceil(nnz / chunk)."""
    mi = n_rows + _ceil_div(int(nnz), int(chunk))
    hdr = _take(buf, 0, 32).view(np.int64).copy()
    n_items, n_split = int(hdr[0]), int(hdr[1])
    assert 0 <= n_items <= mi, f"row plan header: n_items {n_items} outside [0, max_items {mi}]"
    assert 0 <= n_split <= n_rows, f"row plan header: n_split {n_split} outside [0, n_rows]"
    off = 64
    item_row = _take(buf, off, n_items * 4).view(np.uint32).astype(np.int64)
    off += _r16(mi * 4)
    item_beg = _take(buf, off, n_items * 8).view(np.int64).copy()
    off += _r16(mi * 8)
    item_end = _take(buf, off, n_items * 8).view(np.int64).copy()
    off += _r16(mi * 8)
    cols = []
    for _ in range(3):  # split_row, split_first, split_cnt
        cols.append(_take(buf, off, n_split * 4).view(np.int32).astype(np.int64))
        off += _r16(n_rows * 4)
    return hdr, item_row, item_beg, item_end, np.stack(cols, axis=1)


def check_row_plan(decoded, ip, chunk):
    """A decoded row-chunk plan equals row_plan(ip, chunk): the items exactly, the splits as a set."""
    hdr, item_row, item_beg, item_end, splits = decoded
    n = len(ip) - 1
    w_row, w_beg, w_end, w_splits = row_plan(ip, chunk)
    assert int(hdr[0]) == len(w_row), f"row plan: n_items {int(hdr[0])}, rules {len(w_row)}"
    assert int(hdr[1]) == len(w_splits), f"row plan: n_split {int(hdr[1])}, rules {len(w_splits)}"
    assert int(hdr[2]) == chunk and int(hdr[3]) == n, "row plan header: chunk or n_rows"
    assert len(item_row) == len(item_beg) == len(item_end) == len(w_row) and len(splits) == len(w_splits), \
        "row plan: decoded arrays of the wrong lengths"
    for name, got, want in (("item_row", item_row, w_row), ("item_beg", item_beg, w_beg), ("item_end", item_end, w_end)):
        bad = np.flatnonzero(np.asarray(got) != want)
        assert len(bad) == 0, (f"row plan: {name} differs at {len(bad)} items, first item {int(bad[0])} "
                               f"(row {int(w_row[bad[0]] & (SPLIT_BIT - 1))}): {int(got[bad[0]])} for {int(want[bad[0]])}")
    got = splits[np.argsort(splits[:, 0], kind="stable")] if len(splits) else splits
    assert np.array_equal(got, w_splits), "row plan: the split table is not the set of (row, first item, count)"


# ---- CSC view (gta_csc_build) -------------------------------------------------------------------
def csc(ip, ix, n_cols):
    """(perm, colptr, rows): the stable sort of the edges by source column."""
    ip, ix = np.asarray(ip, np.int64), np.asarray(ix)
    perm = np.argsort(ix, kind="stable")
    colptr = np.concatenate([[0], np.cumsum(np.bincount(ix, minlength=n_cols))]).astype(np.int64)
    row_of_edge = np.repeat(np.arange(len(ip) - 1, dtype=np.int64), np.diff(ip))
    return perm, colptr, row_of_edge[perm]


# ---- fp64 aggregate of chosen rows --------------------------------------------------------------
def aggregate_rows(ip, ix, x, w=None, rows=None):
    """(y, sum|terms|) in float64 of y[i] = sum_{e in row i} w[e, head] * x[ix[e]] for the rows asked
    for (None: all), visiting only their edges; column c uses head c // (F / H)."""
    ip = np.asarray(ip, np.int64)
    rows = np.arange(len(ip) - 1) if rows is None else np.asarray(rows, np.int64)
    deg = ip[rows + 1] - ip[rows]
    start = np.cumsum(deg) - deg
    e = np.repeat(ip[rows] - start, deg) + np.arange(int(deg.sum()), dtype=np.int64)
    X = np.asarray(x)[np.asarray(ix, np.int64)[e]].astype(np.float64)
    if w is not None:
        X = X * np.repeat(np.asarray(w)[e].astype(np.float64), X.shape[1] // w.shape[1], axis=1)
    y, ab = np.zeros((len(rows), X.shape[1])), np.zeros((len(rows), X.shape[1]))
    ne = deg > 0
    if ne.any():
        y[ne] = np.add.reduceat(X, start[ne], axis=0)
        ab[ne] = np.add.reduceat(np.abs(X), start[ne], axis=0)
    return y, ab
