"""tests/prep_ref.py checked without a GPU: the vectorised references equal plain per-row loops, the
decoders read back what the documented layouts hold, and the checkers that the GPU tests rely on
(tests/test_gpu_blocked_classes.py, tests/test_gpu_prep_scale.py) accept a valid plan and reject
each corruption a broken builder would produce -- the proof that those tests can fail."""
import numpy as np
import pytest

from oracle import isa_ref

from . import prep_ref
from .test_gpu_blocked_classes import _csr_of, _degenerate, _items_graph

_DEGENERATE = ["all_light", "empty_class", "few_rows", "one_row"]


def _merge_of(deg, B, row_edges):
    m = 1
    while row_edges and deg and m < B and deg * m < row_edges * B:
        m *= 2
    return m


def _items_per_row_loop(ip, ix, n_cols, blocks, item_edges, row_edges):
    """The per-row loop the plan checker ran before it was vectorised: the independent restatement."""
    n = len(ip) - 1
    deg = np.diff(ip)
    bsize = -(-n_cols // blocks)
    m_of = np.array([_merge_of(int(d), blocks, row_edges) for d in deg])
    want_rows = np.zeros(n, np.int64)
    for r in range(n):
        seg = np.bincount(ix[ip[r]:ip[r + 1]] // bsize, minlength=blocks)
        seg = np.array([seg[j:j + m_of[r]].sum() for j in range(0, blocks, m_of[r])])
        want_rows[r] = int(np.sum(-(-seg // item_edges)))
    return m_of, want_rows


def _named_graph(name):
    if name == "items600":
        ip, ix = _items_graph(600)
        return ip, ix, 600
    deg, n_cols, _, _ = _degenerate(name)
    ip, ix = _csr_of(deg, n_cols, seed=1)
    return ip, ix, n_cols


@pytest.mark.parametrize("row_edges", [0, 16, 40])
@pytest.mark.parametrize("blocks", [1, 5, 16, 63])
@pytest.mark.parametrize("name", ["items600"] + _DEGENERATE)
def test_items_per_row_equals_the_row_loop(name, blocks, row_edges):
    ip, ix, n_cols = _named_graph(name)
    for item_edges in (5, 7, 256):
        m_loop, want = _items_per_row_loop(ip, ix, n_cols, blocks, item_edges, row_edges)
        assert np.array_equal(prep_ref.merge_of(np.diff(ip), blocks, row_edges), m_loop)
        assert np.array_equal(prep_ref.items_per_row(ip, ix, n_cols, blocks, item_edges, row_edges), want)


def _row_plan_loop(ip, chunk):
    rows, begs, ends, splits = [], [], [], []
    for r in range(len(ip) - 1):
        b, e = int(ip[r]), int(ip[r + 1])
        nc = 1 if e - b <= chunk else -(-(e - b) // chunk)
        if nc > 1:
            splits.append((r, len(rows), nc))
        for j in range(nc):
            rows.append(r | (1 << 31) if nc > 1 else r)
            begs.append(b + j * chunk)
            ends.append(min(b + (j + 1) * chunk, e))
    return (np.array(rows, np.int64), np.array(begs, np.int64), np.array(ends, np.int64),
            np.array(splits, np.int64).reshape(-1, 3))


def _row_plan_degrees(n, chunk, seed=0):
    """Degrees 0..3 with the special rows of the row-chunk plan: empty, exactly chunk, chunk + 1,
    40 chunks, and a split last row (a one-row graph: that row alone)."""
    deg = np.random.default_rng(seed).integers(0, 4, n)
    if n >= 5:
        deg[0], deg[n // 3], deg[n // 2], deg[2 * n // 3] = 0, chunk, chunk + 1, 40 * chunk
    deg[n - 1] = 2 * chunk + 5
    return deg


@pytest.mark.parametrize("chunk", [64, 512])
@pytest.mark.parametrize("n", [1, 7, 1023, 1025])
def test_row_plan_equals_the_row_loop(n, chunk):
    ip = np.concatenate([[0], np.cumsum(_row_plan_degrees(n, chunk))]).astype(np.int64)
    for got, want in zip(prep_ref.row_plan(ip, chunk), _row_plan_loop(ip, chunk)):
        assert np.array_equal(got, want)


def test_csc_and_aggregate_rows_equal_the_plain_forms():
    ip, ix = prep_ref.random_csr(np.random.default_rng(3).integers(0, 9, 300), 41, seed=4)
    assert all((np.diff(ix[ip[r]:ip[r + 1]]) >= 0).all() for r in range(300))  # random_csr: sorted rows
    perm, colptr, rows = prep_ref.csc(ip, ix, 41)
    edges = sorted(range(len(ix)), key=lambda e: (ix[e], e))
    assert perm.tolist() == edges
    assert colptr.tolist() == [int((ix < j).sum()) for j in range(42)]
    assert rows.tolist() == [int(np.searchsorted(ip, e, side="right") - 1) for e in edges]
    rng = np.random.default_rng(5)
    x, w = rng.standard_normal((41, 16)).astype(np.float32), rng.random((len(ix), 4)).astype(np.float32)
    y, ab = prep_ref.aggregate_rows(ip, ix, x, w)
    assert np.allclose(y, isa_ref.aggregate(ip, ix, x, "src", w), rtol=1e-13, atol=1e-13)
    assert np.allclose(ab, isa_ref.aggregate_abs(ip, ix, x, "src", w), rtol=1e-13, atol=1e-13)
    pick = np.array([299, 0, 17, 17, 120])
    y2, ab2 = prep_ref.aggregate_rows(ip, ix, x, w, pick)
    assert np.array_equal(y2, y[pick]) and np.array_equal(ab2, ab[pick])


# ---- the plan checker: accepts the reference plan, rejects corrupted ones ------------------------
_N, _B, _IE, _RE = 20000, 5, 7, 16  # more rows than one scan tile (16,384)
_BIG = {}


def _big():
    if not _BIG:
        deg = np.random.default_rng(1).integers(0, 6, _N)
        deg[100], deg[17000] = 5000, 700
        _BIG["g"] = prep_ref.random_csr(deg, _N, seed=2)
    return _BIG["g"]


def _decoded(ip, ix, n_cols, blocks, item_edges, row_edges, class_major):
    items, row_ptr, row_items = prep_ref.blocked_plan(ip, ix, n_cols, blocks, item_edges, row_edges, class_major)
    hdr = prep_ref.blocked_header(ip, n_cols, blocks, item_edges, row_edges, class_major, len(items))
    return hdr, items, row_ptr, row_items


@pytest.mark.parametrize("class_major", [1, 0])
@pytest.mark.parametrize("name", ["items600", "big"] + _DEGENERATE)
def test_checker_accepts_the_reference_plan(name, class_major):
    if name == "big":
        ip, ix = _big()
        cases = [(_N, _B, _IE, _RE), (_N, 63, 256, 16), (_N, 1, 7, 0)]
    else:
        ip, ix, n_cols = _named_graph(name)
        cases = [(n_cols, b, ie, re_) for b in (1, 5, 16, 63) for ie in (5, 256) for re_ in (0, 16, 40)]
    for n_cols, blocks, item_edges, row_edges in cases:
        d = _decoded(ip, ix, n_cols, blocks, item_edges, row_edges, class_major)
        prep_ref.check_blocked(d, ip, ix, n_cols, blocks, item_edges, row_edges, class_major)
        # near-equal parts: a row's list is in edge order, so the items of one (row, merged block)
        # are neighbours in it; their lengths differ by at most one
        beg, ln = d[1][d[3], 0], d[1][d[3], 2]
        bsize = -(-n_cols // blocks)
        m = prep_ref.merge_of(np.diff(ip), blocks, row_edges)[d[1][d[3], 1]]
        same = (np.diff(d[1][d[3], 1]) == 0) & (np.diff(ix[beg] // bsize // m) == 0)
        assert (np.abs(np.diff(ln))[same] <= 1).all() and ln.min() >= 1 and ln.max() <= item_edges


def _corrupt(kind, ip, d, class_major):
    """One host-side corruption of a decoded plan; the message the checker must give."""
    hdr, items, row_ptr, row_items = d[0].copy(), d[1].copy(), d[2].copy(), d[3].copy()
    beg, row, ln = items[:, 0], items[:, 1], items[:, 2]
    if kind == "row_ptr_tile_offset":      # a lost tile offset: everything from the second scan tile on
        row_ptr[16384:] -= 1
        msg = "row_ptr is not the scan"
    elif kind == "item_longer":            # an edge covered twice
        slot = np.flatnonzero((ln[row_items][:-1] < _IE) & (row[row_items][:-1] == row[row_items][1:]))[0]
        items[row_items[slot], 2] += 1
        msg = "an edge in no item, or in two"
    elif kind == "groups_swapped":         # two items of different groups trade ids; the row lists follow
        a, b = 0, len(items) - 1
        items[[a, b]] = items[[b, a]]
        ia, ib = np.flatnonzero(row_items == a)[0], np.flatnonzero(row_items == b)[0]
        row_items[[ia, ib]] = [b, a]
        msg = r"not \(class, merged block\)-major"
    elif kind == "row_items_swapped":      # two entries of one row's list
        r = int(np.flatnonzero(np.diff(row_ptr) >= 2)[0])
        s = int(row_ptr[r])
        row_items[[s, s + 1]] = row_items[[s + 1, s]]
        msg = "does not start at the row's first edge|not in \\(block, part\\) order"
    elif kind == "item_to_next_row":
        k = int(np.flatnonzero(row < len(ip) - 2)[0])
        items[k, 1] += 1
        msg = "an item lies outside its row"
    else:
        raise KeyError(kind)
    return (hdr, items, row_ptr, row_items), msg


@pytest.mark.parametrize("class_major", [1, 0])
@pytest.mark.parametrize("kind", ["row_ptr_tile_offset", "item_longer", "groups_swapped", "row_items_swapped",
                                  "item_to_next_row"])
def test_checker_rejects_a_corrupted_plan(kind, class_major):
    ip, ix = _big()
    d = _decoded(ip, ix, _N, _B, _IE, _RE, class_major)
    bad, msg = _corrupt(kind, ip, d, class_major)
    with pytest.raises(AssertionError, match=msg):
        prep_ref.check_blocked(bad, ip, ix, _N, _B, _IE, _RE, class_major)
    prep_ref.check_blocked(d, ip, ix, _N, _B, _IE, _RE, class_major)  # the corruption touched a copy


def test_checker_rejects_a_wrong_item_count():
    ip, ix = _big()
    hdr, items, row_ptr, row_items = _decoded(ip, ix, _N, _B, _IE, _RE, 1)
    with pytest.raises(AssertionError, match="n_items"):
        prep_ref.check_blocked((hdr, items, row_ptr, row_items), ip, ix, _N, _B, _IE, _RE, 1, n_items=len(items) - 1)
    hdr2 = hdr.copy()
    hdr2[3] = 1
    with pytest.raises(AssertionError, match="plan header"):
        prep_ref.check_blocked((hdr2, items, row_ptr, row_items), ip, ix, _N, _B, _IE, _RE, 1)


# ---- the decoders against buffers packed by the documented layouts --------------------------------
def _pad16(a):
    raw = np.ascontiguousarray(a).view(np.uint8).ravel()
    return np.concatenate([raw, np.zeros(-len(raw) % 16, np.uint8)])


def test_decode_blocked_reads_the_layout():
    ip, ix, n_cols = _named_graph("items600")
    n, B, ie, re_ = 600, 5, 7, 16
    hdr, items, row_ptr, row_items = _decoded(ip, ix, n_cols, B, ie, re_, 1)
    mi = int(hdr[6])
    it = np.zeros((mi, 4), np.int32)
    it[:len(items), :2] = items[:, 0].astype(np.int64).reshape(-1, 1).view(np.int32)
    it[:len(items), 2], it[:len(items), 3] = items[:, 1], items[:, 2]
    ri = np.full(mi, -1, np.int32)
    ri[:len(items)] = row_items
    fixed = [np.full(n, 7, np.int32), np.full(n * (B + 1), 7, np.int32), np.zeros(512, np.int32), np.zeros(256, np.int32),
             row_ptr, np.full(n * B, 7, np.int32), np.zeros(4097, np.int64), np.zeros(2 * 128 * 257, np.int32)]
    body = np.concatenate([_pad16(a) for a in fixed + [it]])
    hdr[7] = 128 + len(body)
    buf = np.concatenate([_pad16(hdr), body, _pad16(ri)])
    got = prep_ref.decode_blocked(buf, n, B)
    for g, w in zip(got, (hdr, items, row_ptr, row_items)):
        assert np.array_equal(g, w)
    prep_ref.check_blocked(got, ip, ix, n_cols, B, ie, re_, 1)


def _packed_row_plan(ip, chunk):
    n, nnz = len(ip) - 1, int(ip[-1])
    mi = n + -(-nnz // chunk)
    w_row, w_beg, w_end, w_splits = prep_ref.row_plan(ip, chunk)
    hdr = np.array([len(w_row), len(w_splits), chunk, n, 0, 0, 0, 0], np.int64)

    def grow(a, size, dtype):
        out = np.full(size, -1, dtype)
        out[:len(a)] = a.astype(np.uint32).view(np.int32) if dtype == np.int32 else a
        return out
    sp = w_splits[::-1]  # the device fills the split table in any order
    parts = [hdr, grow(w_row, mi, np.int32), grow(w_beg, mi, np.int64), grow(w_end, mi, np.int64)]
    parts += [grow(sp[:, c], n, np.int32) for c in range(3)]
    return np.concatenate([_pad16(a) for a in parts])


@pytest.mark.parametrize("chunk", [64, 512])
def test_row_plan_checker_accepts_and_rejects(chunk):
    n = 2049
    ip = np.concatenate([[0], np.cumsum(_row_plan_degrees(n, chunk))]).astype(np.int64)
    d = prep_ref.decode_row_plan(_packed_row_plan(ip, chunk), n, int(ip[-1]), chunk)
    prep_ref.check_row_plan(d, ip, chunk)
    hdr, item_row, item_beg, item_end, splits = d
    assert len(splits) == 3 and int(item_row[-1]) >> 31 == 1
    # a wrong item_beg after row 1,024 (a thread of the one-workgroup scan started from a wrong offset)
    k = int(np.flatnonzero((item_row & (prep_ref.SPLIT_BIT - 1)) > 1024)[0])
    bad_beg = item_beg.copy()
    bad_beg[k:] += 1
    with pytest.raises(AssertionError, match="item_beg differs"):
        prep_ref.check_row_plan((hdr, item_row, bad_beg, item_end, splits), ip, chunk)
    # a missing split entry: the table, and the table with its count
    with pytest.raises(AssertionError, match="decoded arrays of the wrong lengths"):
        prep_ref.check_row_plan((hdr, item_row, item_beg, item_end, splits[1:]), ip, chunk)
    hdr2 = hdr.copy()
    hdr2[1] -= 1
    with pytest.raises(AssertionError, match="n_split"):
        prep_ref.check_row_plan((hdr2, item_row, item_beg, item_end, splits[1:]), ip, chunk)
    dup = splits.copy()
    dup[0] = dup[1]
    with pytest.raises(AssertionError, match="split table"):
        prep_ref.check_row_plan((hdr, item_row, item_beg, item_end, dup), ip, chunk)
    no_bit = item_row.copy()
    no_bit[-1] &= prep_ref.SPLIT_BIT - 1
    with pytest.raises(AssertionError, match="item_row differs"):
        prep_ref.check_row_plan((hdr, no_bit, item_beg, item_end, splits), ip, chunk)
