"""Guard-band tests: every libgta entry point touches only the memory it is given.

tests/test_gpu_ops.py compares every kernel with the fp64 oracle on fresh contiguous tensors, where
a store past column F, past row M or past `*_workspace_bytes` lands in allocator slack and goes
unseen.  Here every tensor of a call is a view into one poisoned byte buffer (Arena):

  * regions are carved at byte offsets the test chooses (16-B aligned, 8 mod 16, 4 mod 8), with
    >= 4 KiB guard bands between them and at both ends;
  * the whole buffer starts as the 16-bit pattern 0x7FC1, a NaN as fp32 (0x7FC17FC1) and as bf16,
    so the same bytes poison the padding of inputs and are the canary around outputs (padded
    output regions hold 0x7FC2, a second NaN: poison that a kernel carries through arithmetic into
    an output's padding keeps its payload and would otherwise go unseen);
  * outputs are [rows, width] views with a leading dimension > width and rows behind them; after
    the call Arena.check(written=[...]) compares every byte outside the declared rows x width
    extents with a snapshot taken just before the call (bitwise, through a byte view): guard bands
    and padding still hold the pattern, inputs, plans and index arrays their contents;
  * index arrays carry in-range slack (indices -> n_cols, an extra NaN row of the table; indptr ->
    nnz), so a kernel that reads an index past the end gathers NaN instead of faulting, and every
    result is asserted finite and within the bound tests/test_gpu_ops.py uses for that op.

Layouts (pad in elements, base alignment): a = (4, 16 B) the widest vector form, b = (1, 16 B)
later rows misaligned -> the scalar / narrow form, c = (2, 8 mod 16) the middle form; index arrays
of layout c start 4 mod 8 (int32) / 8 mod 16 (int64).  Where the library refuses a layout the test
asserts the documented error and still checks the guards.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, graph as G, ops
from oracle import isa_ref

from .test_gpu_ops import _check

gpu = pytest.mark.gpu

PATTERN = 0x7FC1   # int16 fill: 0x7FC17FC1 is an fp32 NaN, 0x7FC1 a bf16 NaN
CANARY = 0x7FC2    # the same for output regions: a NaN too, but not the one a kernel gets by
                   # computing on input poison (the payload survives arithmetic), so poison carried
                   # into an output's padding changes its bytes
GUARD = 4096       # bytes between regions and at both ends
SLACK = 1024       # in-range elements behind every index array
LAYOUTS = {"a": (4, 0), "b": (1, 0), "c": (2, 8)}  # name -> (pad elements, base offset mod 16)
_IDX_MIS = {"a": (0, 0), "b": (0, 0), "c": (8, 4)}  # (int64, int32) index array base offsets


class Arena:
    """One byte buffer (CPU or device) from which a test carves named regions; see the module doc."""

    def __init__(self, device, capacity):
        capacity = (int(capacity) + 2 * GUARD + 63) // 64 * 64
        raw = torch.empty(capacity + 64, dtype=torch.uint8, device=device)
        shift = (-raw.data_ptr()) % 64
        self.buf = raw[shift:shift + capacity]  # 64-B aligned base: region offsets fix the alignment
        self.buf.view(torch.int16).fill_(PATTERN)
        self.cap = capacity
        self.cursor = GUARD
        self.regions = {}  # name -> (first byte, end byte)
        self.fill = {}     # name -> its 16-bit pattern
        self.snap = None

    # -- carving -----------------------------------------------------------------------------
    def raw(self, name, nbytes, mis=0):
        """nbytes at a byte offset == mis (mod 64), a guard band before and after: a uint8 view."""
        assert name not in self.regions and 0 <= mis < 64 and mis % 2 == 0
        start = (self.cursor + 63) // 64 * 64 + mis
        end = start + int(nbytes)
        assert end + GUARD <= self.cap, f"arena too small for {name}: {end + GUARD} > {self.cap}"
        self.regions[name] = (start, end)
        self.fill[name] = PATTERN
        self.cursor = end + GUARD
        return self.buf[start:end]

    def mat(self, name, rows, width, dtype=torch.float32, pad=0, mis=0, tail_rows=2):
        """A [rows, width] view with leading dimension width + pad and tail_rows more rows behind
        it inside the region; padding columns and tail rows keep the pattern (guards / NaN)."""
        es = torch.empty(0, dtype=dtype).element_size()
        ld = width + pad
        r = self.raw(name, (rows + tail_rows) * ld * es, mis)
        return r.view(dtype).view(rows + tail_rows, ld)[:rows, :width]

    def vec(self, name, n, dtype, slack=0, slack_fill=None, mis=0):
        """A contiguous [n] view followed by `slack` elements set to slack_fill (an in-range value)."""
        es = torch.empty(0, dtype=dtype).element_size()
        v = self.raw(name, (n + slack) * es, mis).view(dtype)
        if slack:
            v[n:].fill_(slack_fill)
        return v[:n]

    def table(self, name, arr, lay, dtype=torch.float32, tail_rows=2):
        """The numpy array arr [rows, width] as a padded view of layout lay."""
        pad, mis = LAYOUTS[lay]
        t = self.mat(name, arr.shape[0], arr.shape[1], dtype, pad, mis, tail_rows)
        t.copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(dtype))
        return t

    def out(self, name, rows, width, lay, dtype=torch.float32):
        pad, mis = LAYOUTS[lay]
        t = self.mat(name, rows, width, dtype, pad, mis)
        self.fill[name] = CANARY
        self.repoison(name)
        return t

    def repoison(self, name):
        s, e = self.regions[name]
        assert s % 2 == 0 and (e - s) % 2 == 0
        self.buf[s:e].view(torch.int16).fill_(self.fill[name])

    # -- checking ----------------------------------------------------------------------------
    def _sync(self):
        if self.buf.is_cuda:
            torch.cuda.synchronize()

    def seal(self):
        """Snapshot the buffer right before the call under test; the bands must hold the pattern."""
        self._sync()
        self.snap = self.buf.clone()
        band = torch.ones(self.cap, dtype=torch.bool, device=self.buf.device)
        for s, e in self.regions.values():
            band[s:e] = False
        pat = torch.tensor([PATTERN & 0xFF, PATTERN >> 8], dtype=torch.uint8, device=self.buf.device).repeat(self.cap // 2)
        assert not bool(((self.buf != pat) & band).any()), "a guard band was written before the call"

    def _extent(self, t):
        """(byte offset, rows, row bytes, pitch bytes) of a 1-D or row-major 2-D view of the buffer."""
        off = t.data_ptr() - self.buf.data_ptr()
        es = t.element_size()
        if t.dim() == 1:
            assert t.numel() <= 1 or t.stride(0) == 1
            return off, 1, t.numel() * es, t.numel() * es
        rows, width = t.shape
        assert width <= 1 or t.stride(1) == 1
        ld = t.stride(0) if rows > 1 else width
        return off, rows, width * es, ld * es

    def check(self, written=(), what=""):
        """Every byte outside the rows x width extents of the `written` views equals the snapshot."""
        assert self.snap is not None, "seal() before the call"
        self._sync()
        allowed = torch.zeros(self.cap, dtype=torch.bool, device=self.buf.device)
        for t in written:
            off, rows, rowb, pitch = self._extent(t)
            if rows == 0 or rowb == 0:
                continue
            assert 0 <= off and off + (rows - 1) * pitch + rowb <= self.cap, "a written view outside the arena"
            allowed.as_strided((rows, rowb), (pitch, 1), off).fill_(True)
        bad = (self.buf != self.snap) & ~allowed
        n_bad = int(bad.sum())
        if n_bad == 0:
            return
        first = int(bad.nonzero()[0])
        name, where = self._locate(first)
        raise AssertionError(f"{what}: {n_bad} byte(s) changed outside the written extents; first in or near "
                             f"region '{name}', {where}")

    def _locate(self, b):
        best = None
        for name, (s, e) in self.regions.items():
            d = 0 if s <= b < e else (s - b if b < s else b - e + 1)
            if best is None or d < best[0]:
                best = (d, name, s, e)
        _, name, s, e = best
        if s <= b < e:
            return name, f"byte +{b - s} inside it (padding or rows behind the written extent)"
        if b >= e:
            return name, f"byte +{b - e} of the band after it"
        return name, f"byte {b - s} of the band before it"


# ---------------------------------------------------------------------------------------------
# the arena catches what it is for (CPU: no device needed)
# ---------------------------------------------------------------------------------------------

def _cpu_arena():
    ar = Arena("cpu", 1 << 16)
    x = ar.mat("x", 5, 3, torch.float32, pad=2, mis=8)
    y = ar.mat("y", 4, 5, torch.float32, pad=4, mis=0)
    z = ar.mat("z", 6, 7, torch.bfloat16, pad=1, mis=4)
    x.copy_(torch.arange(15, dtype=torch.float32).view(5, 3))
    return ar, x, y, z


def test_arena_layout_and_in_bounds_write_passes():
    ar, x, y, z = _cpu_arena()
    assert x.data_ptr() % 16 == 8 and y.data_ptr() % 16 == 0 and z.data_ptr() % 8 == 4
    assert y.stride(0) == 9 and z.stride(0) == 8 and x.stride(0) == 5
    full = ar.buf[ar.regions["y"][0]:ar.regions["y"][1]].view(torch.float32)
    assert bool(torch.isnan(full).all()) and full.view(torch.int32)[0].item() == 0x7FC17FC1
    assert bool(torch.isnan(ar.buf.view(torch.bfloat16).float()).sum() == ar.cap // 2 - 15 * 2)
    o = ar.out("o", 3, 5, "c")  # an output region: the second NaN, in padding and rows behind it too
    s, e = ar.regions["o"]
    assert o.data_ptr() % 16 == 8 and o.stride(0) == 7 and e - s == 5 * 7 * 4
    assert bool((ar.buf[s:e].view(torch.int32) == 0x7FC27FC2).all()) and bool(torch.isnan(o).all())
    starts = sorted(ar.regions.values())
    assert starts[0][0] >= GUARD and ar.cap - starts[-1][1] >= GUARD
    assert all(b[0] - a[1] >= GUARD for a, b in zip(starts, starts[1:]))
    ar.seal()
    y.copy_(torch.ones(4, 5))
    z[5, 6] = 2.0
    ar.check(written=[y, z], what="in bounds")
    with pytest.raises(AssertionError, match="region 'z'"):
        ar.check(written=[y], what="z undeclared")
    ar.seal()
    x[2, 1] = -1.0
    with pytest.raises(AssertionError, match="region 'x'"):  # inputs must come back unchanged
        ar.check(written=[], what="input written")


def test_arena_catches_a_write_into_a_padding_column():
    ar, x, y, z = _cpu_arena()
    s, e = ar.regions["y"]
    full = ar.buf[s:e].view(torch.float32).view(6, 9)
    ar.seal()
    y.fill_(3.0)
    full[1, 5] = 3.0  # column width = 5 of a [4, 5] view with ld 9: the first padding column
    with pytest.raises(AssertionError) as ei:
        ar.check(written=[y], what="pad")
    msg = str(ei.value)
    assert "region 'y'" in msg and "4 byte(s)" in msg and f"byte +{(1 * 9 + 5) * 4} inside" in msg
    ar.seal()
    full[4, 0] = 1.0  # a row behind the 4 written rows
    with pytest.raises(AssertionError, match=rf"region 'y', byte \+{4 * 9 * 4} inside"):
        ar.check(written=[y], what="row group past M")


def test_arena_catches_a_write_into_the_band_after_a_region():
    ar, x, y, z = _cpu_arena()
    s, e = ar.regions["z"]
    assert (e - s) == 8 * 8 * 2
    ar.seal()
    z.fill_(1.0)
    ar.buf[e + 6:e + 8].view(torch.bfloat16)[0] = 1.0  # one bf16 element, 6 bytes past the region
    with pytest.raises(AssertionError) as ei:
        ar.check(written=[z], what="band")
    msg = str(ei.value)
    assert "region 'z'" in msg and "byte +6 of the band after it" in msg and "2 byte(s)" in msg
    with pytest.raises(AssertionError, match="guard band was written before"):
        ar.seal()  # a dirty band is never taken as the snapshot
    ar, x, y, z = _cpu_arena()
    ar.seal()
    ar.buf[ar.regions["x"][0] - 3] = 0  # just before the first region
    with pytest.raises(AssertionError, match=r"region 'x', byte -3 of the band before it"):
        ar.check(written=[x, y, z], what="band before")


# ---------------------------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------------------------

CAP = 48 << 20  # bytes per device arena (the largest case carves ~21 MB)
LAYOUTS["a8"] = (8, 0)  # bf16 tables: 8 elements = 16 B of padding
_IDX_MIS["a8"] = (0, 0)
_MEMO = {}  # expected values and inputs, computed once and shared by the layouts of a test
_START = {}


@pytest.fixture(scope="module", autouse=True)
def _knobs_unchanged():
    """A leaked knob would change later tests: the module leaves ops.knob_state() as it found it."""
    _START["state"] = ops.knob_state()
    _START["mm"] = (ops.MM_FORM, ops.MM_ROWS_MIN_M, ops.APPLY_EDGE_FLAT)
    yield
    assert ops.knob_state() == _START["state"]
    assert (ops.MM_FORM, ops.MM_ROWS_MIN_M, ops.APPLY_EDGE_FLAT) == _START["mm"]


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


def _p(t):
    return None if t is None else t.data_ptr()


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _ok(got, ref, scale, what):
    """Finite (no poison reached the result) and within test_gpu_ops' bound 1e-5 * scale + 1e-6."""
    g = got.detach().float().cpu().numpy()
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} non-finite outputs (poison was read and used)"
    _check(got.detach().float(), ref, scale, what)


def _bf(a):
    """a rounded to bf16 (RNE), as float32."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def _csr(n, e, seed, n_cols=None, heavy=700, empty=5, last=1, sort=False, heavy_last=False):
    """A CSR with one `heavy`-edge row, empty rows and a short (or empty, or the heavy) last row."""
    def make():
        rng = np.random.default_rng(seed)
        deg = rng.multinomial(e, np.full(n, 1.0 / n))
        if empty:
            deg[rng.choice(n - 1, empty, replace=False)] = 0
        if heavy:
            deg[n - 1 if heavy_last else n // 2] = heavy
        if last is not None and not heavy_last:
            deg[-1] = last
        ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        ix = rng.integers(0, n if n_cols is None else n_cols, int(ip[-1])).astype(np.int32)
        if sort:
            for r in range(n):
                ix[ip[r]:ip[r + 1]].sort()
        return ip, ix
    return _memo(("csr", n, e, seed, n_cols, heavy, empty, last, sort, heavy_last), make)


def _graph_in(ar, ip, ix, n_cols, lay, name="g"):
    """The CSR as views of the arena; the slack behind indptr holds nnz (empty rows) and the slack
    behind indices n_cols (the NaN row behind every source table), so an index read past the end
    stays inside an allocation and poisons the result."""
    m64, m32 = _IDX_MIS[lay]
    n, nnz = len(ip) - 1, len(ix)
    ipv = ar.vec(name + ".indptr", n + 1, torch.int64, SLACK, nnz, m64)
    ixv = ar.vec(name + ".indices", nnz, torch.int32, SLACK, n_cols, m32)
    ipv.copy_(torch.from_numpy(ip))
    ixv.copy_(torch.from_numpy(ix))
    g = G.Graph(ipv, ixv, n_cols=n_cols)
    assert g.indptr.data_ptr() == ipv.data_ptr() and g.indices.data_ptr() == ixv.data_ptr()
    return g


def _refused(ar, fn, exc, pattern, what):
    """fn() must be refused on the host with exactly this error, and write nothing."""
    ar.seal()
    with pytest.raises(exc, match=pattern):
        fn()
    ar.check([], what + " (refused)")


# ---------------------------------------------------------------------------------------------
# aggregate
# ---------------------------------------------------------------------------------------------

N_AGG, E_AGG = 130, 3000


def _agg_heads(F):
    return sorted({1, F} | set([h for h in (8, 4, 2) if F % h == 0 and h < F][:1]))


def _agg_data(F):
    def make():
        ip, ix = _csr(N_AGG, E_AGG, 1)
        rng = np.random.default_rng(100 + F)
        d = {"ip": ip, "ix": ix, "x": rng.standard_normal((N_AGG, F)).astype(np.float32),
             "xs": rng.standard_normal((N_AGG, F)).astype(np.float32),
             "xe": rng.standard_normal((len(ix), F)).astype(np.float32),
             "rs": (1.0 / np.maximum(np.diff(ip), 1)).astype(np.float32),
             "y0": rng.standard_normal((N_AGG, F)).astype(np.float32)}
        for h in _agg_heads(F) + [4]:
            d["w", h] = rng.random((len(ix), h)).astype(np.float32)
        return d
    return _memo(("aggdata", F), make)


def _agg_ref(F, mode, h, rs, bf=False):
    def make():
        d = _agg_data(F)
        x = d["xe"] if mode == "edge" else d["x"]
        if bf:
            x = _bf(x)
        w = None if h is None else d["w", h]
        r = d["rs"] if rs else None
        return (isa_ref.aggregate(d["ip"], d["ix"], x, mode, w, r), isa_ref.aggregate_abs(d["ip"], d["ix"], x, mode, w, r))
    return _memo(("aggref", F, mode, h, rs, bf), make)


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("F", [3, 100, 128, 130, 256, 602])
def test_aggregate_f32(dev, F, lay):
    """gta_aggregate, fp32 rows: x_mode src / dst / edge, per-row and chunk-64 plan (a 700-edge row:
    k_aggregate_combine writes), no / head / one / full-width weights, accumulate, row_scale.

    x_mode dst without weights sums deg copies of ONE value: the roundings of its running fp32 sum
    all fall the same way, up to (deg - 1) * 2^-24 of the sum (4.2e-5 at the 700-edge row), above
    the 1e-5 * sum|terms| that holds for the oracle tests' random terms.  So the per-row dst form
    runs with weights (random terms), and the unweighted dst form under the chunk-64 plan, where a
    partial sums <= 64 copies (3.8e-6) and the combine kernel adds the 11 partials."""
    d = _agg_data(F)
    n, hs = N_AGG, _agg_heads(F)
    ar = Arena(dev, CAP)
    g = _graph_in(ar, d["ip"], d["ix"], n, lay)
    xt, xet = ar.table("x", d["x"], lay), ar.table("xe", d["xe"], lay)
    wt = {h: ar.table(f"w{h}", d["w", h], lay) for h in hs}
    rst = ar.vec("row_scale", n, torch.float32)
    rst.copy_(torch.from_numpy(d["rs"]))
    y = ar.out("y", n, F, lay)
    V = [("src", h, p, False, False) for h in [None] + hs for p in (None, 64)]
    V += [("src", None, 64, True, True), ("src", 1, None, True, False), ("dst", None, 64, False, False),
          ("dst", hs[-2] if len(hs) > 2 else 1, None, False, True), ("dst", 1, 64, False, False),
          ("edge", None, 64, False, False),
          ("edge", F, None, False, False), ("edge", 1, 64, False, False)]
    for mode, h, plan, acc, rs in V:
        what = f"aggregate F={F} lay={lay} {mode} h={h} plan={plan} acc={acc} rs={rs}"
        ar.repoison("y")
        if acc:
            y.copy_(torch.from_numpy(d["y0"]))
        ar.seal()
        ops.aggregate(g, xet if mode == "edge" else xt, mode, None if h is None else wt[h],
                      row_scale=rst if rs else None, out=y, accumulate=acc, plan=plan)
        ar.check([y], what)
        ref, ab = _agg_ref(F, mode, h, rs)
        if acc:
            ref, ab = ref + d["y0"], ab + np.abs(d["y0"])
        _ok(y, ref, ab, what)


@gpu
@pytest.mark.parametrize("lay", ["a", "a8", "b", "c"])
@pytest.mark.parametrize("F", [8, 12, 36, 100, 200])
def test_aggregate_bf16_rows(dev, F, lay):
    """bf16 x: the 16-B-piece form (agg_bf16_vw8 4 / 8, the last lane's piece clamped inside the row)
    where the layout admits it and the 8-B / element forms elsewhere, src / dst, per-row and plan."""
    d = _agg_data(F)
    n = N_AGG
    ar = Arena(dev, CAP)
    g = _graph_in(ar, d["ip"], d["ix"], n, lay)
    xt = ar.table("x", d["x"], lay, torch.bfloat16)
    wt = {h: ar.table(f"w{h}", d["w", h], lay if lay != "a8" else "a") for h in (1, 4)}
    y = ar.out("y", n, F, lay)
    for vw8 in (4, 8, 0):
        with _knobs(agg_bf16_vw8=vw8):
            for mode in ("src", "dst"):
                for h in (None, 1, 4):
                    for plan in (None, 64):
                        what = f"aggregate bf16 F={F} lay={lay} vw8={vw8} {mode} h={h} plan={plan}"
                        ar.repoison("y")
                        ar.seal()
                        ops.aggregate(g, xt, mode, None if h is None else wt[h], out=y, plan=plan)
                        ar.check([y], what)
                        _ok(y, *_agg_ref(F, mode, h, False, bf=True), what)


@gpu
@pytest.mark.parametrize("lay", ["a", "a8", "b", "c"])
@pytest.mark.parametrize("F", [36, 100, 128])
def test_aggregate_self_term(dev, F, lay):
    """gta_aggregate_self with fp32 and bf16 y at every width (the F <= 40 band of
    test_aggregate_self_term_bf16_out, generalised): fp32 / bf16 x, per-row and plan (the combine
    kernel's store), row_scale.  The bf16 y is the RNE rounding of the fp32 y, bitwise."""
    d = _agg_data(F)
    n = N_AGG
    sval = np.float32(1.1)
    for xdt in (torch.float32, torch.bfloat16):
        ar = Arena(dev, CAP)
        g = _graph_in(ar, d["ip"], d["ix"], n, lay)
        xt, xst = ar.table("x", d["x"], lay, xdt), ar.table("xs", d["xs"], lay, xdt)
        w1 = ar.table("w1", d["w", 1], lay if lay != "a8" else "a")
        rst = ar.vec("row_scale", n, torch.float32)
        rst.copy_(torch.from_numpy(d["rs"]))
        s = ar.vec("s", 1, torch.float32)
        s.fill_(float(sval))
        y32, y16 = ar.out("y32", n, F, lay), ar.out("y16", n, F, lay, torch.bfloat16)
        bf = xdt == torch.bfloat16
        xs = (_bf(d["xs"]) if bf else d["xs"]).astype(np.float64) * np.float64(sval)
        for h in (None, 1):
            for plan in (None, 64):
                for rs in (False, True):
                    what = f"aggregate_self F={F} lay={lay} x={xdt} h={h} plan={plan} rs={rs}"
                    for y, odt in ((y32, torch.float32), (y16, torch.bfloat16)):
                        ar.repoison("y32" if y is y32 else "y16")
                        ar.seal()
                        ops.aggregate(g, xt, "src", None if h is None else w1, row_scale=rst if rs else None, out=y,
                                      plan=plan, self_term=(xst, s), out_dtype=odt)
                        ar.check([y], what + f" y={odt}")
                    ref, ab = _agg_ref(F, "src", h, rs, bf=bf)
                    _ok(y32, xs + ref, np.abs(xs) + ab, what)
                    assert torch.equal(y16, y32.to(torch.bfloat16)), what + ": bf16 y != RNE(fp32 y)"


# ---------------------------------------------------------------------------------------------
# aggregate_expr (no out= in ops: the ABI directly)
# ---------------------------------------------------------------------------------------------

EXPR = {  # shape -> (operand modes, bins, sfs)
    1: (("src", "dst"), ("MUL",), ("TANH",)),
    2: (("src", "dst", "edge"), ("ADD", "MUL"), ("RELU", "NONE")),
    3: (("edge", "src", "row", "dst"), ("MUL", "ADD", "ADD"), ("NONE", "SIGMOID", "NONE")),
}
_EXPR_BIN = {"ADD": _lib.BIN_ADD, "MUL": _lib.BIN_MUL}


def _expr_data(F):
    def make():
        ip, ix = _csr(N_AGG, E_AGG, 1)
        rng = np.random.default_rng(300 + F)
        rows = {"src": N_AGG, "dst": N_AGG, "edge": len(ix), "row": 1}
        d = {m: rng.standard_normal((r, F)).astype(np.float32) for m, r in rows.items()}
        d["src2"] = rng.standard_normal((N_AGG, F)).astype(np.float32)
        return d
    return _memo(("exprdata", F), make)


def _expr_ref(F, shape):
    """fp64 value of the expression's gather and the scale of its fp32 error: every step is rounded
    to fp32 (<= 2^-24 of its operands' magnitudes, a few ulp for tanh / sigmoid, whose slopes are
    <= 1 and <= 1/4), so per edge the error is a small multiple of 2^-24 * m(e) with m(e) the
    magnitudes entering the last step; the bound is the aggregates' 1e-5 * sum m(e) + 1e-6."""
    def make():
        ip, ix = _csr(N_AGG, E_AGG, 1)
        d = _expr_data(F)
        E = {m: isa_ref.edge_operand(ip, ix, d[m].astype(np.float64), m) for m in ("src", "dst", "edge")}
        row = np.broadcast_to(d["row"].astype(np.float64), E["edge"].shape)
        if shape == 1:
            p = E["src"] * E["dst"]
            t, m = np.tanh(p), np.abs(p) + 1.0
        elif shape == 2:
            t = np.maximum(E["src"] + E["dst"], 0.0) * E["edge"]
            m = (np.abs(E["src"]) + np.abs(E["dst"])) * np.abs(E["edge"])
        else:
            u = E["edge"] * E["src"]
            t = u + 1.0 / (1.0 + np.exp(-(row + E["dst"])))
            m = np.abs(u) + np.abs(row) + np.abs(E["dst"]) + 1.0
        return isa_ref.gather_add(ip, t), isa_ref.gather_add(ip, m)
    return _memo(("exprref", F, shape), make)


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c", "mixed"])
@pytest.mark.parametrize("F", [64, 128, 256, 100, 102, 200])
def test_aggregate_expr(dev, F, lay):
    """gta_aggregate_expr shapes 1-3 with and without a chunk-64 plan: k_agg_expr (rows that exactly
    fill a wave: F = 128 at 8 B per lane, F = 256 at 16 B) and k_aggregate's expression form (F = 64,
    100; F = 102 and 200, whose 51 / 50 lanes of a 64-lane row once took the unmasked k_agg_expr and
    stored past column F).  The fused gather has kernels for 16-B lanes and for 8-B lanes
    filling a wave: y rows that admit neither (layout b; layout c at F = 64) and operands narrower
    than y's vector width ("mixed": y of layout a, operands of layout b) are GTA_ERR_UNSUPPORTED."""
    import ctypes
    L = _lib.load()
    d = _expr_data(F)
    ip, ix = _csr(N_AGG, E_AGG, 1)
    ar = Arena(dev, CAP)
    ylay, olay = ("a", "b") if lay == "mixed" else (lay, lay)
    g = _graph_in(ar, ip, ix, N_AGG, ylay)
    T = {m: ar.table(m, d[m], olay) for m in ("src", "dst", "edge", "row")}
    y = ar.out("y", N_AGG, F, ylay)
    refused = lay in ("b", "mixed") or (lay == "c" and F == 64)
    plan = g.plan(64)
    for shape, (modes, bins, sfs) in EXPR.items():
        ptrs, cm, lds = (ctypes.c_void_p * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int64 * 4)()
        for l, m in enumerate(modes):
            ptrs[l] = T[m].data_ptr()
            cm[l] = {"src": _lib.IDX_SRC, "dst": _lib.IDX_DST, "edge": _lib.IDX_EDGE, "row": _lib.IDX_EDGE}[m]
            lds[l] = 0 if m == "row" else T[m].stride(0)
        cb = (ctypes.c_int * 3)(*([_EXPR_BIN[b] for b in bins] + [0] * (3 - len(bins))))
        cs = (ctypes.c_int * 3)(*([_lib.SF[s] for s in sfs] + [0] * (3 - len(sfs))))
        for pl in (None, plan):
            what = f"aggregate_expr F={F} lay={lay} shape={shape} plan={pl is not None}"
            ar.repoison("y")
            ar.seal()
            rc = L.gta_aggregate_expr(_p(g.indptr), _p(g.indices), g.n_rows, g.nnz, shape, ptrs, cm, lds, cb, cs, 0, F,
                                      _p(y), y.stride(0), _p(pl.buf) if pl else None, 64 if pl else 0,
                                      _p(pl.workspace(F)) if pl else None, _st(dev))
            if refused:
                assert rc == _lib.ERR_UNSUPPORTED, f"{what}: rc {rc} {L.gta_last_error()}"
                assert b"aggregate" in L.gta_last_error()
                ar.check([], what)
                continue
            assert rc == 0, f"{what}: {L.gta_last_error()}"
            ar.check([y], what)
            _ok(y, *_expr_ref(F, shape), what)


# ---------------------------------------------------------------------------------------------
# column-blocked aggregates
# ---------------------------------------------------------------------------------------------

def _blk_data(F):
    def make():
        ip, ix = _csr(N_AGG, E_AGG, 2, sort=True)
        rng = np.random.default_rng(500 + F)
        H = F // 16
        d = {"ip": ip, "ix": ix, "x": rng.standard_normal((N_AGG, F)).astype(np.float32),
             "y0": rng.standard_normal((N_AGG, F)).astype(np.float32),
             "rs": (1.0 / np.maximum(np.diff(ip), 1)).astype(np.float32), "H": H,
             "a": rng.standard_normal((N_AGG, H)).astype(np.float32),
             "b": rng.standard_normal((N_AGG, H)).astype(np.float32)}
        for h in (1, H):
            d["w", h] = rng.random((len(ix), h)).astype(np.float32)
        return d
    return _memo(("blkdata", F), make)


def _blk_ref(F, h, rs):
    def make():
        d = _blk_data(F)
        w = None if h is None else d["w", h]
        r = d["rs"] if rs else None
        return isa_ref.aggregate(d["ip"], d["ix"], d["x"], "src", w, r), isa_ref.aggregate_abs(d["ip"], d["ix"], d["x"], "src", w, r)
    return _memo(("blkref", F, h, rs), make)


def _gat_ref(F, normalize, key="blkdata", data=None):
    def make():
        d = data or _blk_data(F)
        ip, ix, H = d["ip"], d["ix"], d["H"]
        x, a, b = (d[k].astype(np.float64) for k in ("x", "a", "b"))
        ref, rsum = isa_ref.gat_aggregate(ip, ix, x, a, b, "EXP_LEAKY_RELU", normalize)
        v, _ = isa_ref.edge_softmax(ip, ix, a, b, "EXP_LEAKY_RELU", False)
        scale = isa_ref.aggregate(ip, ix, np.abs(x), "src", v)
        if normalize:  # test_gat_aggregate_blocked_matches_oracle's bound
            scale = scale / np.repeat(np.where(rsum > 0, rsum, 1.0), F // H, axis=1) * 4
        return ref, scale, rsum
    return _memo(("gatref", key, F, normalize), make)


@gpu
@pytest.mark.parametrize("lay", ["a", "b"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_aggregate_blocked(dev, F, lay):
    """gta_aggregate_blocked: quarter / half-wave items (layout a; seg_lean on and off) and the
    one-item-per-wave form (layout b at F = 64); blocks 1 / 5, item_edges 7 / 64, accumulate with
    row_scale.  Layout b at F = 128 / 256 has no aligned vector width of F / 64: refused."""
    d = _blk_data(F)
    n, H = N_AGG, d["H"]
    ar = Arena(dev, CAP)
    g = _graph_in(ar, d["ip"], d["ix"], n, lay)
    xt = ar.table("x", d["x"], lay)
    wt = {h: ar.table(f"w{h}", d["w", h], lay) for h in (1, H)}
    rst = ar.vec("row_scale", n, torch.float32)
    rst.copy_(torch.from_numpy(d["rs"]))
    y = ar.out("y", n, F, lay)
    refused = lay == "b" and F != 64
    hs = [None, H] + ([1] if lay == "a" and F == 128 else [])  # one weight per edge: the half-wave form's
    for blocks in (1, 5):
        for ie in (7, 64):
            plan = g.blocked_plan(blocks, ie)
            for lean in (1, 0):
                with _knobs(seg_lean=lean):
                    for h, acc in [(h, False) for h in hs] + [(H, True)]:
                        what = f"aggregate_blocked F={F} lay={lay} B={blocks} items={ie} seg_lean={lean} h={h} acc={acc}"
                        call = lambda: ops.aggregate_blocked(g, xt, None if h is None else wt[h], rst if acc else None,
                                                             out=y, accumulate=acc, plan=plan, blocks=blocks)
                        ar.repoison("y")
                        if acc:
                            y.copy_(torch.from_numpy(d["y0"]))
                        if refused:
                            _refused(ar, call, _lib.GTAError, r"\(-3\): aggregate_blocked: F must be 64, 128 or 256", what)
                            continue
                        ar.seal()
                        call()
                        ar.check([y], what)
                        ref, ab = _blk_ref(F, h, acc)
                        if acc:
                            ref, ab = ref + d["y0"], ab + np.abs(d["y0"])
                        _ok(y, ref, ab, what)


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "mixed"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_gat_aggregate_blocked(dev, F, lay):
    """gta_gat_aggregate_blocked: y and sums, normalize on / off, sf_out, att_lean on and off.  It
    needs 16-B x rows: layout b is refused; "mixed" keeps x in layout a and puts a_dst, b_src and y
    in layout b (y rows then admit F / 64 floats per lane only at F = 64)."""
    d = _blk_data(F)
    n, H = N_AGG, d["H"]
    ar = Arena(dev, CAP)
    xlay, olay = ("a", "b") if lay == "mixed" else (lay, lay)
    g = _graph_in(ar, d["ip"], d["ix"], n, xlay)
    xt = ar.table("x", d["x"], xlay)
    at, bt = ar.table("a_dst", d["a"], olay), ar.table("b_src", d["b"], olay)
    y = ar.out("y", n, F, olay)
    sums = ar.mat("sums", n, H)  # contiguous by contract: only the bands around it are guards
    refused = lay == "b" or (lay == "mixed" and F != 64)
    for blocks in (1, 5):
        for ie in (7, 64):
            plan = g.blocked_plan(blocks, ie)
            for lean in (1, 0):
                with _knobs(att_lean=lean):
                    for normalize, sf_out, ws in ((True, None, True), (False, None, True), (True, "RELU", False)):
                        what = f"gat_aggregate_blocked F={F} lay={lay} B={blocks} items={ie} att_lean={lean} " \
                               f"norm={normalize} sf_out={sf_out}"
                        call = lambda: ops.gat_aggregate_blocked(g, xt, at, bt, normalize=normalize, out=y,
                                                                 sums=sums if ws else None, plan=plan, blocks=blocks,
                                                                 sf_out=sf_out)
                        ar.repoison("y")
                        ar.repoison("sums")
                        if refused:
                            _refused(ar, call, _lib.GTAError, r"\(-3\): gat_aggregate_blocked: F in \{64,128,256\}, 16-B rows",
                                     what)
                            continue
                        ar.seal()
                        call()
                        ar.check([y] + ([sums] if ws else []), what)
                        ref, scale, rsum = _gat_ref(F, normalize)
                        _ok(y, np.maximum(ref, 0.0) if sf_out else ref, scale, what)
                        if ws:
                            _ok(sums, rsum, rsum, what + " sums")


# ---------------------------------------------------------------------------------------------
# gather / scatter / element-wise ops / edge softmax
# ---------------------------------------------------------------------------------------------

NC_G = 97  # source columns of the rectangular graph (!= its 130 rows)


def _close(got, ref, what):
    """test_apply_edge / test_apply_node's bound, on a finite result."""
    g = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all(), f"{what}: non-finite outputs (poison was read and used)"
    assert np.allclose(g, ref, rtol=2e-6, atol=1e-6), f"{what}: max err {np.abs(g - ref).max():.3e}"


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("F", [1, 16, 130])
def test_gather_add(dev, F, lay):
    ip, ix = _csr(N_AGG, E_AGG, 3, n_cols=NC_G)
    xe = _memo(("gxe", F), lambda: np.random.default_rng(F).standard_normal((len(ix), F)).astype(np.float32))
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, NC_G, lay)
    xet = ar.table("xe", xe, lay)
    yr, yc = ar.out("yR", N_AGG, F, lay), ar.out("yC", NC_G, F, lay)
    for direction, y in (("R", yr), ("C", yc)):
        ref = _memo(("gref", F, direction), lambda: (isa_ref.gather_add(ip, xe, direction, ix, NC_G),
                                                     isa_ref.gather_add(ip, np.abs(xe), direction, ix, NC_G)))
        if direction == "C":
            g.csc()  # built outside the sealed call: its buffers are the library user's, not the arena's
        for acc in (False, True):
            what = f"gather_add {direction} F={F} lay={lay} acc={acc}"
            ar.repoison("y" + direction)
            if acc:
                y.fill_(1.5)
            ar.seal()
            ops.gather_add(g, xet, out=y, accumulate=acc, direction=direction)
            ar.check([y], what)
            _ok(y, ref[0] + (1.5 if acc else 0.0), ref[1] + (1.5 if acc else 0.0), what)
    # direction C on the ABI, the CSC view in the arena too: the slack behind perm names the NaN
    # row behind xe, the slack behind colptr holds nnz
    L = _lib.load()
    nnz = len(ix)
    m64, m32 = _IDX_MIS[lay]
    colptr = ar.vec("colptr", NC_G + 1, torch.int64, SLACK, nnz, m64)
    perm = ar.vec("perm", nnz, torch.int32, SLACK, nnz, m32)
    c = g.csc()
    colptr.copy_(c.colptr)
    perm.copy_(c.perm)
    ar.repoison("yC")
    ar.seal()
    rc = L.gta_gather_add(_lib.DIR_C, _p(g.indptr), N_AGG, nnz, _p(colptr), _p(perm), NC_G, _p(xet), xet.stride(0), F, _p(yc),
                          yc.stride(0) if NC_G > 1 else F, 0, _st(dev))
    assert rc == 0, L.gta_last_error()
    ar.check([yc], f"gather_add C (ABI) F={F} lay={lay}")
    _ok(yc, *_memo(("gref", F, "C"), None), f"gather_add C (ABI) F={F} lay={lay}")


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("F", [1, 3, 128, 602])
def test_scatter(dev, F, dtype, lay):
    ip, ix = _csr(N_AGG, E_AGG, 3, n_cols=NC_G)
    xr, xc = _memo(("sx", F), lambda: tuple(_bf(np.random.default_rng(F + i).standard_normal((r, F)).astype(np.float32))
                                            for i, r in enumerate((N_AGG, NC_G))))
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, NC_G, lay)
    tr, tc = ar.table("xR", xr, lay, dtype), ar.table("xC", xc, lay, dtype)
    out = ar.out("out", len(ix), F, lay, dtype)
    for direction, t, x in (("R", tr, xr), ("C", tc, xc)):
        what = f"scatter {direction} F={F} {dtype} lay={lay}"
        ar.repoison("out")
        ar.seal()
        ops.scatter(g, t, direction, out=out)
        ar.check([out], what)
        assert np.array_equal(out.float().cpu().numpy(), isa_ref.scatter(ip, ix, x, direction)), what  # bit-exact copy


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("form", ["generic", "sweep", "flat"])
@pytest.mark.parametrize("Fo", [1, 3, 8, 48, 128, 602])
def test_apply_edge(dev, Fo, form, lay):
    """The three forms test_apply_edge_forms_agree switches between (flat applies at Fo = 128 on
    aligned rows; elsewhere ops takes the row-sweep entry): same-width operands, a head-broadcast
    b and a broadcast row."""
    ip, ix = _csr(N_AGG, E_AGG, 3, n_cols=NC_G)
    Fh = Fo // 8 if Fo % 8 == 0 else 1

    def data():
        rng = np.random.default_rng(700 + Fo)
        return {"dst": rng.standard_normal((N_AGG, Fo)).astype(np.float32), "src": rng.standard_normal((NC_G, Fo)).astype(np.float32),
                "edge": rng.standard_normal((len(ix), Fo)).astype(np.float32), "srch": rng.standard_normal((NC_G, Fh)).astype(np.float32),
                "row": rng.standard_normal((1, Fo)).astype(np.float32)}
    d = _memo(("aedata", Fo), data)
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, NC_G, lay)
    T = {k: ar.table(k, v, lay) for k, v in d.items()}
    out = ar.out("out", len(ix), Fo, lay)
    if form == "flat":
        g.row_of_edge()
    old = ops.APPLY_EDGE_FLAT
    try:
        ops.APPLY_EDGE_FLAT = form == "flat"
        with _knobs(apply_edge_form=0 if form == "generic" else 1):
            for a, am, b, bm, brow in (("src", "src", "dst", "dst", False), ("edge", "edge", "srch", "src", False),
                                       ("dst", "dst", "row", "edge", True)):
                what = f"apply_edge Fo={Fo} {form} lay={lay} a={a} b={b}"
                ar.repoison("out")
                ar.seal()
                ops.apply_edge(g, "MUL", "LEAKY_RELU", T[a], am, T[b], bm, out=out, b_broadcast_row=brow)
                ar.check([out], what)
                ref = _memo(("aeref", Fo, a, b), lambda: isa_ref.apply_edge(ip, ix, "MUL", "LEAKY_RELU", d[a], am, d[b], bm, brow))
                _close(out, ref, what)
    finally:
        ops.APPLY_EDGE_FLAT = old


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_apply_edge_flat(dev, F, lay):
    """gta_apply_edge_flat directly, an edge count that is no multiple of 8: rows must be aligned to
    F / 64 floats, so layout b (F = 128, 256) and layout c (F = 256) are GTA_ERR_UNSUPPORTED."""
    L = _lib.load()
    ip, ix = next(c for c in (_csr(N_AGG, E_AGG, 3, n_cols=NC_G, last=k) for k in (1, 2, 3)) if len(c[1]) % 8)
    nnz = len(ix)

    def data():
        rng = np.random.default_rng(800 + F)
        return rng.standard_normal((N_AGG, F)).astype(np.float32), rng.standard_normal((NC_G, F // 8)).astype(np.float32)
    a, b = _memo(("aefdata", F), data)
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, NC_G, lay)
    er = ar.vec("edge_rows", nnz, torch.int32, SLACK, N_AGG, _IDX_MIS[lay][1])  # slack: the NaN row behind a
    er.copy_(torch.from_numpy(isa_ref.row_of_edge(ip).astype(np.int32)))
    at, bt = ar.table("a", a, lay), ar.table("b", b, lay)
    out = ar.out("out", nnz, F, lay)
    what = f"apply_edge_flat F={F} lay={lay} nnz={nnz}"
    ar.seal()
    rc = L.gta_apply_edge_flat(_lib.BIN_ADD, _lib.SF["EXP"], _p(er), _p(g.indices), nnz, _p(at), _lib.IDX_DST, at.stride(0), F,
                               _p(bt), _lib.IDX_SRC, bt.stride(0), F // 8, _p(out), out.stride(0), _st(dev))
    if (lay == "b" and F != 64) or (lay == "c" and F == 256):
        assert rc == _lib.ERR_UNSUPPORTED and b"apply_edge_flat: the output must be 64, 128 or 256 columns" in L.gta_last_error()
        ar.check([], what)
        return
    assert rc == 0, L.gta_last_error()
    ar.check([out], what)
    g64 = out.cpu().numpy().astype(np.float64)
    ref = isa_ref.apply_edge(ip, ix, "ADD", "EXP", a, "dst", b, "src")
    assert np.isfinite(g64).all() and np.allclose(g64, ref, rtol=1e-5, atol=1e-5), what  # test_apply_edge_flat_bitwise's bound


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("vec", [1, 0])
@pytest.mark.parametrize("adt", [torch.float32, torch.bfloat16])
def test_apply_node(dev, adt, vec, lay):
    """k_apply_node4 (layout a, and c never: rows 8 mod 16) and the generic kernel, fp32 and bf16 a:
    same-shape b, one value per node, one broadcast row, no b, a head-broadcast b."""
    n = 301
    ar = Arena(dev, CAP)
    with _knobs(apply_node_vec=vec):
        for Fa, Fb, bcast, bin_kind, sf in ((100, 100, False, "ADD", None), (128, 1, False, "MUL", "ELU"), (100, 1, True, "MUL", None),
                                            (128, None, False, None, "RELU"), (128, 16, False, "ADD", None), (3, 3, False, "SUB", "SIGMOID")):
            def data():
                rng = np.random.default_rng(Fa + (Fb or 0))
                return (_bf(rng.standard_normal((n, Fa)).astype(np.float32)),
                        None if Fb is None else (rng.random((1 if bcast else n, Fb)) + 0.5).astype(np.float32))
            a, b = _memo(("andata", Fa, Fb, bcast), data)
            tag = f"{Fa}_{Fb}_{int(bcast)}"
            at = ar.table("a" + tag, a, lay, adt)
            bt = None if b is None else ar.table("b" + tag, b, lay)
            out = ar.out("out" + tag, n, max(Fa, Fb or 0), lay)
            what = f"apply_node {adt} vec={vec} lay={lay} Fa={Fa} Fb={Fb} bcast={bcast}"
            ar.seal()
            ops.apply_node(bin_kind, sf, at, bt, out=out, b_broadcast_row=bcast)
            ar.check([out], what)
            _close(out, _memo(("anref", Fa, Fb, bcast), lambda: isa_ref.apply_node(bin_kind, sf, a, b, b_broadcast_row=bcast)), what)


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("last", ["empty", "heavy"])
@pytest.mark.parametrize("heads", [1, 8, 64])
def test_edge_softmax(dev, heads, last, lay):
    """out and sums are contiguous by contract (their bands are the guards); a_dst / b_src are padded
    tables.  The edge-per-lane form (esm_lane, 8 heads on 16-B b rows) and the generic one."""
    ip, ix = _csr(N_AGG, E_AGG, 4, n_cols=NC_G, last=0, heavy_last=last == "heavy")
    a, b = _memo(("esm", heads), lambda: tuple(np.random.default_rng(heads + i).standard_normal((r, heads)).astype(np.float32)
                                               for i, r in enumerate((N_AGG, NC_G))))
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, NC_G, lay)
    at, bt = ar.table("a_dst", a, lay), ar.table("b_src", b, lay)
    out = ar.mat("out", len(ix), heads, mis=LAYOUTS[lay][1])
    sums = ar.mat("sums", N_AGG, heads, mis=LAYOUTS[lay][1])
    deg = np.diff(ip)[isa_ref.row_of_edge(ip)][:, None]
    for lane in (1, 0):
        with _knobs(esm_lane=lane):
            for normalize in (True, False):
                what = f"edge_softmax H={heads} last={last} lay={lay} esm_lane={lane} norm={normalize}"
                ar.repoison("out")
                ar.repoison("sums")
                ar.seal()
                ops.edge_softmax(g, at, bt, normalize=normalize, out=out, sums=sums)
                ar.check([out, sums], what)
                ref, rsum = _memo(("esmref", heads, last, normalize), lambda: isa_ref.edge_softmax(
                    ip, ix, a.astype(np.float64), b.astype(np.float64), "EXP_LEAKY_RELU", normalize))
                _ok(sums, rsum, rsum, what + " sums")
                _ok(out, ref, np.abs(ref) * np.maximum(deg, 1), what)  # test_edge_softmax_matches_oracle's bound


# ---------------------------------------------------------------------------------------------
# UPDATE: every GEMM form the knobs reach, and the fused MLP
# ---------------------------------------------------------------------------------------------

MM_FORMS = {  # name -> (ops.MM_FORM, knobs)
    "tile": ("tile", {}),
    "default": ("rows", {}),
    "rows": ("rows", {"mm_ring": 0, "mm_split": 0}),
    "ring_fr1": ("rows", {"mm_ring": 1, "mm_ring_fr": 1, "mm_split": 0}),
    "ring_fr2": ("rows", {"mm_ring": 1, "mm_ring_fr": 2, "mm_split": 0}),
    "wave": ("rows", {"mm_ring": 1, "mm_wave": 2, "mm_split": 0}),
    "wave_fr3": ("rows", {"mm_ring": 1, "mm_wave": 2, "mm_wave_fr": 3, "mm_split": 0}),
    "wave_fr4": ("rows", {"mm_ring": 1, "mm_wave": 2, "mm_wave_fr": 4, "mm_split": 0}),
    "split2": ("rows", {"mm_split": 2}),
    "split3": ("rows", {"mm_split": 3}),
}
MM_CASES = [(f, "f32") for f in MM_FORMS] + [(f, dt) for dt in ("bf16", "mixed") for f in ("tile", "default", "rows", "split2")]


def _mm_data(M, K, N, dt):
    """x [M + 10, K] (rows M.. are reached by the gathered form only), w [K, N], row ids, and the
    fp64 products of the operands as the kernels see them (bf16-rounded where the dtype says so)."""
    def make():
        rng = np.random.default_rng(M + 7 * K + 13 * N)
        x = rng.standard_normal((M + 10, K)).astype(np.float32)
        w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
        idx = rng.integers(0, M + 10, M).astype(np.int32)
        if dt == "bf16":
            x = _bf(x)
        if dt != "f32":
            w = _bf(w)
        xr = (_bf(x) if dt == "mixed" else x).astype(np.float64)
        wf = w.astype(np.float64)
        return {"x": x, "w": w, "idx": idx, "ref": xr @ wf, "abs": np.abs(xr) @ np.abs(wf)}
    return _memo(("mm", M, K, N, dt), make)


def _mm_run(dev, ar, d, M, K, N, dt, lay, gathered, sf, what):
    xdt = torch.bfloat16 if dt == "bf16" else torch.float32
    wdt = torch.float32 if dt == "f32" else torch.bfloat16
    xt = ar.table("x", d["x"] if gathered else d["x"][:M], lay, xdt)
    wt = ar.table("w", d["w"], lay, wdt)
    ri = None
    if gathered:
        ri = ar.vec("row_idx", M, torch.int32, SLACK, M + 10, _IDX_MIS[lay][1])  # slack: the NaN row behind x
        ri.copy_(torch.from_numpy(d["idx"]))
    out = ar.out("out", M, N, lay)
    ar.seal()
    ops.update_mm(xt, wt, ri, sf=sf, out=out)
    ar.check([out], what)
    ref, ab = (d["ref"][d["idx"]], d["abs"][d["idx"]]) if gathered else (d["ref"][:M], d["abs"][:M])
    _ok(out, isa_ref.sf(sf, ref), ab, what)


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("form,dt", MM_CASES)
def test_update_mm(dev, form, dt, lay):
    """M off the 64 / 128-row groups, N with a column tail, a non-vector store and two column
    blocks, K with every tail class; gathered rows (N = 100) and an SF epilogue (N = 66)."""
    mm_form, knobs = MM_FORMS[form]
    old = ops.MM_FORM, ops.MM_ROWS_MIN_M
    try:
        ops.MM_FORM, ops.MM_ROWS_MIN_M = mm_form, 0
        with _knobs(**knobs):
            for M in (130, 3001):
                for N in (33, 66, 100, 128, 200):
                    for K in (37, 100, 602):
                        if form.startswith("split") and K < 100:
                            continue  # slices are >= 16 k: nothing to split
                        ar = Arena(dev, 16 << 20)
                        _mm_run(dev, ar, _mm_data(M, K, N, dt), M, K, N, dt, lay, N == 100, "RELU" if N == 66 else None,
                                f"update_mm {form} {dt} lay={lay} M={M} K={K} N={N}")
    finally:
        ops.MM_FORM, ops.MM_ROWS_MIN_M = old


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
def test_update_mm_persistent_ring(dev, lay):
    """Many row groups per block: the persistent 3-deep k_mm_ring (1094 64-row groups, N = 33)."""
    M, K, N = 70000, 32, 33
    with _knobs(mm_wave=0):
        _mm_run(dev, Arena(dev, CAP), _mm_data(M, K, N, "f32"), M, K, N, "f32", lay, False, "RELU",
                f"update_mm persistent ring lay={lay}")


@gpu
@pytest.mark.parametrize("lay", ["a", "b", "c"])
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M", [1, 4099])
def test_update_mlp(dev, M, xdt, lay):
    """gta_update_mlp needs 16-B aligned x rows: ops refuses x in layouts b (more than one row) and
    c; out takes every layout.  Bitwise equal to the two unfused update_mm calls, as in
    test_update_mlp_bitwise."""
    K1, N1 = 100, 64
    rng = np.random.default_rng(M)
    x = _bf(rng.standard_normal((M, K1)).astype(np.float32))
    w1 = torch.from_numpy((rng.standard_normal((K1, N1)) / np.sqrt(K1)).astype(np.float32)).to(torch.bfloat16).to(dev)
    for N2 in (8, 20, 100, 128):
        w2 = torch.from_numpy((rng.standard_normal((N1, N2)) / np.sqrt(N1)).astype(np.float32)).to(torch.bfloat16).to(dev)
        want = ops.update_mm(ops.update_mm(torch.from_numpy(x).to(dev), w1, sf="RELU"), w2, sf="ELU")
        ar = Arena(dev, CAP)
        out = ar.out("out", M, N2, lay)
        what = f"update_mlp M={M} {xdt} lay={lay} N2={N2}"
        xin = ar.table("x_" + lay, x, lay, xdt)
        if lay == "c" or (lay == "b" and M > 1):
            _refused(ar, lambda: ops.update_mlp(xin, w1, w2, "RELU", "ELU", out=out), ValueError, "update_mlp: fp32 / bf16 x", what)
            xin = ar.table("x_a", x, "a", xdt)
        ar.seal()
        ops.update_mlp(xin, w1, w2, "RELU", "ELU", out=out)
        ar.check([out], what)
        assert bool(torch.isfinite(out).all()), what
        assert torch.equal(out, want), what


# ---------------------------------------------------------------------------------------------
# setup and metadata kernels (no out= in ops: the ABI directly)
# ---------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("lay", ["a", "c"])
def test_tile_nnz(dev, lay):
    """counts [ceil(n / T), n_cols] with n % T != 0: the last tile is partial."""
    L = _lib.load()
    T = 64
    ip, ix = _csr(N_AGG, E_AGG, 5, n_cols=NC_G, sort=True)
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, NC_G, lay)
    counts = ar.mat("counts", -(-N_AGG // T), NC_G, torch.int32, mis=_IDX_MIS[lay][1])
    counts.zero_()  # the caller zeroes counts
    ar.seal()
    rc = L.gta_tile_nnz(_p(g.indptr), _p(g.indices), N_AGG, NC_G, T, _p(counts), _st(dev))
    assert rc == 0, L.gta_last_error()
    ar.check([counts], f"tile_nnz lay={lay}")
    assert np.array_equal(counts.cpu().numpy(), isa_ref.tile_nnz(ip, ix, NC_G, T))


@gpu
@pytest.mark.parametrize("lay", ["a", "c"])
def test_synth_alpha_and_row_ids(dev, lay):
    from gta_graph_tensor_acclelrator_for_general_gnn_amd import metric
    L = _lib.load()
    ip, ix = _csr(N_AGG, E_AGG, 6, last=0)
    nnz = len(ix)
    gen = np.random.default_rng(6).permutation(nnz).astype(np.int64) * 3 + 1
    m64, m32 = _IDX_MIS[lay]
    ar = Arena(dev, CAP)
    ipv = ar.vec("indptr", N_AGG + 1, torch.int64, SLACK, nnz, m64)
    ipv.copy_(torch.from_numpy(ip))
    genv = ar.vec("gen", nnz, torch.int64, SLACK, 0, m64)
    genv.copy_(torch.from_numpy(gen))
    lip, gend = torch.from_numpy(ip).to(dev), torch.from_numpy(gen).to(dev)
    for heads in (1, 8, 64):
        out = ar.mat(f"alpha{heads}", nnz, heads, mis=m32)
        want = metric.alpha_rows_torch(lip, gend, dev, heads=heads)
        ar.seal()
        rc = L.gta_synth_alpha(_p(ipv), _p(genv), N_AGG, nnz, heads, metric.SEED, metric.STREAM_LOGIT, _p(out), _st(dev))
        assert rc == 0, L.gta_last_error()
        ar.check([out], f"synth_alpha H={heads} lay={lay}")
        assert bool(torch.isfinite(out).all()) and torch.equal(out, want)  # test_gpu_metric's bitwise reference
    rid = ar.vec("row_ids", nnz, torch.int64, mis=m64)
    ar.seal()
    rc = L.gta_row_ids(_p(ipv), N_AGG, nnz, _p(rid), _st(dev))
    assert rc == 0, L.gta_last_error()
    ar.check([rid], f"row_ids lay={lay}")
    assert np.array_equal(rid.cpu().numpy(), isa_ref.row_of_edge(ip))


@gpu
@pytest.mark.parametrize("n_cols", [1, 255, 257, 70000])
def test_csc_build_exact_workspace(dev, n_cols):
    """gta_csc_build (one and three radix passes) with exactly gta_csc_workspace_bytes, edge counts
    around the 256-thread block so the last radix block is partial; one byte less is GTA_ERR_ARG."""
    L = _lib.load()
    n_rows = 50
    for nnz in (1, 255, 256, 257, 5000):
        rng = np.random.default_rng(n_cols + nnz)
        ip = np.concatenate([[0], np.cumsum(rng.multinomial(nnz, np.full(n_rows, 1.0 / n_rows)))]).astype(np.int64)
        ix = rng.integers(0, n_cols, nnz).astype(np.int32)
        ar = Arena(dev, 4 << 20)
        ipv = ar.vec("indptr", n_rows + 1, torch.int64, SLACK, nnz)
        ixv = ar.vec("indices", nnz, torch.int32, SLACK, n_cols - 1, 4)  # keys stay in [0, n_cols), as the ABI asks
        ipv.copy_(torch.from_numpy(ip))
        ixv.copy_(torch.from_numpy(ix))
        colptr = ar.vec("colptr", n_cols + 1, torch.int64, mis=8)
        perm, rows = ar.vec("perm", nnz, torch.int32, mis=4), ar.vec("rows", nnz, torch.int32)
        wsb = int(L.gta_csc_workspace_bytes(n_cols, nnz))
        ws = ar.raw("workspace", wsb)
        what = f"csc_build n_cols={n_cols} nnz={nnz}"
        args = (_p(ipv), _p(ixv), n_rows, n_cols, nnz, _p(colptr), _p(perm), _p(rows), _p(ws))
        ar.seal()
        assert L.gta_csc_build(*args, wsb - 1, _st(dev)) == _lib.ERR_ARG and b"workspace smaller" in L.gta_last_error()
        ar.check([], what + " one byte short")
        assert L.gta_csc_build(*args, wsb, _st(dev)) == 0, L.gta_last_error()
        ar.check([colptr, perm, rows, ws], what)
        order = np.argsort(ix, kind="stable")
        assert np.array_equal(perm.cpu().numpy(), order), what
        assert np.array_equal(rows.cpu().numpy(), isa_ref.row_of_edge(ip)[order]), what
        assert np.array_equal(colptr.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(ix, minlength=n_cols))])), what


# ---------------------------------------------------------------------------------------------
# plans and workspaces at exactly the advertised size (the ABI directly)
# ---------------------------------------------------------------------------------------------

def _plan_graph(kind):
    rng = np.random.default_rng(11)
    if kind == "tight":  # every row non-empty and <= chunk, except rows of k * chunk + 1 edges
        deg = rng.integers(1, 65, 40)
        deg[[3, 17, 39]] = (65, 129, 641)
        deg[5] = 64
    elif kind == "empty":
        deg = np.zeros(37, np.int64)
    else:  # one row holds every edge
        deg = np.array([0, 0, 1000, 0, 0])
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return ip, rng.integers(0, len(deg), int(ip[-1])).astype(np.int32)


@gpu
@pytest.mark.parametrize("kind", ["tight", "empty", "one_row"])
@pytest.mark.parametrize("F", [100, 128])
def test_row_chunk_plan_exact(dev, F, kind):
    """gta_aggregate_plan_build into exactly gta_aggregate_plan_bytes, then gta_aggregate,
    gta_aggregate_self and gta_aggregate_expr with exactly gta_aggregate_workspace_bytes."""
    import ctypes
    L = _lib.load()
    chunk = 64
    ip, ix = _plan_graph(kind)
    n, nnz = len(ip) - 1, len(ix)
    deg = np.diff(ip)
    rng = np.random.default_rng(F)
    x, xs = rng.standard_normal((n, F)).astype(np.float32), rng.standard_normal((n, F)).astype(np.float32)
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, n, "a")
    pb, wsb = int(L.gta_aggregate_plan_bytes(n, nnz, chunk)), int(L.gta_aggregate_workspace_bytes(n, nnz, chunk, F))
    assert wsb == (n + -(-nnz // chunk)) * F * 4
    plan, ws = ar.raw("plan", pb), ar.raw("workspace", wsb)
    xt, xst = ar.table("x", x, "a"), ar.table("xs", xs, "a")
    s = ar.vec("s", 1, torch.float32)
    s.fill_(1.1)
    ys = [ar.out(f"y{i}", n, F, "a") for i in range(3)]
    what = f"row-chunk plan {kind} F={F}"
    ar.seal()
    assert L.gta_aggregate_plan_build(_p(g.indptr), n, nnz, chunk, _p(plan), pb - 1, _st(dev)) == _lib.ERR_ARG
    assert b"plan buffer too small" in L.gta_last_error()
    ar.check([], what + " one byte short")
    assert L.gta_aggregate_plan_build(_p(g.indptr), n, nnz, chunk, _p(plan), pb, _st(dev)) == 0, L.gta_last_error()
    ar.check([plan], what + " build")
    hdr = plan[:16].view(torch.int64).cpu()
    assert int(hdr[0]) == int(np.where(deg <= chunk, 1, -(-deg // chunk)).sum()) <= n + -(-nnz // chunk)
    assert int(hdr[1]) == int((deg > chunk).sum())
    ref, ab = isa_ref.aggregate(ip, ix, x, "src"), isa_ref.aggregate_abs(ip, ix, x, "src")
    gi = (_p(g.indptr), _p(g.indices), n, nnz)
    ar.seal()
    assert L.gta_aggregate(*gi, _lib.IDX_SRC, _p(xt), xt.stride(0), F, _lib.GTA_F32, None, 0, 0, None, _p(ys[0]), ys[0].stride(0),
                           0, _p(plan), chunk, _p(ws), _st(dev)) == 0, L.gta_last_error()
    ar.check([ws, ys[0]], what + " aggregate")
    _ok(ys[0], ref, ab, what + " aggregate")
    ar.seal()
    assert L.gta_aggregate_self(*gi, _lib.IDX_SRC, _p(xt), xt.stride(0), F, _lib.GTA_F32, None, 0, 0, None, _p(xst), xst.stride(0),
                                _p(s), _p(ys[1]), ys[1].stride(0), _lib.GTA_F32, _p(plan), chunk, _p(ws), _st(dev)) == 0, L.gta_last_error()
    ar.check([ws, ys[1]], what + " aggregate_self")
    _ok(ys[1], ref + np.float64(np.float32(1.1)) * xs, ab + 1.1 * np.abs(xs), what + " aggregate_self")
    ptrs, cm, lds = (ctypes.c_void_p * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int64 * 4)()
    for l, (t, m) in enumerate(((xt, _lib.IDX_SRC), (xst, _lib.IDX_DST), (xt, _lib.IDX_SRC), (xt, _lib.IDX_SRC))):
        ptrs[l], cm[l], lds[l] = t.data_ptr(), m, t.stride(0)
    cb, cs = (ctypes.c_int * 3)(_lib.BIN_MUL, 0, 0), (ctypes.c_int * 3)(_lib.SF["TANH"], 0, 0)
    ar.seal()
    assert L.gta_aggregate_expr(*gi, 1, ptrs, cm, lds, cb, cs, 0, F, _p(ys[2]), ys[2].stride(0), _p(plan), chunk, _p(ws),
                                _st(dev)) == 0, L.gta_last_error()
    ar.check([ws, ys[2]], what + " aggregate_expr")
    p = x.astype(np.float64)[ix] * xs.astype(np.float64)[isa_ref.row_of_edge(ip)]
    _ok(ys[2], isa_ref.gather_add(ip, np.tanh(p)), isa_ref.gather_add(ip, np.abs(p) + 1.0), what + " aggregate_expr")


@gpu
@pytest.mark.parametrize("variant", ["tight", "row_edges", "item_1", "item_inf"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_blocked_plan_exact(dev, F, variant):
    """blocked_max_items = min(n_rows * B, nnz) + nnz / item_edges is reached exactly when every
    (row, block) segment is non-empty with length == 1 (mod item_edges) and n_rows * B < item_edges:
    4 rows x 2 blocks of 65 sorted columns each at item_edges 64 give 16 items, the bound.  The last
    plan slot and the last slab row are then really used, by both consumers, with the plan and the
    workspaces exactly as long as the *_bytes functions say."""
    L = _lib.load()
    n, B, nc, H = 4, 2, 200, F // 16
    ie, re_ = {"tight": (64, 0), "row_edges": (64, 100), "item_1": (1, 0), "item_inf": (1 << 30, 0)}[variant]
    rng = np.random.default_rng(F)
    ix = np.concatenate([np.sort(rng.integers(b * 100, (b + 1) * 100, 65)) for _ in range(n) for b in range(B)]).astype(np.int32)
    ip = (np.arange(n + 1) * 130).astype(np.int64)
    nnz = len(ix)
    d = {"ip": ip, "ix": ix, "H": H, "x": rng.standard_normal((nc, F)).astype(np.float32),
         "a": rng.standard_normal((n, H)).astype(np.float32), "b": rng.standard_normal((nc, H)).astype(np.float32)}
    w = rng.random((nnz, H)).astype(np.float32)
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, nc, "a")
    pb = int(L.gta_aggregate_blocked_plan_bytes(n, nnz, B, ie))
    wsb = int(L.gta_aggregate_blocked_workspace_bytes(n, nnz, B, F, ie))
    wsb2 = int(L.gta_gat_aggregate_blocked_workspace_bytes(n, nnz, B, F, H, ie))
    mi = min(n * B, nnz) + nnz // ie
    assert wsb == mi * F * 4 and wsb2 == mi * (F + (H + 3) // 4 * 4) * 4
    plan, ws, ws2 = ar.raw("plan", pb), ar.raw("slabs", wsb), ar.raw("slabs_att", wsb2)
    xt, wt = ar.table("x", d["x"], "a"), ar.table("w", w, "a")
    at, bt = ar.table("a_dst", d["a"], "a"), ar.table("b_src", d["b"], "a")
    y, y2, sums = ar.out("y", n, F, "a"), ar.out("y_att", n, F, "a"), ar.mat("sums", n, H)
    what = f"blocked plan {variant} F={F}"
    build = (_p(g.indptr), _p(g.indices), n, nc, nnz, B, ie, re_, _p(plan))
    ar.seal()
    assert L.gta_aggregate_blocked_plan_build(*build, pb - 1, _st(dev)) == _lib.ERR_ARG and b"plan buffer too small" in L.gta_last_error()
    ar.check([], what + " one byte short")
    assert L.gta_aggregate_blocked_plan_build(*build, pb, _st(dev)) == 0, L.gta_last_error()
    ar.check([plan], what + " build")
    hdr = plan[:64].view(torch.int64).cpu()
    assert int(hdr[3]) == 0 and int(hdr[6]) == mi
    assert int(hdr[4]) == {"tight": 16, "row_edges": 12, "item_1": nnz, "item_inf": 8}[variant]
    if variant == "tight":
        assert int(hdr[4]) == mi  # the bound itself
    gi = (_p(g.indptr), _p(g.indices), n, nc, nnz)
    ar.seal()
    assert L.gta_aggregate_blocked(*gi, _p(xt), xt.stride(0), F, _p(wt), wt.stride(0), H, None, _p(y), y.stride(0), 0, _p(plan), B, ie,
                                   _p(ws), _st(dev)) == 0, L.gta_last_error()
    ar.check([ws, y], what + " aggregate_blocked")
    _ok(y, isa_ref.aggregate(ip, ix, d["x"], "src", w), isa_ref.aggregate_abs(ip, ix, d["x"], "src", w), what + " aggregate_blocked")
    ar.seal()
    assert L.gta_gat_aggregate_blocked(*gi, _p(xt), xt.stride(0), F, _p(at), at.stride(0), _p(bt), bt.stride(0), H,
                                       _lib.SF["EXP_LEAKY_RELU"], 1, 0, _p(y2), y2.stride(0), _p(sums), _p(plan), B, ie, _p(ws2),
                                       _st(dev)) == 0, L.gta_last_error()
    ar.check([ws2, y2, sums], what + " gat_aggregate_blocked")
    ref, scale, rsum = _gat_ref(F, True, key=variant, data=d)
    _ok(y2, ref, scale, what + " gat y")
    _ok(sums, rsum, rsum, what + " gat sums")


@gpu
@pytest.mark.parametrize("ldw_pad", [0, 1])
@pytest.mark.parametrize("N", [16, 128])
@pytest.mark.parametrize("K", [290, 1433])
def test_split_k_exact_workspace(dev, K, N, ldw_pad):
    """gta_update_mm_t_split with exactly gta_update_mm_t_split_workspace_bytes: the library's own
    slice count and forced ones (mm_split 2, 3, and 9, where ceil(K / 9) rounded up to 16 leaves
    fewer than 9 slices at K = 290), K with a short last slice, 16-B aligned W^T rows (the ring at
    N = 128) and misaligned ones (k_mm_rows); one byte less is GTA_ERR_ARG."""
    L = _lib.load()
    M = 333
    d = _mm_data(M, K, N, "f32")
    ar = Arena(dev, CAP)
    xt = ar.table("x", d["x"][:M], "a")
    wt = ar.mat("wt", N, K, pad=-(-K // 4) * 4 - K + 4 * ldw_pad + ldw_pad)
    wt.copy_(torch.from_numpy(np.ascontiguousarray(d["w"].T)))
    for mode in (-1, 2, 3, 9):
        with _knobs(mm_split=mode):
            splits = int(L.gta_update_mm_t_splits(M, K, N, _lib.GTA_F32, _st(dev)))
        assert splits >= 1 and (mode < 0 or splits == mode)
        wsb = int(L.gta_update_mm_t_split_workspace_bytes(M, K, N, splits))
        assert wsb == splits * M * N * 4
        ws, out = ar.raw(f"workspace{mode}", wsb), ar.out(f"out{mode}", M, N, "b")
        what = f"split-K K={K} N={N} ldwt={wt.stride(0)} mm_split={mode} splits={splits}"
        args = (_p(xt), xt.stride(0), None, M, K, _p(wt), wt.stride(0), N, _lib.GTA_F32, _lib.SF["RELU"], _p(out), out.stride(0),
                splits, _p(ws))
        ar.seal()
        assert L.gta_update_mm_t_split(*args, wsb - 1, _st(dev)) == _lib.ERR_ARG and b"workspace too small" in L.gta_last_error()
        ar.check([], what + " one byte short")
        assert L.gta_update_mm_t_split(*args, wsb, _st(dev)) == 0, L.gta_last_error()
        ar.check([ws, out], what)
        _ok(out, np.maximum(d["ref"][:M], 0.0), d["abs"][:M], what)


@gpu
def test_zz_knobs_left_as_found(dev):
    """Last in the module: no test above leaked a knob into the tests that follow."""
    assert ops.knob_state() == _START["state"]
    assert (ops.MM_FORM, ops.MM_ROWS_MIN_M, ops.APPLY_EDGE_FLAT) == _START["mm"]
