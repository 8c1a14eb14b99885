"""TEST-ONLY numpy reference of the shifted (overflow-safe) softmax (include/gta.h, ABI 15 additive).

The score s(e, h) = g(fl32(a_dst[dst(e), h] + b_src[src(e), h])) and its row maximum m are emulated
in np.float32 exactly (one IEEE add, then g: t > 0 ? t : 0.2f * t, or t itself for EXP); everything
after them -- v = exp(s - m), the row sums, alpha and y -- is computed in fp64 from those fp32 s and
m.  A reference built from a.astype(float64) + b would test the conditioning of the inputs instead
of the kernels: at |a| = 120 the rounding of a + b alone moves v by about 1e-5 relative.

  case(...)         the inputs of the tests: b = 3 N(0, 1), a = N(0, 1) + a per-row offset cycling
                    through {0, +120, -600} (offsets=False: plain N(0, 1) scores)
  scores / shift    fp32, bit for bit what the kernels must form
  reference(...)    fp64 v, sums, alpha, and for a feature table x: y, the numerator, sum v |x|
  emulate_fp32(...) the shifted algorithm itself in fp32 (sequential sums): what any fp32
                    implementation of it can be expected to reach; the CPU tests confirm it stays
                    inside the bounds the GPU tests assert
The bounds are the project's: |d| <= 1e-5 * scale + 1e-6, with
  sums: scale = sums_ref;  alpha: scale = |alpha_ref| * max(deg, 1);
  y: scale = sum_e v |x| (divided by the row sum and times 4 when normalized), as _gat_ref in
  tests/test_gpu_footprint.py.
"""
import numpy as np

OFFSETS = (0.0, 120.0, -600.0)
F32 = np.float32


def rows_of(ip):
    return np.repeat(np.arange(len(ip) - 1, dtype=np.int64), np.diff(ip))


def csr(deg, n_cols, seed, sort=False):
    """A CSR with the given row degrees and uniform random source columns."""
    rng = np.random.default_rng(seed)
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = rng.integers(0, n_cols, int(ip[-1])).astype(np.int32)
    if sort:
        for r in range(len(deg)):
            ix[ip[r]:ip[r + 1]].sort()
    return ip, ix


def softmax_graph():
    """70 rows x 90 columns; degrees 0, 1, 63, 64, 65, 257 and one row of 700 among short rows."""
    rng = np.random.default_rng(11)
    deg = rng.integers(0, 13, 70)
    deg[[3, 10, 20, 30, 40, 50, 60]] = [0, 1, 63, 64, 65, 257, 700]
    return csr(deg, 90, 12) + (90,)


def blocked_graph(empty=5):
    """300 x 300, about 6,000 edges, columns sorted, `empty` rows without edges (the others have at
    least one), one 700-edge row."""
    rng = np.random.default_rng(21)
    deg = np.maximum(rng.multinomial(5300, np.full(300, 1.0 / 300)), 1)
    deg[rng.choice(np.arange(151, 300), empty, replace=False)] = 0
    deg[150] = 700
    return csr(deg, 300, 22, sort=True) + (300,)


def case(n_rows, n_cols, H, seed, offsets=True):
    """(a [n_rows, H], b [n_cols, H]) fp32: the issue's inputs."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n_rows, H)).astype(F32)
    b = (3.0 * rng.standard_normal((n_cols, H))).astype(F32)
    if offsets:
        a = (a + np.asarray(OFFSETS, F32)[np.arange(n_rows) % 3][:, None]).astype(F32)
    return a, b


def g_of(sf, t):
    assert t.dtype == F32
    if sf == "EXP":
        return t
    assert sf == "EXP_LEAKY_RELU"
    return np.where(t > 0, t, F32(0.2) * t).astype(F32)


def scores(ip, ix, a, b, sf):
    """fp32 [E, H]: g(fl32(a[dst] + b[src]))."""
    t = a.astype(F32)[rows_of(ip)] + b.astype(F32)[ix.astype(np.int64)]
    return g_of(sf, t.astype(F32))


def shift(ip, ix, a, b, sf):
    """fp32 [n_rows, H]: the row maxima of the scores, rows without edges 0; NaN propagates.  Formed as
    the kernel forms it, g(a + max b): equal to the maximum of the scores because fp32 addition and
    g are monotone (the CPU tests check that equality on the test inputs)."""
    n, H = len(ip) - 1, a.shape[1]
    mb = np.full((n, H), -np.inf, F32)
    np.maximum.at(mb, rows_of(ip), b.astype(F32)[ix.astype(np.int64)])  # np.maximum propagates NaN
    m = g_of(sf, (a.astype(F32)[:n] + mb).astype(F32))
    m[np.diff(ip) == 0] = 0
    return m


def shift_from_scores(ip, ix, a, b, sf):
    n, H = len(ip) - 1, a.shape[1]
    m = np.full((n, H), -np.inf, F32)
    np.maximum.at(m, rows_of(ip), scores(ip, ix, a, b, sf))
    m[np.diff(ip) == 0] = 0
    return m


def _segsum(rows, vals, n):
    out = np.zeros((n, vals.shape[1]), vals.dtype)
    np.add.at(out, rows, vals)  # unbuffered, in edge order
    return out


def reference(ip, ix, a, b, sf, x=None, shifted=True):
    """fp64 from the fp32 scores (and shift): dict with v [E, H], sums [n, H], alpha [E, H], deg, and
    with x [n_cols, F] also num = sum v x, y = num / sums (0 for empty rows) and vabs = sum v |x|.
    shifted=False: v = exp(s), the unshifted kernels' value (finite inputs only)."""
    n, H = len(ip) - 1, a.shape[1]
    rows = rows_of(ip)
    s = scores(ip, ix, a, b, sf).astype(np.float64)
    m = shift(ip, ix, a, b, sf).astype(np.float64) if shifted else np.zeros((n, H))
    v = np.exp(s - m[rows])
    sums = _segsum(rows, v, n)
    safe = np.where(sums > 0, sums, 1.0)
    out = {"v": v, "sums": sums, "alpha": v / safe[rows], "deg": np.diff(ip), "m": m}
    if x is not None:
        F = x.shape[1]
        xe = x.astype(np.float64)[ix.astype(np.int64)]
        ve = np.repeat(v, F // H, axis=1)
        out["num"] = _segsum(rows, ve * xe, n)
        out["vabs"] = _segsum(rows, ve * np.abs(xe), n)
        out["y"] = out["num"] / np.repeat(safe, F // H, axis=1)
    return out


def bounds(ref, F=None):
    """The scales of the project's bound for sums, alpha, and (F given) y normalized / not."""
    rows = np.repeat(np.arange(len(ref["deg"])), ref["deg"])
    sc = {"sums": ref["sums"], "alpha": np.abs(ref["alpha"]) * np.maximum(ref["deg"], 1)[rows][:, None], "v": ref["v"]}
    if F is not None:
        H = ref["sums"].shape[1]
        safe = np.repeat(np.where(ref["sums"] > 0, ref["sums"], 1.0), F // H, axis=1)
        sc["y"] = ref["vabs"] / safe * 4
        sc["num"] = ref["vabs"]
    return sc


def within(got, ref, scale):
    """(ok, max excess) of |got - ref| <= 1e-5 * scale + 1e-6 over every element."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = 1e-5 * scale + 1e-6
    return bool(np.all(err <= bound)), float((err - bound).max()) if err.size else 0.0


def emulate_fp32(ip, ix, a, b, sf, x=None):
    """The shifted algorithm in fp32 throughout: v = exp32(s - m), sequential fp32 sums, fp32 divides."""
    n, H = len(ip) - 1, a.shape[1]
    rows = rows_of(ip)
    s, m = scores(ip, ix, a, b, sf), shift(ip, ix, a, b, sf)
    v = np.exp((s - m[rows]).astype(F32)).astype(F32)
    sums = _segsum(rows, v, n)
    safe = np.where(sums > 0, sums, F32(1))
    out = {"v": v, "sums": sums, "alpha": (v / safe[rows]).astype(F32)}
    if x is not None:
        F = x.shape[1]
        ve = np.repeat(v, F // H, axis=1)
        out["num"] = _segsum(rows, (ve * x.astype(F32)[ix.astype(np.int64)]).astype(F32), n)
        out["y"] = (out["num"] / np.repeat(safe, F // H, axis=1)).astype(F32)
    return out
