"""Non-finite values INSIDE the data of a sum: locality and class, for every gather / sum form.

The guard-band suite poisons memory around the operands; here +inf, -inf and NaN are ordinary
values of three source rows.  The gather kernels handle tails with clamped re-reads of a row's last
edge and zeroed weights: a form that masked by multiplying instead of selecting would leak
0 * inf = NaN into a row whose true value is +inf, or into a neighbouring item of the same wave.

One graph (nonfinite_graph): 96 x 96, degrees cycling through {0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65,
130} (the tails of the 8-edge step, the 32-edge chunk, the 64-lane wave and a plan chunk of 64),
columns sorted.  The hot sources 93 (+inf in one column), 94 (-inf in the whole row) and 95 (NaN in
one column) are the highest ids, so a hot edge is the LAST edge of its row -- the one clamped loads
re-read.  HOT_OF fixes which destination rows reference which hot source; half the non-empty rows
reference none.  Weights are uniform in [0.5, 1.5], so classes are unambiguous.

Two assertions per call:
  locality  every output row that references no hot value is BITWISE the same call's output with
            the hot rows replaced by finite values;
  class     every element's class (finite, +inf, -inf, NaN) is the fp64 oracle's under IEEE rules
            (+inf alone stays +inf, never NaN; a hot edge of weight 0 gives NaN), and finite elements
            stay within the suite's bound |d| <= 1e-5 * sum|terms| + 1e-6.
Every index is in range: nothing here reads or writes out of bounds.
"""
import contextlib

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops
from oracle import isa_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 96
DEGS = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 130)
HOT = (93, 94, 95)                      # +inf in one column, -inf in the whole row, NaN in one column
# destination rows by cycle of 12: cycle 0 references 93, 1 -> 94, 2 -> 95, 3 -> 93 and 94, 4 .. 7 none
HOT_OF = {0: (93,), 1: (94,), 2: (95,), 3: (93, 94)}


def nonfinite_graph():
    rng = np.random.default_rng(96)
    deg = np.array([DEGS[r % 12] for r in range(N)])
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = np.empty(ip[-1], np.int32)
    touched = np.zeros(N, bool)
    for r in range(N):
        hot = HOT_OF.get(r // 12, ()) if deg[r] else ()
        hot = hot[:deg[r]]
        cold = np.sort(rng.integers(0, HOT[0], deg[r] - len(hot)))
        ix[ip[r]:ip[r + 1]] = np.concatenate([cold, hot]).astype(np.int32)
        touched[r] = len(hot) > 0
    # built as described: sorted rows, hot edges last, at least half of the non-empty rows cold
    for r in range(N):
        row = ix[ip[r]:ip[r + 1]]
        assert np.all(np.diff(row) >= 0)
        assert touched[r] == (deg[r] > 0 and row[-1] >= HOT[0]) == bool(np.isin(row, HOT).any())
    assert 2 * (~touched & (deg > 0)).sum() >= (deg > 0).sum() and touched.sum() == 44
    assert 0 <= ix.min() and ix.max() < N
    return ip, ix, touched


IP, IX, TOUCHED = nonfinite_graph()
ROWS = np.repeat(np.arange(N), np.diff(IP))
E = int(IP[-1])
HOT_EDGE = np.isin(IX, HOT)


def tables(F, seed=0):
    """(x_hot, x_fin) [96, F] fp32: equal but for rows 93, 94, 95."""
    rng = np.random.default_rng(seed + F)
    x = rng.standard_normal((N, F)).astype(F32)
    hot = x.copy()
    hot[93, F // 3] = np.inf
    hot[94, :] = -np.inf
    hot[95, F - 1] = np.nan
    return hot, x


def weights(cols, zero_hot=False, seed=1):
    if not cols:
        return None
    w = (np.random.default_rng(seed + cols).random((E, cols)) + 0.5).astype(F32)
    if zero_hot:
        w[HOT_EDGE] = 0
    return w


def cls(a):
    a = np.asarray(a)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 0)))


def finite_part(a):
    return np.where(np.isfinite(a), a, 0).astype(a.dtype)


def dt(a, dev, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


@contextlib.contextmanager
def knobs(**kv):
    old = {k: ops.get_debug(k) for k in kv}
    try:
        for k, v in kv.items():
            ops.set_debug(k, v)
        yield
    finally:
        for k, v in old.items():
            ops.set_debug(k, v)


def check(y_hot, y_fin, touched, ref, scale, what):
    """The two assertions.  ref: fp64 oracle of the hot call (IEEE); scale: sum |terms| of its finite
    elements; touched: the output rows a hot value reaches."""
    got, fin = y_hot.detach().float().cpu().numpy(), y_fin.detach().float().cpu().numpy()
    cold = ~touched
    same = got[cold].view(np.uint32) == fin[cold].view(np.uint32)
    assert same.all(), f"{what}: locality: {(~same).sum()} elements of rows {np.flatnonzero(cold)[(~same).any(1)][:8]} " \
                       f"change with the hot rows, classes {np.unique(cls(got[cold])[~same])}"
    assert np.isfinite(fin).all(), f"{what}: the finite call gave non-finite values"
    cg, cr = cls(got), cls(ref)
    bad = cg != cr
    assert not bad.any(), f"{what}: class: {bad.sum()} elements, rows {np.unique(np.nonzero(bad)[0])[:8]}, " \
                          f"got {cg[bad][:6]} want {cr[bad][:6]} (0 finite, 1 +inf, 2 -inf, 3 NaN)"
    f = cr == 0
    err = np.abs(np.where(f, got, 0).astype(np.float64) - np.where(f, ref, 0))[f]
    bound = (1e-5 * scale + 1e-6)[f]
    assert (err <= bound).all(), f"{what}: {(err > bound).sum()} finite elements out of tolerance, max err {err.max():.3e}"
    assert cr[touched].max() > 0  # the case does carry non-finite values into the touched rows


def agg_refs(x, mode, w, row_scale=None):
    with np.errstate(all="ignore"):
        ref = isa_ref.aggregate(IP, IX, x, mode, w, row_scale)
    return ref, isa_ref.aggregate_abs(IP, IX, finite_part(x), mode, w, row_scale)


def operand(x, mode):
    """x as the operand of `mode`: the node table, or the edge tensor x[src(e)] (same hot edges)."""
    return x[IX.astype(np.int64)] if mode == "edge" else x


def touched_of(mode):
    if mode == "dst":  # y[i] sums x[i]: the hot destinations (all three have edges)
        t = np.zeros(N, bool)
        t[list(HOT)] = True
        return t
    return TOUCHED


W_COLS = {"none": 0, "one": 1, "heads": 4, "full": None}


@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("plan", [None, 64])
@pytest.mark.parametrize("wk", list(W_COLS))
@pytest.mark.parametrize("mode", ["src", "dst", "edge"])
@pytest.mark.parametrize("F", [128, 100])
def test_aggregate(dev, F, mode, wk, plan, lean):
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    hot, fin = tables(F)
    w = weights(F if wk == "full" else W_COLS[wk])
    wd = dt(w, dev)
    with knobs(agg_lean=lean):
        ys = [ops.aggregate(g, dt(operand(x, mode), dev), mode, wd, plan=plan) for x in (hot, fin)]
    ref, scale = agg_refs(operand(hot, mode), mode, w)
    check(ys[0], ys[1], touched_of(mode), ref, scale, f"aggregate F={F} {mode} w={wk} plan={plan} lean={lean}")


@pytest.mark.parametrize("form,wk,plan", [("aggregate", wk, plan) for wk in ("one", "heads", "full") for plan in (None, 64)]
                         + [(form, wk, None) for form in ("blocked1", "blocked5") for wk in ("one", "heads")])
def test_hot_edge_of_weight_zero_is_nan(dev, form, wk, plan):
    """0 * inf: a hot edge whose weight is 0 gives NaN (never a silently dropped term)."""
    F = 128
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    hot, fin = tables(F)
    w = weights(F if wk == "full" else {"one": 1, "heads": 8}[wk], zero_hot=True)
    wd = dt(w, dev)
    if form == "aggregate":
        ys = [ops.aggregate(g, dt(x, dev), "src", wd, plan=plan) for x in (hot, fin)]
    else:
        ys = [ops.aggregate_blocked(g, dt(x, dev), wd, blocks=int(form[-1])) for x in (hot, fin)]
    ref, scale = agg_refs(hot, "src", w)
    assert np.isnan(ref[TOUCHED]).any() and not np.isinf(ref[:36]).any()
    check(ys[0], ys[1], TOUCHED, ref, scale, f"{form} zero-weight hot edge w={wk} plan={plan}")


@pytest.mark.parametrize("vw8", [4, 8, 0])
@pytest.mark.parametrize("plan", [None, 64])
@pytest.mark.parametrize("wk", ["none", "one", "heads"])
@pytest.mark.parametrize("mode", ["src", "dst"])
def test_aggregate_bf16_rows(dev, mode, wk, plan, vw8):
    F = 100
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    hot, fin = (dt(x, dev, torch.bfloat16) for x in tables(F))
    w = weights(W_COLS[wk])
    with knobs(agg_bf16_vw8=vw8):
        ys = [ops.aggregate(g, x, mode, dt(w, dev), plan=plan) for x in (hot, fin)]
    ref, scale = agg_refs(hot.float().cpu().numpy(), mode, w)
    check(ys[0], ys[1], touched_of(mode), ref, scale, f"aggregate bf16 {mode} w={wk} plan={plan} vw8={vw8}")


@pytest.mark.parametrize("plan", [None, 64])
@pytest.mark.parametrize("wk", ["none", "heads"])
@pytest.mark.parametrize("F", [128, 36])
def test_aggregate_row_scale_accumulate(dev, F, wk, plan):
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    hot, fin = tables(F)
    w = weights(W_COLS[wk])
    rng = np.random.default_rng(3)
    rs = (rng.random(N) + 0.5).astype(F32)
    y0 = rng.standard_normal((N, F)).astype(F32)
    ys = [ops.aggregate(g, dt(x, dev), "src", dt(w, dev), row_scale=dt(rs, dev), out=dt(y0, dev), accumulate=True,
                        plan=plan) for x in (hot, fin)]
    ref, scale = agg_refs(hot, "src", w, rs)
    check(ys[0], ys[1], TOUCHED, y0 + ref, scale + np.abs(y0), f"aggregate row_scale accumulate F={F} w={wk} plan={plan}")


@pytest.mark.parametrize("plan", [None, 64])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_aggregate_self(dev, dtype, scaled, plan):
    """y = x_self * s + row_scale * sum: the self term is a finite table, so the touched rows stay TOUCHED."""
    F = 100
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    td = torch.bfloat16 if dtype == "bf16" else None
    hot, fin = (dt(x, dev, td) for x in tables(F))
    xs = dt(tables(F, seed=9)[1], dev, td)
    s = torch.tensor([[1.25]], device=dev)
    rs = (np.random.default_rng(4).random(N) + 0.5).astype(F32) if scaled else None
    ys = [ops.aggregate(g, x, "src", None, row_scale=dt(rs, dev), plan=plan, self_term=(xs, s)) for x in (hot, fin)]
    ref, scale = agg_refs(hot.float().cpu().numpy(), "src", None, rs)
    xsn = xs.float().cpu().numpy().astype(np.float64)
    check(ys[0], ys[1], TOUCHED, ref + 1.25 * xsn, scale + 1.25 * np.abs(xsn), f"aggregate_self {dtype} scaled={scaled} plan={plan}")


SEG_FORMS = {"default": {}, "seg_lean0": {"seg_lean": 0}, "seg_lean_w1_0": {"seg_lean_w1": 0},
             "seg_alpha1_0": {"seg_alpha1": 0}, "seg_pf1": {"seg_pf": 1}, "seg_pf2": {"seg_pf": 2},
             "seg_pf3": {"seg_pf": 3}, "seg_pf4": {"seg_pf": 4}, "seg_pf5": {"seg_pf": 5}}


@pytest.mark.parametrize("form", list(SEG_FORMS))
@pytest.mark.parametrize("heads", [0, 1, 8, 4])
@pytest.mark.parametrize("blocks", [1, 5])
@pytest.mark.parametrize("F", [128, 64])
def test_aggregate_blocked(dev, F, blocks, heads, form):
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    hot, fin = tables(F)
    w = weights(heads)
    with knobs(**SEG_FORMS[form]):
        ys = [ops.aggregate_blocked(g, dt(x, dev), dt(w, dev), blocks=blocks) for x in (hot, fin)]
    ref, scale = agg_refs(hot, "src", w)
    check(ys[0], ys[1], TOUCHED, ref, scale, f"aggregate_blocked F={F} B={blocks} H={heads} {form}")


def _gat_refs(x, a, b, normalize, F, H):
    with np.errstate(all="ignore"):
        ref, rsum = isa_ref.gat_aggregate(IP, IX, x.astype(np.float64), a.astype(np.float64), b.astype(np.float64),
                                          "EXP_LEAKY_RELU", normalize)
        v, _ = isa_ref.edge_softmax(IP, IX, a.astype(np.float64), b.astype(np.float64), "EXP_LEAKY_RELU", False)
    scale = isa_ref.aggregate(IP, IX, np.abs(finite_part(x).astype(np.float64)), "src", finite_part(v))
    if normalize:
        scale = scale / np.repeat(np.where(rsum > 0, rsum, 1.0), F // H, axis=1) * 4
    return ref, rsum, scale


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lean,direct", [(1, 1), (1, 0), (1, 2), (0, 1)])
@pytest.mark.parametrize("blocks", [1, 5])
@pytest.mark.parametrize("F,H", [(128, 8), (64, 4)])
def test_gat_aggregate_blocked_hot_x(dev, F, H, blocks, lean, direct, normalize):
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    hot, fin = tables(F)
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal((N, H)).astype(F32), rng.standard_normal((N, H)).astype(F32)
    with knobs(att_lean=lean, att_direct=direct):
        ys = [ops.gat_aggregate_blocked(g, dt(x, dev), dt(a, dev), dt(b, dev), normalize=normalize, blocks=blocks)[0]
              for x in (hot, fin)]
    ref, _, scale = _gat_refs(hot, a, b, normalize, F, H)
    check(ys[0], ys[1], TOUCHED, ref, scale, f"gat F={F} B={blocks} lean={lean} direct={direct} norm={normalize}")


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lean,direct", [(1, 1), (1, 0), (1, 2), (0, 1)])
@pytest.mark.parametrize("blocks", [1, 5])
def test_gat_aggregate_blocked_hot_score(dev, blocks, lean, direct, normalize):
    """A hot b_src score of -inf gives weight exp(-inf) = 0 and leaves the row finite: the fp64
    oracle's value, and the untouched rows bitwise.  (Rows whose ONLY edge is the hot one have a zero
    row sum: 0 / 0 when normalized, which gta.h leaves unspecified -- left out there.)"""
    F, H = 128, 8
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    x = tables(F)[1]
    rng = np.random.default_rng(8)
    a, b = rng.standard_normal((N, H)).astype(F32), rng.standard_normal((N, H)).astype(F32)
    bh = b.copy()
    bh[list(HOT)] = -np.inf
    with knobs(att_lean=lean, att_direct=direct):
        ys = [ops.gat_aggregate_blocked(g, dt(x, dev), dt(a, dev), dt(bb, dev), normalize=normalize, want_sums=True,
                                        blocks=blocks) for bb in (bh, b)]
    ref, rsum, scale = _gat_refs(x, a, bh, normalize, F, H)
    got, fin = (y[0].cpu().numpy() for y in ys)
    cold = ~TOUCHED
    assert np.array_equal(got[cold].view(np.uint32), fin[cold].view(np.uint32))
    rows = np.diff(IP) >= (2 if normalize else 1)
    assert np.isfinite(got[rows]).all(), "a weight-0 edge made a row non-finite"
    err = np.abs(got.astype(np.float64) - ref)[rows]
    assert (err <= (1e-5 * scale + 1e-6)[rows]).all(), f"max err {err.max():.3e}"
    sums = ys[0][1].cpu().numpy()
    assert np.isfinite(sums).all() and (np.abs(sums - rsum) <= 1e-5 * rsum + 1e-6).all()


@pytest.mark.parametrize("F", [128, 36, 5])
def test_gather_add_direction_c(dev, F):
    """Edge tensor xe[e] = x[src(e)] summed to the SOURCE nodes: only outputs 93, 94, 95 are touched."""
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    hot, fin = tables(F)
    ys = [ops.gather_add(g, dt(operand(x, "edge"), dev), direction="C") for x in (hot, fin)]
    with np.errstate(all="ignore"):
        ref = isa_ref.gather_add(IP, operand(hot, "edge"), "C", IX, N)
    scale = isa_ref.gather_add(IP, np.abs(finite_part(operand(hot, "edge"))), "C", IX, N)
    t = np.zeros(N, bool)
    t[list(HOT)] = True
    check(ys[0], ys[1], t, ref, scale, f"gather_add C F={F}")
    yr = [ops.gather_add(g, dt(operand(x, "edge"), dev), direction="R") for x in (hot, fin)]
    ref, scale = agg_refs(operand(hot, "edge"), "edge", None)
    check(yr[0], yr[1], TOUCHED, ref, scale, f"gather_add R F={F}")


@pytest.mark.parametrize("plan", [None, 64])
@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("F", [128, 256, 36])
def test_aggregate_expr(dev, F, lean, plan):
    """shape 1: y[i] = sum_e x[src(e)] * w[e] with a full-width edge operand w."""
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    hot, fin = tables(F)
    w = weights(F)
    with knobs(expr_lean=lean):
        ys = [ops.aggregate_expr(g, 1, [(dt(x, dev), "src"), (dt(w, dev), "edge")], ["MUL"], plan=plan) for x in (hot, fin)]
    assert ys[0] is not None
    ref, scale = agg_refs(hot, "src", w)
    check(ys[0], ys[1], TOUCHED, ref, scale, f"aggregate_expr F={F} lean={lean} plan={plan}")


@pytest.mark.parametrize("lane", [1, 0])
@pytest.mark.parametrize("H", [4, 8, 16, 2, 32])
def test_edge_softmax_hot_scores(dev, H, lane):
    """Hot b_src scores: +inf in one head of source 93 (v = inf), -inf in every head of 94 (v = 0), NaN
    in one head of 95.  v (normalize off) and the row sums by class against the oracle; with
    normalize on, the edges of untouched rows bitwise."""
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    rng = np.random.default_rng(H)
    a = rng.standard_normal((N, H)).astype(F32)
    bh, b = tables(H, seed=5)
    ad = dt(a, dev)
    with knobs(esm_lane=lane):
        (vh, sh), (vf, sf_) = (ops.edge_softmax(g, ad, dt(bb, dev), normalize=False, want_sums=True) for bb in (bh, b))
        nh, nf = (ops.edge_softmax(g, ad, dt(bb, dev), normalize=True)[0] for bb in (bh, b))
    with np.errstate(all="ignore"):
        v, sums = isa_ref.edge_softmax(IP, IX, a.astype(np.float64), bh.astype(np.float64), "EXP_LEAKY_RELU", False)
    te = TOUCHED[ROWS]
    what = f"edge_softmax H={H} lane={lane}"
    # per edge: only the hot edges themselves carry a non-finite v
    got, fin = vh.cpu().numpy(), vf.cpu().numpy()
    assert np.array_equal(got[~HOT_EDGE].view(np.uint32), fin[~HOT_EDGE].view(np.uint32)), what
    assert np.array_equal(cls(got), cls(v)), what
    f = np.isfinite(v)
    assert (np.abs(got[f].astype(np.float64) - v[f]) <= 1e-5 * np.abs(v[f]) + 1e-6).all(), what
    check(sh, sf_, TOUCHED, sums, finite_part(sums), what + " sums")
    assert np.array_equal(nh.cpu().numpy()[~te].view(np.uint32), nf.cpu().numpy()[~te].view(np.uint32)), what


@pytest.mark.parametrize("plan", [None, 64])
@pytest.mark.parametrize("F,dtype,mode", [(F, "f32", m) for F in (128, 36) for m in ("src", "dst", "edge")]
                         + [(100, "bf16", "src"), (100, "bf16", "dst")])  # bf16 rows are gathered by index
def test_reduce_add(dev, F, dtype, mode, plan):
    g = G.from_numpy(IP, IX, device=dev, n_cols=N)
    hot, fin = (dt(operand(x, mode), dev, torch.bfloat16 if dtype == "bf16" else None) for x in tables(F))
    ys = [ops.reduce(g, x, "ADD", mode, plan=plan) for x in (hot, fin)]
    ref, scale = agg_refs(hot.float().cpu().numpy(), mode, None)
    check(ys[0], ys[1], touched_of(mode), ref, scale, f"reduce ADD F={F} {dtype} {mode} plan={plan}")
