"""Special values (+-0, denormals, +-inf, NaN, the over / underflow edges) at every element-wise site
of libgta: the SFs, the binary ops and every SF epilogue (include/gta.h, "Special values of the SFs").

  1. gta_apply_node anchors accuracy: every SF on tests/special_ref.py's PROBES against the staged
     fp64 reference, within SF_ULPS (the maxima measured on the MI355X plus one ulp).
     The reference is sf_stated: sf_ref but for SIGMOID's flushed denormal tail, which gta.h states
     (+0 from x <= -88.7228) and this pins exactly.
  2. every other SF site -- apply_edge (per-row, generic and flat forms), aggregate_expr,
     edge_softmax, both sf_out sites of the fused attention aggregate, every GEMM form's epilogue
     and the fused MLP -- is BITWISE equal to gta_apply_node on the same pre-SF values, NaN
     positions included ("same function as gta_apply_node's SF", gta.h).  Each site is driven so
     that its pre-SF value is a probe exactly; the non-idempotent SFs catch an SF applied twice.
  3. ADD, SUB, MUL and DIV over the 576 pairs of 24 probes: numpy's fp32 bits.
Non-finite VALUES are ordinary data here: every graph index is in range.
"""
import contextlib

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops
from tests import special_ref as S

pytestmark = pytest.mark.gpu

F32 = np.float32
P, PB = S.PROBES, S.PROBES_BF16


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


@contextlib.contextmanager
def module_attr(name, value):
    old = getattr(ops, name)
    setattr(ops, name, value)
    try:
        yield
    finally:
        setattr(ops, name, old)


def table(rows, F, probes=P, offset=0):
    """[rows, F] fp32: the probes laid out cyclically from probes[offset]."""
    idx = (np.arange(rows * F) + offset) % probes.size
    return np.ascontiguousarray(probes[idx].reshape(rows, F))


def dev_t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().float().cpu().numpy()


def assert_bits(got, want, what, inputs=None, mod_zero=False):
    """got == want bit for bit, NaNs by position (mod_zero: +0 and -0 equal, where a sum with +0
    legitimately follows the SF)."""
    got, want = host(got), host(want)
    ok = S.bits_same(got, want)
    if mod_zero:
        ok |= (got == 0) & (want == 0)
    assert ok.all(), f"{what}: " + S.describe(ok, want if inputs is None else inputs, got, want)


def sf_node(sf, pre):
    """The anchor: gta_apply_node's SF on the device tensor pre (generic and vector forms are
    compared with each other in test_apply_node_sf_on_probes)."""
    return ops.apply_node(None, sf, pre.contiguous())


def check_pre(pre, probes, what):
    """The site's pre-SF values are the probes (the sign of a zero apart: a sum with +0)."""
    ok = S.same(host(pre), probes.astype(np.float64))
    assert ok.all(), f"{what}: pre-SF values are not the probes: " + S.describe(ok, probes, host(pre), probes)


# ---------------------------------------------------------------- 1. the anchor

@pytest.mark.parametrize("vec", [1, 0])
@pytest.mark.parametrize("F", [4, 5])
@pytest.mark.parametrize("sf", S.SFS)
def test_apply_node_sf_on_probes(dev, sf, F, vec):
    rows = -(-P.size // F)
    a = table(rows, F)
    with knobs(apply_node_vec=vec):
        got = host(ops.apply_node(None, sf, dev_t(a, dev)))
    want = S.sf_stated(sf, a)
    ok = S.same(got, want, ulps=S.SF_ULPS[sf], zero_sign=S.zero_sign_fixed(sf, a))
    worst = S.ulp_diff(got, want).max()
    print(f"apply_node {sf} F={F} vec={vec}: max ulp {worst:.6f}")
    assert ok.all(), f"{sf}: " + S.describe(ok, a, got, want)


@pytest.mark.parametrize("sf", S.SFS)
def test_apply_node_sf_dense(dev, sf):
    """PROBES plus 4,096 log-spaced magnitudes per sign over [1e-6, 1e2]: the set SF_ULPS was measured on."""
    v = S.dense()
    a = table(-(-v.size // 4), 4, v)
    got = host(ops.apply_node(None, sf, dev_t(a, dev)))
    want = S.sf_stated(sf, a)
    ok = S.same(got, want, ulps=S.SF_ULPS[sf], zero_sign=S.zero_sign_fixed(sf, a))
    print(f"apply_node {sf} dense: max ulp {S.ulp_diff(got, want).max():.6f}")
    assert ok.all(), f"{sf}: " + S.describe(ok, a, got, want)


@pytest.mark.parametrize("vec", [1, 0])
@pytest.mark.parametrize("F", [4, 5])
@pytest.mark.parametrize("sf", S.SFS)
def test_apply_node_sf_bf16_operand(dev, sf, F, vec):
    """A bf16 `a` is widened exactly: the same bound on PROBES_BF16, and the fp32 call's bits."""
    a = table(-(-PB.size // F), F, PB)
    ab = dev_t(a, dev, torch.bfloat16)
    assert S.bits_same(host(ab), a).all()
    with knobs(apply_node_vec=vec):
        got_t = ops.apply_node(None, sf, ab)
        assert_bits(got_t, ops.apply_node(None, sf, dev_t(a, dev)), f"bf16 a vs fp32 a {sf}", a)
    got, want = host(got_t), S.sf_stated(sf, a)
    ok = S.same(got, want, ulps=S.SF_ULPS[sf], zero_sign=S.zero_sign_fixed(sf, a))
    assert ok.all(), f"{sf}: " + S.describe(ok, a, got, want)


# ---------------------------------------------------------------- 2. every other SF site

def _edge_graph(dev):
    """16 rows of degrees 0, 1, 2, 65 (cycling), 64 source columns, every column referenced."""
    deg = np.tile([0, 1, 2, 65], 4)
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = (np.arange(ip[-1]) * 7 % 64).astype(np.int32)
    assert set(ix.tolist()) == set(range(64))
    return G.from_numpy(ip, ix, device=dev, n_cols=64), ip, ix


@pytest.mark.parametrize("mode", ["src", "dst", "edge", "row"])
@pytest.mark.parametrize("form,F", [("rows", 4), ("rows", 5), ("generic", 4), ("generic", 5), ("flat", 64)])
@pytest.mark.parametrize("sf", S.SFS)
def test_apply_edge_sf_sites(dev, sf, form, F, mode):
    """out[e] = sf(a[idx(e)]) (modes src, dst, edge) and sf(a[e] * 1) with the ones a broadcast row:
    the pre-SF value is a probe exactly; bitwise gta_apply_node's SF of it."""
    g, ip, ix = _edge_graph(dev)
    rows_of = np.repeat(np.arange(16), np.diff(ip))
    n_rows = {"src": 64, "dst": 16, "edge": g.nnz, "row": g.nnz}[mode]
    sel = {"src": ix.astype(np.int64), "dst": rows_of, "edge": np.arange(g.nnz), "row": np.arange(g.nnz)}[mode]
    seen = 0
    with knobs(apply_edge_form=0 if form == "generic" else 1), module_attr("APPLY_EDGE_FLAT", form == "flat"):
        for off in range(0, P.size, n_rows * F):  # dst mode at F = 4: three tables cover the probes
            a = table(n_rows, F, P, off)
            ad = dev_t(a, dev)
            if mode == "row":
                got = ops.apply_edge(g, "MUL", sf, ad, "edge", torch.ones(1, F, device=dev), "edge", b_broadcast_row=True)
            else:
                got = ops.apply_edge(g, None, sf, ad, mode)
            want = sf_node(sf, ad)[torch.from_numpy(sel).to(dev)]
            assert_bits(got, want, f"apply_edge {form} {mode} {sf} F={F}", a[sel])
            seen += 1
    assert seen >= 1


@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("F,mode", [(128, "edge"), (128, "src"), (36, "edge"), (36, "src")])
@pytest.mark.parametrize("sf", S.SFS)
def test_aggregate_expr_sf_site(dev, sf, F, mode, lean):
    """Shape 1, bin NONE, every row exactly one edge: y[i] = 0 + sf(L0): gta_apply_node's bits (the
    sign of a zero apart: the sum starts from +0)."""
    n = -(-P.size // F)
    ip = np.arange(n + 1, dtype=np.int64)
    ix = np.arange(n, dtype=np.int32)[::-1].copy()
    g = G.from_numpy(ip, ix, device=dev, n_cols=n)
    a = table(n, F)
    ad = dev_t(a, dev)
    with knobs(expr_lean=lean):
        got = ops.aggregate_expr(g, 1, [(ad, mode)], [None], [sf])
    assert got is not None
    sel = ix.astype(np.int64) if mode == "src" else np.arange(n)
    want = sf_node(sf, ad)[torch.from_numpy(sel).to(dev)]
    assert_bits(got, want, f"aggregate_expr {sf} F={F} {mode} lean={lean}", a[sel], mod_zero=True)


@pytest.mark.parametrize("lane", [1, 0])
@pytest.mark.parametrize("sf", S.SFS)
def test_edge_softmax_sf_site(dev, sf, lane):
    """normalize off, a = probes, b = 0: out[e] = sf(a[dst] + 0)."""
    g, ip, ix = _edge_graph(dev)
    H = 16
    a = table(16, H)  # 256 slots
    ad, bd = dev_t(a, dev), torch.zeros(64, H, device=dev)
    with knobs(esm_lane=lane):
        got, _ = ops.edge_softmax(g, ad, bd, sf=sf, normalize=False)
    rows_of = torch.from_numpy(np.repeat(np.arange(16), np.diff(ip))).to(dev)
    want = ops.apply_node("ADD", sf, ad, torch.zeros_like(ad))[rows_of]
    assert_bits(got, want, f"edge_softmax {sf} lane={lane}", a[rows_of.cpu().numpy()])


@pytest.mark.parametrize("F,H,lean,direct", [(128, 8, 1, 1), (128, 8, 1, 0), (128, 8, 1, 2), (128, 8, 0, 1), (64, 4, 1, 1)])
@pytest.mark.parametrize("sf_out", S.SFS)
def test_gat_aggregate_sf_out_sites(dev, sf_out, F, H, lean, direct):
    """Both sf_out sites: single-item rows are written by the gather kernel, two-item rows
    (item_edges = 1, two edges) by the reduce.  a = b = 0 with sf = EXP makes every weight exactly 1
    and the partner edge points at an all-zero x row, so the pre-SF value is p + 0; rows without
    edges give sf_out(0), RECIP(0) = +inf included."""
    npr = -(-P.size // F)                       # probe rows of x: columns 1 .. npr (column 0: zeros)
    x = np.concatenate([np.zeros((1, F), F32), table(npr, F)])
    deg = np.array([1] * npr + [2] * npr + [0, 0])
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = np.concatenate([[c] for c in range(1, npr + 1)] + [[0, c] for c in range(1, npr + 1)]).astype(np.int32)
    n = len(deg)
    g = G.from_numpy(ip, ix, device=dev, n_cols=npr + 1)
    plan = g.blocked_plan(2, 1, 0)
    xd = dev_t(x, dev)
    a, b = torch.zeros(n, H, device=dev), torch.zeros(npr + 1, H, device=dev)
    with knobs(att_lean=lean, att_direct=direct):
        pre, _ = ops.gat_aggregate_blocked(g, xd, a, b, sf="EXP", normalize=False, plan=plan, blocks=2)
        got, _ = ops.gat_aggregate_blocked(g, xd, a, b, sf="EXP", normalize=False, plan=plan, blocks=2, sf_out=sf_out)
    probes = np.concatenate([x[1:], x[1:], np.zeros((2, F), F32)])
    check_pre(pre, probes, f"gat sf_out F={F}")
    assert_bits(got, sf_node(sf_out, pre), f"gat sf_out {sf_out} F={F} lean={lean} direct={direct}", probes)
    want0 = host(sf_node(sf_out, torch.zeros(1, F, device=dev)))[0]
    assert S.bits_same(host(got)[-2:], np.stack([want0, want0])).all()
    if sf_out == "RECIP":
        assert np.all(host(got)[-2:] == np.inf)


M_MM, N_MM = 333, 40   # 64-row groups plus a tail that is no multiple of 16; N > 32, N % 4 == 0, a column tail

MM_FORMS = {  # name -> (dtype, K, knobs, module attrs)
    "tile": ("f32", 48, {}, {"MM_FORM": "tile"}),
    "rows": ("f32", 48, {"mm_ring": 0}, {}),
    "rows_pf0": ("f32", 48, {"mm_ring": 0, "mm_prefetch": 0}, {}),
    "rows_pf2": ("f32", 48, {"mm_ring": 0, "mm_prefetch": 2}, {}),
    "ring": ("f32", 48, {"mm_ring": 1, "mm_wave": 0}, {}),
    "ring_fr2": ("f32", 48, {"mm_ring": 1, "mm_wave": 0, "mm_ring_fr": 2}, {}),
    "wave": ("f32", 48, {"mm_ring": 1, "mm_wave": 2}, {}),
    "ring_bf_mixed": ("mixed", 48, {"mm_ring": 1}, {}),
    "ring_bf_bf16": ("bf16", 48, {"mm_ring": 1}, {}),
    "rows_mixed_pf0": ("mixed", 48, {"mm_ring": 0, "mm_prefetch": 0}, {}),
    "rows_bf16_pf2": ("bf16", 48, {"mm_ring": 0, "mm_prefetch": 2}, {}),
    "tile_bf16": ("bf16", 48, {}, {"MM_FORM": "tile"}),
    "split2_ring": ("f32", 256, {"mm_split": 2, "mm_ring": 1}, {}),
    "split3_ring": ("f32", 256, {"mm_split": 3, "mm_ring": 1}, {}),
    "split2_rows": ("f32", 256, {"mm_split": 2, "mm_ring": 0}, {}),
    "split3_rows": ("f32", 256, {"mm_split": 3, "mm_ring": 0}, {}),
    "split3_mixed": ("mixed", 256, {"mm_split": 3}, {}),
    "split2_bf16": ("bf16", 256, {"mm_split": 2}, {}),
}


def _one_hot(M, K, probes):
    x = np.zeros((M, K), F32)
    m = np.arange(M)
    x[m, m % K] = probes[m % probes.size]
    return x, probes[m % probes.size]


@pytest.mark.parametrize("form", list(MM_FORMS))
def test_update_mm_sf_epilogues(dev, form):
    """Every GEMM form's SF epilogue through an exact-by-construction product: row m of x is zero but
    for one probe at column m % K and W is all ones, so every product is p * 1 or 0 * 1, every sum
    p + 0, and no inf * 0 arises.  out == gta_apply_node's SF of the SF-less product bitwise, for every
    SF (SIGMOID, EXP, ELU, RECIP and TANH are not idempotent: applied in both the slice kernel and
    the slice sum, or to a wrong accumulator fragment of the row / column tail, they differ)."""
    dt, K, kn, attrs = MM_FORMS[form]
    probes = P if dt == "f32" else PB
    assert M_MM >= probes.size
    x, p = _one_hot(M_MM, K, probes)
    xd = dev_t(x, dev, torch.bfloat16 if dt == "bf16" else None)
    wd = torch.ones(K, N_MM, device=dev, dtype=torch.float32 if dt == "f32" else torch.bfloat16)
    with contextlib.ExitStack() as st:
        st.enter_context(knobs(**kn))
        for k, v in attrs.items():
            st.enter_context(module_attr(k, v))
        if "mm_split" in kn:
            assert ops._mm_splits(M_MM, K, N_MM, {"f32": 0, "bf16": 1, "mixed": 2}[dt], dev) == kn["mm_split"]
        pre = ops.update_mm(xd, wd)
        outs = {sf: ops.update_mm(xd, wd, sf=sf) for sf in S.SFS}
    torch.cuda.synchronize()
    pp = np.repeat(p[:, None], N_MM, axis=1)
    check_pre(pre, pp, f"update_mm {form}")
    for sf, got in outs.items():
        assert_bits(got, sf_node(sf, pre), f"update_mm {form} {sf}", pp)


@pytest.mark.parametrize("sf1,sf2", [("RELU", "RELU"), ("RELU", None), (None, "RELU"), (None, None),
                                     ("SIGMOID", "TANH"), ("ELU", "EXP"), ("LEAKY_RELU", "RECIP")])
@pytest.mark.parametrize("xdt", ["f32", "bf16"])
def test_update_mlp_sf_sites(dev, sf1, sf2, xdt):
    """The fused MLP (template-specialised RELU / NONE pairs and the runtime SF pairs) == the two
    gta_update_mm_t calls bitwise on inputs that contain the probes, NaN positions included."""
    K1, N1, N2 = 48, 40, 24
    rng = np.random.default_rng(5)
    x, p = _one_hot(M_MM, K1, PB)
    w1 = dev_t(rng.standard_normal((K1, N1)).astype(F32), dev, torch.bfloat16)
    w2 = dev_t(rng.standard_normal((N1, N2)).astype(F32), dev, torch.bfloat16)
    xd = dev_t(x, dev)
    xin = xd.to(torch.bfloat16) if xdt == "bf16" else xd
    got = ops.update_mlp(xin, w1, w2, sf1, sf2)
    want = ops.update_mm(ops.update_mm(xd, w1, sf=sf1), w2, sf=sf2)
    assert_bits(got, want, f"update_mlp {sf1} {sf2} {xdt}", np.repeat(p[:, None], N2, axis=1))
    assert np.isnan(host(got)[np.isnan(p)]).all()


@pytest.mark.parametrize("sf1,sf2", [("RELU", "RELU"), ("RELU", None), (None, "RELU"), (None, None)])
def test_update_mlp_exact_values(dev, sf1, sf2):
    """One-hot x, W1 with ones in column 0 (zeros elsewhere), W2 with ones in row 0: every output of a
    finite probe p is sf2(bf16(sf1(bf16(p)))) exactly; NaN gives NaN, and so does +-inf (inf * 0 in
    W1's zero columns)."""
    K1, N1, N2 = 48, 40, 24
    rng = np.random.default_rng(6)
    x, p = _one_hot(M_MM, K1, P)
    w1 = np.zeros((K1, N1), F32)
    w1[:, 0] = 1
    w2 = S.bf16_round(rng.standard_normal((N1, N2)).astype(F32))
    w2[0] = 1
    got = host(ops.update_mlp(dev_t(x, dev), dev_t(w1, dev, torch.bfloat16), dev_t(w2, dev, torch.bfloat16), sf1, sf2))
    relu = lambda k, v: np.maximum(v, F32(0)) if k == "RELU" else v
    with np.errstate(all="ignore"):
        want = relu(sf2, S.bf16_round(relu(sf1, S.bf16_round(p))))
    want = np.where(np.isfinite(S.bf16_round(p)), want, F32(np.nan)).astype(F32)   # FLT_MAX rounds to inf
    want = np.repeat(want[:, None], N2, axis=1)
    ok = S.same(got, want.astype(np.float64))
    assert ok.all(), f"update_mlp {sf1} {sf2}: " + S.describe(ok, np.repeat(p[:, None], N2, axis=1), got, want)


# ---------------------------------------------------------------- 3. the binary ops

def _pairs():
    b = S.bin_probes()
    return np.repeat(b, b.size), np.tile(b, b.size)


@pytest.mark.parametrize("a_bf16", [False, True])
@pytest.mark.parametrize("vec", [1, 0])
@pytest.mark.parametrize("kind", S.BINS)
def test_apply_node_binary_ops(dev, kind, vec, a_bf16):
    a, b = _pairs()
    if a_bf16:
        a = S.bf16_round(a)
    a, b = a.reshape(-1, 4), b.reshape(-1, 4)
    with knobs(apply_node_vec=vec):
        got = host(ops.apply_node(kind, None, dev_t(a, dev, torch.bfloat16 if a_bf16 else None), dev_t(b, dev)))
    want = S.bin_ref(kind, a, b)
    ok = S.same(got, want, zero_sign=True)
    assert ok.all(), f"{kind}: " + S.describe(ok, np.stack([a, b], -1).reshape(-1, 2)[:, 0], got, want) + \
        f" (b: {b.ravel()[np.flatnonzero(~ok.ravel())[:6]]})"


@pytest.mark.parametrize("form,F", [("rows", 4), ("generic", 4), ("flat", 64)])
@pytest.mark.parametrize("kind", S.BINS)
def test_apply_edge_binary_ops(dev, kind, form, F):
    a, b = _pairs()
    a, b = a.reshape(-1, F), b.reshape(-1, F)
    e = a.shape[0]
    deg = np.zeros(16, np.int64)
    deg[[1, 2, 5]] = [1, 2, e - 3]
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    g = G.from_numpy(ip, (np.arange(e) % 16).astype(np.int32), device=dev, n_cols=16)
    with knobs(apply_edge_form=0 if form == "generic" else 1), module_attr("APPLY_EDGE_FLAT", form == "flat"):
        got = host(ops.apply_edge(g, kind, None, dev_t(a, dev), "edge", dev_t(b, dev), "edge"))
    want = S.bin_ref(kind, a, b)
    ok = S.same(got, want, zero_sign=True)
    assert ok.all(), f"{kind} {form}: " + S.describe(ok, a, got, want) + \
        f" (b: {b.ravel()[np.flatnonzero(~ok.ravel())[:6]]})"
