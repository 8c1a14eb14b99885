"""The shifted (overflow-safe) softmax on the GPU: gta_softmax_shift, gta_edge_softmax_shifted,
gta_gat_aggregate_blocked_shifted, and the whole GAT layer with pipeline.Layer(stable_softmax=True).

Reference and bounds: tests/softmax_shift_ref.py -- the scores and their row maxima emulated in
np.float32 exactly, everything after them in fp64; bounds |d| <= 1e-5 * scale + 1e-6 with the
project's scales.  tests/test_softmax_shift_cpu.py confirms on the CPU that an fp32 numpy emulation
of the shifted algorithm stays inside these bounds for every element of every input used here
(test_reference_properties_and_fp32_emulation_on_the_softmax_inputs,
test_fp32_emulation_on_the_aggregate_inputs).

Inputs: b_src = 3 N(0, 1); a_dst = N(0, 1) plus a per-row offset cycling through {0, +120, -600}.
+120 makes the unshifted expf overflow (inf / inf); -600 gives g of about -120, so every unshifted v
and the row sum underflow to 0 (0 / 0).  Every tensor of a call is a view into a poisoned arena
(tests/test_gpu_footprint.py): padded tables (lda, ldb > heads), guard bands checked after the call.
"""
import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import executor, frontend, graph as G, ops, pipeline, workloads

from . import softmax_shift_ref as R
from .test_gpu_footprint import Arena, _graph_in, _knobs
from .test_gpu_ops import _check

gpu = pytest.mark.gpu
CAP = 8 << 20
SFS = ["EXP_LEAKY_RELU", "EXP"]
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _np(t):
    return t.detach().float().cpu().numpy()


def _ok(got, ref, scale, what):
    g = _np(got)
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} non-finite outputs"
    _check(got.detach().float(), ref, scale, what)


def _softmax_case(H, sf):
    def make():
        ip, ix, nc = R.softmax_graph()
        a, b = R.case(len(ip) - 1, nc, H, 100 + H)
        ref = R.reference(ip, ix, a, b, sf)
        return ip, ix, nc, a, b, ref, R.bounds(ref)
    return _memo(("softmax", H, sf), make)


# ---------------------------------------------------------------------------------------------
# 1. the row maxima are exact
# ---------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("lay", ["a", "b"])
@pytest.mark.parametrize("sf", SFS)
@pytest.mark.parametrize("H", [1, 8, 16, 64])
def test_softmax_shift_is_exact(dev, H, sf, lay):
    """Bitwise the fp32 emulation (up to the sign of a zero) on rows of degree 0, 1, 63, 64, 65, 257
    and 700; one NaN in b_src reaches exactly the rows that reference it, in that head."""
    ip, ix, nc, a, b, _, _ = _softmax_case(H, sf)
    n = len(ip) - 1
    assert {0, 1, 63, 64, 65, 257, 700} <= set(np.diff(ip).tolist())
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, nc, lay)
    at, bt = ar.table("a_dst", a, lay), ar.table("b_src", b, lay)
    assert at.stride(0) > H and bt.stride(0) > H
    sh = ar.mat("shift", n, H)
    ar.seal()
    assert ops.softmax_shift(g, at, bt, sf, out=sh) is sh
    ar.check([sh], f"softmax_shift H={H} {sf} lay={lay}")
    want = R.shift(ip, ix, a, b, sf)
    assert np.isfinite(want).all() and (want[np.diff(ip) == 0] == 0).all()
    assert np.array_equal(_np(sh), want), f"max |d| = {np.abs(_np(sh) - want).max()}"
    # NaN propagates: the row every degree class references most, one head
    src, h0 = int(np.bincount(ix, minlength=nc).argmax()), H // 2
    b2 = b.copy()
    b2[src, h0] = np.nan
    bt.copy_(torch.from_numpy(b2))
    ar.seal()
    ops.softmax_shift(g, at, bt, sf, out=sh)
    ar.check([sh], "softmax_shift with a NaN source score")
    want2 = R.shift(ip, ix, a, b2, sf)
    hit = np.zeros((n, H), bool)
    hit[np.unique(R.rows_of(ip)[ix == src]), h0] = True
    assert hit.any() and not hit.all() and np.array_equal(np.isnan(want2), hit)
    assert np.array_equal(np.isnan(_np(sh)), hit)
    assert np.array_equal(_np(sh), want2, equal_nan=True)


@gpu
def test_softmax_shift_without_edges_writes_zeros(dev):
    g = G.from_numpy(np.zeros(6, np.int64), np.zeros(0, np.int32), device=dev, n_cols=4)
    a = torch.full((5, 8), float("nan"), device=dev)
    out = torch.full((5, 8), 7.0, device=dev)
    ops.softmax_shift(g, a, torch.empty(4, 8, device=dev), out=out)
    assert (out == 0).all()


# ---------------------------------------------------------------------------------------------
# 2. edge softmax
# ---------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("sf", SFS)
@pytest.mark.parametrize("H", [1, 8, 16])
def test_edge_softmax_shifted(dev, H, sf):
    """Generic form (esm_lane 0, and H = 1) and the edge-per-lane form (H = 8: 4 chunks kept, H = 16:
    2; the 700-edge row parks its later chunks in `out`), normalize on and off.  Values within the
    bounds, every output finite, every non-empty row's sum >= 1 -- and the unshifted call on the same
    inputs gives non-finite alpha on the offset rows: the gap this closes."""
    ip, ix, nc, a, b, ref, sc = _softmax_case(H, sf)
    n, deg = len(ip) - 1, np.diff(ip)
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, nc, "a")
    at, bt = ar.table("a_dst", a, "a"), ar.table("b_src", b, "a")
    out, sums, sh = ar.mat("out", len(ix), H), ar.mat("sums", n, H), ar.mat("shift", n, H)
    ops.softmax_shift(g, at, bt, sf, out=sh)
    for lane in (1, 0):
        with _knobs(esm_lane=lane):
            for normalize in (True, False):
                what = f"edge_softmax shifted H={H} {sf} esm_lane={lane} norm={normalize}"
                ar.repoison("out")
                ar.repoison("sums")
                ar.seal()
                ops.edge_softmax(g, at, bt, sf, normalize=normalize, out=out, sums=sums, shift=sh)
                ar.check([out, sums], what)
                _ok(sums, ref["sums"], sc["sums"], what + " sums")
                if normalize:
                    _ok(out, ref["alpha"], sc["alpha"], what)
                else:
                    _ok(out, ref["v"], sc["v"], what)
                    assert (_np(out) <= 1).all()
                assert (_np(sums)[deg > 0] >= 1).all() and (_np(sums)[deg == 0] == 0).all()
            alpha, _ = ops.edge_softmax(g, at, bt, sf, normalize=True)  # unshifted, same inputs
            bad = ~np.isfinite(_np(alpha)).all(axis=1)
            rows = R.rows_of(ip)
            assert bad[rows % 3 != 0].all(), "the unshifted softmax survived +120 / -600 offsets"
            assert not bad[rows % 3 == 0].any()


# ---------------------------------------------------------------------------------------------
# 3. the fused attention aggregate
# ---------------------------------------------------------------------------------------------

def _agg_case(F, H, sf, offsets=True):
    def make():
        ip, ix, nc = R.blocked_graph()
        a, b = R.case(300, nc, H, 200 + F + H, offsets)
        x = np.random.default_rng(300 + F).standard_normal((nc, F)).astype(np.float32)
        ref = R.reference(ip, ix, a, b, sf, x=x)
        return ip, ix, nc, a, b, x, ref, R.bounds(ref, F)
    return _memo(("agg", F, H, sf, offsets), make)


@gpu
@pytest.mark.parametrize("F,H,sf", [(128, 8, "EXP_LEAKY_RELU"), (128, 4, "EXP_LEAKY_RELU"), (64, 4, "EXP_LEAKY_RELU"),
                                    (256, 16, "EXP_LEAKY_RELU"), (128, 8, "EXP")])
def test_gat_aggregate_blocked_shifted(dev, F, H, sf):
    """(128, 8): the lean k_att_h32 (att_lean 1) and the half-wave generic form (0); (128, 4) the
    half-wave form; (64, 4), (256, 16) the quarter-wave forms; EXP at (128, 8) the run-time-SF
    form.  Blocks 1 / 2 (the direct epilogue) / 5, item_edges 7 / 64, normalize on and off with sums,
    sf_out RELU.  Within the bounds, finite, guard bands untouched, and the fused y against
    edge_softmax_shifted followed by the weighted aggregate, to the same bound."""
    ip, ix, nc, a, b, x, ref, sc = _agg_case(F, H, sf)
    n = 300
    ar = Arena(dev, CAP)
    g = _graph_in(ar, ip, ix, nc, "a")
    xt, at, bt = ar.table("x", x, "a"), ar.table("a_dst", a, "a"), ar.table("b_src", b, "a")
    y = ar.out("y", n, F, "a")
    sums, sh = ar.mat("sums", n, H), ar.mat("shift", n, H)
    ops.softmax_shift(g, at, bt, sf, out=sh)
    unfused = {}
    for normalize in (True, False):
        w, _ = ops.edge_softmax(g, at, bt, sf, normalize=normalize, shift=sh)
        unfused[normalize] = _np(ops.aggregate(g, xt, "src", w)).astype(np.float64)
    leans = (1, 0) if (F, H, sf) == (128, 8, "EXP_LEAKY_RELU") else (1,)
    for blocks in (1, 2, 5):
        for ie in (7, 64):
            plan = g.blocked_plan(blocks, ie)
            for lean in leans:
                with _knobs(att_lean=lean):
                    for normalize, sf_out, ws in ((True, None, True), (False, None, True), (True, "RELU", False)):
                        what = f"gat_aggregate_blocked shifted F={F} H={H} {sf} B={blocks} items={ie} att_lean={lean} " \
                               f"norm={normalize} sf_out={sf_out}"
                        ar.repoison("y")
                        ar.repoison("sums")
                        ar.seal()
                        ops.gat_aggregate_blocked(g, xt, at, bt, sf, normalize=normalize, out=y,
                                                  sums=sums if ws else None, plan=plan, blocks=blocks, sf_out=sf_out,
                                                  shift=sh)
                        ar.check([y] + ([sums] if ws else []), what)
                        want, scale = (ref["y"], sc["y"]) if normalize else (ref["num"], sc["num"])
                        post = (lambda v: np.maximum(v, 0.0)) if sf_out else (lambda v: v)
                        _ok(y, post(want), scale, what)
                        _check(y.detach().float(), post(unfused[normalize]), scale, what + " against the unfused ops")
                        if ws:
                            _ok(sums, ref["sums"], sc["sums"], what + " sums")
    # the gap: unshifted, the offset rows are not finite
    y0, _ = ops.gat_aggregate_blocked(g, xt, at, bt, sf, normalize=True, plan=g.blocked_plan(2, 64), blocks=2)
    bad = ~np.isfinite(_np(y0)).all(axis=1)
    off = (np.arange(n) % 3 != 0) & (np.diff(ip) > 0)
    assert bad[off].all() and not bad[~off].any()


# ---------------------------------------------------------------------------------------------
# 4. where nothing overflows the shift changes nothing
# ---------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("sf", SFS)
def test_shifted_equals_unshifted_on_unit_scores(dev, sf):
    """N(0, 1) scores: shifted and unshifted alpha and normalized y both lie within the bounds of
    the one fp64 reference (alpha and y do not depend on the shift)."""
    F, H = 128, 8
    ip, ix, nc, a, b, x, ref, sc = _agg_case(F, H, sf, offsets=False)
    g = G.from_numpy(ip, ix, device=dev, n_cols=nc)
    xt, at, bt = (torch.from_numpy(t).to(dev) for t in (x, a, b))
    sh = ops.softmax_shift(g, at, bt, sf)
    for shift in (None, sh):
        what = f"{sf} {'shifted' if shift is not None else 'unshifted'}"
        alpha, sums = ops.edge_softmax(g, at, bt, sf, normalize=True, want_sums=True, shift=shift)
        _ok(alpha, ref["alpha"], sc["alpha"], what + " alpha")
        for blocks in (1, 5):
            yv, _ = ops.gat_aggregate_blocked(g, xt, at, bt, sf, normalize=True, blocks=blocks, shift=shift)
            _ok(yv, ref["y"], sc["y"], what + f" y B={blocks}")
        if shift is not None:
            _ok(sums, ref["sums"], sc["sums"], what + " sums")


# ---------------------------------------------------------------------------------------------
# 5. the whole layer
# ---------------------------------------------------------------------------------------------

def _gat_layer(g, reorder, **kw):
    """GAT layer 1 (F = 128, 8 heads).  None of the search's first candidates for the reordered form
    lowers on a graph this small: it runs with every op in a block of its own."""
    if not reorder:
        return pipeline.Layer("GAT", 1, g, 128, heads=8, **kw)
    n = len(frontend.gen_ops("GAT", 1, g.n_rows, g.nnz, 128, True, 8))
    return pipeline.Layer("GAT", 1, g, 128, reorder=True, heads=8, op_array=[[i] for i in range(n)],
                          tile_size_list=[[64, 1]] * n, **kw)


def _layer_tensors(lay, g, offsets):
    """make_tensors' inputs; with offsets, feature 0 of h = x W0 carries the per-row offset (x[:, 0]
    = offset, W0 passes column 0 through alone), the destination score weights add it to every head
    and the source score weights ignore it and are scaled by 3."""
    t = workloads.make_tensors(lay.opgraph, g, "GAT", seed=7)
    if offsets:
        n = g.n_rows
        off = torch.tensor(R.OFFSETS, dtype=torch.float32)[torch.arange(n) % 3]
        t["x"][:, 0] = off.to(t["x"].device)
        w0, w1, w2 = t["w:0"], t["w:1"], t["w:2"]
        w0[0, :], w0[:, 0], w0[0, 0] = 0.0, 0.0, 1.0
        w1[0, :] = 1.0
        w2 *= 3.0
        w2[0, :] = 0.0
    return t


def _layer_ref(lay, ex, ip, ix):
    """The layer's tail in fp64 from the run's own fp32 h = x W0 and scores (ops 0-2, whose GEMMs
    other tests cover): s and m emulated in fp32, then alpha, the aggregate and ELU in fp64.  The
    bound is the fused aggregate's (ELU is 1-Lipschitz)."""
    h, a, b = (_np(ex.tensor_of(i)) for i in (0, 1, 2))
    ref = R.reference(ip, ix, a, b, "EXP_LEAKY_RELU", x=h)
    y = ref["y"]
    return np.where(y > 0, y, np.expm1(np.minimum(y, 0))), R.bounds(ref, h.shape[1])["y"]


@gpu
@pytest.mark.parametrize("reorder", [False, True])
def test_gat_layer_with_stable_softmax(dev, reorder):
    ip, ix, nc = R.blocked_graph(empty=0)  # GAT-trans divides 0 / 0 on a row without edges, with or without the shift
    g = G.from_numpy(ip, ix, device=dev, n_cols=nc)
    executor.clear_auto_graphs()
    try:
        lay = _gat_layer(g, reorder, stable_softmax=True)
        t = _layer_tensors(lay, g, offsets=True)
        res, ex = lay.run(t)
        assert ex.softmax_shift is True
        (k, out), = res.outputs.items()
        first = out.clone()
        want, scale = _layer_ref(lay, ex, ip, ix)
        _ok(first, want, scale, f"GAT layer reorder={reorder} stable_softmax")
        rows = np.arange(300)
        assert (np.abs(want[(rows % 3 != 0) & (np.diff(ip) > 0)]) > 0).any()
        for _ in range(3):  # the second call captures the layer as a HIP graph, later ones replay it
            res2, _ = lay.run(t)
            assert torch.equal(res2.outputs[k], first)
        assert any(e.run is not None for e in executor._AUTO.values()), "the layer was not captured"
        # the option off, the same inputs: inf / inf and 0 / 0
        plain = _gat_layer(g, reorder)
        assert plain.stable_softmax is False
        res0, ex0 = plain.run(t)
        assert ex0.softmax_shift is False
        bad = ~np.isfinite(_np(res0.outputs[k])).all(axis=1)
        off = (rows % 3 != 0) & (np.diff(ip) > 0)
        assert bad[off].all() and not bad[~off].any()
    finally:
        executor.clear_auto_graphs()


@gpu
@pytest.mark.parametrize("reorder", [False, True])
def test_gat_layer_default_is_the_unshifted_path_bitwise(dev, reorder):
    """Option off, N(0, 1) inputs: the layer's aggregate is bitwise the unshifted op called directly
    on the layer's own h and scores, as before this option existed."""
    ip, ix, nc = R.blocked_graph(empty=0)  # GAT-trans divides 0 / 0 on a row without edges, with or without the shift
    g = G.from_numpy(ip, ix, device=dev, n_cols=nc)
    executor.clear_auto_graphs()
    try:
        lay = _gat_layer(g, reorder)
        t = _layer_tensors(lay, g, offsets=False)
        res, ex = lay.run(t)
        assert not ex._att_shift and ex.softmax_shift is False
        h, a, b = (ex.tensor_of(i).contiguous() for i in (0, 1, 2))
        B = ops.BlockedPlan.auto_blocks(g, 128)
        (k, out), = res.outputs.items()
        if reorder:
            num, sums = ops.gat_aggregate_blocked(g, h, a, b, normalize=False, want_sums=True, blocks=B)
            assert torch.equal(ex.tensor_of(10), num) and torch.equal(ex.tensor_of(9), sums)
        else:
            y, _ = ops.gat_aggregate_blocked(g, h, a, b, normalize=True, blocks=B, sf_out="ELU")
            assert torch.equal(out, y)
    finally:
        executor.clear_auto_graphs()
