"""bf16 gathered tables in the column-blocked aggregate and the fused GAT attention aggregate
(gta_aggregate_blocked_x / gta_gat_aggregate_blocked_x, include/gta.h).

The contract is bitwise: a bf16 element widens to fp32 exactly and enters the fp32 kernel's own chain,
so a bf16 call equals the fp32 call on x.float() bit for bit, with the same plan, blocks, item_edges and
knobs.  Results are compared as int32 bit patterns (NaN != NaN), and once per shape with the fp64 oracle
at tests/test_gpu_ops.py's bound.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, executor, graph as G, ir, ops, pipeline, workloads
from gta_graph_tensor_acclelrator_for_general_gnn_amd.semantics import Semantics
from oracle import isa_ref
from oracle.exec_ref import execute_ref

from .test_gpu_footprint import Arena, _csr, _graph_in
from .test_gpu_ops import _check
from .test_ir_executor_cpu import compare

pytestmark = pytest.mark.gpu

_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, what
    diff = _bits(a) != _bits(b)
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} of {diff.numel()} elements differ in their bits"


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


def _graphs():
    """name -> (ip, ix): the two synthetic graphs (one with 400-edge rows: several items per row at
    item_edges 7, full unmasked steps at 256, two items of unequal length per wave) and one with empty
    rows, a 3-edge row and a heavy row; columns sorted per row."""
    def make():
        out = {}
        for name, (n, e) in {"g900": (900, 30000), "g5": (5, 2000)}.items():
            out[name] = G.synthetic(n, e, seed=11).numpy()
        rng = np.random.default_rng(4)
        deg = np.diff(out["g900"][0])[:300].copy()
        deg[[0, 17, 18, 299]] = 0
        deg[5], deg[6] = 1500, 3
        ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        ix = np.concatenate([np.sort(rng.integers(0, 300, d)) for d in deg]).astype(np.int32)
        out["empty"] = (ip, ix)
        return out
    return _memo("graphs", make)


def _dev_graph(name, dev):
    return _memo(("dg", name), lambda: G.from_numpy(*_graphs()[name], device=dev))


def _table(name, F, dev, seed=0):
    """The bf16 table of a graph, on the device, with its fp32 widening."""
    def make():
        n = len(_graphs()[name][0]) - 1
        g = torch.Generator().manual_seed(1000 * F + seed)
        xb = torch.randn(n, F, generator=g).to(torch.bfloat16).to(dev)
        return xb, xb.float()
    return _memo(("x", name, F, seed), make)


def _weights(name, heads, dev):
    def make():
        e = len(_graphs()[name][1])
        g = torch.Generator().manual_seed(77 + heads)
        return torch.rand(e, heads, generator=g).to(dev)
    return None if not heads else _memo(("w", name, heads), make)


def _plain_ref(name, F, heads, dev):
    def make():
        ip, ix = _graphs()[name]
        x = _table(name, F, dev)[1].cpu().numpy().astype(np.float64)
        w = _weights(name, heads, dev)
        w = None if w is None else w.cpu().numpy().astype(np.float64)
        return isa_ref.aggregate(ip, ix, x, "src", w), isa_ref.aggregate_abs(ip, ix, x, "src", w)
    return _memo(("ref", name, F, heads), make)


# ---------------------------------------------------------------------------------------------
# 1. bitwise twin, plain aggregate
# ---------------------------------------------------------------------------------------------

PLAIN = [(128, 0), (128, 8), (128, 1), (128, 4), (64, 0), (64, 4), (256, 16)]


@pytest.mark.parametrize("item_edges", [7, 256])
@pytest.mark.parametrize("blocks", [1, 5])
@pytest.mark.parametrize("F,heads", PLAIN)
def test_plain_bitwise_twin(dev, F, heads, blocks, item_edges):
    """aggregate_blocked(x_bf16) == aggregate_blocked(x_bf16.float()) bit for bit, and both match the
    fp64 oracle: half-wave lean and generic forms (F = 128: unweighted, 8 heads, one weight per edge,
    4 heads), quarter-wave forms (F = 64 / 256); split rows and short tails (item_edges 7), full
    unmasked steps (256)."""
    for name in ("g900", "g5", "empty"):
        g = _dev_graph(name, dev)
        xb, xf = _table(name, F, dev)
        w = _weights(name, heads, dev)
        plan = g.blocked_plan(blocks, item_edges)
        yb = ops.aggregate_blocked(g, xb, w, plan=plan)
        yf = ops.aggregate_blocked(g, xf, w, plan=plan)
        what = f"plain {name} F={F} heads={heads} B={blocks} items={item_edges}"
        _same_bits(yb, yf, what)
        ref, ab = _plain_ref(name, F, heads, dev)
        _check(yb, ref, ab, what)


def test_plain_row_scale_accumulate(dev):
    g = _dev_graph("g900", dev)
    xb, xf = _table("g900", 128, dev)
    w = _weights("g900", 8, dev)
    ip, ix = _graphs()["g900"]
    rs = torch.from_numpy((1.0 / np.maximum(np.diff(ip), 1)).astype(np.float32)).to(dev)
    y0 = torch.randn(g.n_rows, 128, generator=torch.Generator().manual_seed(3)).to(dev)
    plan = g.blocked_plan(5, 7)
    yb = ops.aggregate_blocked(g, xb, w, rs, out=y0.clone(), accumulate=True, plan=plan)
    yf = ops.aggregate_blocked(g, xf, w, rs, out=y0.clone(), accumulate=True, plan=plan)
    _same_bits(yb, yf, "row_scale + accumulate")
    x64, w64, r64 = xf.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64), rs.cpu().numpy().astype(np.float64)
    ref = isa_ref.aggregate(ip, ix, x64, "src", w64, r64) + y0.cpu().numpy()
    ab = isa_ref.aggregate_abs(ip, ix, x64, "src", w64, r64) + np.abs(y0.cpu().numpy())
    _check(yb, ref, ab, "row_scale + accumulate")


@pytest.mark.parametrize("F,heads", [(128, 8), (64, 4), (256, 16)])
def test_plain_pitched_view(dev, F, heads):
    """ldx = F + 8: a view into a wider table (16-B aligned rows that are not whole lines)."""
    g = _dev_graph("g900", dev)
    xb, xf = _table("g900", F, dev)
    wide = torch.full((g.n_cols, F + 8), float("nan"), dtype=torch.bfloat16, device=dev)
    wide[:, :F] = xb
    view = wide[:, :F]
    assert view.stride(0) == F + 8
    w = _weights("g900", heads, dev)
    for blocks, ie in ((1, 256), (5, 7)):
        plan = g.blocked_plan(blocks, ie)
        _same_bits(ops.aggregate_blocked(g, view, w, plan=plan), ops.aggregate_blocked(g, xf, w, plan=plan),
                   f"pitched F={F} B={blocks}")


@pytest.mark.parametrize("knob", ["seg_lean", "seg_lean_w1", "seg_alpha1"])
def test_plain_under_each_knob(dev, knob):
    g = _dev_graph("g900", dev)
    xb, xf = _table("g900", 128, dev)
    plan = g.blocked_plan(5, 256)
    base = {}
    for heads in (0, 1, 8):
        w = _weights("g900", heads, dev)
        base[heads] = ops.aggregate_blocked(g, xb, w, plan=plan)
    with _knobs(**{knob: 0}):
        for heads in (0, 1, 8):
            w = _weights("g900", heads, dev)
            yb = ops.aggregate_blocked(g, xb, w, plan=plan)
            _same_bits(yb, ops.aggregate_blocked(g, xf, w, plan=plan), f"{knob}=0 heads={heads}")
            _same_bits(yb, base[heads], f"{knob}=0 vs the default form, heads={heads}")  # every form: the same chain
    assert ops.get_debug(knob) == 1


# ---------------------------------------------------------------------------------------------
# 2. bitwise twin, attention
# ---------------------------------------------------------------------------------------------

def _scores(name, H, dev):
    def make():
        ip, _ = _graphs()[name]
        g = torch.Generator().manual_seed(500 + H)
        n = len(ip) - 1
        return torch.randn(n, H, generator=g).to(dev), torch.randn(n, H, generator=g).to(dev)
    return _memo(("ab", name, H), make)


def _att_pair(g, xb, xf, a, b, plan, what, **kw):
    yb, sb = ops.gat_aggregate_blocked(g, xb, a, b, want_sums=True, plan=plan, **kw)
    yf, sf = ops.gat_aggregate_blocked(g, xf, a, b, want_sums=True, plan=plan, **kw)
    _same_bits(yb, yf, what + " y")
    _same_bits(sb, sf, what + " sums")
    return yb, sb


@pytest.mark.parametrize("blocks", [1, 5])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("F,H", [(128, 8), (128, 4), (64, 4), (256, 16)])
def test_attention_bitwise_twin(dev, F, H, normalize, blocks):
    """gat_aggregate_blocked(x_bf16) == gat_aggregate_blocked(x_bf16.float()) bit for bit, y and sums:
    the lean k_att_h32 (with its direct write), the half-wave and quarter-wave generic forms, shifted
    and unshifted, with and without sf_out; (128, 8) under att_lean 0 / 1 and att_direct 0 / 1 / 2."""
    knob_sets = [{}]
    if (F, H) == (128, 8):
        knob_sets = [{"att_lean": l, "att_direct": d} for l in (0, 1) for d in (0, 1, 2)]
    for name in ("g900", "g5", "empty"):
        g = _dev_graph(name, dev)
        xb, xf = _table(name, F, dev)
        a, b = _scores(name, H, dev)
        shift = ops.softmax_shift(g, a, b, "EXP_LEAKY_RELU")
        for ie in (7, 256):
            plan = g.blocked_plan(blocks, ie)
            for ks in knob_sets:
                with _knobs(**ks):
                    for sh in (None, shift):
                        for sf_out in (None, "ELU"):
                            what = f"att {name} F={F} H={H} norm={normalize} B={blocks} items={ie} {ks} " \
                                   f"shifted={sh is not None} sf_out={sf_out}"
                            _att_pair(g, xb, xf, a, b, plan, what, normalize=normalize, shift=sh, sf_out=sf_out)
    # and the oracle, once per shape (unshifted, no sf_out), at test_gpu_ops' bound
    ip, ix = _graphs()["g900"]
    g = _dev_graph("g900", dev)
    xb, xf = _table("g900", F, dev)
    a, b = _scores("g900", H, dev)
    y, sums = ops.gat_aggregate_blocked(g, xb, a, b, normalize=normalize, want_sums=True, plan=g.blocked_plan(blocks, 256))
    x64, a64, b64 = (t.cpu().numpy().astype(np.float64) for t in (xf, a, b))
    ref, rsum = isa_ref.gat_aggregate(ip, ix, x64, a64, b64, "EXP_LEAKY_RELU", normalize)
    v, _ = isa_ref.edge_softmax(ip, ix, a64, b64, "EXP_LEAKY_RELU", False)
    scale = isa_ref.aggregate(ip, ix, np.abs(x64), "src", v)
    if normalize:
        scale = scale / np.repeat(np.where(rsum > 0, rsum, 1.0), F // H, axis=1) * 4
    _check(sums, rsum, rsum, "att sums vs oracle")
    _check(y, ref, scale, "att y vs oracle")


def test_attention_other_score_function(dev):
    """sf = EXP: the run-time-sf instantiations, shifted and unshifted."""
    g = _dev_graph("g900", dev)
    for F, H in ((128, 8), (64, 4)):
        xb, xf = _table("g900", F, dev)
        a, b = _scores("g900", H, dev)
        a, b = 0.2 * a, 0.2 * b
        shift = ops.softmax_shift(g, a, b, "EXP")
        for sh in (None, shift):
            _att_pair(g, xb, xf, a, b, g.blocked_plan(5, 7), f"att EXP F={F} shifted={sh is not None}", sf="EXP", shift=sh)


# ---------------------------------------------------------------------------------------------
# 3. special values: the widening is exact
# ---------------------------------------------------------------------------------------------

SPECIAL = {3: 0x7FC0, 10: 0x7F80, 20: 0xFF80, 30: 0x8000, 40: 0x0001, 41: 0x8001, 50: 0x007F}  # row -> bf16 bits


@pytest.mark.parametrize("F,heads", [(128, 8), (128, 0), (64, 4), (256, 16)])
def test_special_values_bitwise(dev, F, heads):
    """NaN, +-inf, -0 and bf16 denormals at known source rows: the bf16 call's bit patterns are the
    fp32 twin's (compared as int32: NaN != NaN), plain and attention; the NaN / inf sources reach
    exactly the rows that gather them."""
    g = _dev_graph("g900", dev)
    ip, ix = _graphs()["g900"]
    xb = _table("g900", F, dev)[0].clone()
    bits = xb.view(torch.int16)
    for r, v in SPECIAL.items():
        bits[r, ::3] = v - 0x10000 if v >= 0x8000 else v
    xf = xb.float()
    assert int(_bits(xf)[40, 0]) == 0x00010000 and int(_bits(xf)[30, 0]) == -0x80000000  # the exact widening itself
    w = _weights("g900", heads, dev)
    for blocks, ie in ((1, 256), (5, 7)):
        plan = g.blocked_plan(blocks, ie)
        yb = ops.aggregate_blocked(g, xb, w, plan=plan)
        _same_bits(yb, ops.aggregate_blocked(g, xf, w, plan=plan), f"special plain F={F} heads={heads} B={blocks}")
        # a row is non-finite in column 0 exactly when it gathers source 3 (NaN), 10 (+inf) or 20 (-inf)
        hit = np.array([np.isin(ix[ip[r]:ip[r + 1]], (3, 10, 20)).any() for r in range(len(ip) - 1)])
        assert np.array_equal(~np.isfinite(yb[:, 0].cpu().numpy()), hit)
        if heads:
            a, b = _scores("g900", heads, dev)
            _att_pair(g, xb, xf, a, b, plan, f"special att F={F} H={heads} B={blocks}")
    # a bf16 denormal gathered alone comes back as the same value: nothing is flushed by the widening
    one = G.from_numpy(np.array([0, 1], dtype=np.int64), np.array([40], dtype=np.int32), device=dev, n_cols=g.n_cols)
    y1 = ops.aggregate_blocked(one, xb, None, blocks=1)
    _same_bits(y1, ops.aggregate_blocked(one, xf, None, blocks=1), "one denormal edge")
    _same_bits(y1, xf[40:41], "a denormal gathered alone")


# ---------------------------------------------------------------------------------------------
# 4. guard band: only y / sums (and the plan's own workspace) are written; x's padding is never used
# ---------------------------------------------------------------------------------------------

N_GB, E_GB = 130, 3000


@pytest.mark.parametrize("F", [64, 128, 256])
def test_guard_band(dev, F):
    ip, ix = _csr(N_GB, E_GB, 2, sort=True)
    rng = np.random.default_rng(600 + F)
    H = F // 16
    x = rng.standard_normal((N_GB, F)).astype(np.float32)
    ar = Arena(dev, 8 << 20)
    g = _graph_in(ar, ip, ix, N_GB, "a8")
    xt = ar.table("x", x, "a8", dtype=torch.bfloat16)  # 8 poisoned padding columns per row, NaN rows behind
    assert xt.stride(0) == F + 8 and xt.data_ptr() % 16 == 0
    xw = xt.float().cpu().numpy().astype(np.float64)
    wt = ar.table("w", rng.random((len(ix), H)).astype(np.float32), "a")
    at = ar.table("a_dst", rng.standard_normal((N_GB, H)).astype(np.float32), "a")
    bt = ar.table("b_src", rng.standard_normal((N_GB, H)).astype(np.float32), "a")
    y = ar.out("y", N_GB, F, "a")
    sums = ar.mat("sums", N_GB, H)
    a64, b64 = at.cpu().numpy().astype(np.float64), bt.cpu().numpy().astype(np.float64)
    for blocks, ie in ((1, 64), (5, 7)):
        plan = g.blocked_plan(blocks, ie)
        for w in (None, wt):
            what = f"guard plain F={F} B={blocks} items={ie} weighted={w is not None}"
            ar.repoison("y")
            ar.seal()
            ops.aggregate_blocked(g, xt, w, out=y, plan=plan)
            ar.check([y], what)
            w64 = None if w is None else w.cpu().numpy().astype(np.float64)
            assert torch.isfinite(y).all(), what + ": poison reached y"
            _check(y, isa_ref.aggregate(ip, ix, xw, "src", w64), isa_ref.aggregate_abs(ip, ix, xw, "src", w64), what)
        shift = ops.softmax_shift(g, at, bt, "EXP_LEAKY_RELU")
        for sh in (None, shift):
            what = f"guard att F={F} B={blocks} items={ie} shifted={sh is not None}"
            ar.repoison("y")
            ar.repoison("sums")
            ar.seal()
            ops.gat_aggregate_blocked(g, xt, at, bt, out=y, sums=sums, plan=plan, shift=sh)
            ar.check([y, sums], what)
            assert torch.isfinite(y).all() and torch.isfinite(sums).all(), what + ": poison reached the outputs"
            ref, _ = isa_ref.gat_aggregate(ip, ix, xw, a64, b64, "EXP_LEAKY_RELU", True)
            np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=1e-4, atol=1e-5, err_msg=what)


# ---------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------

def _raw_plain(g, x_ptr, ldx, F, dtype, y, plan, dev):
    L = _lib.load()
    ws = plan.workspace(F)
    return L.gta_aggregate_blocked_x(g.indptr.data_ptr(), g.indices.data_ptr(), g.n_rows, g.n_cols, g.nnz, x_ptr, ldx, F,
                                     dtype, None, 0, 0, None, y.data_ptr(), y.stride(0), 0, plan.buf.data_ptr(),
                                     plan.blocks, plan.item_edges, ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)


def _raw_att(g, x_ptr, ldx, F, dtype, a, b, y, plan, dev):
    L = _lib.load()
    H = a.shape[1]
    ws = plan.workspace_att(F, H)
    return L.gta_gat_aggregate_blocked_x(g.indptr.data_ptr(), g.indices.data_ptr(), g.n_rows, g.n_cols, g.nnz, x_ptr,
                                         ldx, F, dtype, a.data_ptr(), H, b.data_ptr(), H, H, _lib.SF["EXP_LEAKY_RELU"], 1,
                                         0, y.data_ptr(), y.stride(0), None, plan.buf.data_ptr(), plan.blocks,
                                         plan.item_edges, ws.data_ptr(), None, torch.cuda.current_stream(dev).cuda_stream)


def test_refusals(dev):
    g = _dev_graph("g900", dev)
    F = 128
    xb, xf = _table("g900", F, dev)
    a, b = _scores("g900", 8, dev)
    plan = g.blocked_plan(4, 256)
    y = torch.zeros(g.n_rows, F, device=dev)
    # misaligned bf16 rows: ldx % 8 != 0 (ops: ValueError before the call; the library: UNSUPPORTED)
    odd = torch.zeros(g.n_cols, F + 4, dtype=torch.bfloat16, device=dev)[:, :F]
    with pytest.raises(ValueError, match="16-B aligned rows"):
        ops.aggregate_blocked(g, odd, None, plan=plan)
    with pytest.raises(ValueError, match="16-B aligned rows"):
        ops.gat_aggregate_blocked(g, odd, a, b, plan=plan)
    assert _raw_plain(g, odd.data_ptr(), F + 4, F, _lib.GTA_BF16, y, plan, dev) == _lib.ERR_UNSUPPORTED
    assert b"aggregate_blocked_x" in _lib.load().gta_last_error()
    assert _raw_att(g, odd.data_ptr(), F + 4, F, _lib.GTA_BF16, a, b, y, plan, dev) == _lib.ERR_UNSUPPORTED
    assert b"gat_aggregate_blocked_x" in _lib.load().gta_last_error()
    # a base that is 8-B but not 16-B aligned
    shifted = torch.zeros(g.n_cols * F + 8, dtype=torch.bfloat16, device=dev)[4:4 + g.n_cols * F].view(g.n_cols, F)
    assert shifted.data_ptr() % 16 == 8
    assert _raw_plain(g, shifted.data_ptr(), F, F, _lib.GTA_BF16, y, plan, dev) == _lib.ERR_UNSUPPORTED
    # a bad x_dtype
    for bad in (_lib.GTA_F32_BF16, 7, -1):
        assert _raw_plain(g, xb.data_ptr(), F, F, bad, y, plan, dev) == _lib.ERR_ARG
        assert _raw_att(g, xb.data_ptr(), F, F, bad, a, b, y, plan, dev) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert not bool(y.any()), "a refused call wrote y"
    # GTA_F32 through the new entry points is the old entry point
    assert _raw_plain(g, xf.data_ptr(), F, F, _lib.GTA_F32, y, plan, dev) == _lib.OK
    _same_bits(y, ops.aggregate_blocked(g, xf, None, plan=plan), "aggregate_blocked_x(GTA_F32)")
    assert _raw_att(g, xf.data_ptr(), F, F, _lib.GTA_F32, a, b, y, plan, dev) == _lib.OK
    _same_bits(y, ops.gat_aggregate_blocked(g, xf, a, b, plan=plan)[0], "gat_aggregate_blocked_x(GTA_F32)")
    # unsupported dtype / width at the ops level
    with pytest.raises(ValueError):
        ops.aggregate_blocked(g, xb.to(torch.float16), None, plan=plan)
    with pytest.raises(ValueError):
        ops.aggregate_blocked(g, torch.zeros(g.n_cols, 96, dtype=torch.bfloat16, device=dev), None, plan=plan)


def test_no_edges_writes_zeros_and_never_reads_x(dev):
    n, F = 37, 128
    g = G.from_numpy(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), device=dev)
    x = torch.full((n, F), float("nan"), dtype=torch.bfloat16, device=dev)
    y = ops.aggregate_blocked(g, x, None, blocks=2)
    assert y.shape == (n, F) and not bool(y.any())
    a = torch.randn(n, 8, device=dev)
    y, sums = ops.gat_aggregate_blocked(g, x, a, a, want_sums=True, blocks=2)
    assert not bool(y.any()) and not bool(sums.any())


# ---------------------------------------------------------------------------------------------
# 6. executor
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cora(golden_dir):
    z = np.load(os.path.join(golden_dir, "cora_graph.npz"))
    return z["indptr"], z["indices"]


def _golden(golden_dir, manifest, network, layer):
    rec = [s for s in manifest["streams"] if "file" in s and s["network"] == network and s["dataset"] == "cora"
           and s["layer"] == layer and not s["reorder"]][0]
    sem = Semantics.for_network(network, False)
    og = ir.OpGraph.load(os.path.join(golden_dir, "ops", rec["op_yaml"]), sem.inputs)
    st = ir.Stream.load(os.path.join(golden_dir, "streams", rec["file"]))
    return og, st, sem


def _executor(og, st, gd, tensors, sem, **kw):
    ex = executor.Executor(og, st, gd, tensors, sem, **kw)
    ex.blocked_min_table_bytes, ex.blocked_blocks = 0, 4
    return ex


def _blocked_plans(gd):
    return [k for k in gd._plans if isinstance(k, tuple) and k[0] == "blocked"]


def test_executor_gcn_layer2_bitwise(golden_dir, manifest, cora, dev):
    """GCN layer 2: the gathered table is the 128-wide model input (mm_first off: the aggregate runs
    at the input width).  On a pre-rounded input gather_dtype=bf16 gathers the same values from half
    the bytes: one cast, and the layer's outputs are bitwise those of the default run."""
    og, st, sem = _golden(golden_dir, manifest, "GCN", 2)
    ip, ix = cora
    gd = G.from_numpy(ip, ix, device=dev)
    tensors = {k: v.to(dev) for k, v in workloads.make_tensors(og, G.from_numpy(ip, ix), "GCN", seed=2).items()}
    assert tensors["x"].shape[1] == 128
    tensors["x"] = tensors["x"].bfloat16().float()
    outs = {}
    for gdt in (None, torch.bfloat16):
        ex = _executor(og, st, gd, tensors, sem, gather_dtype=gdt)
        ex.mm_first = False
        outs[gdt] = {k: v.clone() for k, v in ex.run().items()}
        assert ex.gather_casts == (0 if gdt is None else 1)
        assert _blocked_plans(gd), "the aggregate did not take the blocked form"
        if gdt is not None:
            (src, ver, cast), = ex._gather_cache.values()
            assert src is tensors["x"] and cast.dtype == torch.bfloat16
            by_bytes = ex.alg_bytes
        else:
            default_bytes = ex.alg_bytes
    for k in outs[None]:
        _same_bits(outs[None][k], outs[torch.bfloat16][k], f"GCN layer 2 output {k}")
    # the accounting follows the table's element size: 2 B fewer per gathered element, plus the cast pass
    assert by_bytes == default_bytes - gd.nnz * 128 * 2 + gd.n_rows * 128 * 6


def test_executor_bf16_model_input_takes_the_blocked_form(golden_dir, manifest, cora, dev):
    """GraphSAGE layer 2 on a bf16 model input: with gather_dtype=bf16 the table is gathered as it is
    (no cast) by the blocked kernels, and every op matches the fp64 oracle of the widened input at
    tests/test_gpu_executor.py's tolerance.  With the option off such a table keeps the row-chunked
    bf16 aggregate, as tests/test_gpu_executor.py pins it."""
    og, st, sem = _golden(golden_dir, manifest, "GraphSAGE", 2)
    ip, ix = cora
    gc = G.from_numpy(ip, ix)
    tensors_c = workloads.make_tensors(og, gc, "GraphSAGE", seed=4)
    xb = tensors_c["x"].bfloat16()
    tensors_c["x"] = xb.float()
    ref = execute_ref(og, sem, ip, ix, {k: v.double().numpy() for k, v in tensors_c.items()})
    for gdt, blocked in ((None, False), (torch.bfloat16, True)):
        gd = G.from_numpy(ip, ix, device=dev)
        tensors = {k: v.to(dev) for k, v in tensors_c.items()}
        tensors["x"] = ops.pitched(xb.to(dev))
        ex = _executor(og, st, gd, tensors, sem, gather_dtype=gdt)
        ex.mm_first = False
        ex.run()
        assert bool(_blocked_plans(gd)) == blocked
        assert ex.gather_casts == 0
        compare({i: ex.tensor_of(i) for i in range(len(og))}, ref, range(len(og)), rtol=2e-4)


def _gat_layer(dev, cora):
    def make():
        ip, ix = cora
        gd = G.from_numpy(ip, ix, device=dev)
        lay = pipeline.Layer("GAT", 1, gd, 1433, heads=8)
        tensors = {k: v.to(dev) for k, v in workloads.make_tensors(lay.opgraph, G.from_numpy(ip, ix), "GAT", seed=6).items()}
        return gd, lay, tensors
    return _memo("gat", make)


@pytest.mark.parametrize("stable", [False, True])
def test_executor_gat_layer1_bound(cora, dev, stable):
    """GAT layer 1, 8 heads, gather_dtype=bf16 against the fp32 run of the same layer.  The bound is
    derived: the normalised aggregate is a convex combination of rows of xW, and RNE to bf16 moves
    each element by at most 2^-9 relative, so before the SF the two runs differ by at most
    2^-9 max_rows |xW[:, c]| in column c; 2^-8 times that covers the fp32 rounding of both runs and an
    SF of Lipschitz constant <= 1."""
    gd, lay, tensors = _gat_layer(dev, cora)
    outs = {}
    for gdt in (None, torch.bfloat16):
        ex = _executor(lay.opgraph, lay.stream, gd, tensors, lay.sem, softmax_shift=stable, gather_dtype=gdt)
        res = ex.run()
        outs[gdt] = res[sorted(res)[-1]].clone()
        assert ex.gather_casts == (0 if gdt is None else 1)
    xw = ops.update_mm(tensors["x"], tensors["w:0"])
    assert xw.shape[1] == outs[None].shape[1] == 128
    bound = 2.0 ** -8 * xw.abs().amax(dim=0, keepdim=True)
    d = (outs[None] - outs[torch.bfloat16]).abs()
    print("GAT layer 1 bf16 gather: max |d| / bound =", float((d / bound).max()))
    assert bool(torch.isfinite(outs[torch.bfloat16]).all())
    assert bool((d <= bound).all()), f"{int((d > bound).sum())} elements past the bound, worst {float((d / bound).max()):.3f} of it"
    assert bool(d.any()), "the bf16 run is bitwise the fp32 run: the option did nothing"


def test_executor_auto_graph_keeps_the_option_apart(cora, dev):
    """run_stream: the replayed HIP graph equals the eager run, and a run with gather_dtype and one
    without never share a captured graph."""
    gd, lay, tensors = _gat_layer(dev, cora)
    executor.clear_auto_graphs()
    try:
        eager = {}
        for gdt in (None, torch.bfloat16):
            ex = executor.Executor(lay.opgraph, lay.stream, gd, tensors, lay.sem, gather_dtype=gdt)
            res = ex.run()
            eager[gdt] = res[sorted(res)[-1]].clone()
        assert not torch.equal(eager[None], eager[torch.bfloat16])
        for rep in range(3):  # call 1 eager, call 2 captures, call 3 replays; the two options interleaved
            for gdt in (None, torch.bfloat16):
                res, ex = executor.run_stream(lay.opgraph, lay.stream, gd, tensors, lay.sem, gather_dtype=gdt)
                out = res.outputs[sorted(res.outputs)[-1]]
                _same_bits(out, eager[gdt], f"run_stream call {rep + 1} gather_dtype={gdt}")
                assert ex.gather_dtype == gdt
        assert len(executor._AUTO) == 2
        assert sum(e.run is not None for e in executor._AUTO.values()) == 2, "a layer was not captured"
        # Layer.run threads the option the same way
        lay2 = pipeline.Layer("GAT", 1, gd, 1433, heads=8, op_array=lay.op_array, tile_size_list=lay.tile_size_list,
                              gather_dtype=torch.bfloat16)
        res, ex = lay2.run(tensors)
        assert ex.gather_dtype == torch.bfloat16
        _same_bits(res.outputs[sorted(res.outputs)[-1]], eager[torch.bfloat16], "Layer.run")
    finally:
        executor.clear_auto_graphs()
