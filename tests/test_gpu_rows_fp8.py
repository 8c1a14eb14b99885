"""e4m3 (GTA_FP8) rows in the row-chunked aggregate (k_agg_rows_f8): every code widens exactly, and
the sums are within the project's bound of the fp64 sum of the widened table (gta.h)."""
import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import executor, graph as G, ops, pipeline, workloads
from oracle import isa_ref
from oracle.sampled import SampledChecker

from .test_gpu_blocked_bf16 import _dev_graph, _graphs, _memo, _same_bits, _weights, cora  # noqa: F401
from .test_gpu_ops import _check

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn
NAMES = ("g900", "g5", "empty")


def _table8(name, F, dev):
    """The e4m3 table of a graph (randn * 40, cast on the CPU: the definition), laid out on the device,
    and its fp32 widening."""
    def make():
        n = len(_graphs()[name][0]) - 1
        xf = ops.to_fp8(torch.randn(n, F, generator=torch.Generator().manual_seed(8000 + F)) * 40).float().to(dev)
        return ops.to_fp8(xf), xf  # (e4m3 values: the second cast rounds nothing)
    return _memo(("rows8 x", name, F), make)


def _ref(name, F, heads, mode, dev, row_scale=None):
    def make():
        ip, ix = _graphs()[name]
        x = _table8(name, F, dev)[1].cpu().numpy().astype(np.float64)
        w = _weights(name, heads, dev)
        w = None if w is None else w.cpu().numpy().astype(np.float64)
        rs = None if row_scale is None else row_scale.cpu().numpy().astype(np.float64)
        return isa_ref.aggregate(ip, ix, x, mode, w, rs), isa_ref.aggregate_abs(ip, ix, x, mode, w, rs)
    return make() if row_scale is not None else _memo(("rows8", name, F, heads, mode), make)


@pytest.mark.parametrize("F", [7, 16, 100, 256])
def test_all_256_codes_widen_exactly(dev, F):
    """Every byte value at every column (every byte position of a piece, the partial last piece, 1 / 8 /
    16 lanes per row), one edge per row: the aggregate is the gathered row of x8.float()."""
    n = 256
    codes = ((torch.arange(n).view(n, 1) + torch.arange(F).view(1, F)) % 256).to(torch.uint8)
    buf = torch.zeros(n, -(-F // 16) * 16, dtype=torch.uint8)
    buf[:, :F] = codes
    x8 = buf.to(dev).view(FP8)[:, :F]
    src = np.random.default_rng(3).permutation(n).astype(np.int32)
    g = G.from_numpy(np.arange(n + 1, dtype=np.int64), src, device=dev)
    y = ops.aggregate(g, x8).cpu().numpy()
    assert np.array_equal(y, codes.view(FP8).float().numpy()[src], equal_nan=True)


@pytest.mark.parametrize("mode", ["src", "dst"])
@pytest.mark.parametrize("plan", [None, 64])
@pytest.mark.parametrize("F,heads", [(4, 0), (20, 1), (100, 0), (100, 1), (128, 8), (200, 0), (256, 16)])
def test_against_fp64_of_the_widened_table(dev, F, heads, plan, mode):
    for name in NAMES:
        g = _dev_graph(name, dev)
        if plan is not None and name == "g900":
            assert g.plan(plan).splits > 0  # heavy rows split: the combine runs
        y = ops.aggregate(g, _table8(name, F, dev)[0], mode, _weights(name, heads, dev), plan=plan)
        _check(y, *_ref(name, F, heads, mode, dev), f"fp8 rows {name} F={F} heads={heads} plan={plan} {mode}")


@pytest.mark.parametrize("plan", [None, 64])
def test_other_forms_at_the_products_width(dev, plan):
    """F = 100 on a 128-B pitch: row_scale, accumulate, the self term from a bf16 x_self into an fp32 and
    a bf16 y (its bound: plus the rounding of the stored value, 2^-8 |ref|); two calls bitwise equal."""
    F, name = 100, "g900"
    g = _dev_graph(name, dev)
    ip, ix = _graphs()[name]
    gen = torch.Generator().manual_seed(5)
    x8 = ops.to_fp8(_table8(name, F, dev)[1], lines=True)
    assert x8.stride(0) == 128
    w = _weights(name, 1, dev)
    ref, scale = _ref(name, F, 1, "src", dev)
    y = ops.aggregate(g, x8, "src", w, plan=plan)
    _check(y, ref, scale, "128-B pitch")
    _same_bits(y, ops.aggregate(g, x8, "src", w, plan=plan), "two calls")
    rs = torch.rand(g.n_rows, generator=gen).to(dev)
    _check(ops.aggregate(g, x8, "src", w, row_scale=rs, plan=plan), *_ref(name, F, 1, "src", dev, rs), "row_scale")
    y0 = torch.randn(g.n_rows, F, generator=gen).to(dev)
    y0n = y0.cpu().numpy().astype(np.float64)
    _check(ops.aggregate(g, x8, "src", w, out=y0.clone(), accumulate=True, plan=plan), y0n + ref, np.abs(y0n) + scale,
           "accumulate")
    xs = ops.pitched((torch.randn(g.n_rows, F, generator=gen) * 30).bfloat16().to(dev))
    s = torch.tensor([1.25], device=dev)
    sref = xs.float().cpu().numpy().astype(np.float64) * 1.25
    yf = ops.aggregate(g, x8, "src", w, plan=plan, self_term=(xs, s))
    _check(yf, sref + ref, np.abs(sref) + scale, "self term, fp32 y")
    yb = ops.aggregate(g, x8, "src", w, plan=plan, self_term=(xs, s), out_dtype=torch.bfloat16)
    assert yb.dtype == torch.bfloat16
    _check(yb.float(), sref + ref, np.abs(sref) + scale + 2.0 ** -8 * np.abs(sref + ref) / 1e-5, "self term, bf16 y")
    with pytest.raises(Exception):  # full-width weights: refused, and y stays as it was
        ops.aggregate(g, x8, "src", torch.rand(g.nnz, F, device=dev), out=y0, accumulate=True)
    assert np.array_equal(y0.cpu().numpy().astype(np.float64), y0n)


def test_executor_gin_layer1_at_the_products_width(cora, dev):
    """GIN layer 1 with a bf16 model input of 100 columns (gin-products' form) holding e4m3 values:
    fp8_rows off is bitwise the run without it; on, the aggregate gathers one cast table and every op
    stays within its bound of the oracle on its own inputs."""
    ip, ix = cora
    gd = G.from_numpy(ip, ix, device=dev)
    lay = pipeline.Layer("GIN", 1, gd, 100)
    t = workloads.make_tensors(lay.opgraph, gd, "GIN", seed=3, dtype_w=torch.bfloat16)
    t["x"] = ops.pitched(ops.to_fp8(t["x"] * 8).float().bfloat16())  # e4m3 values: the cast rounds nothing
    outs = {}
    for key, kw in (("plain", {}), ("off", dict(gather_dtype=FP8)), ("on", dict(gather_dtype=FP8, fp8_rows=True))):
        ex = executor.Executor(lay.opgraph, lay.stream, gd, t, lay.sem, **kw)
        outs[key] = {k: v.clone() for k, v in ex.run().items()}
        assert ex.gather_casts == (1 if key == "on" else 0), key
        if key == "on":
            (_, _, cast), = ex._gather_cache.values()
            assert cast.dtype == FP8 and cast.stride(0) == 128
            assert SampledChecker(ex, ip, ix).check(n_samples=32, seed=1, n_gather=128)
    for k in outs["plain"]:
        assert torch.equal(outs["plain"][k], outs["off"][k]), f"fp8_rows off moved output {k}"
