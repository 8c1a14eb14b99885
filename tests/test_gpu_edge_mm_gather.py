"""gta_aggregate_edge_mm on the GPU against numpy fp64, per element within
    sum_e [1e-5 (sum_k |ef||W| + |p| + |q|) + 1e-6]  +  deg 2^-23 sum_e |t|  +  sum_e SF_ULPS[sf] ulp32(t)
(gta_update_mm_t's GTA_F32 bound through a 1-Lipschitz SF and the sum, the sequential fp32 summation
bound with a factor 2, special_ref's SF accuracy); its footprint in an Arena; the executor's route."""
import functools

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, executor, graph as G, ops, pipeline, workloads

from . import exec_trace, special_ref
from .test_gpu_footprint import Arena, _graph_in, _p, _st

pytestmark = pytest.mark.gpu
SF_ULPS = dict(special_ref.SF_ULPS, NONE=0.0)
SF64 = {"NONE": lambda z: z, "RELU": lambda z: np.maximum(z, 0.0), "TANH": np.tanh}


def _csr():
    # empty rows at both ends, degree 1, a row ending on edge 64, a 300-edge row starting there, 81 rows of degree 1-3
    rng = np.random.default_rng(7)
    mixed = rng.integers(0, 41, 100)
    mixed[::9] = 0
    deg = np.concatenate([[0, 0, 0, 1, 61, 2, 300], np.tile([1, 2, 3], 27), mixed, [1, 37, 0, 0]])
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    assert ip[6] == 64 and ip[-1] % 64 != 0 and ip[-1] < 3000 and len(deg) > 190
    return ip, rng.integers(0, len(deg), int(ip[-1])).astype(np.int32)


GRAPHS = {"built": _csr(), "tiny": (np.array([0, 0, 5, 5, 27, 29], np.int64), np.arange(29, dtype=np.int32) % 5),
          "empty": (np.zeros(8, np.int64), np.zeros(0, np.int32))}
_sums = lambda ip, t: np.vstack([t[a:b].sum(0) for a, b in zip(ip[:-1], ip[1:])])  # noqa: E731  (row sums, fp64)


@functools.lru_cache(None)
def _case(name, K, N):
    ip, ix = GRAPHS[name]
    n, E, rng = len(ip) - 1, len(ix), np.random.default_rng(K * 1000 + N)
    ef, w = rng.standard_normal((E, K), np.float32), (rng.standard_normal((K, N), np.float32) / np.sqrt(K)).astype(np.float32)
    p, q = rng.standard_normal((n, N), np.float32), rng.standard_normal((n, N), np.float32)
    return dict(ip=ip, ix=ix, ef=ef, w=w, p=p, q=q, m=ef.astype(np.float64) @ w, mabs=np.abs(ef).astype(np.float64) @ np.abs(w))


def _bound(ip, mag, t, sf):
    """The module docstring's bound: mag = sum_k |ef||W| + |p| + |q| and t = the fp64 edge values, [E, N]."""
    ulp = np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)
    return _sums(ip, 1e-5 * mag + 1e-6 + SF_ULPS[sf] * ulp) + np.diff(ip)[:, None] * 2.0 ** -23 * _sums(ip, np.abs(t))


@pytest.mark.parametrize("sf", ["NONE", "RELU", "TANH"])
@pytest.mark.parametrize("use_p,use_q", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("name,K,N", [("built", 32, 64), ("built", 100, 128), ("built", 130, 128), ("built", 500, 64),
                                      ("tiny", 100, 128), ("empty", 32, 64)])
def test_kernel_against_fp64(dev, name, K, N, use_p, use_q, sf):
    c = _case(name, K, N)
    ip, ix = c["ip"], c["ix"]
    g = G.from_numpy(ip, ix, n_cols=len(ip) - 1).to(dev)
    ef, w, p, q = (torch.from_numpy(c[k]).to(dev) for k in ("ef", "w", "p", "q"))
    y1, y2 = (ops.aggregate_edge_mm(g, ef, w, p if use_p else None, q if use_q else None, None if sf == "NONE" else sf)
              for _ in range(2))
    assert y1 is not None and torch.equal(y1, y2), "two calls differ"
    z, mag = c["m"].copy(), c["mabs"].copy()
    for use, t, idx in ((use_p, c["p"], ix), (use_q, c["q"], np.repeat(np.arange(len(ip) - 1), np.diff(ip)))):
        if use:
            z, mag = z + t[idx], mag + np.abs(t[idx])
    t = SF64[sf](z)
    err, bound = np.abs(y1.cpu().numpy().astype(np.float64) - _sums(ip, t)), _bound(ip, mag, t, sf)
    print(f"{name} K={K} N={N} p={use_p} q={use_q} {sf}: max err {err.max(initial=0):.3e}, max bound {bound.max(initial=0):.3e}")
    assert (err <= bound).all()
    assert not y1.cpu().numpy()[np.diff(ip) == 0].any(), "a row without edges is 0.0, not sf(0)"


def test_footprint_padded_rows_and_exact_workspace(dev):
    K, N, c = 100, 128, _case("built", 100, 128)
    n, E = len(c["ip"]) - 1, len(c["ix"])
    ar = Arena(dev, 8 << 20)
    g = _graph_in(ar, c["ip"], c["ix"], n, "a")
    ef = ar.table("ef", c["ef"], "b")                       # rows 4-B aligned only
    wt = ar.table("wt", np.ascontiguousarray(c["w"].T), "a")
    p, q = ar.table("p", np.concatenate([c["p"], np.full((1, N), np.nan, np.float32)]), "a"), ar.table("q", c["q"], "a")
    y = ar.out("y", n, N, "a")
    L = _lib.load()
    ws = ar.raw("ws", L.gta_aggregate_edge_mm_workspace_bytes(E, N))
    ar.seal()
    rc = L.gta_aggregate_edge_mm(_p(g.indptr), _p(g.indices), n, E, _p(ef), ef.stride(0), K, _p(wt), wt.stride(0), N,
                                 _lib.GTA_F32, _p(p), p.stride(0), _p(q), q.stride(0), _lib.SF["RELU"], _p(y), y.stride(0),
                                 _p(ws), _st(dev))
    assert rc == _lib.OK, L.gta_last_error()
    ar.check([y, ws], "aggregate_edge_mm")
    assert torch.isfinite(y).all()                          # no poison was read and used


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("layer", [1, 2, 3])
def test_route_through_the_executor(dev, manifest, layer, reorder):
    """Layers 1, 2: one aggregate_edge_mm call, no E-row update_mm / aggregate_expr, every sink within the kernel bound
    B scaled by the following GEMM, (B |s|) |W10|; layer 3 (fout 16) falls back and equals the default bitwise."""
    g = G.synthetic(300, 3000).to(dev)
    rec = next(r for r in manifest["streams"] if "file" in r and (r["network"], r["layer"], r["reorder"]) == ("PNA", layer, reorder))
    lay = pipeline.Layer("PNA", layer, g, 96, reorder=reorder, op_array=rec["op_array"], tile_size_list=rec["tile_size_list"])
    tensors = {k: v.to(dev) for k, v in workloads.make_tensors(lay.opgraph, g, "PNA", seed=layer).items()}
    outs, calls, exs = {}, {}, {}
    for flag in (False, True):
        tr = exec_trace.Recorder(ops, g, tensors)
        with exec_trace.patched(executor, ops=tr):
            exs[flag] = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, edge_mm_gather=flag)
            outs[flag], calls[flag] = {k: v.clone() for k, v in exs[flag].run().items()}, list(tr.calls)
    big = lambda c, *names: c.startswith(names) and f"[{g.nnz}x" in c  # noqa: E731
    assert [sum(c.startswith("aggregate_edge_mm(") for c in calls[f]) for f in (False, True)] == [0, 1]
    if layer == 3:
        assert any(big(c, "update_mm(") for c in calls[True])
        assert all(torch.equal(outs[True][k], outs[False][k]) for k in outs[False])
        return
    assert not any(big(c, "update_mm(", "aggregate_expr(") for c in calls[True])
    f64 = lambda t: t.double().cpu().numpy()  # noqa: E731
    ex = exs[False]
    mag = np.abs(f64(tensors["x_edge"])) @ np.abs(f64(tensors["w:2"])) + np.abs(f64(ex.tensor_of(3))) + np.abs(f64(ex.tensor_of(4)))
    B = _bound(g.indptr.cpu().numpy(), mag, f64(ex.tensor_of(7)), "RELU")
    s = np.abs(f64(tensors["ext:9:1"])) if "ext:9:1" in tensors else 1.0  # (no scaler given: op 9 passes the gather on)
    tol = (B * s) @ np.abs(f64(tensors["w:10"]))
    for k in outs[False]:
        d = np.abs(f64(outs[True][k]) - f64(outs[False][k]))
        print(f"layer {layer} reorder {reorder} sink {k}: max diff {d.max():.3e}, min (tol - diff) {(tol - d).min():.3e}")
        assert (d <= tol).all()
