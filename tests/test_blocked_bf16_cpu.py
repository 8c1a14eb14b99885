"""bf16 gathered tables in the blocked aggregates: what can be checked without a GPU -- the shape
rules, the two _x entry points' argument validation (it runs before any device work), and the option's
way from the CLI down to the layer, which leaves the op graph and the lowered stream alone."""
import json
import os

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _build, _lib, cli, executor, frontend, graph as G, ops, pipeline

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    if _build.needs_build():
        _build.build(verbose=False)
    return _lib.load()


def test_blocked_plan_supports_bf16():
    BP = ops.BlockedPlan
    assert torch.bfloat16 in BP.DTYPES and torch.float32 in BP.DTYPES
    for F, heads in [(128, 8), (128, 0), (128, 1), (128, 4), (64, 0), (64, 4), (256, 16)]:
        assert BP.supports(F, heads, torch.bfloat16), (F, heads)
        assert BP.supports(F, heads, torch.float32), (F, heads)
    assert not BP.supports(100, 0, torch.bfloat16)       # gin-products' width is not a blocked width
    assert not BP.supports(128, 8, torch.float16)
    assert BP.auto_blocks.__defaults__ == (4,)           # callers pass elem=2 for a bf16 table


P = 4096  # a 16-B aligned stand-in for every pointer: refused calls never dereference one


def _plain(lib, x=P, x_dtype=_lib.GTA_BF16, n_rows=10, nnz=5, F=128, blocks=4, item_edges=256):
    return lib.gta_aggregate_blocked_x(P, P, n_rows, 10, nnz, x, 128, F, x_dtype, None, 0, 0, None, P, 128, 0, P, blocks,
                                       item_edges, P, None)


def _att(lib, x=P, x_dtype=_lib.GTA_BF16, n_rows=10, nnz=5, F=128, blocks=4, item_edges=256, heads=8, shift=None):
    return lib.gta_gat_aggregate_blocked_x(P, P, n_rows, 10, nnz, x, 128, F, x_dtype, P, heads, P, heads, heads,
                                           _lib.SF["EXP_LEAKY_RELU"], 1, 0, P, 128, None, P, blocks, item_edges, P, shift,
                                           None)


def test_x_entry_points_validate_before_any_device_work(lib):
    """Every call here is refused on the host: the (bogus, never dereferenced) pointers are not read."""
    assert lib.gta_abi_version() == 15 == _lib.ABI_VERSION
    for call, name in ((_plain, b"aggregate_blocked_x"), (_att, b"gat_aggregate_blocked_x")):
        for kw in ({"x_dtype": 7}, {"x_dtype": -1}, {"x_dtype": _lib.GTA_F32_BF16}):
            assert call(lib, **kw) == _lib.ERR_ARG, (name, kw)
            assert name in lib.gta_last_error() and b"x_dtype" in lib.gta_last_error()
        for kw in ({"x": None}, {"n_rows": -1}, {"nnz": -1}, {"blocks": 0}, {"blocks": 64}, {"item_edges": 0}):
            assert call(lib, **kw) == _lib.ERR_ARG, (name, kw)
            assert name in lib.gta_last_error()
        assert call(lib, F=96) < 0 and name in lib.gta_last_error()      # not a blocked width
        assert call(lib, x=P + 8) == _lib.ERR_UNSUPPORTED                # bf16 rows not 16-B aligned
        assert name in lib.gta_last_error() and b"16-B" in lib.gta_last_error()
    assert _plain(lib, F=0) == _lib.ERR_ARG
    assert _att(lib, heads=0) == _lib.ERR_ARG
    assert _att(lib, heads=3) == _lib.ERR_UNSUPPORTED                    # heads must divide F
    # the shifted form's restriction on sf holds for either dtype
    for dt in (_lib.GTA_F32, _lib.GTA_BF16):
        rc = lib.gta_gat_aggregate_blocked_x(P, P, 10, 10, 5, P, 128, 128, dt, P, 8, P, 8, 8, _lib.SF["SIGMOID"], 1, 0, P,
                                             128, None, P, 4, 256, P, P, None)
        assert rc == _lib.ERR_UNSUPPORTED and b"gat_aggregate_blocked_x" in lib.gta_last_error()
    # the old entry points keep their names in their messages
    assert lib.gta_aggregate_blocked(P, P, -1, 10, 5, P, 128, 128, None, 0, 0, None, P, 128, 0, P, 4, 256, P, None) < 0
    assert lib.gta_last_error().startswith(b"aggregate_blocked:")


def test_cli_parses_gather_dtype():
    base = ["--dataset", "cora", "--network", "GAT"]
    assert cli.parser().parse_args(base).gather_dtype == "f32"
    assert cli.parser().parse_args(base + ["--gather-dtype", "bf16"]).gather_dtype == "bf16"
    assert cli.parser().parse_args(base + ["--gather-dtype", "f32"]).gather_dtype == "f32"
    with pytest.raises(SystemExit):
        cli.parser().parse_args(base + ["--gather-dtype", "fp16"])


def _golden_layer(**kw):
    m = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    rec = [s for s in m["streams"] if s.get("file") == "GAT-cora-layer1-original-c0.yaml"][0]
    z = np.load(os.path.join(GOLDEN, "cora_graph.npz"))
    g = G.from_numpy(z["indptr"], z["indices"])
    return pipeline.Layer("GAT", 1, g, 1433, op_array=rec["op_array"], tile_size_list=rec["tile_size_list"], **kw), g


def test_layer_stores_the_option_and_lowers_the_same_stream():
    plain, g = _golden_layer()
    assert plain.gather_dtype is None
    assert _golden_layer(gather_dtype=torch.float32)[0].gather_dtype is None
    bf, _ = _golden_layer(gather_dtype=torch.bfloat16)
    assert bf.gather_dtype == torch.bfloat16
    with pytest.raises(ValueError):
        _golden_layer(gather_dtype=torch.float16)
    # an execution option only: the op graph and the lowered instruction stream are byte-identical
    assert bf.records == plain.records and repr(bf.records).encode() == repr(plain.records).encode()
    assert bf.stream_records == plain.stream_records
    assert repr(bf.stream_records).encode() == repr(plain.stream_records).encode()
    assert bf.records == frontend.gen_ops("GAT", 1, g.n_rows, g.nnz, 1433, False, 16, "ADD")


def test_layer_run_passes_the_option_only_when_set(monkeypatch):
    seen = []

    def fake(opgraph, stream, graph, tensors, semantics=None, plan_chunk=512, **kw):
        seen.append(kw)
        return None, None
    monkeypatch.setattr(pipeline.executor, "run_stream", fake)
    plain, _ = _golden_layer()
    plain.run({})
    bf, _ = _golden_layer(gather_dtype=torch.bfloat16, stable_softmax=True)
    bf.run({})
    assert seen == [{"sync": True}, {"sync": True, "softmax_shift": True, "gather_dtype": torch.bfloat16}]


def test_executor_option_defaults_off():
    plain, g = _golden_layer()
    ex = executor.Executor(plain.opgraph, plain.stream, g, {}, plain.sem)
    assert ex.gather_dtype is None and ex.gather_casts == 0
    ex = executor.Executor(plain.opgraph, plain.stream, g, {}, plain.sem, gather_dtype=torch.bfloat16)
    assert ex.gather_dtype == torch.bfloat16
    t = torch.randn(4, 128)
    assert executor.Executor(plain.opgraph, plain.stream, g, {}, plain.sem)._gather_cast(t) is t   # off: the table itself
    with pytest.raises(ValueError):
        executor.Executor(plain.opgraph, plain.stream, g, {}, plain.sem, gather_dtype=torch.float16)
