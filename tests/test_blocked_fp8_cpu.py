"""e4m3 gathered tables in the blocked aggregates, without a GPU: ops.to_fp8, the two _x entry points'
argument checks (they run before any device work), the option from the CLI to the executor."""
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, cli, executor, ops

from .test_blocked_bf16_cpu import P, _att, _golden_layer, _plain, lib  # noqa: F401

FP8 = torch.float8_e4m3fn
NAN = float("nan")
# value -> the e4m3 code to_fp8 must store: clamp (torch's own cast gives NaN past 464), NaN, -0, the
# denormals m * 2^-9, ties to even at both ends of the range
SWEEP = [(500.0, 0x7E), (-1e9, 0xFE), (464.0, 0x7E), (448.0, 0x7E), (NAN, 0x7F), (-0.0, 0x80), (0.0, 0x00),
         (2.0 ** -9, 0x01), (-7 * 2.0 ** -9, 0x87), (2.0 ** -6, 0x08), (2.0 ** -10, 0x00), (3 * 2.0 ** -10, 0x02),
         (2.0 ** -10 * 1.01, 0x01), (2.0 ** -11, 0x00), (1.0625, 0x38), (1.1875, 0x3A), (-1.0, 0xB8), (432.0, 0x7E),
         (416.0, 0x7D), (424.0, 0x7D)]


def test_to_fp8_value_sweep_and_layout():
    vals = torch.tensor([[v for v, _ in SWEEP]])
    r = ops.to_fp8(vals)
    assert r.dtype == FP8 and r.shape == vals.shape
    assert r.view(torch.uint8).tolist() == [[c for _, c in SWEEP]]
    assert r.stride(0) % 16 == 0 and r.data_ptr() % 16 == 0      # 20 columns on a 32-byte pitch
    t = ops.to_fp8(torch.randn(9, 128))
    assert t.stride() == (128, 1) and torch.equal(ops.to_fp8(t.float()).view(torch.uint8), t.view(torch.uint8))
    BP = ops.BlockedPlan
    assert FP8 not in BP.DTYPES and not BP.supports(128, 8, FP8)  # the reducers consult these
    assert all(BP.supports_fp8(F, h) for F, h in [(128, 0), (128, 8), (128, 1), (128, 4), (64, 0), (64, 4), (256, 16)])
    assert not BP.supports_fp8(128, 32) and not BP.supports_fp8(96, 0)


def test_x_entry_points_take_fp8_past_the_dtype_check(lib):
    """Every call is refused, or returns for n_rows = 0, on the host: the bogus pointers are never read."""
    assert _lib.GTA_FP8 == 3 and lib.gta_abi_version() == 15
    for call, name in ((_plain, b"aggregate_blocked_x"), (_att, b"gat_aggregate_blocked_x")):
        assert call(lib, x_dtype=_lib.GTA_FP8, n_rows=0) == _lib.OK
        assert call(lib, x_dtype=7, n_rows=0) == _lib.ERR_ARG and b"x_dtype" in lib.gta_last_error()
        for kw in ({"x": P + 8}, {"x": P + 4}):                   # a base off 16 B
            assert call(lib, x_dtype=_lib.GTA_FP8, **kw) == _lib.ERR_UNSUPPORTED
            assert name in lib.gta_last_error() and b"x_dtype" not in lib.gta_last_error()
    # ldx % 16 != 0 (bytes), and 32 heads of 4 columns where a lane holds 8
    assert lib.gta_aggregate_blocked_x(P, P, 10, 10, 5, P, 136, 128, _lib.GTA_FP8, None, 0, 0, None, P, 128, 0, P, 4, 256,
                                       P, None) == _lib.ERR_UNSUPPORTED and b"fp8" in lib.gta_last_error()
    assert lib.gta_aggregate_blocked_x(P, P, 10, 10, 5, P, 128, 128, _lib.GTA_FP8, P, 32, 32, None, P, 128, 0, P, 4, 256,
                                       P, None) == _lib.ERR_UNSUPPORTED and b"fp8" in lib.gta_last_error()
    assert lib.gta_gat_aggregate_blocked_x(P, P, 10, 10, 5, P, 136, 128, _lib.GTA_FP8, P, 8, P, 8, 8, _lib.SF["EXP"], 1, 0, P,
                                           128, None, P, 4, 256, P, None, None) == _lib.ERR_UNSUPPORTED
    # every other entry point keeps refusing 3
    assert lib.gta_reduce_blocked(_lib.RED_MAX, P, P, 10, 10, 5, P, 128, 128, _lib.GTA_FP8, P, 128, P, 4, 256, P,
                                  None) == _lib.ERR_ARG and b"x_dtype must be F32 or BF16" in lib.gta_last_error()


def test_option_from_the_cli_to_the_executor():
    base = ["--dataset", "cora", "--network", "GAT"]
    assert cli.parser().parse_args(base + ["--gather-dtype", "fp8"]).gather_dtype == "fp8"
    assert cli.GATHER_DTYPES["fp8"] == FP8 and cli.GATHER_DTYPES["f32"] is None
    lay, g = _golden_layer(gather_dtype=FP8)
    assert lay.gather_dtype == FP8
    with pytest.raises(ValueError):
        _golden_layer(gather_dtype=torch.float16)
    ex = executor.Executor(lay.opgraph, lay.stream, g, {}, lay.sem, gather_dtype=FP8)
    t = torch.randn(4, 128)
    c = ex._gather_cast(t)
    assert c.dtype == FP8 and ex._gather_cast(t) is c and ex.gather_casts == 1   # one cast per table value
    assert ex._gather_cast(t, reduce=True) is t                                   # the reducers keep the uncast table
    with pytest.raises(ValueError):
        executor.Executor(lay.opgraph, lay.stream, g, {}, lay.sem, gather_dtype=torch.float16)
