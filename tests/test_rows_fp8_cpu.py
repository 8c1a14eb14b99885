"""e4m3 rows in the row-chunked aggregate (gta_aggregate / gta_aggregate_self with GTA_FP8), without a
GPU: the argument checks run before any device work, the line-pitched cast, and the option's way
from the CLI to the executor."""
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, cli, executor, ops

from .test_blocked_bf16_cpu import P, _golden_layer, lib  # noqa: F401

FP8 = torch.float8_e4m3fn
SRC, DST, EDGE = _lib.IDX_SRC, _lib.IDX_DST, _lib.IDX_EDGE


def _agg(lib, n_rows=10, x_mode=SRC, x=P, ldx=128, F=100, x_dtype=_lib.GTA_FP8, w=None, ldw=0, heads=0, y=P, ldy=100):
    return lib.gta_aggregate(P, P, n_rows, 20, x_mode, x, ldx, F, x_dtype, w, ldw, heads, None, y, ldy, 0, None, 0, None,
                             None)


def _self(lib, x_self=P, ld_self=104, y=P, ldy=104, y_dtype=_lib.GTA_BF16):
    return lib.gta_aggregate_self(P, P, 10, 20, SRC, P, 128, 100, _lib.GTA_FP8, None, 0, 0, None, x_self, ld_self, P, y,
                                  ldy, y_dtype, None, 0, None, None)


REFUSED = [dict(x_mode=EDGE), dict(w=P, ldw=100, heads=100), dict(w=P, ldw=4, heads=4, F=96, ldx=96, ldy=96),
           dict(F=257, ldx=272, ldy=260), dict(x=P + 8), dict(ldx=120), dict(ldx=96), dict(y=P + 8), dict(ldy=102)]


def test_entry_points_take_fp8_and_refuse_on_the_host(lib):
    assert lib.gta_abi_version() == 15
    assert _agg(lib, n_rows=0) == _lib.OK
    for kw in REFUSED:
        assert _agg(lib, **kw) == _lib.ERR_UNSUPPORTED, kw
        assert lib.gta_last_error().startswith(b"aggregate"), kw
    for kw in (dict(x_self=P + 8), dict(ld_self=100), dict(ldy=100), dict(y=P + 8), dict(y_dtype=_lib.GTA_F32, ldy=102)):
        assert _self(lib, **kw) == _lib.ERR_UNSUPPORTED, kw
    for dt in (7, 2, -1):
        assert _agg(lib, x_dtype=dt) == _lib.ERR_ARG
        assert lib.gta_last_error() == b"aggregate: x_dtype must be F32 or BF16"
    rc = lib.gta_reduce(_lib.RED_ADD, P, P, 10, 20, SRC, P, 128, 100, _lib.GTA_FP8, P, 100, None, 0, None, None)
    assert rc == _lib.ERR_ARG and lib.gta_last_error() == b"reduce (ADD): aggregate: x_dtype must be F32 or BF16"


def test_to_fp8_line_pitch():
    t = torch.randn(9, 100)
    a, b = ops.to_fp8(t, lines=True), ops.to_fp8(t)
    assert a.stride(0) == 128 and b.stride(0) == 112 and a.dtype == FP8
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and a.data_ptr() % 16 == 0
    assert ops.to_fp8(torch.randn(9, 20), lines=True).stride(0) == 32   # a line would be > 1.5x the row
    assert ops.to_fp8(t.bfloat16(), lines=True).stride(0) == 128


def test_option_from_cli_to_executor():
    base = ["--dataset", "cora", "--network", "GIN", "--gather-dtype", "fp8"]
    assert cli.parser().parse_args(base).fp8_rows is False
    assert cli.parser().parse_args(base + ["--fp8-rows"]).fp8_rows is True
    lay, g = _golden_layer(gather_dtype=FP8, fp8_rows=True)
    assert lay.fp8_rows and not _golden_layer(gather_dtype=FP8)[0].fp8_rows
    mk = lambda **kw: executor.Executor(lay.opgraph, lay.stream, g, {}, lay.sem, **kw)  # noqa: E731
    assert mk().fp8_rows is False and mk(gather_dtype=FP8, fp8_rows=True).fp8_rows is True
    ex = mk(gather_dtype=FP8, fp8_rows=True)
    t = torch.randn(6, 100).bfloat16()
    assert ex._gather_cast(t) is t                       # the blocked route leaves a bf16 table alone
    c = ex._gather_cast(t, rows=True)
    assert c.dtype == FP8 and c.stride(0) == 128 and ex._gather_cast(t, rows=True) is c and ex.gather_casts == 1
    w1, w4 = torch.rand(8, 1), torch.rand(8, 4)
    assert ex._fp8_rows_take(t, "src", None) and ex._fp8_rows_take(t, "src", w1) and not ex._fp8_rows_take(t, "src", w4)
    assert not ex._fp8_rows_take(t, "dst", None) and not ex._fp8_rows_take(torch.randn(6, 260), "src", None)
    assert not mk(gather_dtype=FP8)._fp8_rows_take(t, "src", None)
    assert not mk(gather_dtype=torch.bfloat16, fp8_rows=True)._fp8_rows_take(t, "src", None)
