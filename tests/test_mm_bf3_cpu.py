"""GTA_F32_BF16X3 without a GPU: the dtype value, which entries take it (argument checks run before any
device work: the stand-in pointers are never read), ops.update_mm's keyword, the CLI flag."""
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _build, _lib, cli, ops

P = 4096  # a 16-B aligned stand-in for every pointer
X3 = 4


@pytest.fixture(scope="module")
def lib():
    if _build.needs_build():
        _build.build(verbose=False)
    return _lib.load()


def test_dtype_value_and_which_entries_take_it(lib):
    assert _lib.GTA_F32_BF16X3 == X3 and lib.gta_abi_version() == 15
    assert lib.gta_update_mm_t_splits(2708, 1433, 128, X3, None) == 1
    assert lib.gta_update_mm_t(None, 8, None, 4, 8, None, 8, 8, X3, 0, None, 8, None) == _lib.ERR_ARG
    assert b"bad arguments" in lib.gta_last_error()
    assert lib.gta_update_mm_t(P, 8, None, 0, 8, P, 8, 8, X3, 0, P, 8, None) == _lib.OK  # M == 0
    assert lib.gta_update_mm_t(P, 8, None, 4, 8, P, 9, 8, X3, 0, P, 8, None) == _lib.ERR_UNSUPPORTED  # ldwt % 4
    assert lib.gta_update_mm(P, 8, None, 4, 8, P, 8, 8, X3, 0, P, 8, None) == _lib.ERR_UNSUPPORTED
    assert b"BF16X3" in lib.gta_last_error()
    assert lib.gta_update_mm_t_split(P, 8, None, 4, 8, P, 8, 8, X3, 0, P, 8, 2, P, 1 << 20, None) == _lib.ERR_UNSUPPORTED


def test_update_mm_keyword():
    with pytest.raises(ValueError):
        ops.update_mm(torch.zeros(4, 8), torch.zeros(8, 8), precision="fp16")
    with pytest.raises(TypeError):
        ops.update_mm(torch.zeros(4, 8), torch.zeros(8, 8, dtype=torch.bfloat16), precision="bf16x3")


def test_cli_flag():
    base = ["--dataset", "cora", "--network", "GCN"]
    assert cli.parser().parse_args(base).mm_precision == "f32"
    assert cli.parser().parse_args(base + ["--mm-precision", "bf16x3"]).mm_precision == "bf16x3"
    with pytest.raises(SystemExit):
        cli.parser().parse_args(base + ["--mm-precision", "tf32"])
