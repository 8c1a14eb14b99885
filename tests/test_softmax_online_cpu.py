"""The online-softmax fused GAT aggregate without a GPU: the two exported symbols, the argument
refusals of gta_gat_aggregate_blocked_online through ctypes, and --stable-softmax online down to
executor.run_stream."""
import pytest

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _build, _lib, cli, executor, tiles

from .test_softmax_shift_cpu import _stand_ins

SF = _lib.SF
NEW = ("gta_gat_aggregate_blocked_online", "gta_gat_aggregate_blocked_online_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    if _build.needs_build():
        _build.build(verbose=False)
    return _lib.load()


def _args(sf=SF["EXP_LEAKY_RELU"], lda=8, F=128):
    # pointers are never dereferenced by a refused call: small non-NULL integers stand for them
    return (1, 1, 10, 10, 20, 1, 128, F, _lib.GTA_F32, 1, lda, 1, 8, 8, sf, 1, 0, 1, 128, 1, 1, 1, 64, 1, None)


def test_symbols_are_exported_and_abi_stays_15(lib):
    assert lib.gta_abi_version() == 15 == _lib.ABI_VERSION
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    # slab rows of F + 2 H floats, 16-B aligned: never smaller than the two-table form's F + H
    two = lib.gta_gat_aggregate_blocked_workspace_bytes(300, 6000, 5, 128, 8, 64)
    assert lib.gta_gat_aggregate_blocked_online_workspace_bytes(300, 6000, 5, 128, 8, 64) * (128 + 8) == two * (128 + 16)
    assert lib.gta_gat_aggregate_blocked_online_workspace_bytes(300, 6000, 0, 128, 8, 64) == _lib.ERR_ARG


@pytest.mark.parametrize("kw,code", [(dict(lda=7), _lib.ERR_ARG), (dict(sf=SF["SIGMOID"]), _lib.ERR_UNSUPPORTED),
                                     (dict(sf=SF["RELU"]), _lib.ERR_UNSUPPORTED), (dict(F=96), _lib.ERR_UNSUPPORTED)])
def test_argument_checks_need_no_device(lib, kw, code):
    assert lib.gta_gat_aggregate_blocked_online(*_args(**kw)) == code
    assert b"gat_aggregate_blocked_online" in lib.gta_last_error()


def test_stable_softmax_online_reaches_run_stream(monkeypatch):
    base = ["--dataset", "cora", "--network", "GAT", "--layers", "1", "--reps", "1", "--heads", "8"]
    assert cli.parser().parse_args(base).stable_softmax is False
    assert cli.parser().parse_args(base + ["--stable-softmax"]).stable_softmax is True
    a = cli.parser().parse_args(base + ["--stable-softmax", "online"])
    assert a.stable_softmax == "online"
    for mod in (executor, tiles):
        monkeypatch.setattr(mod, "ops", _stand_ins([]))
    calls = []
    real_run = executor.run_stream
    monkeypatch.setattr(executor, "run_stream",
                        lambda *a_, **k: calls.append(k.get("softmax_shift")) or real_run(*a_, **k))
    cli.run(a, "cpu", log=lambda *_: None)
    assert calls and all(c == "online" for c in calls)
