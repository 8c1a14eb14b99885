"""gta_aggregate_edge_mm without a GPU: host-side refusals, workspace size, the matcher, routing over fake_ops, plumbing."""
import os

import numpy as np
import pytest

from gta_graph_tensor_acclelrator_for_general_gnn_amd import _lib, cli, executor, ir, rewrites, workloads
from gta_graph_tensor_acclelrator_for_general_gnn_amd.semantics import Semantics

from . import exec_trace, fake_ops
from .conftest import GOLDEN, load_manifest
from .test_blocked_bf16_cpu import P, _golden_layer, lib  # noqa: F401


def _emm(lib, n_rows=10, ef=P, K=100, ldwt=100, N=128, dtype=_lib.GTA_F32, y=P, ldy=128):
    return lib.gta_aggregate_edge_mm(P, P, n_rows, 20, ef, 100, K, P, ldwt, N, dtype, P, 128, P, 128, 1, y, ldy, P, None)


def test_refusals_before_any_device_work(lib):
    """Every call is refused on the host: the bogus pointers are never read."""
    for kw in (dict(N=16, ldy=16), dict(N=96), dict(K=16), dict(ldwt=102), dict(dtype=_lib.GTA_BF16), dict(dtype=_lib.GTA_F32_BF16X3)):
        assert _emm(lib, **kw) == _lib.ERR_UNSUPPORTED, kw
    for kw in (dict(y=None), dict(ef=None)):
        assert _emm(lib, **kw) == _lib.ERR_ARG, kw
    assert _emm(lib, n_rows=0) == _lib.OK
    size = lib.gta_aggregate_edge_mm_workspace_bytes
    assert all(size(nnz, N) == -(-nnz // 32) * 2 * N * 4 for nnz in (0, 1, 32, 33, 899756) for N in (64, 128))
    assert size(-1, 64) < 0 and size(5, 0) < 0


def _golden(network, reorder):
    rec = next(s for s in load_manifest()["streams"]
               if "file" in s and s["dataset"] == "cora" and s["network"] == network and s["reorder"] == reorder)
    sem = Semantics.for_network(network, reorder)
    og = ir.OpGraph.load(os.path.join(GOLDEN, "ops", rec["op_yaml"]), sem.inputs)
    return og, ir.Stream.load(os.path.join(GOLDEN, "streams", rec["file"])), sem


@pytest.mark.parametrize("network,reorder,want", [("PNA", False, {8: (2, 2)}), ("PNA", True, {8: (2, 2)}),
                                                   ("DGN", False, {}), ("DGN", True, {}), ("GAT", False, {})])
def test_matcher_on_the_golden_op_graphs(network, reorder, want):
    og, st, sem = _golden(network, reorder)
    ex = executor.Executor(og, st, exec_trace._cora(), {}, sem)
    assert ex.emm == {} and ex.edge_mm_gather is False       # off by default: nothing is matched
    assert rewrites.edge_mm_gather(og, ex.consumers, ex.expr) == want


def _stand_in(graph, ef, w, p=None, q=None, sf=None, out=None):
    ip, ix = graph.numpy()
    z = fake_ops._np(ef) @ fake_ops._np(w)
    z = z + (fake_ops._np(p)[ix] if p is not None else 0) + (np.repeat(fake_ops._np(q)[:graph.n_rows], np.diff(ip), 0) if q is not None else 0)
    return fake_ops.gather_add(graph, fake_ops.apply_edge(graph, None, sf, fake_ops._t(z)))


@pytest.mark.parametrize("reorder", [False, True])
def test_routing_with_fake_ops(reorder):
    """(aggregate_edge_mm calls, aggregate_expr calls): the flag routes once, a None return falls back, off is today's route."""
    og, st, sem = _golden("PNA", reorder)
    g = exec_trace._cora()
    tensors, seen = workloads.make_tensors(og, g, "PNA", seed=1), {}
    for key, flag, emm in (("off", False, _stand_in), ("on", True, _stand_in), ("refused", True, lambda *a, **k: None)):
        before = fake_ops.EXPR_CALLS[0]
        with exec_trace.patched(fake_ops, aggregate_edge_mm=emm):
            calls = exec_trace.record(og, st, g, tensors, sem, edge_mm_gather=flag)["calls"]
        seen[key] = (sum(c.startswith("aggregate_edge_mm(") for c in calls), fake_ops.EXPR_CALLS[0] - before)
    assert seen == {"off": (0, 1), "on": (1, 0), "refused": (1, 1)}


def test_option_from_cli_to_layer():
    parse = lambda *a: cli.parser().parse_args(["--dataset", "cora", "--network", "PNA", *a]).edge_mm_gather  # noqa: E731
    assert parse() is False and parse("--edge-mm-gather") is True
    assert _golden_layer()[0].edge_mm_gather is False and _golden_layer(edge_mm_gather=True)[0].edge_mm_gather is True
