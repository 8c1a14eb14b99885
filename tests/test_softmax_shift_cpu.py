"""The shifted (overflow-safe) softmax without a GPU: the exported symbols and their argument checks
through ctypes, the --stable-softmax flag down to pipeline.Layer, the executor's routing with op
stand-ins (tests/fake_ops.py wrapped here with `shift`-aware forms), the column-shard refusal, and
the numerics the GPU tests rely on: an fp32 emulation of the shifted algorithm stays inside the
project's bounds on every input the GPU tests use."""
import types

import numpy as np
import pytest
import torch

from gta_graph_tensor_acclelrator_for_general_gnn_amd import (_build, _lib, cli, executor, frontend, graph as G, pipeline,
                                                              tiles, workloads)

from . import fake_ops, softmax_shift_ref as R

NEW = ("gta_softmax_shift", "gta_edge_softmax_shifted", "gta_gat_aggregate_blocked_shifted")
SF = _lib.SF


# ------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    if _build.needs_build():
        _build.build(verbose=False)
    return _lib.load()


def test_the_three_symbols_are_exported_and_abi_stays_15(lib):
    assert lib.gta_abi_version() == 15 == _lib.ABI_VERSION
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None


def _shift_args(sf=SF["EXP_LEAKY_RELU"], lda=8, ldb=8, shift=1):
    # pointers are never dereferenced by a refused call: small non-NULL integers stand for them
    return (1, 1, 10, 20, 1, lda, 1, ldb, 8, sf, shift or None, None)


def _esm_args(sf=SF["EXP_LEAKY_RELU"], lda=8, ldb=8, shift=1):
    return (1, 1, 10, 20, 1, lda, 1, ldb, 8, sf, 1, 1, 1, shift or None, None)


def _gat_args(sf=SF["EXP_LEAKY_RELU"], lda=8, ldb=8, shift=1):
    return (1, 1, 10, 10, 20, 1, 128, 128, 1, lda, 1, ldb, 8, sf, 1, 0, 1, 128, 1, 1, 1, 64, 1, shift or None, None)


@pytest.mark.parametrize("name,args,tag", [("gta_softmax_shift", _shift_args, b"softmax_shift"),
                                           ("gta_edge_softmax_shifted", _esm_args, b"edge_softmax_shifted"),
                                           ("gta_gat_aggregate_blocked_shifted", _gat_args,
                                            b"gat_aggregate_blocked_shifted")])
def test_argument_checks_need_no_device(lib, name, args, tag):
    fn = getattr(lib, name)
    assert fn(*args(shift=0)) == _lib.ERR_ARG and tag in lib.gta_last_error()  # NULL shift
    for sf in ("SIGMOID", "RELU", "NONE", "TANH"):
        assert fn(*args(sf=SF[sf])) == _lib.ERR_UNSUPPORTED and tag in lib.gta_last_error()
    assert fn(*args(lda=7)) == _lib.ERR_ARG and tag in lib.gta_last_error()
    assert fn(*args(ldb=7)) == _lib.ERR_ARG and tag in lib.gta_last_error()


def test_unshifted_twins_keep_their_messages(lib):
    assert lib.gta_edge_softmax(1, 1, 10, 20, 1, 7, 1, 8, 8, SF["EXP_LEAKY_RELU"], 1, 1, 1, None) == _lib.ERR_ARG
    assert lib.gta_last_error() == b"edge_softmax: leading dimension < heads"
    assert lib.gta_gat_aggregate_blocked(*_gat_args(lda=7)[:-2], None) == _lib.ERR_ARG
    assert lib.gta_last_error() == b"gat_aggregate_blocked: bad sizes"


def test_ops_refuse_cpu_tensors():
    from gta_graph_tensor_acclelrator_for_general_gnn_amd import ops
    g = G.synthetic(20, 60, seed=0)
    with pytest.raises(_lib.GTAError):
        ops.softmax_shift(g, torch.zeros(20, 4), torch.zeros(20, 4))
    with pytest.raises(_lib.GTAError):
        ops.edge_softmax(g, torch.zeros(20, 4), torch.zeros(20, 4), shift=torch.zeros(20, 4))


# ------------------------------------------------------------------------------- CLI and pipeline
def test_stable_softmax_flag_reaches_the_layer(monkeypatch):
    a = cli.parser().parse_args(["--dataset", "cora", "--network", "GAT"])
    assert a.stable_softmax is False
    a = cli.parser().parse_args(["--dataset", "cora", "--network", "GAT", "--stable-softmax", "--layers", "1",
                                 "--reps", "1", "--heads", "8"])
    assert a.stable_softmax is True
    for mod in (executor, tiles):
        monkeypatch.setattr(mod, "ops", _stand_ins([]))
    seen = []
    real = pipeline.Layer

    class Spy(real):
        def __init__(self, *args, **kw):
            seen.append(kw.get("stable_softmax"))
            super().__init__(*args, **kw)
    monkeypatch.setattr(pipeline, "Layer", Spy)
    calls = []
    real_run = executor.run_stream
    monkeypatch.setattr(executor, "run_stream",
                        lambda *a_, **k: calls.append(k.get("softmax_shift")) or real_run(*a_, **k))
    cli.run(a, "cpu", log=lambda *_: None)
    assert seen and all(seen) and calls and all(c is True for c in calls)
    assert real("GAT", 1, G.synthetic(50, 200), 64, heads=8).stable_softmax is False


# ------------------------------------------------------------------------------ executor routing
def _stand_ins(log):
    """fake_ops with the three ops of the feature: softmax_shift, and edge_softmax /
    gat_aggregate_blocked taking `shift` (fp64 from the fp32 scores, tests/softmax_shift_ref.py).
    Without `shift` they are fake_ops' own functions, whose signatures have no such argument."""
    def f32(t):
        return t.detach().cpu().float().numpy()

    def softmax_shift(graph, a_dst, b_src, sf="EXP_LEAKY_RELU", out=None):
        ip, ix = graph.numpy()
        t = torch.from_numpy(R.shift(ip, ix, f32(a_dst), f32(b_src), sf))
        log.append(("softmax_shift", t))
        return t

    def edge_softmax(graph, a_dst, b_src, sf="EXP_LEAKY_RELU", normalize=True, out=None, sums=None, want_sums=False,
                     **kw):
        if "shift" not in kw:
            log.append(("edge_softmax", None))
            return fake_ops.edge_softmax(graph, a_dst, b_src, sf, normalize, out, sums, want_sums)
        log.append(("edge_softmax", kw["shift"]))
        ip, ix = graph.numpy()
        ref = R.reference(ip, ix, f32(a_dst), f32(b_src), sf)
        return fake_ops._t(ref["alpha"] if normalize else ref["v"]), fake_ops._t(ref["sums"])

    def gat_aggregate_blocked(graph, x, a_dst, b_src, sf="EXP_LEAKY_RELU", normalize=True, out=None, sums=None,
                              want_sums=False, plan=None, blocks=16, sf_out=None, **kw):
        if "shift" not in kw:
            log.append(("gat_aggregate_blocked", None))
            return fake_ops.gat_aggregate_blocked(graph, x, a_dst, b_src, sf, normalize, out, sums, want_sums, plan,
                                                  blocks, sf_out)
        log.append(("gat_aggregate_blocked", kw["shift"]))
        ip, ix = graph.numpy()
        ref = R.reference(ip, ix, f32(a_dst), f32(b_src), sf, x=f32(x))
        y = ref["y"] if normalize else ref["num"]
        if sf_out is not None:
            from oracle import isa_ref
            y = isa_ref.sf(sf_out, y)
        return fake_ops._t(y), (fake_ops._t(ref["sums"]) if (want_sums or sums is not None) else None)

    ns = types.SimpleNamespace(**{k: v for k, v in vars(fake_ops).items() if not k.startswith("__")})
    ns.softmax_shift, ns.edge_softmax, ns.gat_aggregate_blocked = softmax_shift, edge_softmax, gat_aggregate_blocked
    return ns


def _gat_layer(reorder):
    ip, ix, nc = R.blocked_graph()
    g = G.from_numpy(ip, ix, n_cols=nc)
    lay = gat_layer(g, reorder)
    return g, lay, workloads.make_tensors(lay.opgraph, g, "GAT", seed=5)


def gat_layer(g, reorder, **kw):
    """GAT layer 1 (F = 128, 8 heads) on g.  None of the search's first candidates for the reordered
    form lowers on a graph this small (the reference's interpret() raises on them, lowering.py):
    it runs with every op in a block of its own."""
    if not reorder:
        return pipeline.Layer("GAT", 1, g, 128, heads=8, **kw)
    n = len(frontend.gen_ops("GAT", 1, g.n_rows, g.nnz, 128, True, 8))
    return pipeline.Layer("GAT", 1, g, 128, reorder=True, heads=8, op_array=[[i] for i in range(n)],
                          tile_size_list=[[64, 1]] * n, **kw)


@pytest.mark.parametrize("reorder", [False, True])
def test_executor_builds_one_table_and_hands_it_to_both_consumers(monkeypatch, reorder):
    log = []
    for mod in (executor, tiles):
        monkeypatch.setattr(mod, "ops", _stand_ins(log))
    g, lay, tensors = _gat_layer(reorder)
    assert executor.SOFTMAX_SHIFT is False

    def run(shift):
        del log[:]
        ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, softmax_shift=shift)
        assert ex.softmax_shift is bool(shift)
        ex.attention_blocks = 2  # the fused attention launch on this small graph
        outs = ex.run()
        pat, = ex.softmax.values()
        alpha_or_v = ex.tensor_of(pat["D"] if pat["D"] is not None else pat["V"])  # forces the edge_softmax launch
        return ex, outs, alpha_or_v

    ex0, out0, w0 = run(None)  # off: today's calls, no shift pass, no `shift` argument
    assert [n for n, _ in log] == ["gat_aggregate_blocked", "edge_softmax"] and all(s is None for _, s in log)
    ex1, out1, w1 = run(True)
    names = [n for n, _ in log]
    assert names.count("softmax_shift") == 1 and names[0] == "softmax_shift"
    table = log[0][1]
    assert [n for n in names[1:]] == ["gat_aggregate_blocked", "edge_softmax"]
    assert all(s is table for _, s in log[1:])  # the same tensor, not an equal one
    assert ex1.launches == ex0.launches + 1 and ex1.alg_bytes > ex0.alg_bytes
    # N(0, 1) scores: nothing overflows, the layer's output is the same function
    for k in out0:
        np.testing.assert_allclose(out1[k].numpy(), out0[k].numpy(), rtol=2e-5, atol=2e-6)
    if not reorder:  # alpha is unchanged by the shift; GAT-trans' v carries the row factor
        np.testing.assert_allclose(w1.numpy(), w0.numpy(), rtol=2e-5, atol=1e-7)


def test_other_score_functions_run_as_today(monkeypatch):
    log = []
    for mod in (executor, tiles):
        monkeypatch.setattr(mod, "ops", _stand_ins(log))
    g, lay, tensors = _gat_layer(False)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, softmax_shift=True)
    pat, = ex.softmax.values()
    monkeypatch.setattr(ex.sem, "sf_of", lambda op, _real=ex.sem.sf_of: "SIGMOID" if op.idx == pat["V"] else _real(op))
    ex.attention_blocks = 2
    ex.run()
    assert log and "softmax_shift" not in [n for n, _ in log] and all(s is None for _, s in log)


def test_column_shards_refuse_the_shift(monkeypatch):
    """A column shard holds part of each row's edges: the row maximum spans ranks."""
    for mod in (executor, tiles):
        monkeypatch.setattr(mod, "ops", _stand_ins([]))
    g, lay, tensors = _gat_layer(False)
    dist = types.SimpleNamespace(local_rows=False, n_local=g.n_rows, s=types.SimpleNamespace(world=2),
                                 src_fill=lambda t: t, gather_rows=lambda x: x, reduce_rows=lambda y: y,
                                 reduce_cols=lambda y: y, replicated=lambda key: None)
    ex = executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0, dist=dist, softmax_shift=True)
    score, = ex.softmax
    with pytest.raises(NotImplementedError, match=rf"op {score}: softmax_shift on column shards"):
        ex.run()
    dist.local_rows = True  # whole rows on the rank: runs
    executor.Executor(lay.opgraph, lay.stream, g, tensors, lay.sem, plan_chunk=0, dist=dist, softmax_shift=True).run()


# ------------------------------------------------------------------------------------- numerics
def _inside(em, ref, sc, keys, what):
    for k in keys:
        ok, excess = R.within(em[k], ref[k], sc[k])
        assert ok, f"{what} {k}: the fp32 emulation leaves the bound by {excess:.3e}"
        assert np.isfinite(em[k]).all()


@pytest.mark.parametrize("sf", ["EXP_LEAKY_RELU", "EXP"])
@pytest.mark.parametrize("H", [1, 8, 16, 64])
def test_reference_properties_and_fp32_emulation_on_the_softmax_inputs(H, sf):
    ip, ix, nc = R.softmax_graph()
    a, b = R.case(len(ip) - 1, nc, H, 100 + H)
    # g(a + max b) is the maximum of the scores, bit for bit (monotone fp32 add and g)
    assert np.array_equal(R.shift(ip, ix, a, b, sf), R.shift_from_scores(ip, ix, a, b, sf))
    ref = R.reference(ip, ix, a, b, sf)
    ne = ref["deg"] > 0
    assert (ref["v"] <= 1).all() and (ref["sums"][ne] >= 1).all() and (ref["sums"][~ne] == 0).all()
    em = R.emulate_fp32(ip, ix, a, b, sf)
    assert (em["v"] <= 1).all() and (em["sums"][ne] >= 1).all()
    _inside(em, ref, R.bounds(ref), ("sums", "alpha", "v"), f"H={H} {sf}")
    # the gap: the unshifted fp32 exp overflows at +120 and underflows to a zero sum at -600
    with np.errstate(over="ignore"):
        raw = np.exp(R.scores(ip, ix, a, b, sf))
    rows = R.rows_of(ip)
    assert np.isinf(raw[rows % 3 == 1]).all() and (raw[rows % 3 == 2] == 0).all()


@pytest.mark.parametrize("F,H,sf", [(128, 8, "EXP_LEAKY_RELU"), (128, 4, "EXP_LEAKY_RELU"), (64, 4, "EXP_LEAKY_RELU"),
                                    (256, 16, "EXP_LEAKY_RELU"), (128, 8, "EXP")])
@pytest.mark.parametrize("offsets", [True, False])
def test_fp32_emulation_on_the_aggregate_inputs(F, H, sf, offsets):
    ip, ix, nc = R.blocked_graph()
    assert len(ip) - 1 == 300 and (np.diff(ip) == 0).sum() == 5 and np.diff(ip).max() == 700 and 5500 < len(ix) < 6500
    a, b = R.case(300, nc, H, 200 + F + H, offsets)
    x = np.random.default_rng(300 + F).standard_normal((nc, F)).astype(np.float32)
    ref = R.reference(ip, ix, a, b, sf, x=x)
    em = R.emulate_fp32(ip, ix, a, b, sf, x=x)
    _inside(em, ref, R.bounds(ref, F), ("sums", "alpha", "y", "num"), f"F={F} H={H} {sf} offsets={offsets}")
