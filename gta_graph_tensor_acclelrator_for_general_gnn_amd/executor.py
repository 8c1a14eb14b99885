"""HIP executor for GTA instruction streams -- the drop-in for the reference's simulate().

Reference boundary: `interpret()` writes Results/Insts/<net>-<ds>-<layer>-<map>.yaml
(code/interpreter.py:805-849) and `simulate(tile_size_list, dataset, network,
layer, isReorder, isSinput) -> (cycles, rw)` replays it as a cycle model
(code/simulator.py:370-502).  `execute()` takes the same leading arguments,
reads the same two YAML files, and runs the stream on real device tensors:

  * blocks run in dependency order (the stream's block order is the
    compiler's component sort, code/compiler.py:60, not a schedule);
  * inside a block, ops run in data-flow order and are mapped onto libgta
    kernels following the stream's own fusion decisions:
      - a scatter whose FETCH was removed (fuse_fetch, code/interpreter.py:764-802)
        is never materialised: its consumer gathers rows by index
        (GTA_IDX_SRC for ORDER C, GTA_IDX_DST for ORDER R);
      - a COMP_MUL_COMP_ADD / COMP_MM_COMP_ADD pair (inst_fusion_x2, :575-636;
        hardware_info.yaml Inst_fused) becomes one aggregate kernel (MUL) or
        an edge GEMM + gather (MM);
      - scatters with a STORE_E are materialised with gta_scatter;
      - a gather reduces with its COMP_TYPE: ADD on the aggregate kernels and every fusion above,
        MAX / MIN on gta_reduce, MEAN on the aggregate with row_scale = 1/deg, VAR / STD on
        gta_reduce_multi (_eval_reduce); sibling gathers of one producer (a PNA layer's
        aggregators) are filled by ONE gta_reduce_multi launch (_eval_multi);
  * numerics the YAML leaves open come from semantics.py.
Returns ExecResult(values per op, outputs of sink ops, elapsed_s, alg_bytes).
"""
import os
import time
import weakref

import numpy as np
import torch

from . import ir, ops, rewrites
from .semantics import Semantics


# [W | W_s1 | ...] column concatenations of sibling weights, cached per source-weight objects and
# versions (weak references: an address alone is never the key), so a forward reuses one tensor --
# and ops._transposed its W^T -- instead of a cat + W^T per call.  Entries are only made outside a
# HIP graph capture; a capture that reads one records (sources, concatenation) in _CAPTURED_WCAT,
# and GraphedRun re-concatenates it when a source weight changes in place.
_WCAT = {}
_CAPTURED_WCAT = []


def _sibling_cat(srcs):
    key = tuple(id(w) for w in srcs)
    vers = tuple(w._version for w in srcs)
    capturing = srcs[0].is_cuda and torch.cuda.is_current_stream_capturing()
    ent = _WCAT.get(key)
    if ent is not None and ent[1] == vers and all(r() is w for r, w in zip(ent[0], srcs)):
        if capturing:
            _CAPTURED_WCAT.append((list(srcs), ent[2]))
        return ent[2]
    Wc = torch.cat(srcs, dim=1).contiguous()
    if not capturing:  # a tensor from the capture's private pool is never handed to eager runs
        if len(_WCAT) >= 64:
            _WCAT.clear()
        _WCAT[key] = (tuple(weakref.ref(w) for w in srcs), vers, Wc)
    return Wc


class NodeT:
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t


class EdgeT:
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t


class Scat:
    """A scatter kept virtual: edge e reads row idx(e) of node tensor t (mode 'src' or 'dst').

    On a destination-row shard (distributed.RowShard) a source-side table is first this rank's
    row block `local`; `fill` exchanges it into the full table (one all-gather) the first time a
    kernel indexes it through `t`.  Node-side GEMMs of the scatter run on `local` and keep `fill`,
    so the exchange carries the GEMM's output, not its input.  `own` (a replicated model input)
    returns this scatter's whole table without an exchange; derived scatters do not inherit it."""
    __slots__ = ("local", "mode", "fill", "own", "_full")

    def __init__(self, t, mode, fill=None, own=None):
        self.local, self.mode, self.fill, self.own, self._full = t, mode, fill, own, None

    @property
    def t(self):
        if self.fill is None and self.own is None:
            return self.local
        if self._full is None:
            self._full = self.own() if self.own is not None else self.fill(self.local)
        return self._full


class Deferred:
    """An applyedge MUL/MM fused into its gather consumer (evaluated by the gather)."""
    __slots__ = ("op",)

    def __init__(self, op):
        self.op = op


class Lazy:
    """An intermediate whose only consumer was fused with it (e.g. an SF post-op);
    computed on demand if anything else ever asks for it."""
    __slots__ = ("fn", "v")

    def __init__(self, fn):
        self.fn, self.v = fn, None

    def force(self):
        if self.v is None:
            self.v = self.fn()
        return self.v


class ExecResult:
    """Real outputs + measured time, and the reference's modelled (cycles, rw) for the same stream."""

    def __init__(self, values, outputs, elapsed_s, alg_bytes, launches):
        self.values, self.outputs = values, outputs
        self.elapsed_s, self.alg_bytes, self.launches = elapsed_s, alg_bytes, launches
        self.model_cycles = None  # simulate()'s first result (code/simulator.py:502), if requested
        self.model_rw = None      # simulate()'s second result: modelled DRAM bytes
        self.trace = None         # Chrome trace events when execute(..., trace=...) asked for them
        self.model_insts = None   # per-instruction model (costmodel.per_instruction), when a model was asked for
        self.model_spans = None   # model="full": (block, index) -> [first start, first cost, last end] cycles
        self.model_arch = None    # (architecture_name, flexible) of a vTCAD-style call

    def simulate_tuple(self):
        """(cycles, rw) in the shape the reference's simulate() returns."""
        return self.model_cycles, self.model_rw

    def __repr__(self):
        return (f"ExecResult(outputs={sorted(self.outputs)}, elapsed_s={self.elapsed_s:.6f}, "
                f"alg_bytes={self.alg_bytes}, launches={self.launches}, model=({self.model_cycles}, "
                f"{self.model_rw}))")


def _forced(v):
    return v.force() if isinstance(v, Lazy) else v


def _memo(cache, key, src, make):
    """A per-run memo of a value derived from tensor src: the entry (src, its version, value) holds
    src itself and hits only for that very object at the version it was stored at, so an address
    (or an id) reused by another tensor never hits."""
    ent = cache.get(key)
    if ent is None or ent[0] is not src or ent[1] != src._version:
        ent = cache[key] = (src, src._version, make())
    return ent[2]


REDUCERS = ("MAX", "MIN", "MEAN")  # gather COMP_TYPEs beside the sum (Executor._eval_reduce)
MOMENTS = ("VAR", "STD")  # and the moment reducers, which only gta_reduce_multi computes (ops.reduce_multi)
# Smallest group of sibling gathers that takes the one row-chunked multi-reducer launch when every
# member would have passed the column-blocked gate on its own (a source table beyond L2): the
# blocked passes are each cheaper there, so a pair stays blocked
MULTI_MIN_BLOCKED = 3


def _mean_scale(g):
    """float32 [n_rows]: 1 / deg of every row of graph g (a CSR, or a CSC view: the out-degree), rows
    without edges 1 (their sum is 0).  Built once per graph or view and kept beside its plans; no
    host sync.  A capture's first use is not kept: its tensor belongs to the graph's private pool."""
    s = g._plans.get("mean_scale")
    if s is None:
        s = 1.0 / g.degrees().to(torch.float32).clamp_min(1.0)
        if not (s.is_cuda and torch.cuda.is_current_stream_capturing()):
            g._plans["mean_scale"] = s
    return s


# Executor.softmax_shift's default.  True: a matched softmax chain whose SF is an exp-form (SHIFT_SFS) subtracts
# its row maximum before the exp (ops.softmax_shift once per chain, then the shifted edge_softmax /
# gat_aggregate_blocked): no overflow to inf / inf, no 0 / 0 for trained attention scores.  False: the unshifted kernels.
SOFTMAX_SHIFT = False
SHIFT_SFS = ("EXP_LEAKY_RELU", "EXP")

EDGE_EXPR = True  # Executor.edge_expr's default (gta_aggregate_expr for applyedge trees); False: unfused (A/B)

MAX_MATERIALIZE_BYTES = 96 << 30  # refuse to materialise a single edge tensor larger than this


class Executor:
    def __init__(self, opgraph, stream, graph, tensors, semantics=None, plan_chunk=512, dist=None,
                 softmax_shift=None, gather_dtype=None, multi_reduce=True):
        self.g = opgraph
        # dist (distributed.Comm): node tensors are this rank's row block; gathers are
        # reduce-scattered to it and dst-side scatters all-gather it (distributed.py)
        self.dist = dist
        self.n_nodes = dist.n_local if dist is not None else (graph.n_rows if graph is not None else 0)
        self.stream = stream
        self.graph = graph
        self.tensors = dict(tensors)
        self.sem = semantics or Semantics()
        self.plan_chunk = plan_chunk
        self.values = {}
        self._nmm = {}  # node GEMMs of _node_mm in this run: (op, sf, id(table)) -> (table, its version, table W)
        self.alg_bytes = 0
        self.launches = 0
        # trace: per evaluated op, device time (HIP events), algorithmic bytes and launches, as
        # Chrome trace events in the reference's schema (vTCAD/code/simulator.py:360-382)
        self.trace = False
        self.trace_events = None
        # execution-level fusion beyond the stream's (results bitwise unchanged):
        #   elide_scatter_stores: a STORE_E'd scatter read back by a later block is read by index
        #   fuse_sf: an SF whose producer feeds only it runs as the producer's post-op
        self.elide_scatter_stores = True
        self.fuse_sf = True
        #   fuse_mlp: MM -> SF -> MM -> SF chains of node GEMMs (GIN's MLP) as one gta_update_mlp launch
        self.fuse_mlp = FUSE_MLP
        self.mlp_bf16_sum = MLP_BF16_SUM
        # weighted/unweighted SpMM aggregates whose gathered table exceeds the chip's L2
        # run column-blocked (L2-resident slices) when the shape allows it
        self.blocked_min_table_bytes = 32 << 20
        self.blocked_blocks = "auto"  # ops.BlockedPlan.auto_blocks, or a fixed count (0 = never)
        #   reduce_blocked: a MAX / MIN gather of a source-gathered node table passes the same gate to
        #   ops.reduce_blocked (values identical to ops.reduce's: every output is one of its inputs);
        #   False keeps the row-chunked gta_reduce (A/B)
        self.reduce_blocked = True
        #   multi_reduce: sibling gathers (rewrites.sibling_gathers: same producer, same ORDER, COMP_TYPEs
        #   among MEAN / MAX / MIN / VAR / STD) are filled by one ops.reduce_multi launch when the first
        #   of them is evaluated -- the messages are read once; False: one launch per gather (A/B).
        #   MAX / MIN are the single launches' values, the moments within their rounding bound.
        self.multi_reduce = bool(multi_reduce)
        self.std_eps = 1e-5  # STD = sqrt(VAR + std_eps)
        self.siblings = {i: grp for grp in rewrites.sibling_gathers(opgraph) for i in grp}
        self._multi_vals = {}  # sibling gather -> its value from the group's launch, until it is evaluated
        # the graph rewrites below are matched once, by rewrites.py (pure functions of the op graph)
        self.consumers = cons = rewrites.consumers_of(opgraph)
        #   fuse_softmax: GAT's score -> SF -> per-row sum (-> divide) chain runs as one
        #   gta_edge_softmax launch (results equal to fp32 rounding, not bitwise)
        # column shards: per-row sums span ranks (unfused ops + exchanges); row shards own whole rows
        self.fuse_softmax = dist is None or dist.local_rows or dist.s.world == 1
        self.softmax = rewrites.softmax(opgraph, cons, self.sem)
        #   fuse_attention: the softmax chain's alpha (or v) * scatter_C(x) -> gather runs as one
        #   column-blocked gta_gat_aggregate_blocked (no [E, heads] tensor); attention_blocks
        #   None = ops.BlockedPlan.auto_blocks (used when >= 4), or a fixed block count
        self.fuse_attention = True
        self.attention_blocks = None
        self.attn = rewrites.attention(opgraph, cons, self.sem, self.softmax)
        self._att_state = {}
        #   softmax_shift: the chains' exp-form SFs run overflow-safe (SOFTMAX_SHIFT above); the row-max
        #   table of a chain is built once, on first use, and handed to both of its launches
        self.softmax_shift = SOFTMAX_SHIFT if softmax_shift is None else bool(softmax_shift)
        self._att_shift = {}  # score op A -> Lazy shift table [n, H] (beside _att_state)
        #   gather_dtype: None (the default: nothing changes), or torch.bfloat16 -- the storage type of
        #   the node tables the column-blocked kernels gather.  An fp32 table that a SpMM-form ADD
        #   aggregate (_spmm, mode src, weighted or not) would gather column-blocked, or that the fused
        #   attention aggregate (_eval_attention) gathers, is rounded once to bf16 (RNE, Tensor.to:
        #   plumbing, capturable) and gathered as bf16 -- half the row bytes, every sum still fp32,
        #   bitwise the fp32 run on the rounded table (gta_aggregate_blocked_x).  A table that is bf16
        #   already (a bf16 model input) takes the blocked form by the same size rule, with no cast.
        #   One cast per table value, shared by its consumers (_gather_cast; gather_casts counts
        #   them).  The MAX / MIN gathers that pass the gate (_eval_reduce, reduce_blocked) take the
        #   same cast table -- rounding commutes with the max -- and under this option only, MEAN runs
        #   as the blocked aggregate with row_scale = 1 / deg.  Left as they are: the row-chunked form
        #   (tables under the size gate), expression gathers, self-term forms, ORDER C and distributed.py.
        if gather_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError(f"gather_dtype: None, torch.float32 or torch.bfloat16, not {gather_dtype}")
        self.gather_dtype = None if gather_dtype == torch.float32 else gather_dtype
        self.gather_casts = 0
        self._gather_cache = {}  # id(table) -> (table, its version, the bf16 copy): identity checked on use
        #   mm_first: a gather whose only consumer is a narrowing applynode MM is executed as
        #   MM-then-aggregate (sum_e w_e x_src) W == sum_e w_e (x W)_src -- the layer's output
        #   to fp32 rounding, the gather's own value computed only if something asks for it
        self.mm_first = True
        self.reorder = rewrites.mm_first(opgraph, cons)
        #   and through two hops (SGC: gather -> scatter C -> MUL -> gather -> MM): A (A x) W == A (A (x W)),
        #   both aggregates at the narrow width; the first gather's value computed only if asked for
        self.two_hop = rewrites.two_hop(opgraph, cons, self.reorder) if dist is None else {}
        #   node_mm: an applyedge MM of a scatter runs on the node tensor, (x W)[r(e)] == x[r(e)] W
        #   (bitwise: the same dot product per row), and stays a virtual scatter of x W
        #   mm_pushdown: MM(scatter a (+) scatter b) == (a W)[r(e)] (+) (b W)[r'(e)] (DGN op 2 -> 3),
        #   to fp32 rounding; the [E, F_in] sum is never built
        self.node_mm = True
        self.mm_pushdown = True
        #   sibling_mm: applynode MMs that multiply the same node tensor run as ONE GEMM over the
        #   concatenated weights (x read once; e.g. GraphSAGE's x W3 and x W4, GAT's scores W1, W2)
        self.sibling_mm = True
        self.pushdown = rewrites.pushdown(opgraph, cons, self.sem)
        #   gather_acc: applynode ADD(gather G, node op T), each the other's only reader (GIN op 4:
        #   agg + (1+eps) x), runs as the aggregate accumulating into T's fresh output buffer:
        #   T + sum == sum + T bitwise, and the ADD pass over [N, F] disappears.  G and T stay
        #   available (recomputed on demand).
        self.gather_acc = dist is None or dist.local_rows or dist.s.world == 1
        self.gacc = rewrites.gather_acc(opgraph, cons, self.sem)
        self.gacc_t = {T: A for A, (_, _, T) in self.gacc.items()}  # node op T -> its ADD consumer
        #   edge_expr: a gather R whose edge value is a tree of applyedge ops (ADD / SUB / MUL / DIV,
        #   SF post-ops, a pushed-down MM), each read only by the next, runs as one
        #   gta_aggregate_expr: no [E, F] tensor for any op of the tree, bitwise the unfused ops and
        #   gather (DGN ops 2-8, PNA ops 5-8).  The tree's ops stay available, computed unfused if read.
        self.edge_expr = EDGE_EXPR
        self.expr = rewrites.edge_expr(opgraph, cons, self.sem, self.softmax, self.attn, self.pushdown, self.gacc)
        self.expr_nodes = {i for e in self.expr.values() for i in e["nodes"]}

    # ---------------------------------------------------------------- inputs
    def _ext(self, op, slot):
        return self.tensors.get(f"ext:{op.idx}:{slot}")

    def _source(self, op, slot):
        src = self.g.inputs[op.idx][slot]
        if src.kind == "op":
            if src.op not in self.values:
                raise RuntimeError(f"op {op.idx} reads op {src.op} before it was produced")
            v = self.values[src.op]
            return v.force() if isinstance(v, Lazy) else v
        t = self._ext(op, slot)
        if src.kind == "ext":
            if t is None:
                raise KeyError(f"op {op.idx} slot {slot}: external input 'ext:{op.idx}:{slot}' not given")
            return self._wrap_ext(t, op)
        if t is not None:  # explicit override of the model input for this slot
            return self._wrap_ext(t, op)
        if op.type == "applyedge":
            t = self.tensors.get("x_edge")
            if t is None:
                raise KeyError(f"edge op {op.idx} reads the model input: give 'x_edge' or 'ext:{op.idx}:{slot}'")
            return EdgeT(t)
        return NodeT(self.tensors["x"])

    def _wrap_ext(self, t, op=None):
        if t.dim() == 1:
            t = t.view(-1, 1)
        if op is not None and op.type in ("scatter", "applynode") and t.shape[0] == self.n_nodes \
                and t.shape[0] != 1:  # N == E (e.g. an empty row shard): these ops read node rows
            return NodeT(t)
        if t.shape[0] == self.graph.nnz and t.shape[0] != self.n_nodes:
            return EdgeT(t)
        if t.shape[0] == 1:
            return ("row", t)
        if t.shape[0] == self.n_nodes and t.shape[0] != self.graph.nnz:
            return NodeT(t)
        return EdgeT(t)  # ambiguous N == E: edge tensor

    def _inputs(self, op):
        return [self._source(op, s) for s in range(len(self.g.inputs[op.idx]))]

    def _pair(self, op, ins=None):
        """op's evaluated operands (ins: those already at hand); an op with one graph input takes
        `ext:<op>:1`, when given, as its second operand."""
        ins = self._inputs(op) if ins is None else ins
        extra = self._ext(op, 1) if len(self.g.inputs[op.idx]) == 1 else None
        return ins if extra is None else ins + [self._wrap_ext(extra)]

    def _pending(self, i):
        """Op i's value is a Lazy nobody has forced: the op was fused away and is still unformed."""
        raw = self.values.get(i)
        return isinstance(raw, Lazy) and raw.v is None

    @staticmethod
    def _fp32(t):
        return t if t.dtype == torch.float32 else t.float()  # exact widening of a bf16 table

    @staticmethod
    def _width(z):
        """Feature width of an evaluated operand (0 for a fused producer not formed yet)."""
        if isinstance(z, tuple):
            return z[1].shape[1]
        return z.t.shape[1] if not isinstance(z, Deferred) else 0

    # ---------------------------------------------------------- materialise
    def _edge_operand(self, v):
        """-> (tensor, mode, broadcast_row) usable by apply_edge / aggregate."""
        if isinstance(v, Deferred):
            v = self._materialize_deferred(v)
        if isinstance(v, EdgeT):
            return v.t, "edge", False
        if isinstance(v, Scat):  # (a bf16 node table is widened: the element-wise kernels are fp32)
            return self._fp32(v.t), v.mode, False
        if isinstance(v, tuple) and v[0] == "row":
            return v[1], "edge", True
        raise TypeError(f"not an edge operand: {type(v).__name__}")

    def _to_edge_tensor(self, v):
        if isinstance(v, EdgeT):
            return v.t
        if isinstance(v, Scat):
            nbytes = self.graph.nnz * v.t.shape[1] * v.t.element_size()
            if nbytes > MAX_MATERIALIZE_BYTES:
                raise MemoryError(f"stream materialises a {nbytes / 2**30:.0f} GiB edge tensor (scatter not fused "
                                  "with its consumer); choose a fusion partition that keeps it virtual")
            self._count(self.graph.nnz * v.t.shape[1] * 4 * 2 + self.graph.nnz * 4)
            return ops.scatter(self.graph, self._fp32(v.t), "C" if v.mode == "src" else "R")  # edge tensors are fp32
        if isinstance(v, Deferred):
            return self._materialize_deferred(v).t
        raise TypeError(type(v).__name__)

    def _materialize_deferred(self, d):
        op = self.g.ops[d.op]
        v = self._eval_applyedge(op)
        self.values[d.op] = v
        return v

    def _count(self, nbytes):
        self.alg_bytes += int(nbytes)
        self.launches += 1

    # ------------------------------------------------------- edge softmax
    def _eval_edge_expr(self, G):
        """G's value from one gta_aggregate_expr launch, or None (then the tree runs unfused)."""
        e = self.expr[G.idx]
        if not all(self._pending(i) for i in e["nodes"]):
            return None
        operands, gathered = [], 0
        for ref in e["leaves"]:
            if ref[0] == "pmm":
                mm = self.g.ops[ref[1]]
                v = self._source(self.g.ops[self.g.inputs[mm.idx][0].op], ref[2])
                if not isinstance(v, Scat):
                    return None
                v = self._node_mm(mm, v)
            else:
                v = self._source(self.g.ops[ref[0]], ref[1])
            if isinstance(v, Scat):
                operands.append((self._fp32(v.t), v.mode))
                gathered += v.mode == "src"
            elif isinstance(v, EdgeT):
                operands.append((v.t, "edge"))
                gathered += 1
            elif isinstance(v, tuple) and v[0] == "row":
                operands.append((v[1], "row"))
            else:
                return None
        F = operands[0][0].shape[1]
        if any(t.shape[1] != F or t.dtype != torch.float32 for t, _ in operands):
            return None
        y = ops.aggregate_expr(self.graph, e["shape"], operands, e["bins"], e["sfs"], e["swap"], plan=self._plan())
        if y is None:
            return None
        for mm in {ref[1] for ref in e["leaves"] if ref[0] == "pmm"}:
            # a pushed-down MM read later is the pushed-down product, as the unfused run forms it,
            # whether or not its sum's value has been asked for in between
            mop, add = self.g.ops[mm], self.g.inputs[mm][0].op
            self.values[mm] = Lazy(lambda mop=mop, add=add: self._pushdown_mm(mop, add))
        n, E = self.graph.n_rows, self.graph.nnz
        self._count(self._gather_bytes(E, n, F, 4 * gathered))  # fp32 rows of every gathered operand
        return NodeT(self.dist.reduce_rows(y) if self.dist is not None else y)

    def _self_term(self, top):
        """(x, s) when node op T = applynode MUL(x, s) of a node tensor x by a one-element scalar s
        (GIN op 3: (1 + eps) x): the aggregate can form T itself (gta_aggregate_self).  Else None."""
        if top.type != "applynode" or top.comp != "MUL" or self._binary(top) != "MUL":
            return None
        ins = self._pair(top)
        if len(ins) != 2:
            return None
        xs = [z for z in ins if isinstance(z, NodeT)]
        rows = [z for z in ins if isinstance(z, tuple) and z[0] == "row"]
        if len(xs) != 1 or len(rows) != 1 or rows[0][1].numel() != 1 or rows[0][1].dtype != torch.float32:
            return None
        return xs[0].t, rows[0][1]

    def _eval_gather_acc(self, A, out_dtype=torch.float32):
        """A = ADD(G, T) as G's aggregate accumulated into T's buffer; None if G's form cannot
        accumulate (then A runs unfused).  When T = x * s (a scalar) and T was left unformed, the
        aggregate forms it in its epilogue instead (no [N, F] T written and read back); only that
        form takes out_dtype bf16 (A stored rounded, for the fused MLP that reads it)."""
        G, slot_t, T = self.gacc[A.idx]
        if not self._pending(G):
            return None
        if self._pending(T):
            st = self._self_term(self.g.ops[T])
            y = self._eval_gather(self.g.ops[G], self_term=st, out_dtype=out_dtype) if st is not None else None
            if y is not None:
                return y  # T stays unformed: recomputed by its own kernel if something reads it
        if out_dtype != torch.float32:
            return None
        t = self._source(A, slot_t)
        if not isinstance(t, NodeT) or t.t.dtype != torch.float32 or not t.t.is_contiguous():
            return None
        y = self._eval_gather(self.g.ops[G], acc=t.t)
        if y.t.data_ptr() != t.t.data_ptr():  # G's form computed a fresh tensor: add it as the ADD would
            self.values[G].v = y
            return None
        top = self.g.ops[T]
        self.values[T] = Lazy(lambda: self._eval_applynode(top))  # T's buffer now holds A
        return y

    def _node_mm(self, op, v, post_sf=None):
        """applyedge MM of a virtual scatter: the GEMM runs over the node rows, the result stays virtual.
        The two scatters of one node table under one MM (DGN op 3's x[src] + x[dst]) share a GEMM."""
        W = self.tensors[f"w:{op.idx}"]
        if W.shape[0] != v.local.shape[1]:
            raise ValueError(f"op {op.idx}: weight rows {W.shape[0]} != feature width {v.local.shape[1]}")

        def gemm():
            x, w = self._mm_dtypes(v.local, W)
            self._count(x.shape[0] * (x.shape[1] * x.element_size() + w.shape[1] * 4) + w.numel() * w.element_size())
            return ops.update_mm(x, w, sf=post_sf)
        # keyed on the source table itself, before any widening: a temporary's address is no identity
        return Scat(_memo(self._nmm, (op.idx, post_sf, id(v.local)), v.local, gemm), v.mode, v.fill)

    def _pushdown_mm(self, op, add_idx, post_sf=None):
        """MM(scatter a + scatter b) as (a W)[r_a(e)] + (b W)[r_b(e)]."""
        if post_sf is not None:
            return None  # the SF acts on the sum: keep the literal order
        a, b = [self._source(self.g.ops[add_idx], k) for k in range(2)]
        if not (isinstance(a, Scat) and isinstance(b, Scat)):
            return None
        sa, sb = self._node_mm(op, a), self._node_mm(op, b)
        out = ops.apply_edge(self.graph, "ADD", None, sa.t, sa.mode, sb.t, sb.mode)
        self._count(self.graph.nnz * out.shape[1] * 4 * 3)
        return EdgeT(out)

    def _pending_siblings(self, x, main_idx, W):
        """Unevaluated applynode MM ops whose input is the node tensor x itself, with weights of
        W's dtype and K and no SF epilogue of their own."""
        if not self.sibling_mm:
            return []
        sib = []
        for op in self.g.ops:
            if op.idx == main_idx or op.idx in self.values or op.type != "applynode" or op.comp != "MM":
                continue
            ins = self.g.inputs[op.idx]
            if len(ins) != 1:
                continue
            src = ins[0]
            if src.kind == "op":
                v = self.values.get(src.op)
                if not (isinstance(v, NodeT) and v.t is x):
                    continue
            elif src.kind == "x":
                if self._ext(op, 0) is not None or self.tensors.get("x") is not x:
                    continue
            else:
                continue
            Ws = self.tensors.get(f"w:{op.idx}")
            if Ws is None or Ws.dtype != W.dtype or Ws.shape[0] != W.shape[0] or self._sf_child_any(op):
                continue
            sib.append(op)
        return sib

    def _sf_child_any(self, op):
        cons = self.consumers[op.idx]
        return self.fuse_sf and len(cons) == 1 and self.g.ops[cons[0]].comp == "SF" \
            and self.g.ops[cons[0]].type == op.type

    def _node_gemm(self, x, main_idx, W, post_sf=None):
        """x W for op main_idx; sibling MMs of the same x ride along in the same GEMM (their
        values are column views of the output).  Returns the main op's [rows, N] result."""
        sibs = [] if post_sf is not None else self._pending_siblings(x, main_idx, W)
        x2, W2 = self._mm_dtypes(x, W)
        if not sibs:
            out = ops.update_mm(x2, W2, sf=post_sf)
            self._count(x.shape[0] * (x.shape[1] * x.element_size() + W.shape[1] * 4) + W.numel() * W.element_size())
            return out
        Wc = _sibling_cat([W] + [self.tensors[f"w:{o.idx}"] for o in sibs])
        x2, Wc2 = self._mm_dtypes(x, Wc)
        out = ops.update_mm(x2, Wc2)
        self._count(x.shape[0] * (x.shape[1] * x.element_size() + Wc.shape[1] * 4) + Wc.numel() * Wc.element_size())
        off = W.shape[1]
        for o in sibs:
            n_o = self.tensors[f"w:{o.idx}"].shape[1]
            self.values[o.idx] = NodeT(out[:, off:off + n_o])
            off += n_o
        return out[:, :W.shape[1]]

    def _gather_value(self, op):
        v = self._eval_gather(op)
        if self.dist is None:
            return v
        return NodeT(self.dist.reduce_cols(v.t) if op.order == "C" else self.dist.reduce_rows(v.t))

    def _mm_first_operands(self, G):
        """(x, w, fill) of a gather G = sum_e w_e x[src(e)] (w None: unweighted), or None."""
        v = self._source(G, 0)
        if isinstance(v, Deferred):
            p = self.g.ops[v.op]
            if p.comp != "MUL" or self.sem.bin_of(p) != "MUL":
                return None
            pins = self._pair(p)
            xs = [z for z in pins if isinstance(z, Scat) and z.mode == "src"]
            ws = [z for z in pins if not (isinstance(z, Scat) and z.mode == "src")]
            if len(xs) != 1 or len(ws) > 1:
                return None
            x, w, fill = xs[0].local, None, xs[0].fill
            if ws:
                if isinstance(ws[0], tuple) or ws[0] is None:
                    return None
                w = self._to_edge_tensor(ws[0])
                if w.shape[1] != 1:
                    return None
        elif isinstance(v, Scat) and v.mode == "src":
            x, w, fill = v.local, None, v.fill
        else:
            return None
        return x, w, fill

    def _eval_two_hop(self, G2, M):
        """M = A (A x) W as A (A (x W)): the first hop G1's value and its scatter stay unformed."""
        G1 = next((g1 for g1, g2 in self.two_hop.items() if g2 == G2.idx), None)
        if not (self.mm_first and G1 is not None and self._pending(G1)):
            return None
        src = self.g.inputs[G2.idx][0]
        P = self.g.ops[src.op]
        w2 = None
        if P.type != "scatter":  # the second hop's weight MUL: its operand that is not the scatter
            pv = self.values.get(P.idx)
            if not isinstance(pv, Deferred) or P.comp != "MUL" or self.sem.bin_of(P) != "MUL":
                return None
            slots = [k for k, x in enumerate(self.g.inputs[P.idx])
                     if not (x.kind == "op" and self.g.ops[x.op].type == "scatter")]
            others = self._pair(P, [self._source(P, k) for k in slots])
            if len(others) > 1 or (others and isinstance(others[0], (tuple, Scat))):
                return None
            if others:
                w2 = self._to_edge_tensor(others[0])
                if w2.shape[1] != 1:
                    return None
        opnd = self._mm_first_operands(self.g.ops[G1])
        if opnd is None:
            return None
        x, w1, fill = opnd
        W = self.tensors[f"w:{M.idx}"]
        if fill is not None or W.shape[0] != x.shape[1]:
            return None
        xw = self._node_gemm(x, M.idx, W).contiguous()
        z = self._spmm(xw, "src", w1)
        y = self._spmm(z, "src", w2)
        n, E, F = self.graph.n_rows, self.graph.nnz, xw.shape[1]
        for w in (w1, w2):
            self._count(self._gather_bytes(E, n, F, 4, heads=int(w is not None)))
        self.values[M.idx] = NodeT(y)
        return Lazy(lambda: self._gather_value(G2))

    def _eval_mm_first(self, G, M):
        """Sets M's value to aggregate(x W) and returns G's value lazily; None if the operands
        do not allow it (head-wise weights, edge-tensor features)."""
        if G.idx in self.two_hop.values():
            v = self._eval_two_hop(G, M)
            if v is not None:
                return v
        opnd = self._mm_first_operands(G)
        if opnd is None:
            return None
        x, w, fill = opnd
        W = self.tensors[f"w:{M.idx}"]
        if W.shape[0] != x.shape[1]:
            return None
        xw = self._node_gemm(x, M.idx, W).contiguous()
        if fill is not None:  # row shards: exchange x W (narrower than x)
            xw = fill(xw)
        n, E, F = self.graph.n_rows, self.graph.nnz, xw.shape[1]
        y = self._spmm(xw, "src", w)
        self._count(self._gather_bytes(E, n, F, 4, heads=int(w is not None)))
        self.values[M.idx] = NodeT(self.dist.reduce_rows(y) if self.dist is not None else y)
        return Lazy(lambda: self._gather_value(G))

    def _eval_attention(self, G2, M, sf_out=None):
        """G2 = gather(scatter_C(x) * alpha|v) as one fused launch; None if the shapes do not allow it.
        sf_out: the SF of G2's only consumer, applied as y is written (the caller owns that op's value)."""
        pat, _, S = self.attn[M]
        st = self._att_state.get(pat["A"])
        sv = self.values.get(S)
        if st is None or not isinstance(sv, Scat) or sv.mode != "src":
            return None
        a, b, sf = st
        shift = self._att_shift.get(pat["A"])
        x = sv.t
        F, H = x.shape[1], a.shape[1]
        if x.dtype not in ops.BlockedPlan.DTYPES or not ops.BlockedPlan.supports_att(F, H):
            return None
        xe = 2 if self.gather_dtype == torch.bfloat16 else x.element_size()  # bytes per gathered element
        B = self.attention_blocks or ops.BlockedPlan.auto_blocks(self.graph, F, xe)
        # the lean fused kernel (F = 128, 8 heads) beats softmax + aggregate even unblocked (B = 1:
        # Flickr 102 vs 168 us; the round-4 probe, profiles/r04/layer_bench_*.log); other shapes need a blocked table
        lean = F == 128 and H == 8
        if B < (1 if (self.attention_blocks or lean) else 4) or not ops.blocked_ready(self.graph, B):
            return None
        norm = pat["D"] is not None
        G = pat["G"]
        want = not norm and self._pending(G)
        E, n = self.graph.nnz, self.graph.n_rows
        x = self._gather_cast(x)
        if shift is not None:
            y, sums = ops.gat_aggregate_blocked(self.graph, x, a, b, sf, normalize=norm, want_sums=want, blocks=B,
                                                sf_out=sf_out, shift=shift.force())
            self._count(self._gather_bytes(E, n, F, xe, heads=H) + n * 8 * H)  # the scores' and the shift's rows
        else:
            y, sums = ops.gat_aggregate_blocked(self.graph, x, a, b, sf, normalize=norm, want_sums=want, blocks=B,
                                                sf_out=sf_out)
            self._count(self._gather_bytes(E, n, F, xe, heads=H) + n * 4 * H)  # the scores' rows
        if want:
            self.values[G] = NodeT(sums)
        return NodeT(y)

    def _eval_softmax(self, A, pat):
        """Registers V, G (and D) as views of one gta_edge_softmax launch; returns A's own value."""
        ins = self._inputs(A)
        if not all(isinstance(x, Scat) for x in ins) or {x.mode for x in ins} != {"dst", "src"}:
            return None
        a = next(x.t for x in ins if x.mode == "dst")
        b = next(x.t for x in ins if x.mode == "src")
        H = a.shape[1]
        if b.shape[1] != H or H > 64 or H & (H - 1):
            return None
        V, sf, norm = self.g.ops[pat["V"]], self.sem.sf_of(self.g.ops[pat["V"]]), pat["D"] is not None
        E, n = self.graph.nnz, self.graph.n_rows
        self._att_state[A.idx] = (a, b, sf)
        shift = None
        if self.softmax_shift and sf in SHIFT_SFS:
            def build_shift():  # one pass over the indices and b; a and the table per row
                t = ops.softmax_shift(self.graph, a, b, sf)
                self._count(E * (4 + 4 * H) + n * (8 + 8 * H))
                return t
            shift = self._att_shift[A.idx] = Lazy(build_shift)

        def launch():
            if shift is not None:
                out, sums = ops.edge_softmax(self.graph, a, b, sf, normalize=norm, want_sums=True,
                                             shift=shift.force())
                self._count(E * (4 + 8 * H) + n * (8 + 12 * H))
                return out, sums
            out, sums = ops.edge_softmax(self.graph, a, b, sf, normalize=norm, want_sums=True)
            self._count(E * (4 + 8 * H) + n * (8 + 8 * H))
            return out, sums
        shared = Lazy(launch)
        self.values[pat["G"]] = Lazy(lambda: NodeT(shared.force()[1]))
        if norm:
            self.values[pat["D"]] = Lazy(lambda: EdgeT(shared.force()[0]))
            self.values[V.idx] = Lazy(lambda: self._eval_applyedge(A, post_sf=sf))
        else:
            self.values[V.idx] = Lazy(lambda: EdgeT(shared.force()[0]))
        return Lazy(lambda: self._eval_applyedge(A))

    # ---------------------------------------------------------------- eval
    def _binary(self, op):
        return self.sem.bin_of(op)

    def _eval_applyedge(self, op, post_sf=None):
        E = self.graph.nnz
        if op.comp == "MM":
            src = self.g.inputs[op.idx][0]
            if self.mm_pushdown and src.kind == "op" and self.pushdown.get(src.op) == op.idx and self._pending(src.op):
                v = self._pushdown_mm(op, src.op, post_sf)  # the sum is still unformed: go through it
                if v is not None:
                    return v
            ins = self._inputs(op)
            if self.node_mm and isinstance(ins[0], Scat):
                return self._node_mm(op, ins[0], post_sf)
            return EdgeT(self._edge_mm(op, ins[0], post_sf))
        ins = self._inputs(op)
        if op.comp == "SF":
            a, am, _ = self._edge_operand(ins[0])
            out = ops.apply_edge(self.graph, None, self.sem.sf_of(op), a, am)
            self._count(E * (a.shape[1] * 8))
            return EdgeT(out)
        bin_ = self._binary(op)
        ins = self._pair(op, ins)
        if len(ins) == 1:  # unary ADD/MUL: identity unless an extra operand is supplied
            return EdgeT(self._to_edge_tensor(ins[0]))
        x, y = ins[0], ins[1]
        if bin_ == "RDIV":
            x, y, bin_ = y, x, "DIV"
        a, am, arow = self._edge_operand(x)
        b, bm, brow = self._edge_operand(y)
        if arow and not brow:  # keep the broadcast row in the b slot (ADD/MUL commute)
            if bin_ in ("ADD", "MUL"):
                a, am, b, bm, arow, brow = b, bm, a, am, False, True
            else:
                a = a.expand(E, a.shape[1]).contiguous()  # a broadcast row on the left of DIV/SUB
                am, arow = "edge", False
        out = ops.apply_edge(self.graph, bin_, post_sf, a, am, b, bm, b_broadcast_row=brow)
        self._count(E * out.shape[1] * 4 * 3)
        return EdgeT(out)

    def _edge_mm(self, op, v, post_sf=None):
        W = self.tensors[f"w:{op.idx}"]
        if isinstance(v, Scat):
            idx = self.graph.indices if v.mode == "src" else self.graph.row_of_edge()
            x, row_idx = v.t, idx
        else:
            x, row_idx = self._to_edge_tensor(v), None
        x, W = self._mm_dtypes(x, W)
        out = ops.update_mm(x, W, row_idx, sf=post_sf, m=self.graph.nnz if row_idx is None else None)
        self._count(self.graph.nnz * (x.shape[1] * x.element_size() + W.shape[1] * 4))
        return out

    @staticmethod
    def _mm_dtypes(x, W):
        # fp32 activations with bf16 weights go straight in: the GEMM rounds x to bf16
        # while staging it into LDS (GTA_F32_BF16); only bf16 x with fp32 W is widened
        if W.dtype == torch.float32 and x.dtype != torch.float32:
            x = x.float()
        return x, W

    def _site(self, v, order):
        """Where a gather of direction `order` reads evaluated operand v: (graph view, table, mode, n_out).
        ORDER R walks the layer's CSR (n_rows outputs): a virtual scatter is read by index from its
        node table in its own mode, anything else is formed as an edge tensor.  ORDER C (DIRECTION
        src, template/ISA_defination.yaml:46-48) walks the stable CSC view (ops.CSC, gta_csc_build:
        a column's edges in CSR order, no atomics; n_cols outputs), always in mode "src" of that
        view: its "dst" rows for a scatter R, the column itself for a scatter C, the permutation
        for an edge tensor.  The only place that knows these rules."""
        if order == "C":
            c = ops.csc(self.graph)
            if isinstance(v, Scat):
                return c.view("dst" if v.mode == "dst" else "src"), v.t, "src", self.graph.n_cols
            return c.view("edge"), self._to_edge_tensor(v), "src", self.graph.n_cols
        if isinstance(v, Scat):
            return self.graph, v.t, v.mode, self.graph.n_rows
        return self.graph, self._to_edge_tensor(v), "edge", self.graph.n_rows

    @staticmethod
    def _gather_bytes(E, n_out, F, row_es, heads=0, out_es=4, index=True):
        """Algorithmic bytes of one aggregate-shaped launch: per edge an index (not in EDGE mode of
        the CSR, index=False), `heads` fp32 weights and a row of F elements of row_es bytes; per
        output row its two pointers and F elements of out_es bytes.  Each site passes the element
        sizes it has always charged (DESIGN.md §1.1 lists where they disagree)."""
        return E * ((4 if index else 0) + 4 * heads + row_es * F) + n_out * (8 + out_es * F)

    def _eval_gather(self, op, acc=None, self_term=None, out_dtype=torch.float32):
        """The ISA gather, both DIRECTIONs (_site).  A fused producer stays virtual: a scatter operand
        is gathered by index, a MUL by an edge weight runs as one weighted aggregate, ORDER R takes an
        MM on the node side; anything else is materialised as an edge tensor and summed.
        self_term (x, s): y = x * s + the aggregate, or None if this gather's form cannot take it;
        out_dtype (self_term only): y's storage dtype."""
        if op.comp in REDUCERS + MOMENTS:  # not the sum: no accumulate, no self term, none of the sum's fusions
            return None if (acc is not None or self_term is not None) else self._eval_reduce(op)
        if op.order == "C" and (acc is not None or self_term is not None):
            return None  # ORDER C takes no accumulator and no self term
        src = self.g.inputs[op.idx][0]
        E = self.graph.nnz
        if self_term is not None:
            v = self._source(op, 0) if not (self.fuse_attention and src.kind == "op" and src.op in self.attn) else None
            if isinstance(v, Deferred):
                p = self.g.ops[v.op]
                pins = self._pair(p)
                if p.comp == "MM" or self._binary(p) != "MUL" or len(pins) != 2:
                    return None
                y = self._weighted_aggregate(pins[0], pins[1], self_term=self_term, out_dtype=out_dtype)
                return None if y is None else NodeT(y)
            if isinstance(v, Scat):
                y = self._spmm(v.t, v.mode, None, self_term=self_term, out_dtype=out_dtype)
                if y is not None:
                    self._count(self._gather_bytes(E, self.graph.n_rows, v.t.shape[1], v.t.element_size(),
                                                   out_es=y.element_size()))
                    return NodeT(y)
            return None
        if self.fuse_attention and src.kind == "op" and src.op in self.attn:  # (its gather is ORDER R: rewrites.attention)
            raw = self.values.get(src.op)
            if isinstance(raw, (Deferred, Lazy)):
                y = self._eval_attention(op, src.op)
                if y is not None:
                    return y
        v = self._source(op, 0)
        if isinstance(v, Deferred):
            p = self.g.ops[v.op]
            if p.comp == "MM":
                if op.order == "R":  # (ORDER C has no node-side form: it sums the formed product)
                    return NodeT(self._gather_mm(p))
            else:
                pins = self._pair(p)
                if len(pins) == 1 and op.order == "R":
                    v = pins[0]  # an identity ADD / MUL: ORDER R gathers its operand as it is, ORDER C forms it
                elif len(pins) == 2 and self._binary(p) == "MUL":
                    y = self._weighted_aggregate(pins[0], pins[1], acc, order=op.order)
                    if y is not None:
                        return NodeT(y)
            if isinstance(v, Deferred):  # any other fused pair: evaluate the producer, then gather
                v = self._materialize_deferred(v)
        scat = isinstance(v, Scat)
        g, t, mode, n_out = self._site(v, op.order)
        F = t.shape[1]
        if op.order == "C":
            # column-blocked like direction R when the table is large, but only for a scatter R over
            # the "dst" view (the transposed aggregate); the byte model charges the table's own rows
            if scat and v.mode == "dst":
                y = self._spmm(t, "src", None, graph=g)
            else:
                y = ops.aggregate(g, t, "src", None, plan=self._plan())
            self._count(self._gather_bytes(E, n_out, F, t.element_size() if scat else 4))
        elif scat:
            y = self._spmm(t, mode, None, acc)
            self._count(self._gather_bytes(E, n_out, F, 4))
        else:
            y = ops.aggregate(g, t, "edge", None, out=acc, accumulate=acc is not None, plan=self._plan())
            self._count(self._gather_bytes(E, n_out, F, 4, index=False))
        return NodeT(y)

    def _gather_mm(self, p):
        """ORDER R gather of a fused applyedge MM p: gather(x[r(e)] W) = SpMM of x W on the node side,
        else the edge GEMM and a plain segment sum."""
        n, E = self.graph.n_rows, self.graph.nnz
        pins = self._inputs(p)
        if self.node_mm and isinstance(pins[0], Scat):
            sw = self._node_mm(p, pins[0])
            y = self._spmm(sw.t, sw.mode, None)
            self._count(self._gather_bytes(E, n, sw.t.shape[1], 4))
            return y
        xe = self._edge_mm(p, pins[0])
        y = ops.gather_add(self.graph, xe)
        self._count(E * xe.shape[1] * 4 + n * xe.shape[1] * 4)
        return y

    def _plan(self):
        return self.plan_chunk if self.plan_chunk else None

    def _eval_reduce(self, op):
        """The ISA gather whose COMP_TYPE is MAX, MIN or MEAN (include/gta.h gta_reduce; the sum's
        COMP_TYPE is ADD), both DIRECTIONs (_site).  A virtual scatter is reduced by index straight from the
        node table (fp32 or bf16; no [E, F] tensor); everything else -- an edge tensor, or a fused
        applyedge MUL / MM producer, which is first formed as the unfused op forms it -- in EDGE
        mode.  MAX / MIN run gta_reduce; MEAN is the plain ADD aggregate with row_scale = 1 / deg
        (empty rows 0; ORDER C: the out-degree from colptr); VAR / STD (MOMENTS) run gta_reduce_multi
        with one member; a gather of a sibling group (self.siblings) runs the group's one launch, or
        takes the value that launch left for it (_eval_multi).  None of the rewrites that rely on the
        gather being a sum applies (mm_first, two_hop, gather_acc, the weighted aggregate, the
        attention chains, edge_expr)."""
        d = self.dist
        if d is not None and d.s.world > 1 and (not d.local_rows or op.order == "C"):
            raise NotImplementedError(
                f"op {op.idx}: gather {op.comp} on a shard that holds only part of each output node's edges "
                "(partial maxima / means cannot be summed across ranks); row-local shards of an ORDER R gather work")
        if op.idx in self._multi_vals:  # a sibling's launch filled it
            return self._multi_vals.pop(op.idx)
        v = self._source(op, 0)
        if isinstance(v, Deferred):
            v = self._materialize_deferred(v)
        scat, col = isinstance(v, Scat), op.order == "C"
        g, t, mode, n_out = self._site(v, op.order)
        E, F = self.graph.nnz, t.shape[1]
        group = self.siblings.get(op.idx) if self.multi_reduce else None
        if group is not None and self._multi_wanted(group, v, t, g, col):
            return self._eval_multi(op, group, g, t, mode, n_out, index=col or scat, row_es=t.element_size() if col else 4)
        if op.comp in MOMENTS:  # one member: the same kernel family, the moment accumulators only
            y, = ops.reduce_multi(g, t, (op.comp,), mode, plan=self._plan(), std_eps=self.std_eps)
            self._count(self._gather_bytes(E, n_out, F, t.element_size() if col else 4, index=col or scat))
            return NodeT(y)
        # (ORDER C charges the table's own element size, ORDER R 4 bytes; EDGE mode of the CSR reads no index)
        nbytes = self._gather_bytes(E, n_out, F, t.element_size() if col else 4, index=col or scat)
        # column-blocked when a source-gathered node table outgrows L2 (_spmm's gate, evaluated before
        # any blocked op is named): ORDER R of a scatter C on the layer's CSR, ORDER C of a scatter R
        # over the transposed view.  MAX / MIN values are identical by construction; MEAN moves only
        # under gather_dtype bf16 (its blocked sum order would change the default bits), and never in
        # ORDER C (the views are not cast)
        B = 0
        if self.reduce_blocked and scat:
            on = self.gather_dtype == torch.bfloat16
            if not col and v.mode == "src" and (op.comp != "MEAN" or on):
                B = self._blocked_blocks(t, "src", 0)
            elif col and v.mode == "dst" and op.comp != "MEAN":
                B = self._blocked_blocks(t, "src", 0, g)
        if B:
            tb = t if col else self._gather_cast(t)
            nbytes = self._gather_bytes(E, n_out, F, tb.element_size())
            if op.comp == "MEAN":
                y = ops.aggregate_blocked(g, tb, None, row_scale=_mean_scale(g), blocks=B)
            else:
                y = ops.reduce_blocked(g, tb, op.comp, blocks=B)
        elif op.comp == "MEAN":
            y = ops.aggregate(g, t, mode, None, row_scale=_mean_scale(g), plan=self._plan())
        else:
            y = ops.reduce(g, t, op.comp, mode, plan=self._plan())
        self._count(nbytes)
        return NodeT(y)

    def _would_block(self, comp, v, t, g, col):
        """_eval_reduce's column-blocked gate for one gather of COMP_TYPE comp reading v (table t)."""
        if not (self.reduce_blocked and isinstance(v, Scat)) or comp in MOMENTS:
            return False
        if not col and v.mode == "src" and (comp != "MEAN" or self.gather_dtype == torch.bfloat16):
            return bool(self._blocked_blocks(t, "src", 0))
        if col and v.mode == "dst" and comp != "MEAN":
            return bool(self._blocked_blocks(t, "src", 0, g))
        return False

    def _multi_wanted(self, group, v, t, g, col):
        """The group launch runs row-chunked only.  Where every member would take the column-blocked
        form on its own, the one pass replaces len(group) cheaper ones: from MULTI_MIN_BLOCKED members."""
        if len(group) >= MULTI_MIN_BLOCKED:
            return True
        return not all(self._would_block(self.g.ops[i].comp, v, t, g, col) for i in group)

    def _eval_multi(self, op, group, g, t, mode, n_out, index, row_es):
        """Every gather of op's sibling group from ONE ops.reduce_multi launch (op: the first of them
        to be evaluated); the others find their value in _multi_vals.  Bytes: the operand read once,
        one output per member."""
        reds = tuple(self.g.ops[i].comp for i in group)
        ys = ops.reduce_multi(g, t, reds, mode, plan=self._plan(), std_eps=self.std_eps)
        E, F = self.graph.nnz, t.shape[1]
        self._count(self._gather_bytes(E, n_out, F, row_es, index=index) + (len(group) - 1) * n_out * 4 * F)
        for i, y in zip(group, ys):
            if i != op.idx:
                self._multi_vals[i] = NodeT(y)
        return NodeT(ys[group.index(op.idx)])

    def _weighted_aggregate(self, u, v, acc=None, self_term=None, out_dtype=torch.float32, order="R"):
        """sum_e u(e) (.) v(e) over each output node's edges (_site): the wider operand is the feature
        row, the narrower the (head) weight.  self_term: see _eval_gather (None back if this form
        cannot take it).  ORDER C reads the weight in CSC order through one permuting copy, and
        gives None back (the caller then forms the product) where ORDER R forms an operand or raises."""
        E, col = self.graph.nnz, order == "C"
        x, w = (u, v) if self._width(u) >= self._width(v) else (v, u)
        if col and (isinstance(x, (tuple, Deferred)) or isinstance(w, Deferred)):
            return None
        if isinstance(w, tuple) and w[0] == "row":  # constant row weight: aggregate then scale (linear)
            if self_term is not None:
                return None
            g, xt, mode, n_out = self._site(x, order)
            y = ops.aggregate(g, xt, mode, None, plan=self._plan())
            if col:  # (ORDER R has never charged this aggregate: DESIGN.md §1.1)
                self._count(self._gather_bytes(E, n_out, y.shape[1], 4))
            return ops.apply_node("MUL", None, y, w[1], b_broadcast_row=True)
        wt = self._to_edge_tensor(w)
        if col:
            if wt.dtype != torch.float32 or self._width(x) % wt.shape[1]:
                return None
            wt = ops.apply_edge(ops.csc(self.graph).view("edge"), None, None, wt, "src")  # wt[perm[k]]: CSC order, once
        g, xt, mode, n_out = self._site(x, order)
        F, H = xt.shape[1], wt.shape[1]
        if col:
            # column-blocked like direction R when the table is large, but only for a scatter R over the "dst" view
            if isinstance(x, Scat) and x.mode == "dst":
                y = self._spmm(xt, "src", wt, graph=g)
            else:
                y = ops.aggregate(g, xt, "src", wt, plan=self._plan())
            self._count(E * 8 * H + self._gather_bytes(E, n_out, F, xt.element_size(), heads=H))  # the permuting copy too
            return y
        if F % H:
            raise ValueError(f"weighted aggregate: weight width {H} does not divide {F}")
        y = self._spmm(xt, mode, wt, acc, self_term, out_dtype)
        if y is None:
            return None
        self._count(self._gather_bytes(E, n_out, F, xt.element_size(), heads=H, out_es=y.element_size()))
        return y

    def _spmm(self, xt, mode, wt, acc=None, self_term=None, out_dtype=torch.float32, graph=None):
        """SpMM-form aggregate: column-blocked when the gathered table outgrows L2, else row-chunked.
        self_term (x, s): y = x * s + the aggregate in one launch (row-chunked form; None back when
        x's dtype is not the gathered table's, or when the column-blocked form is the better one:
        the caller then accumulates into the formed x * s instead).  graph: the graph the rows
        and indices come from (default the layer's CSR; a CSC view for the ORDER-C gathers)."""
        g = self.graph if graph is None else graph
        B = self._blocked_blocks(xt, mode, 0 if wt is None else wt.shape[1], g)
        if B and self_term is None and graph is None:
            xb = self._gather_cast(xt)
            if xb is not xt:  # the callers count xt's rows per edge: take off what the narrower rows save
                self.alg_bytes -= g.nnz * xt.shape[1] * (xt.element_size() - xb.element_size())
                xt = xb
        if self_term is not None:
            xs, sc = self_term
            if B or xs.dtype != xt.dtype or xs.shape[1] != xt.shape[1] or xs.shape[0] < g.n_rows:
                return None
            return ops.aggregate(g, xt, mode, wt, plan=self._plan(), self_term=(xs, sc), out_dtype=out_dtype)
        if B:
            return ops.aggregate_blocked(g, xt, wt, out=acc, accumulate=acc is not None, blocks=B)
        return ops.aggregate(g, xt, mode, wt, out=acc, accumulate=acc is not None, plan=self._plan())

    def _blocked_blocks(self, xt, mode, heads, graph=None):
        """Column blocks of the blocked aggregate for this gathered table, or 0 for the row-chunked
        form: a source table of at least blocked_min_table_bytes (its own element size) of a dtype
        and width the blocked kernels take."""
        g = self.graph if graph is None else graph
        # the table as it will be gathered: with gather_dtype bf16, _spmm rounds an fp32 table of the
        # layer's own CSR (not of the ORDER-C views) to bf16, and a bf16 table is taken as it is; with
        # the option off only fp32 tables take the blocked form
        on = self.gather_dtype == torch.bfloat16
        dt = torch.bfloat16 if on and xt.dtype == torch.float32 and graph is None else xt.dtype
        es = 2 if dt == torch.bfloat16 else xt.element_size()
        if not (mode == "src" and self.blocked_blocks and (dt == torch.float32 or (on and dt == torch.bfloat16))
                and xt.shape[0] * xt.shape[1] * es >= self.blocked_min_table_bytes
                and ops.BlockedPlan.supports(xt.shape[1], heads, dt)):
            return 0
        B = self.blocked_blocks
        if B == "auto":
            B = ops.BlockedPlan.auto_blocks(g, xt.shape[1], es)
            B = B if B >= 4 else 0
        return B if B and g.blocked_plan(B).sorted else 0

    def _gather_cast(self, t):
        """The node table t as the blocked kernels gather it under gather_dtype: t itself (no option,
        or t already of that type), else its RNE rounding to bf16 -- made once per table value and
        shared by its consumers (_memo: identity and version checked)."""
        if self.gather_dtype != torch.bfloat16 or t.dtype != torch.float32:
            return t
        def cast():
            self._count(t.shape[0] * t.shape[1] * 6)
            self.gather_casts += 1
            return ops.pitched(t.to(torch.bfloat16))
        return _memo(self._gather_cache, id(t), t, cast)

    def _eval_applynode(self, op, post_sf=None):
        if self.gather_acc and post_sf is None and op.idx in self.gacc:
            y = self._eval_gather_acc(op)
            if y is not None:
                self._count(self.n_nodes * y.t.shape[1] * 4)  # the aggregate's extra read of T
                return y
        ins = self._inputs(op)
        n = self.n_nodes
        if op.comp == "MM":
            W = self.tensors[f"w:{op.idx}"]
            x = self._node(ins[0])
            return NodeT(self._node_gemm(x, op.idx, W, post_sf))
        if op.comp == "SF":
            a = self._node(ins[0])
            y = ops.apply_node(None, self.sem.sf_of(op), a)
            self._count(n * a.shape[1] * 8)
            return NodeT(y)
        bin_ = self._binary(op)
        ins = self._pair(op, ins)
        if len(ins) == 1:
            return NodeT(self._node(ins[0]))
        x, y = ins[0], ins[1]
        if bin_ == "RDIV":
            x, y, bin_ = y, x, "DIV"
        if isinstance(x, tuple) and bin_ in ("ADD", "MUL"):
            x, y = y, x
        a = self._node(x)
        brow = isinstance(y, tuple)
        b = y[1] if brow else self._node(y)
        out = ops.apply_node(bin_, post_sf, a, b, b_broadcast_row=brow)
        self._count(n * out.shape[1] * 4 * 3)
        return NodeT(out)

    def _node(self, v):
        if isinstance(v, NodeT):
            return v.t
        if isinstance(v, tuple) and v[0] == "row":
            return v[1].expand(self.n_nodes, v[1].shape[1]).contiguous()
        raise TypeError(f"applynode operand is not a node tensor ({type(v).__name__})")

    def _eval(self, op, block, expr=True):
        if expr and self.edge_expr and op.idx in self.expr_nodes:
            # a node of a fused expression tree: its gather runs it; computed unfused only if read
            return Lazy(lambda: _forced(self._eval(op, block, expr=False)))
        fused_into = {p: c for p, c, _ in block.fused}
        if op.type == "scatter":
            src = self.g.inputs[op.idx][0]
            if src.kind == "op" and self._pending(src.op):  # keep a fused-away producer unforced
                raw = self.values[src.op]
                return Lazy(lambda: (raw.force(), self._eval(op, block))[1])
            v = self._source(op, 0)
            if isinstance(v, tuple):
                v = NodeT(self._node(v))
            if not isinstance(v, NodeT):
                raise TypeError(f"scatter op {op.idx} needs a node tensor")
            t, fill, own = v.t, None, None
            if self.dist is not None:  # row shards fill source tables lazily; column shards gather dst rows
                if op.order == "C":
                    fill = self.dist.src_fill
                    if src.kind != "op":  # a model input the rank may hold whole
                        key = f"ext:{op.idx}:0"
                        own = self.dist.replicated(key if key in self.tensors else "x")
                else:
                    t = self.dist.gather_rows(t)
            s = Scat(t, "src" if op.order == "C" else "dst", fill, own)
            # a STORE_E'd scatter is only materialised when nothing reads it back (a sink):
            # every consumer kernel gathers by index, which is the same bytes
            if op.idx in block.stored and not (self.elide_scatter_stores and self.consumers[op.idx]):
                return EdgeT(self._to_edge_tensor(s))
            return s
        if self.softmax_shift and not self.fuse_softmax and op.idx in self.softmax \
                and self.sem.sf_of(self.g.ops[self.softmax[op.idx]["V"]]) in SHIFT_SFS:
            raise NotImplementedError(
                f"op {op.idx}: softmax_shift on column shards (a row's maximum spans ranks); row-local shards work")
        if self.fuse_softmax and op.idx in self.softmax:
            v = self._eval_softmax(op, self.softmax[op.idx])
            if v is not None:
                return v
        if self.mm_pushdown and op.idx in self.pushdown:
            return Lazy(lambda: self._eval_applyedge(op))  # its MM consumer computes through the sum
        if self.fuse_attention and op.idx in self.attn and fused_into.get(op.idx) is None:
            return Lazy(lambda: self._eval_applyedge(op))  # its gather consumer runs the fused kernel
        if op.type == "applyedge":
            c = fused_into.get(op.idx)
            if c is not None and self.g.ops[c].type == "gather" and op.comp in ("MUL", "MM"):
                return Deferred(op.idx)
        if op.type == "applynode" and op.comp == "MM":
            v = self._eval_mlp(op)
            if v is not None:
                return v
        sf_child = self._sf_child(op, block)
        if sf_child is not None:
            ev = self._eval_applyedge if op.type == "applyedge" else self._eval_applynode
            self.values[sf_child.idx] = ev(op, post_sf=self.sem.sf_of(sf_child))
            return Lazy(lambda: ev(op))
        if op.type == "applyedge":
            return self._eval_applyedge(op)
        if op.type == "gather":
            if self.edge_expr and op.idx in self.expr:
                v = self._eval_edge_expr(op)
                if v is not None:
                    return v
            if self.gather_acc and any(g == op.idx for g, _, _ in self.gacc.values()):
                return Lazy(lambda: self._gather_value(op))  # its ADD consumer accumulates it
            if self.mm_first and op.idx in self.two_hop:
                return Lazy(lambda: self._gather_value(op))  # the second hop's MM-first form runs it
            if self.mm_first and op.idx in self.reorder:
                v = self._eval_mm_first(op, self.g.ops[self.reorder[op.idx]])
                if v is not None:
                    return v
            v = self._attention_with_sf(op, block)
            if v is not None:
                return v
            return self._gather_value(op)
        if op.type == "applynode":
            if self.mlp_bf16_sum and self.gather_acc and op.idx in self.gacc and self._mlp_input(op) is not None:
                return Lazy(lambda: self._eval_applynode(op))  # the MLP it feeds may take it in bf16
            if self.gather_acc and op.idx in self.gacc_t and self._self_term(op) is not None:
                return Lazy(lambda: self._eval_applynode(op))  # its ADD consumer's aggregate may form it
            return self._eval_applynode(op)
        raise ValueError(op.type)

    def _attention_with_sf(self, op, block):
        """An attention gather whose only consumer is an applynode SF (GAT op 12 -> op 13): one fused
        launch writes the SF's value (the reduce applies it as y is stored, bitwise what apply_node
        computes); the gather's own value stays available, recomputed unfused if read.  The SF may sit
        in a later block (GAT Reddit's stream puts op 13 in a block of its own): its block then finds
        the value present, as for any fused post-op."""
        if not (self.fuse_sf and self.fuse_attention) or self.dist is not None or op.order != "R":
            return None
        src = self.g.inputs[op.idx][0]
        if src.kind != "op" or src.op not in self.attn or not isinstance(self.values.get(src.op), (Deferred, Lazy)):
            return None
        cons = self.consumers[op.idx]
        if len(cons) != 1:
            return None
        c = self.g.ops[cons[0]]
        if c.comp != "SF" or c.type != "applynode" or len(self.g.inputs[c.idx]) != 1:
            return None
        y = self._eval_attention(op, src.op, sf_out=self.sem.sf_of(c))
        if y is None:
            return None
        self.values[c.idx] = y
        return Lazy(lambda: self._gather_value(op))

    def _only_consumer(self, op, comp):
        """op's single consumer when it is an applynode of kind comp reading only op, else None."""
        cons = self.consumers[op.idx]
        if len(cons) != 1:
            return None
        c = self.g.ops[cons[0]]
        if c.type != "applynode" or c.comp != comp or len(self.g.inputs[c.idx]) != 1 or self._ext(c, 1) is not None:
            return None
        return c

    def _mlp_chain(self, a):
        """(b, c, d) of a chain a -> [SF b] -> MM c -> [SF d] of node GEMMs, each intermediate read
        only by the next op, with weights gta_update_mlp takes; else None."""
        if not (self.fuse_mlp and a.type == "applynode" and a.comp == "MM" and len(self.g.inputs[a.idx]) == 1):
            return None
        b = self._only_consumer(a, "SF") if self.fuse_sf else None
        c = self._only_consumer(b if b is not None else a, "MM")
        if c is None:
            return None
        d = self._only_consumer(c, "SF") if self.fuse_sf else None
        w1, w2 = self.tensors[f"w:{a.idx}"], self.tensors[f"w:{c.idx}"]
        return (b, c, d) if ops.update_mlp_weights_ok(w1.shape[0], w1, w2) else None

    def _mlp_input(self, A):
        """The MLP head a when node op A's only consumer heads a fusable MLP chain, else None."""
        a = self._only_consumer(A, "MM")
        return a if a is not None and self._mlp_chain(a) is not None else None

    def _eval_mlp(self, a):
        """Two chained node GEMMs a -> [SF b] -> MM c -> [SF d] (GIN's MLP, genGraphOP.py:103-108)
        as one gta_update_mlp launch when the shapes allow it (fp32 or bf16 x, bf16 weights, widths
        <= 128).  When a's input is the still-unformed GIN sum A = (1 + eps) x + aggregate, the
        aggregate stores A in bf16 (ABI 10): the MLP rounds an fp32 x to bf16 anyway, so the bits
        are unchanged and A's [N, F] write and read halve.  The chain's last value is set; A, a, b
        and c stay available, recomputed unfused (fp32) if something reads them (the tests read
        them all).  None when the chain or its operands do not fit."""
        chain = self._mlp_chain(a)
        if chain is None:
            return None
        b, c, d = chain
        w1, w2 = self.tensors[f"w:{a.idx}"], self.tensors[f"w:{c.idx}"]
        x = None
        src = self.g.inputs[a.idx][0]
        if self.mlp_bf16_sum and self.gather_acc and src.kind == "op" and src.op in self.gacc:
            if self._pending(src.op):
                y = self._eval_gather_acc(self.g.ops[src.op], out_dtype=torch.bfloat16)
                if y is not None and ops.update_mlp_supported(y.t, w1, w2):
                    x = y.t
        if x is None:
            x = self._node(self._inputs(a)[0])
            if not ops.update_mlp_supported(x, w1, w2):
                return None
        sf1 = self.sem.sf_of(b) if b is not None else None
        sf2 = self.sem.sf_of(d) if d is not None else None
        out = ops.update_mlp(x, w1, w2, sf1=sf1, sf2=sf2)
        self._count(x.shape[0] * (x.shape[1] * x.element_size() + w2.shape[1] * 4) + w1.numel() * 2 + w2.numel() * 2)
        self.values[(d if d is not None else c).idx] = NodeT(out)
        if d is not None:
            self.values[c.idx] = Lazy(lambda: self._eval_applynode(c))
        if b is not None:
            self.values[b.idx] = Lazy(lambda: self._eval_applynode(a, post_sf=sf1))
        return Lazy(lambda: self._eval_applynode(a))

    def _sf_child(self, op, block):
        """The SF op this op's output feeds exclusively (same kind, same block), if fusable."""
        if not self.fuse_sf or op.type not in ("applyedge", "applynode") or op.comp == "SF" or not op.out_list:
            return None
        cons = self.consumers[op.idx]
        if len(cons) != 1:
            return None
        c = self.g.ops[cons[0]]
        if c.comp != "SF" or c.type != op.type or c.idx not in block.ops:
            return None
        if op.comp in ("ADD", "MUL") and len(self.g.inputs[op.idx]) < 2 and self._ext(op, 1) is None:
            return None  # identity pass-through: no kernel to carry the post-op
        return c

    # ---------------------------------------------------------------- run
    def block_order(self):
        owner = {}
        for b in self.stream.blocks:
            for o in b.ops:
                owner.setdefault(o, b.index)
        deps = {b.index: set() for b in self.stream.blocks}
        for b in self.stream.blocks:
            for o in b.ops:
                for p in self.g.producers(o):
                    if p in owner and owner[p] != b.index:
                        deps[b.index].add(owner[p])
        order, done = [], set()
        pending = [b.index for b in self.stream.blocks]
        while pending:
            for i in pending:
                if deps[i] <= done:
                    order.append(i)
                    done.add(i)
                    pending.remove(i)
                    break
            else:
                raise ValueError(f"stream blocks have a cyclic dependency: {pending}")
        return order

    def run(self):
        covered = set()
        for b in self.stream.blocks:
            covered.update(b.ops)
        missing = set(range(len(self.g))) - covered
        if missing:
            raise ValueError(f"stream does not cover ops {sorted(missing)}")
        tracer = _Tracer(self) if self.trace else None
        for bi in self.block_order():
            block = self.stream.blocks[bi]
            for i in self.g.topo(block.ops):
                if i in self.values:  # produced early as a fused post-op
                    continue
                if tracer:
                    tracer.begin()
                self.values[i] = self._eval(self.g.ops[i], block)
                if tracer:
                    tracer.end(i, block)
        if tracer:
            self.trace_events = tracer.events()
        outputs = {}
        for op in self.g.ops:
            if not op.out_list:
                v = self.values[op.idx]
                outputs[op.idx] = self._final(v)
        return outputs

    def _final(self, v):
        if isinstance(v, Lazy):
            v = v.force()
        if isinstance(v, (NodeT, EdgeT)):
            return v.t
        if isinstance(v, Scat):
            return self._to_edge_tensor(v)
        if isinstance(v, Deferred):
            return self._materialize_deferred(v).t
        return v

    def tensor_of(self, op_idx):
        return self._final(self.values[op_idx])


class _Tracer:
    """Brackets each op evaluation with HIP events on the current stream (host clock on CPU)."""

    def __init__(self, ex):
        self.ex = ex
        dev = ex.graph.device if ex.graph is not None else torch.device("cpu")
        self.cuda = dev.type == "cuda"
        self.dev = dev
        self.recs = []
        self.t0 = self._mark()

    def _mark(self):
        if self.cuda:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(self.dev))
            return e
        return time.perf_counter()

    def _us(self, a, b):
        if self.cuda:
            return a.elapsed_time(b) * 1e3
        return (b - a) * 1e6

    def begin(self):
        self.cur = (self._mark(), self.ex.alg_bytes, self.ex.launches)

    def end(self, i, block):
        m0, b0, l0 = self.cur
        self.recs.append((i, block, m0, self._mark(), self.ex.alg_bytes - b0, self.ex.launches - l0))

    def events(self):
        if self.cuda:
            torch.cuda.synchronize(self.dev)
        out = []
        for i, block, m0, m1, nbytes, nl in self.recs:
            op = self.ex.g.ops[i]
            insts = [ins for ins in getattr(block, "insts", []) if ins.kind == "comp" and
                     any(p[0] == i for p in ins.parts)]
            name = insts[0].type if insts else f"{op.type.upper()}_{op.comp}"
            cat = insts[0].id if insts else f"{i}_{op.type}_0"
            out.append({"name": name, "cat": cat, "ph": "X", "ts": self._us(self.t0, m0),
                        "dur": self._us(m0, m1), "pid": "MI355X", "tid": f"block {block.index}",
                        "args": {"op": i, "alg_bytes": nbytes, "launches": nl}})
        return out


def save_chrome_trace(events, path):
    """Chrome trace JSON (chrome://tracing, Perfetto), as the reference's save_timeline_to_json."""
    import json
    import os
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(events, f, indent=1)


def aggregate_trace(events):
    """{name: (count, total µs, total algorithmic bytes)} -- the reference's aggregate_timeline /
    aggregate_rw_record (code/simulator.py:107-146) over measured events."""
    agg = {}
    for e in events:
        c, t, b = agg.get(e["name"], (0, 0.0, 0))
        agg[e["name"]] = (c + 1, t + e["dur"], b + e["args"]["alg_bytes"])
    return agg


# Repeated calls replay a HIP graph (execute() / run_stream / pipeline.Layer.run): the second call
# with the same op graph, stream, CSR and input tensors (same objects; their CONTENTS may change in
# place) captures the whole stream execution once (GraphedRun) and every later call replays it --
# one graph launch instead of one Python-driven launch per op, which is what small layers (Cora,
# Flickr) are bound by, and no host gaps between the kernels of large ones (round 4, every size:
# GAT Reddit 5.61 -> 5.30 ms, GraphSAGE Reddit 4.84 -> 4.73, GIN products 6.54 -> 6.47,
# profiles/r04/layer_bench_graph_all.log).  The outputs of a replayed call are the graph's own
# tensors: the next call with the same inputs overwrites them (clone what must survive it).  A
# captured graph keeps its intermediates in a private memory pool (a few GB for the Reddit-scale
# layers, against 288 GB of HBM); AUTO_GRAPH_MAX_EDGES bounds the graphs it applies to,
# AUTO_GRAPH = False turns it off (set_auto_graph(False) also drops every captured graph).  A replay is keyed by the objects AND their storage (data_ptr,
# shape, stride), the calling thread's libgta knob state (ops.knob_state) and stays eager on a stream with an attached
# knob set; weights changed in place are re-transposed into the graph's W^T before the replay.
FUSE_MLP = True  # default of Executor.fuse_mlp (layer benches A/B it)
MLP_BF16_SUM = True  # default of Executor.mlp_bf16_sum: GIN's sum stored in bf16 for the fused MLP (ABI 10)
AUTO_GRAPH = True
AUTO_GRAPH_MAX_EDGES = 1 << 40  # every graph (round 3: 1 << 23, launch-bound layers only)
AUTO_GRAPH_MAX_ENTRIES = 32
AUTO_GRAPH_MAX_POOL_BYTES = 64 << 30  # private pools of all captured graphs together: the
                                      # largest other entries are dropped beyond it
_AUTO = {}


class _AutoEntry:
    def __init__(self, refs, tensors):
        self.refs, self.tensors = refs, tensors  # strong references: ids and addresses stay unique
        self.ptrs = {k: t.data_ptr() for k, t in tensors.items()}
        self.src = None                          # the caller's dict last seen with these tensors
        self.calls, self.run, self.failed = 0, None, False
        self.pool_bytes = 0                      # device memory the capture reserved (its private pool)
        self.last_use = 0                        # _AUTO_CLOCK value of the latest call (LRU eviction)
        self.evicted = False                     # its graph was dropped for room: it stays eager from then on


_AUTO_CLOCK = [0]
_AUTO_FAST = {}  # (ids of the call's objects, id of its tensors dict, knob state) -> entry: the per-call lookup


def clear_auto_graphs():
    """Drop every captured graph (and the inputs, CSRs and memory pools they hold)."""
    _AUTO.clear()
    _AUTO_FAST.clear()


def set_auto_graph(flag):
    global AUTO_GRAPH
    AUTO_GRAPH = bool(flag)
    if not AUTO_GRAPH:
        clear_auto_graphs()


def _auto_graph(opgraph, stream, graph, tensors, semantics, plan_chunk, softmax_shift=None, gather_dtype=None):
    """-> a GraphedRun to replay for this call, or None (run eagerly)."""
    if ops.Tuning.attached(torch.cuda.current_stream(graph.device)):
        return None  # a knob set on this stream: every call reads it (gta.h), so no cached graph
    refs = (opgraph, stream, graph, semantics)
    shifted = SOFTMAX_SHIFT if softmax_shift is None else bool(softmax_shift)
    gdt = None if gather_dtype == torch.float32 else gather_dtype
    fkey = (id(opgraph), id(stream), id(graph), id(semantics), (plan_chunk, shifted, gdt), id(tensors), ops.knob_state())
    ent = _AUTO_FAST.get(fkey)
    if ent is not None and not (ent.src is tensors and all(a is b for a, b in zip(ent.refs, refs)) and
                                len(tensors) == len(ent.tensors) and
                                all(tensors.get(k) is t and t.data_ptr() == ent.ptrs[k]
                                    for k, t in ent.tensors.items())):
        ent = None
    if ent is None:
        if not all(torch.is_tensor(t) and t.is_cuda for t in tensors.values()):
            return None
        key = fkey[:5] + (fkey[6],
                          tuple(sorted((k, id(t), t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)
                                       for k, t in tensors.items())))
        ent = _AUTO.get(key)
        if ent is not None and not all(a is b for a, b in zip(ent.refs, refs)):
            ent = None
        if ent is None:
            if len(_AUTO) >= AUTO_GRAPH_MAX_ENTRIES:
                _AUTO.pop(next(iter(_AUTO)))
                _AUTO_FAST.clear()
            ent = _AUTO[key] = _AutoEntry(refs, dict(tensors))
        ent.src = tensors
        if len(_AUTO_FAST) >= 4 * AUTO_GRAPH_MAX_ENTRIES:
            _AUTO_FAST.clear()
        _AUTO_FAST[fkey] = ent
    ent.calls += 1
    _AUTO_CLOCK[0] += 1
    ent.last_use = _AUTO_CLOCK[0]
    if ent.failed or ent.evicted or ent.calls < 2:
        return None
    if ent.run is None:
        before = torch.cuda.memory_reserved(graph.device)
        try:
            ent.run = GraphedRun(opgraph, stream, graph, ent.tensors, semantics, plan_chunk, warmup=1,
                                 softmax_shift=shifted, gather_dtype=gdt)
        except Exception:  # something in this stream is not capturable: stay eager for this key
            ent.failed = True
            torch.cuda.synchronize(graph.device)
            return None
        ent.pool_bytes = max(0, torch.cuda.memory_reserved(graph.device) - before)
        _evict_pools(keep=ent)
    return ent.run


def _evict_pools(keep):
    """Keep the captured graphs' pools within AUTO_GRAPH_MAX_POOL_BYTES (a Reddit / products-sized
    layer holds GBs of intermediates): drop the graphs of the least recently used entries other than
    `keep`, and mark those entries to stay eager.  (deleting the largest other entry made
    two large alternating layers evict each other on every capture and recapture two calls later --
    repeated captures and warm-ups instead of replays.  An evicted entry keeps its call history, so
    it is never recaptured.)  pool_bytes is the memory_reserved() growth across the capture: the
    caching allocator's view, which may under-count a pool that reused freed blocks."""
    total = sum(e.pool_bytes for e in _AUTO.values() if e.run is not None)
    while total > AUTO_GRAPH_MAX_POOL_BYTES:
        victims = [(e.last_use, i, e) for i, e in enumerate(_AUTO.values()) if e.run is not None and e is not keep]
        if not victims:
            break
        _, _, e = min(victims)
        total -= e.pool_bytes
        e.run, e.evicted = None, True


def run_stream(opgraph, stream, graph, tensors, semantics=None, plan_chunk=512, sync=True, trace=False,
               softmax_shift=None, gather_dtype=None):
    """softmax_shift: Executor.softmax_shift for this call (None: the module's SOFTMAX_SHIFT).
    gather_dtype: Executor.gather_dtype for this call (None: tables are gathered as they are)."""
    dev = graph.device
    if not AUTO_GRAPH and _AUTO:
        clear_auto_graphs()
    if AUTO_GRAPH and not trace and dev.type == "cuda" and graph.nnz <= AUTO_GRAPH_MAX_EDGES:
        gr = _auto_graph(opgraph, stream, graph, tensors, semantics, plan_chunk, softmax_shift, gather_dtype)
        if gr is not None:
            if sync:
                torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            outputs = gr.replay()
            if sync:
                torch.cuda.synchronize(dev)
            ex = gr.executor
            return ExecResult(ex.values, outputs, time.perf_counter() - t0, ex.alg_bytes, ex.launches), ex
    ex = Executor(opgraph, stream, graph, tensors, semantics, plan_chunk, softmax_shift=softmax_shift,
                  gather_dtype=gather_dtype)
    ex.trace = trace
    sync = sync and dev.type == "cuda"
    if sync:
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    outputs = ex.run()
    if sync:
        torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    return ExecResult(ex.values, outputs, dt, ex.alg_bytes, ex.launches), ex


def _tiles_for(graph, sparse=True):
    """T -> the tile counts of graph for the cost model, cached on the graph object like its plans:
    sparse (tiles.sparse_counts, O(E)) for the closed-form per-instruction model, or the dense flat
    list (gta_tile_nnz on the GPU, row-major [ceil(N/T)][n_cols]) the cycle loop walks.  Like the
    reference's dense adjacency they count a repeated (dst, src) once when rows are column-sorted."""
    from . import tiles
    cache = graph.__dict__.setdefault("_tile_nnz_cache", {})

    def tiles_for(T):
        key = (T, sparse)
        if key not in cache:
            cache[key] = (tiles.sparse_counts(graph, int(T)) if sparse
                          else ops.tile_nnz(graph, int(T)).flatten().cpu().numpy().astype(np.int64))
        return cache[key]
    return tiles_for


def attach_model(res, stream_records, tile_size_list, graph, model="rw", isSinput=False, dataset=None):
    """The reference's modelled numbers for the stream just executed (simulate(), code/simulator.py:370-502):
      "rw"   res.model_rw, the closed form (one tile-count pass at T = N);
      "inst" also res.model_insts, the per-instruction model (costmodel.per_instruction: each
             instruction's rw_record bytes and unit-busy cycles, closed form over sparse tile counts:
             runs at Reddit / products scale), res.model_rw its sum;
      "full" also res.model_cycles and res.model_spans via the exact cycle-loop restatement
             (costmodel.simulate_stream with each instruction's first start / last end; Python
             speed: Cora / Flickr-sized graphs)."""
    from . import costmodel
    if model is None:
        return res
    n = graph.n_rows
    sp = SPARSITY.get(dataset, 1)
    if model == "rw":
        cache = graph.__dict__.setdefault("_tile_nnz_cache", {})
        if ("sum", n) not in cache:
            cache[("sum", n)] = int(ops.tile_nnz(graph, n).sum().item())
        res.model_rw = costmodel.model_rw(stream_records, n, cache[("sum", n)])
        return res
    res.model_insts = costmodel.per_instruction(stream_records, tile_size_list, n, _tiles_for(graph), isSinput, sp)
    res.model_rw = sum(r["rw_bytes"] for r in res.model_insts)
    if model == "full":
        res.model_cycles, rw, res.model_spans = costmodel.simulate_stream(
            stream_records, tile_size_list, n, _tiles_for(graph, sparse=False), isSinput, sp, record=True)
        assert rw == res.model_rw, (rw, res.model_rw)
    return res


def model_trace(res, events=None):
    """The modelled numbers beside the measured Chrome trace.  Every measured op event gets, in
    args.model, the stream instructions that execute it (by the op ids in their IDs) with their
    modelled bytes (rw_record) and unit-busy cycles / µs at the reference's 1 GHz clock
    (code/start.py:56 reports cycles/1e9 s).  With model="full" the modelled timeline is added as
    its own tracks: one event per instruction from its first start to its last end, pid
    "GTA model", tid = the reference's hardware unit (vTCAD/code/simulator.py:360-382 schema)."""
    insts = getattr(res, "model_insts", None) or []
    by_op = {}
    for r in insts:
        for op in {p[0] for p in ir.parse_id(r["ID"])}:
            by_op.setdefault(op, []).append({"TYPE": r["TYPE"], "ID": r["ID"], "bytes": r["record_bytes"],
                                             "busy_cycles": r["busy"], "model_us": r["busy"] / 1e3,
                                             "iterations": r["starts"]})
    out = []
    for e in events or []:
        e = dict(e, args=dict(e["args"]))
        e["args"]["model"] = by_op.get(e["args"]["op"], [])
        out.append(e)
    spans = getattr(res, "model_spans", None)
    if spans:
        for r in insts:
            sp = spans.get((r["block"], r["index"]))
            if sp is None:
                continue
            out.append({"name": r["TYPE"], "cat": r["ID"], "ph": "X", "ts": sp[0] / 1e3, "dur": (sp[2] - sp[0]) / 1e3,
                        "pid": "GTA model", "tid": r["unit"],
                        "args": {"bytes": r["record_bytes"], "busy_cycles": r["busy"], "iterations": r["starts"],
                                 "block": r["block"]}})
    return out


SPARSITY = {"cora": 0.012, "pubmed": 0.1, "flickr": 0.46, "reddit": 1}  # code/simulator.py:381-392


_LOADED = {}


def _load(network, reorder, semantics, op_path, inst_path):
    """(semantics, op graph, stream records, stream) of a layer, kept while its files are unchanged:
    repeated execute() calls then hand run_stream the same objects, so they replay one HIP graph."""
    def stamp(p):
        st = os.stat(p)
        return p, st.st_mtime_ns, st.st_size
    key = (network, bool(reorder), id(semantics), stamp(op_path), stamp(inst_path))
    hit = _LOADED.get(key)
    if hit is None or hit[0] is not semantics:
        sem = semantics or Semantics.for_network(network, reorder)
        g = ir.OpGraph.load(op_path, sem.inputs)
        records = ir.read_yaml(inst_path)
        if len(_LOADED) >= 64:
            _LOADED.clear()
        hit = _LOADED[key] = (semantics, sem, g, records, ir.Stream(records))
    return hit[1:]


ARCHITECTURES = ("GTA", "HyGCN", "GCNAX", "OPU")  # vTCAD/code/simulator.py:489-509


def execute(tile_size_list, dataset, network, layer, isReorder, isSinput=False, isFlexibleHardware=False,
            architecture_name="GTA", *, graph, tensors, inst_root="Results/Insts", op_root="Network", inst_path=None,
            op_path=None, semantics=None, plan_chunk=512, model="rw", trace=None):
    """Drop-in for simulate(tile_size_list, dataset, network, layer, isReorder, isSinput)
    (code/simulator.py:370): same leading arguments, same files, real execution.

    Returns ExecResult: the sink ops' device tensors, measured elapsed_s, and the
    reference's modelled numbers for the same stream (attach_model): model_rw (always, closed
    form), model_insts (model="inst" or "full": per instruction, the bytes simulate() records in
    rw_record and the unit-busy cycles, closed form at any graph size) and model_cycles /
    model_spans (model="full"; exact restatement of the cycle loop, Python-speed, meant for
    Cora/Flickr-sized graphs).  `res.simulate_tuple()` is what simulate() would have returned.
    trace: True (events in res.trace) or a path for a Chrome trace JSON of the measured per-op
    device time, as the reference's chrome_timeline.json, each op event carrying its
    instructions' modelled bytes and cycles (model_trace; model="full" adds the modelled timeline).

    Also takes vTCAD's call, simulate(tile_size_list, dataset, network, layer, isReorder, isSinput,
    isFlexibleHardware, architecture_name) (vTCAD/code/simulator.py:423, called positionally at
    vTCAD/code/test.py:15; bind() gives a callable that takes exactly that line).  The names are
    checked as vTCAD checks them (:489-510: an unknown architecture is an error -- vTCAD returns -1,
    this raises) and kept in res.model_arch.  They select the modelled ASIC, not the execution: the
    GPU runs the same kernels for every architecture, and the modelled numbers restate
    code/simulator.py's fixed-hardware GTA model; vTCAD's other presets and its per-block search
    over flexible unit counts are ASIC design-space models outside the hot path.

    From the second call with the same stream, CSR and input tensor objects on (graphs of at most
    AUTO_GRAPH_MAX_EDGES edges: every graph by default), the execution replays a captured HIP graph: the outputs are then
    the graph's own tensors and the next such call overwrites them -- clone what must outlive it
    (AUTO_GRAPH = False keeps every call eager, with fresh outputs)."""
    if architecture_name not in ARCHITECTURES:
        raise ValueError(f"architecture_name {architecture_name!r}: vTCAD knows {', '.join(ARCHITECTURES)} "
                         "(vTCAD/code/simulator.py:489-510)")
    if not isinstance(isFlexibleHardware, (bool, int)):
        raise TypeError("isFlexibleHardware must be a bool")
    op_path = op_path or ir.op_yaml_path(network, dataset, layer, isReorder, op_root)
    inst_path = inst_path or ir.inst_path(network, dataset, layer, isReorder, inst_root)
    sem, g, records, s = _load(network, isReorder, semantics, op_path, inst_path)
    res, ex = run_stream(g, s, graph, tensors, sem, plan_chunk, trace=trace is not None)
    # a trace carries the per-instruction model beside the measured ops
    attach_model(res, records, tile_size_list, graph, "inst" if (trace is not None and model == "rw") else model,
                 isSinput, dataset)
    if trace is not None:
        res.trace = model_trace(res, ex.trace_events)
        if isinstance(trace, str):
            save_chrome_trace(res.trace, trace)
    # vTCAD turns flexible hardware off for every preset but GTA (:493-507)
    res.model_arch = (architecture_name, bool(isFlexibleHardware) and architecture_name == "GTA")
    return res


def bind(graph, tensors, **kw):
    """A simulate()-shaped callable over one graph and its tensors: bind(g, t)(tile_size_list,
    dataset, network, layer, isReorder, isSinput[, isFlexibleHardware, architecture_name]) -- the
    reference callers' lines (code/start.py:51, code/genetic_algorithm.py:603, vTCAD/code/test.py:15)
    unchanged once `simulate` names it."""
    import functools
    return functools.partial(execute, graph=graph, tensors=tensors, **kw)


class GraphedRun:
    """A stream execution captured once as a HIP graph and replayed (torch.cuda.CUDAGraph is
    hipGraph on ROCm): every libgta launch of the layer is recorded, so a replay costs one graph
    launch instead of one Python-driven launch per op -- the launch-bound small graphs (Cora,
    Flickr) are where it matters.  Inputs are the tensors given here (static addresses: update
    them in place between replays); outputs are the same tensors after every replay.  The
    warm-up run builds every plan, workspace and W^T cache outside the capture.  The graph keeps
    the W^T tensors (and sibling-weight concatenations) it reads alive, and a weight changed in
    place (its version moved) is re-concatenated / re-transposed into them before the next replay."""

    def __init__(self, opgraph, stream, graph, tensors, semantics=None, plan_chunk=512, warmup=2,
                 softmax_shift=None, gather_dtype=None):
        if graph.device.type != "cuda":
            raise RuntimeError("GraphedRun captures device launches: the graph must be on a HIP device")
        self.tensors = tensors
        side = torch.cuda.Stream(graph.device)
        side.wait_stream(torch.cuda.current_stream(graph.device))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                Executor(opgraph, stream, graph, tensors, semantics, plan_chunk, softmax_shift=softmax_shift,
                         gather_dtype=gather_dtype).run()
        torch.cuda.current_stream(graph.device).wait_stream(side)
        torch.cuda.synchronize(graph.device)
        self.cuda_graph = torch.cuda.CUDAGraph()
        del ops._CAPTURED_WT[:]
        del _CAPTURED_WCAT[:]
        try:
            with torch.cuda.graph(self.cuda_graph):
                self.executor = Executor(opgraph, stream, graph, tensors, semantics, plan_chunk,
                                         softmax_shift=softmax_shift, gather_dtype=gather_dtype)
                self.outputs = self.executor.run()
        finally:
            taken, ops._CAPTURED_WT[:] = list(ops._CAPTURED_WT), []
            cats, _CAPTURED_WCAT[:] = list(_CAPTURED_WCAT), []
        # (sibling weights, their concatenation read by the graph, the versions it holds); refreshed
        # before the W^T below, so a re-concatenation moves Wc's version and re-transposes it too
        self._wcats = [[srcs, wc, tuple(w._version for w in srcs)]
                       for srcs, wc in {id(wc): (srcs, wc) for srcs, wc in cats}.values()]
        # (weight, its W^T read by the graph, the weight version that W^T holds)
        self._wts = [[w, wt, w._version] for w, wt in {id(wt): (w, wt) for w, wt in taken}.values()]

    def replay(self):
        for ent in self._wcats:
            srcs, wc, vers = ent
            now = tuple(w._version for w in srcs)
            if now != vers:  # a sibling weight changed in place: re-concatenate into the graph's copy
                wc.copy_(torch.cat(srcs, dim=1))
                ent[2] = now
        for ent in self._wts:
            w, wt, ver = ent
            if w._version != ver:  # changed in place since the capture: refresh the graph's W^T
                wt.copy_(w.t())
                ent[2] = w._version
        self.cuda_graph.replay()
        return self.outputs

