"""TEST-ONLY fp64 / numpy reference of the gather reducers MAX, MIN and MEAN (and ADD).

The oracle (oracle/isa_ref.py, oracle/exec_ref.py) sums every gather, whatever its COMP_TYPE, and
is left as it is; the reducers' reference lives here:

  segment(seg, vals, n_out, red)   red over the values of each segment id (np.maximum.at /
                                   np.minimum.at on a -inf / +inf fill -- not reduceat, which
                                   mishandles empty segments); empty segments give 0; NaN propagates
  reduce_csr / reduce_csc          the ISA gather of both DIRECTIONs with the operand read per x_mode
  layer_ref                        a layer's op graph op by op in fp64 (exec_ref's walk with the
                                   gathers' COMP_TYPE honoured), each value with the sum of |terms|
                                   that the project's bound 1e-5 * sum|terms| + 1e-6 scales by

Values keep the dtype they are given (float32 inputs give bitwise float32 maxima: a max returns one
of its inputs), so MAX / MIN results are compared with `==`.
"""
import numpy as np

from oracle import isa_ref, opgraph_ref

REDS = ("ADD", "MAX", "MIN", "MEAN")


def rows_of(indptr):
    """int64 [E]: the row of every CSR position."""
    indptr = np.asarray(indptr, np.int64)
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))


def segment(seg, vals, n_out, red):
    """out[s] = red over vals[seg == s]; segments without a value give 0 (the ADD gather's value)."""
    vals = np.asarray(vals)
    seg = np.asarray(seg, np.int64)
    cnt = np.bincount(seg, minlength=n_out)
    if red in ("MAX", "MIN"):
        out = np.full((n_out, vals.shape[1]), -np.inf if red == "MAX" else np.inf, vals.dtype)
        (np.maximum if red == "MAX" else np.minimum).at(out, seg, vals)
        out[cnt == 0] = 0
        return out
    out = np.zeros((n_out, vals.shape[1]), np.float64)
    np.add.at(out, seg, np.asarray(vals, np.float64))
    if red == "MEAN":
        out /= np.maximum(cnt, 1)[:, None]
    elif red != "ADD":
        raise ValueError(red)
    return out


def edge_values(indptr, indices, x, x_mode):
    """[E, F]: the operand of every CSR edge, read as gta_aggregate's x_mode reads it."""
    x = np.asarray(x)
    if x_mode == "src":
        return x[np.asarray(indices, np.int64)]
    if x_mode == "dst":
        return x[rows_of(indptr)]
    if x_mode == "edge":
        return x[:len(indices)]
    raise ValueError(x_mode)


def reduce_csr(indptr, indices, x, red, x_mode="src"):
    """DIRECTION dst (ORDER R): y[i] = red over the edges of destination row i; y [n_rows, F]."""
    return segment(rows_of(indptr), edge_values(indptr, indices, x, x_mode), len(indptr) - 1, red)


def reduce_csc(indptr, indices, n_cols, x, red, x_mode="edge"):
    """DIRECTION src (ORDER C): y[j] = red over the edges whose source is j; y [n_cols, F]."""
    return segment(np.asarray(indices, np.int64), edge_values(indptr, indices, x, x_mode), n_cols, red)


class _OpView:  # what Semantics.sf_of / bin_of read
    __slots__ = ("idx", "comp")

    def __init__(self, idx, comp):
        self.idx, self.comp = idx, comp


def layer_ref(records, sem, indptr, indices, tensors, patches=None):
    """{op index: (kind, value fp64, sum of |terms| fp64)} of a layer's op records, every op unfused in
    data-flow order.  A gather reduces with its COMP_TYPE (ADD / MAX / MIN / MEAN), to the destination
    (ORDER R) or the source (ORDER C).  The |terms| of a MAX / MIN are the largest |terms| of its
    segment (a max moves by at most its inputs' largest error and adds none of its own); of a MEAN
    the summed |terms| over the degree; through an MM |x| |W|."""
    ip, ix = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n, e = len(ip) - 1, len(ix)
    flow = opgraph_ref.dataflow(records, patches)
    rows = rows_of(ip)
    vals = {}

    def operand(t):
        t = np.asarray(t, np.float64)
        if t.ndim == 1:
            t = t[:, None]
        kind = "row" if t.shape[0] == 1 else ("edge" if t.shape[0] == e and t.shape[0] != n else
                                              ("node" if t.shape[0] == n else "edge"))
        return kind, t, np.abs(t)

    def src(i, kind_of_op, slot):
        k, ref = flow[i][slot]
        if k == "op":
            return vals[ref]
        key = f"ext:{i}:{slot}"
        if key in tensors:
            return operand(tensors[key])
        if k == "ext":
            raise KeyError(key)
        return operand(tensors["x_edge"] if kind_of_op == "applyedge" else tensors["x"])

    def spread(v, m):  # a (kind, value, abs) triple as m full rows
        return tuple(np.broadcast_to(a, (m, a.shape[1])) if v[0] == "row" else a for a in v[1:])

    for i in opgraph_ref.topo(records, patches):
        r = records[i]
        typ, comp, order = r["TYPE"], r.get("COMP_TYPE", "NONE"), r.get("ORDER", "R")
        if typ == "scatter":
            a, ab = spread(src(i, typ, 0), n)
            pick = rows if order == "R" else ix
            vals[i] = ("edge", a[pick], ab[pick])
        elif typ == "gather":
            a, ab = spread(src(i, typ, 0), e)
            seg, n_out = (ix, n) if order == "C" else (rows, n)
            red = comp if comp in REDS else "ADD"
            y = np.asarray(segment(seg, a, n_out, red), np.float64)
            yab = segment(seg, ab, n_out, {"ADD": "ADD", "MEAN": "MEAN", "MAX": "MAX", "MIN": "MAX"}[red])
            vals[i] = ("node", y, np.asarray(yab, np.float64))
        else:
            kind = "edge" if typ == "applyedge" else "node"
            m = e if kind == "edge" else n
            if comp == "MM":
                a, ab = spread(src(i, typ, 0), m)
                W = np.asarray(tensors[f"w:{i}"], np.float64)
                vals[i] = (kind, a @ W, ab @ np.abs(W))
            elif comp == "SF":
                a, ab = spread(src(i, typ, 0), m)
                y = isa_ref.sf(sem.sf_of(_OpView(i, comp)), a)
                vals[i] = (kind, y, np.maximum(ab, np.abs(y)))
            else:
                b = sem.bin_of(_OpView(i, comp))
                ins = [src(i, typ, s) for s in range(len(flow[i]))]
                if len(ins) == 1 and f"ext:{i}:1" in tensors:
                    ins.append(operand(tensors[f"ext:{i}:1"]))
                if len(ins) == 1:
                    a, ab = spread(ins[0], m)
                    vals[i] = (kind, a.copy(), ab.copy())
                    continue
                (a, aa), (c, ca) = spread(ins[0], m), spread(ins[1], m)
                if b == "RDIV":
                    a, aa, c, ca, b = c, ca, a, aa, "DIV"
                y = isa_ref.binop(b, a, c)
                # the |terms| with the same head broadcast of the narrower operand
                yab = isa_ref.binop({"SUB": "ADD"}.get(b, b), aa, np.abs(c) if b == "DIV" else ca)
                vals[i] = (kind, y, yab)
    return vals
