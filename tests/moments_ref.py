"""TEST-ONLY fp64 / numpy reference of the moment reducers MEAN, VAR and STD (gta_reduce_multi).

  moments_seg(seg, vals, first, n_out, eps)  per segment: MEAN and VAR in fp64 by the two-pass
                                   definition (the mean, then the mean of the squared deviations:
                                   the population variance), STD = sqrt(VAR + eps), each with the
                                   bound the project's rule 1e-5 * sum|terms| + 1e-6
                                   (oracle/sampled.py) gives for the SHIFTED form about
                                   k = vals[first[s]] in fp64:
                                     MEAN: T = |k| + (1/d) sum |x - k|
                                     VAR:  T = (1/d) sum (x - k)^2 + ((1/d) sum |x - k|)^2
                                     STD:  VAR's bound / sqrt(VAR + eps) + 1e-6
                                           (|sqrt a - sqrt b| <= |a - b| / sqrt a)
                                   empty segments give 0 in all three
  moments_csr / moments_csc        both DIRECTIONs with the operand read per x_mode (reduce_ref's)
  emulate_f32                      the kernel's arithmetic in numpy float32, edge by edge: the
                                   shifted form, and the naive E[x^2] - E[x]^2 it must not be
  layer_ref                        reduce_ref.layer_ref (wrapped, not edited) with VAR / STD gathers
"""
import numpy as np

from . import reduce_ref

MOMENTS = ("MEAN", "VAR", "STD")
EPS = 1e-5


def bound(terms):
    return 1e-5 * terms + 1e-6


def moments_seg(seg, vals, first, n_out, eps=EPS, vabs=None):
    """{"MEAN" | "VAR" | "STD": (value fp64 [n_out, F], bound fp64 [n_out, F])}.  first[s]: the
    position in vals of segment s's shift (its first edge); ignored for empty segments.
    vabs: None (vals are exact), or the sum of |terms| of every value (an op's output, itself within
    1e-5 * vabs): an error u_e of x_e moves MEAN by mean(u) and VAR = mean((x - m)^2) by
    2 mean((x - m)(u - mean u)) to first order, so T grows by mean(vabs), and by
    2 mean(|x - m| vabs) + 2 mean|x - m| mean(vabs)."""
    vals = np.asarray(vals, np.float64)
    seg = np.asarray(seg, np.int64)
    cnt = np.bincount(seg, minlength=n_out)
    d = np.maximum(cnt, 1)[:, None].astype(np.float64)
    has = (cnt > 0)[:, None]

    def mean_of(v):
        out = np.zeros((n_out, vals.shape[1]))
        np.add.at(out, seg, v)
        return out / d

    mean = mean_of(vals)
    var = mean_of((vals - mean[seg]) ** 2)  # two-pass
    k = np.where(has, vals[np.where(cnt > 0, np.asarray(first, np.int64), 0)], 0.0)
    dev = vals - k[seg]
    t_mean = np.abs(k) + mean_of(np.abs(dev))
    t_var = mean_of(dev ** 2) + mean_of(np.abs(dev)) ** 2
    if vabs is not None:
        va = np.asarray(vabs, np.float64)
        adev = np.abs(vals - mean[seg])
        t_mean = t_mean + mean_of(va)
        t_var = t_var + 2 * mean_of(adev * va) + 2 * mean_of(adev) * mean_of(va)
    std = np.sqrt(var + eps)
    b_var = bound(t_var)
    out = {"MEAN": (mean, bound(t_mean)), "VAR": (var, b_var), "STD": (std, b_var / std + 1e-6)}
    return {r: (np.where(has, v, 0.0), b) for r, (v, b) in out.items()}


def moments_csr(indptr, indices, x, x_mode="src", eps=EPS):
    """DIRECTION dst (ORDER R): the shift is the operand at CSR position indptr[i]."""
    ip = np.asarray(indptr, np.int64)
    return moments_seg(reduce_ref.rows_of(ip), reduce_ref.edge_values(ip, indices, x, x_mode), ip[:-1], len(ip) - 1, eps)


def csc_order(indices, n_cols):
    """(perm, colptr): the CSR positions grouped by source, CSR order kept inside a group (a stable
    sort: the order gta_csc_build gives), and the groups' bounds."""
    ix = np.asarray(indices, np.int64)
    perm = np.argsort(ix, kind="stable")
    colptr = np.concatenate([[0], np.cumsum(np.bincount(ix, minlength=n_cols))]).astype(np.int64)
    return perm, colptr


def moments_csc(indptr, indices, n_cols, x, x_mode="edge", eps=EPS):
    """DIRECTION src (ORDER C): segment j = the edges whose source is j; its shift is the operand of
    the first of them in CSR order."""
    perm, colptr = csc_order(indices, n_cols)
    first = perm[np.minimum(colptr[:-1], max(len(perm) - 1, 0))] if len(perm) else np.zeros(n_cols, np.int64)
    return moments_seg(np.asarray(indices, np.int64), reduce_ref.edge_values(indptr, indices, x, x_mode), first, n_cols, eps)


def emulate_f32(indptr, vals, eps=EPS, shifted=True):
    """(MEAN, VAR, STD) float32 [n_rows, F] of the edge values vals [E, F] in fp32 arithmetic, one
    edge after the other.  shifted: s1 = sum (x - k), s2 = sum (x - k)^2 about k = the row's first
    value, MEAN = k + s1/d, VAR = max(s2/d - (s1/d)^2, 0).  Not shifted: the same with k = 0, the
    naive E[x^2] - E[x]^2."""
    ip = np.asarray(indptr, np.int64)
    v = np.asarray(vals, np.float32)
    n, F = len(ip) - 1, v.shape[1]
    mean, var = np.zeros((n, F), np.float32), np.zeros((n, F), np.float32)
    for i in range(n):
        b, e = int(ip[i]), int(ip[i + 1])
        if e == b:
            continue
        k = v[b] if shifted else np.zeros(F, np.float32)
        s1, s2 = np.zeros(F, np.float32), np.zeros(F, np.float32)
        for j in range(b, e):
            d = v[j] - k
            s1 = s1 + d
            s2 = s2 + d * d
        deg = np.float32(e - b)
        m = s1 / deg
        mean[i] = k + m
        var[i] = np.maximum(s2 / deg - m * m, np.float32(0))
    std = np.where((np.diff(ip) > 0)[:, None], np.sqrt(var + np.float32(eps)), np.float32(0)).astype(np.float32)
    return mean, var, std


def first_of(seg, n_out):
    """int64 [n_out]: the first position of every segment id in seg (0 for an empty segment)."""
    seg = np.asarray(seg, np.int64)
    first = np.full(n_out, len(seg), np.int64)
    np.minimum.at(first, seg, np.arange(len(seg), dtype=np.int64))
    return np.where(first < len(seg), first, 0)


def layer_ref(records, sem, indptr, indices, tensors, patches=None, eps=EPS):
    """reduce_ref.layer_ref for a layer whose gathers may be VAR / STD: the same walk, the same
    rules for every other op.  reduce_ref's walk reduces each gather with two calls of its module's
    segment() -- the values, then the |terms| -- in data-flow order; for the time of the walk that
    name is bound to a function that answers the two calls of a moment gather from moments_seg
    (the value; then T with bound = 1e-5 T + 1e-6, the operand's own |terms| included) and hands
    every other call to the real one.  The records it walks name those gathers MEAN, a reducer the
    walk knows; nothing else about them differs."""
    order = [i for i in reduce_ref.opgraph_ref.topo(records, patches) if records[i]["TYPE"] == "gather"]
    kinds = [records[i].get("COMP_TYPE") for i in order]
    if not any(k in ("VAR", "STD") for k in kinds):
        return reduce_ref.layer_ref(records, sem, indptr, indices, tensors, patches)
    renamed = [dict(r, COMP_TYPE="MEAN") if r["TYPE"] == "gather" and r.get("COMP_TYPE") in ("VAR", "STD") else r
               for r in records]
    real = reduce_ref.segment
    state = {"calls": 0, "a": None}

    def segment(seg, vals, n_out, red):
        g, second = divmod(state["calls"], 2)
        state["calls"] += 1
        if kinds[g] not in ("VAR", "STD"):
            return real(seg, vals, n_out, red)
        if not second:
            state["a"] = np.array(vals, np.float64)
            return moments_seg(seg, state["a"], first_of(seg, n_out), n_out, eps)[kinds[g]][0]
        _, b = moments_seg(seg, state["a"], first_of(seg, n_out), n_out, eps, vabs=vals)[kinds[g]]
        return (b - 1e-6) / 1e-5

    reduce_ref.segment = segment
    try:
        vals = reduce_ref.layer_ref(renamed, sem, indptr, indices, tensors, patches)
    finally:
        reduce_ref.segment = real
    assert state["calls"] == 2 * len(order), "reduce_ref.layer_ref no longer reduces a gather with two segment() calls"
    return vals
