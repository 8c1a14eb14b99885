"""The executor's graph rewrites, matched: pure functions of the op graph, its consumers map and
Semantics.  No tensor and no kernel is named here; Executor.__init__ calls these once and keeps the
results (executor.py says what each rewrite then runs as).
"""


def consumers_of(g):
    """{op: the ops that read it, in op order}."""
    cons = {i: [] for i in range(len(g))}
    for i in range(len(g)):
        for src in g.inputs[i]:
            if src.kind == "op":
                cons[src.op].append(i)
    return cons


def only(cons, i):
    """The single consumer of op i, or None."""
    return cons[i][0] if len(cons[i]) == 1 else None


def op_inputs(g, i):
    """The inputs of op i that are ops."""
    return [x.op for x in g.inputs[i] if x.kind == "op"]


def is_sum_gather(G):
    return G.type == "gather" and G.order == "R" and G.comp == "ADD"


MULTI_COMPS = ("MEAN", "MAX", "MIN", "VAR", "STD")  # what one gta_reduce_multi launch can fill


def sibling_gathers(g):
    """[(gather ops, in op order)] for every group of two or more gathers that read the same
    producer op with the same ORDER and whose COMP_TYPEs are distinct members of MULTI_COMPS (a PNA
    layer's aggregators over the same edge messages): one multi-reducer launch fills them all.  A
    producer that also feeds a gather of that ORDER with any other COMP_TYPE (ADD: the sum has its
    own fusions) gives no group for that ORDER."""
    by_site = {}
    for G in g.ops:
        ins = g.inputs[G.idx]
        if G.type == "gather" and len(ins) == 1 and ins[0].kind == "op":
            by_site.setdefault((ins[0].op, G.order), []).append(G)
    found = []
    for _, gs in sorted(by_site.items()):
        comps = [G.comp for G in gs]
        if len(gs) >= 2 and all(c in MULTI_COMPS for c in comps) and len(set(comps)) == len(comps):
            found.append(tuple(G.idx for G in gs))
    return found


def one_scatter(g, P):
    """The one scatter among applyedge P's inputs, or None (none, or several)."""
    sc = [i for i in op_inputs(g, P.idx) if g.ops[i].type == "scatter"]
    return g.ops[sc[0]] if len(sc) == 1 else None


def sums_scatter_c(g, G):
    """G sums a scatter C of a node tensor, directly or through a MUL with exactly one scatter (the
    weighted aggregate): the form mm_first and two_hop move an MM across."""
    if not is_sum_gather(G):
        return False
    src = g.inputs[G.idx][0]
    if src.kind != "op":
        return False
    P = g.ops[src.op]
    if P.type == "applyedge" and P.comp == "MUL":
        P = one_scatter(g, P)
    return P is not None and P.type == "scatter" and P.order == "C"


def softmax(g, cons, sem):
    """GAT edge-softmax chains keyed by their score op A (vTCAD/GraphOP/genGraphOP.py:51-60):
        A = applyedge ADD(scatter R(a), scatter C(b));  V = applyedge SF(A);  G = gather R(V)
      original (ops 6,7,8,10,9): D = applyedge V / scatter R(G)  -> alpha, one launch
      trans    (ops 6,8,9):      V and G from one launch (V's other consumer aggregates it)"""
    ops_, ins = g.ops, g.inputs
    found = {}
    for A in ops_:
        if A.type != "applyedge" or A.comp != "ADD" or len(ins[A.idx]) != 2:
            continue
        srcs = op_inputs(g, A.idx)
        if len(srcs) != 2:
            continue
        orders = sorted(ops_[i].order for i in srcs if ops_[i].type == "scatter")
        if orders != ["C", "R"] or sem.bin_of(A) != "ADD":
            continue
        v = only(cons, A.idx)
        if v is None or ops_[v].type != "applyedge" or ops_[v].comp != "SF":
            continue
        gs = [c for c in cons[v] if ops_[c].type == "gather" and ops_[c].order == "R"]
        if len(gs) != 1 or ops_[gs[0]].comp != "ADD":  # the chain's gather is the softmax SUM
            continue
        G = gs[0]
        pat = {"A": A.idx, "V": v, "G": G, "D": None}
        S = only(cons, G)
        if S is not None and ops_[S].type == "scatter" and ops_[S].order == "R":
            D = only(cons, S)
            if D is not None and set(cons[v]) == {G, D} and ops_[D].type == "applyedge":
                dins = [x.op if x.kind == "op" else None for x in ins[D]]
                b = sem.bin_of(ops_[D])
                if (b == "DIV" and dins == [v, S]) or (b == "RDIV" and dins == [S, v]):
                    pat["D"], pat["S"] = D, S
        found[A.idx] = pat
    return found


def attention(g, cons, sem, softmax):
    """{MUL op M: (softmax pattern, gather G2, x scatter S)} for M = scatter_C(x) * alpha (original,
    alpha = the pattern's D) or * v (trans, v = V), whose only consumer is a gather R."""
    ops_, ins = g.ops, g.inputs
    found = {}
    for pat in softmax.values():
        w_op = pat["D"] if pat["D"] is not None else pat["V"]
        cands = [c for c in cons[w_op] if c != pat["G"]]
        if len(cands) != 1:
            continue
        M = cands[0]
        m = ops_[M]
        if m.type != "applyedge" or m.comp != "MUL" or sem.bin_of(m) != "MUL" or len(ins[M]) != 2:
            continue
        other = [o for o in (x.op if x.kind == "op" else None for x in ins[M]) if o != w_op]
        if len(other) != 1 or other[0] is None:
            continue
        S, G2 = other[0], only(cons, M)
        if ops_[S].type != "scatter" or ops_[S].order != "C" or G2 is None or not is_sum_gather(ops_[G2]):
            continue
        found[M] = (pat, G2, S)
    return found


def mm_first(g, cons):
    """{gather G: MM op M} for G -> M with M the only consumer, narrowing the width, and G
    reading a scatter C directly or through a (weight) MUL (GraphSAGE / GCN layer 1)."""
    found = {}
    for G in g.ops:
        if not is_sum_gather(G) or only(cons, G.idx) is None:
            continue  # (sum_e w x) W == sum_e w (x W) holds for the sum only
        M = g.ops[only(cons, G.idx)]
        if M.type != "applynode" or M.comp != "MM" or len(g.inputs[M.idx]) != 1:
            continue
        if M.out_width and G.out_width and M.out_width < G.out_width and sums_scatter_c(g, G):
            found[G.idx] = M.idx
    return found


def two_hop(g, cons, reorder):
    """{first gather G1: second gather G2} for G1 -> scatter C -> [MUL by an edge weight] -> G2 with
    G2 in reorder (its narrowing MM), each intermediate read only by the next op, and G1 of the
    form mm_first takes (sums_scatter_c)."""
    ops_, ins = g.ops, g.inputs
    found = {}
    for G2 in reorder:
        P = S = ops_[ins[G2][0].op]
        if P.type != "scatter":
            S = one_scatter(g, P)
            if S is None or cons[S.idx] != [P.idx]:
                continue
        if S.order != "C" or not ins[S.idx] or ins[S.idx][0].kind != "op":
            continue
        G1 = ops_[ins[S.idx][0].op]
        if cons[G1.idx] == [S.idx] and sums_scatter_c(g, G1):
            found[G1.idx] = G2
    return found


def pushdown(g, cons, sem):
    """{applyedge ADD of two scatters: its only consumer, a single-input applyedge MM}."""
    found = {}
    for op in g.ops:
        if op.type != "applyedge" or op.comp != "ADD" or len(g.inputs[op.idx]) != 2:
            continue
        srcs = op_inputs(g, op.idx)
        if len(srcs) != 2 or any(g.ops[i].type != "scatter" for i in srcs) or only(cons, op.idx) is None:
            continue
        m = g.ops[only(cons, op.idx)]
        if m.type == "applyedge" and m.comp == "MM" and len(g.inputs[m.idx]) == 1 and sem.bin_of(op) == "ADD":
            found[op.idx] = m.idx
    return found


def gather_acc(g, cons, sem):
    """{applynode ADD A: (gather G, slot of T, node op T)} for A = ADD(G, T) where A is G's and T's
    only consumer, T a two-operand applynode ADD/MUL/DIV/SUB (so its output is a tensor it
    allocated itself) and A carries no SF post-op."""
    found = {}
    for A in g.ops:
        ins = g.inputs[A.idx]
        if A.type != "applynode" or A.comp != "ADD" or len(ins) != 2 or any(x.kind != "op" for x in ins):
            continue
        if sem.bin_of(A) != "ADD":
            continue
        kinds = [g.ops[x.op].type for x in ins]
        if sorted(kinds) != ["applynode", "gather"] or ins[0].op == ins[1].op:
            continue
        gs = 0 if kinds[0] == "gather" else 1
        G, T = g.ops[ins[gs].op], g.ops[ins[1 - gs].op]
        if G.order != "R" or G.comp != "ADD" or cons[G.idx] != [A.idx] or cons[T.idx] != [A.idx]:
            continue
        if T.comp not in ("ADD", "MUL") or len(g.inputs[T.idx]) != 2:
            continue
        c = only(cons, A.idx)
        if c is not None and g.ops[c].comp == "SF" and g.ops[c].type == "applynode":
            continue  # keep A's SF post-op fusion
        found[A.idx] = (G.idx, 1 - gs, T.idx)
    return found


def edge_expr(g, cons, sem, softmax, attn, pushdown, gacc):
    """{gather G: plan} for a gather R (ADD) of an applyedge tree that gta_aggregate_expr's shapes
    cover.  plan: shape, swap, bins, sfs, leaves ((op, slot) of a computed operand, or ("pmm", MM
    op, k): the k-th scatter of a pushed-down MM's sum, multiplied on its node rows) and nodes (the
    tree's ops, deferred until G runs).  Trees the existing fusions take are left to them: a lone
    MUL / MM (the weighted aggregate), the attention chains, the GIN self-term gathers."""
    ops_, ins = g.ops, g.inputs
    att = set(attn)
    for pat in softmax.values():
        att.update(i for i in (pat["A"], pat["V"], pat["D"]) if i is not None)
    acc_g = {G for G, _, _ in gacc.values()}

    def node(i):  # -> ("bin", bin, sf, left, right, ops) | ("leaf", ref) | None (not coverable)
        o = ops_[i]
        if o.type != "applyedge" or i in att:
            return None
        if o.comp == "SF":
            if len(ins[i]) != 1 or ins[i][0].kind != "op" or cons[ins[i][0].op] != [i]:
                return None
            c = node(ins[i][0].op)
            if c is None or c[0] != "bin" or c[2] is not None or c[1] == "PMM":
                return None  # an SF on a pushed-down MM acts on the sum: not this tree
            return ("bin", c[1], sem.sf_of(o), c[3], c[4], c[5] + [i])
        if o.comp == "MM":
            src = ins[i][0] if len(ins[i]) == 1 else None
            if src is None or src.kind != "op" or pushdown.get(src.op) != i:
                return None
            return ("bin", "PMM", None, ("leaf", ("pmm", i, 0)), ("leaf", ("pmm", i, 1)), [i])
        if o.comp not in ("ADD", "SUB", "MUL", "DIV") or len(ins[i]) != 2:
            return None
        b = sem.bin_of(o)
        kids = []
        for slot, x in enumerate(ins[i]):
            sub = None
            if x.kind == "op" and cons[x.op] == [i] and ops_[x.op].type == "applyedge":
                sub = node(x.op)
            kids.append(sub if sub is not None else ("leaf", (i, slot)))
        if b == "RDIV":
            b, kids = "DIV", kids[::-1]
        if b not in ("ADD", "SUB", "MUL", "DIV"):
            return None
        return ("bin", b, None, kids[0], kids[1], [i])

    def leafy(t):
        return t[0] == "bin" and t[3][0] == "leaf" and t[4][0] == "leaf"

    def b_of(t):
        return "ADD" if t[1] == "PMM" else t[1]

    found = {}
    for G in ops_:
        if not is_sum_gather(G) or G.idx in acc_g:
            continue
        src = ins[G.idx][0] if len(ins[G.idx]) == 1 else None
        if src is None or src.kind != "op" or cons[src.op] != [G.idx]:
            continue
        t = node(src.op)
        if t is None:
            continue
        L, R = t[3], t[4]
        if leafy(t):
            if t[1] in ("MUL", "PMM") and t[2] is None:
                continue  # the weighted aggregate / the pushed-down MM's own path
            e = dict(shape=1, swap=False, bins=[b_of(t)], sfs=[t[2]], leaves=[L[1], R[1]], nodes=t[5])
        elif leafy(L) and R[0] == "leaf":
            e = dict(shape=2, swap=False, bins=[b_of(L), t[1]], sfs=[L[2], t[2]], leaves=[L[3][1], L[4][1], R[1]],
                     nodes=L[5] + t[5])
        elif L[0] == "leaf" and leafy(R):
            e = dict(shape=2, swap=True, bins=[b_of(R), t[1]], sfs=[R[2], t[2]], leaves=[R[3][1], R[4][1], L[1]],
                     nodes=R[5] + t[5])
        elif leafy(L) and leafy(R):
            e = dict(shape=3, swap=False, bins=[b_of(L), b_of(R), t[1]], sfs=[L[2], R[2], t[2]],
                     leaves=[L[3][1], L[4][1], R[3][1], R[4][1]], nodes=L[5] + R[5] + t[5])
        else:
            continue
        found[G.idx] = e
    return found
