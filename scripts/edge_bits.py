"""Result bits of the edge-wise / node-wise element kernels and the unfused GAT softmax, one sha256 per
case: python scripts/edge_bits.py [--out FILE] [--full FILE]

Run in two builds (the parent's checkout and this tree) the two listings must be identical: the
check that a change to k_scatter, k_apply_edge*, k_apply_node*, k_edge_softmax*, k_softmax_shift or
their dispatch moved no result bit.  One sha256 is taken per case over the raw bytes of every output
(`out`, and `sums` / `shift` where there are any).  --full writes every case, `<family> | <case>
<sha256>`; --out (or stdout) is the short listing that is kept with a change, one line per family:
`<family> cases=<n> <sha256 over the family's full lines>`.  A case that raises is listed as refused
and the script exits 1.

One graph of 40 rows whose lengths (0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 257, 300
and a second helping of the short ones) reach the 4-edge unroll and its tail, the 64-index chunk and
its tail and more than 4 kept chunks; the first and the last row are empty and the edge count is
no multiple of 8.  Inputs are seeded normals with NaN, +-Inf and -0.0 planted in a and in b."""
import contextlib
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import graph as G, ops  # noqa: E402

DEGREES = [0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 257, 300,
           2, 6, 1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 10, 12, 0, 11, 13, 66, 0]
EDGE_SHAPES = [(1, 1), (8, 1), (16, 16), (32, 4), (3, 3), (48, 48), (100, 4), (128, 128), (128, 8), (8, 128), (256, 16),
               (64, 64), (602, 602), (128, None), (100, None), (8, None)]
EDGE_MODES = [("src", "dst", False), ("edge", "src", False), ("dst", "edge", False), ("src", "dst", True)]  # last: one b row
BINS = ("ADD", "MUL", "DIV", "SUB")
SFS = (None, "RELU", "EXP_LEAKY_RELU")
SPECIALS = (float("nan"), float("inf"), float("-inf"), -0.0)


@contextlib.contextmanager
def knobs(**kv):
    old = {k: ops.get_debug(k) for k in kv}
    try:
        for k, v in kv.items():
            ops.set_debug(k, v)
        yield
    finally:
        for k, v in old.items():
            ops.set_debug(k, v)


def main():
    if not torch.cuda.is_available():
        print("error: no HIP device", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    full = []

    def emit(family, case, fn):  # fn returns the outputs; a case that raises is listed as refused
        try:
            outs = fn()
            torch.cuda.synchronize(dev)
            h = hashlib.sha256()
            for t in outs:
                h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
            d = h.hexdigest()
        except (RuntimeError, ValueError, TypeError) as e:
            d = f"refused: {e}"
        full.append(f"{family} | {case} {d}")

    rng = np.random.default_rng(20)
    ip = np.concatenate([[0], np.cumsum(DEGREES)]).astype(np.int64)
    n = len(DEGREES)
    ix = np.concatenate([np.sort(rng.integers(0, n, d)) for d in DEGREES]).astype(np.int32)
    g = G.from_numpy(ip, ix, device=dev)
    assert g.nnz % 8 and g.nnz % 32

    def table(rows, F, seed, slice_off=0, dtype=torch.float32):
        """Seeded normals with the special values planted; slice_off = 1: a column slice one float in."""
        v = np.random.default_rng(seed).standard_normal((rows, F)).astype(np.float32)
        flat = v.reshape(-1)
        for i, s in enumerate(SPECIALS):
            flat[(7 + 131 * i + seed) % flat.size] = s
        t = torch.from_numpy(v).to(dev).to(dtype)
        if slice_off:
            wide = torch.zeros(rows, F + 2 * slice_off, dtype=dtype, device=dev)
            wide[:, slice_off:slice_off + F] = t
            return wide[:, slice_off:slice_off + F]
        return t

    rows_of = {"edge": g.nnz, "src": g.n_cols, "dst": g.n_rows}

    # apply_edge: generic, row-sweep and flat forms
    old_flat = ops.APPLY_EDGE_FLAT
    try:
        for form, flat_on in (("generic", False), ("sweep", False), ("flat", True)):
            ops.APPLY_EDGE_FLAT = flat_on
            with knobs(apply_edge_form=0 if form == "generic" else 1):
                for Fa, Fb in EDGE_SHAPES:
                    Fo = max(Fa, Fb or 0)
                    if form == "flat" and Fo not in (64, 128, 256):
                        continue
                    for sliced in (0, 1, 2):  # column slices 1 float in (rows 4-B aligned: VW 1) and 2 in (8-B: VW 2)
                        if sliced and (form == "flat" or Fo not in (128, 256, 100, 8)):
                            continue  # sliced rows make flat refuse and the row-sweep forms are taken
                        for am, bm, brow in EDGE_MODES:
                            if Fb is None and brow:
                                continue
                            a = table(rows_of[am], Fa, 3 * Fa + len(am), sliced)
                            b = None if Fb is None else table(1 if brow else rows_of[bm], Fb, 5 * Fb + len(bm), sliced)
                            for bn in (BINS if b is not None else (None,)):
                                for sf in SFS:
                                    def run():
                                        wide = torch.zeros(g.nnz, Fo + 2 * sliced, device=dev)
                                        ops.apply_edge(g, bn, sf, a, am, b, bm, out=wide[:, sliced:sliced + Fo],
                                                       b_broadcast_row=brow)
                                        return (wide,)
                                    emit(f"apply_edge {form} Fa={Fa} Fb={Fb}",
                                         f"a={am} b={'row' if brow else bm} {bn} {sf} sliced={sliced}", run)
    finally:
        ops.APPLY_EDGE_FLAT = old_flat

    # apply_node
    N = 300
    for vec in (0, 1):
        with knobs(apply_node_vec=vec):
            for F in (4, 100, 128):
                for dt in (torch.float32, torch.bfloat16):
                    for bkind in ("none", "full", "per_node", "one_row", "a_narrow"):
                        a = table(N, F // 4 if bkind == "a_narrow" else F, F + 1, dtype=dt)
                        b = {"none": None, "full": table(N, F, F + 2), "per_node": table(N, 1, F + 3),
                             "one_row": table(1, 1, F + 4), "a_narrow": table(N, F, F + 5)}[bkind]
                        for bn in (BINS if b is not None else (None,)):
                            for sf in SFS:
                                for sliced in (0, 1):
                                    def run():
                                        wide = torch.zeros(N, F + 2 * sliced, device=dev)
                                        ops.apply_node(bn, sf, a, b, out=wide[:, sliced:sliced + F],
                                                       b_broadcast_row=bkind == "one_row")
                                        return (wide,)
                                    emit(f"apply_node vec={vec} F={F} {str(dt).split('.')[-1]}",
                                         f"b={bkind} {bn} {sf} sliced={sliced}", run)

    # scatter: copy units 16, 8, 4 and 2 bytes
    for direction in ("R", "C"):
        for dt in (torch.float32, torch.bfloat16):
            for F in (1, 2, 3, 4, 8):
                for sliced in (0, 1):
                    x = table(n, F, 40 + F, sliced, dtype=dt)

                    def run():
                        wide = torch.zeros(g.nnz, F + 2 * sliced, dtype=dt, device=dev)
                        ops.scatter(g, x, direction, out=wide[:, sliced:sliced + F])
                        return (wide,)
                    emit(f"scatter {direction} {str(dt).split('.')[-1]}", f"F={F} sliced={sliced}", run)

    # softmax_shift and edge_softmax
    for H in (1, 2, 4, 8, 16, 32, 64):
        a = table(n, H, 60 + H)
        for ldb in (H, H + 3):
            b = table(n, ldb, 70 + H)[:, :H]
            shifts = {}
            for sf in ("EXP_LEAKY_RELU", "EXP"):
                def run_shift():
                    shifts[sf] = ops.softmax_shift(g, a, b, sf)
                    return (shifts[sf],)
                emit(f"softmax_shift H={H}", f"ldb={ldb} {sf}", run_shift)
            for lane in (0, 1):
                with knobs(esm_lane=lane):
                    for sf, shifted in (("EXP_LEAKY_RELU", False), ("SIGMOID", False), ("EXP_LEAKY_RELU", True), ("EXP", True)):
                        for normalize in (False, True):
                            for want_sums in (False, True):
                                def run():
                                    out, sums = ops.edge_softmax(g, a, b, sf=sf, normalize=normalize, want_sums=want_sums,
                                                                 shift=shifts[sf] if shifted else None)
                                    return (out,) if sums is None else (out, sums)
                                emit(f"edge_softmax H={H} esm_lane={lane}",
                                     f"ldb={ldb} {sf} shifted={shifted} normalize={normalize} sums={want_sums}", run)

    fam = {}
    for line in full:
        fam.setdefault(line.split(" | ")[0], []).append(line)
    short = [f"{k} cases={len(ls)} " + (f"refused={sum(' refused: ' in v for v in ls)} " if any(' refused: ' in v for v in ls) else "")
             + hashlib.sha256("\n".join(ls).encode()).hexdigest() for k, ls in fam.items()]
    text = "\n".join(short) + "\n"
    if "--full" in sys.argv:
        write(sys.argv[sys.argv.index("--full") + 1], "\n".join(full) + "\n")
    if "--out" in sys.argv:
        write(sys.argv[sys.argv.index("--out") + 1], text)
        print(f"{len(full)} cases, {len(short)} families")
    else:
        sys.stdout.write(text)
    refused = [ln for ln in full if " refused: " in ln]
    if refused:
        print(f"error: {len(refused)} cases raised, the first: {refused[0]}", file=sys.stderr)
        return 1
    return 0


def write(path, text):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
