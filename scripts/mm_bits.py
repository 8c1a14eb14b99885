"""Result bits of every UPDATE GEMM form, one sha256 per case: python scripts/mm_bits.py [--out FILE] [--full FILE]

Run in two builds (the parent's checkout and this tree) the two listings must be identical: the
check that a change to the MFMA UPDATE kernels (k_mm_rows, k_mm_ring, k_mm_wave, k_mm_ring_bf,
k_mlp_bf, the 64x64 tile kernels) or their dispatch moved no result bit.  A sha256 over the raw bytes
of `out` is taken per case (shape, form), some 16,600 of them.  --full writes them all,
`<shape and operands> [<forms>] <sha256>`, the forms of a shape whose digests agree on one line (most
do: every one-pass form is bitwise k_mm_rows): 0.66 MB, the file to diff when something moved.  --out
(or stdout) is the short listing that is kept with a change: one line per family -- every K and form
of one dtype, M and N -- `<family> cases=<n> <sha256 over the family's full lines>`.  Every case is
one the entry points take: a case that raises is listed as refused (`refused=<n>` on its family's
line) and the script exits 1.

Forms: MM_FORM "tile"; under "rows" the default, k_mm_rows (prefetch auto / never / always), the
ring at FR 1 and 2, the wave kernel at FR 2 / 3 / 4 / auto, split K in 2, 3 and auto slices with the
ring on and off.  Dtypes f32, mixed (fp32 x, bf16 W) and bf16.  Small shapes at the tile edges (K
below one stage, an exact stage, a ring tail, a register tail, bf16 K > 256; N tails; one row; a
partial row group), with a gathered row_idx, SFs, an `out` column slice (the per-element store) and
x rows that are only 4-B aligned; large shapes where a block runs several row groups; update_mlp."""
import contextlib
import hashlib
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gta_graph_tensor_acclelrator_for_general_gnn_amd import ops  # noqa: E402

FORMS = [  # (name, knobs)
    ("default", {}),
    ("rows", {"mm_ring": 0, "mm_split": 0}),
    ("rows_pf0", {"mm_ring": 0, "mm_prefetch": 0}),
    ("rows_pf2", {"mm_ring": 0, "mm_prefetch": 2}),
    ("ring_fr1", {"mm_ring_fr": 1, "mm_wave": 0, "mm_split": 0}),
    ("ring_fr2", {"mm_ring_fr": 2, "mm_wave": 0, "mm_split": 0}),
    ("wave_fr2", {"mm_wave": 2, "mm_wave_fr": 2, "mm_split": 0}),
    ("wave_fr3", {"mm_wave": 2, "mm_wave_fr": 3, "mm_split": 0}),
    ("wave_fr4", {"mm_wave": 2, "mm_wave_fr": 4, "mm_split": 0}),
    ("wave_auto", {"mm_wave": 2, "mm_split": 0}),
] + [(f"split{'_auto' if n < 0 else n}_ring{r}", {"mm_split": n, "mm_ring": r}) for n in (2, 3, -1) for r in (1, 0)]
F32_ONLY = ("ring_fr", "wave_")  # forms that only change what fp32 runs: bf16 / mixed would repeat "default"

SMALL_M = (1, 77, 130, 3001)
SMALL_N = (8, 20, 33, 64, 100, 128, 200)
SMALL_K = (5, 16, 31, 32, 37, 48, 100, 128, 257, 602, 1433)
LARGE = [("f32", 70000, 32, 33), ("f32", 70000, 602, 128), ("f32", 120000, 100, 128),
         ("mixed", 120000, 100, 128), ("bf16", 120000, 100, 128), ("mixed", 120000, 128, 64), ("bf16", 120000, 128, 64)]
MLP = [(4099, 36, 64, 20, None, "ELU"), (20000, 100, 128, 128, "RELU", "RELU"), (100003, 100, 128, 128, "RELU", None)]


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


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    if not torch.cuda.is_available():
        print("error: no HIP device", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cases = {}  # shape tag -> {digest: [forms]}, both in first-seen order

    def emit(tag, form, fn):  # a case that raises is listed as refused, and fails the run at the end
        try:
            t = fn()
            torch.cuda.synchronize(dev)
            d = digest(t)
        except (RuntimeError, ValueError, TypeError) as e:
            d = f"refused: {e}"
        cases.setdefault(tag, {}).setdefault(d, []).append(form)

    def operands(dt, M, K, N, seed):
        rng = np.random.default_rng(seed)
        x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).to(dev)
        w = torch.from_numpy((rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)).to(dev)
        if dt != "f32":
            w = w.to(torch.bfloat16)
        if dt == "bf16":
            x = ops.pitched(x.to(torch.bfloat16))
        return x, w

    def run_forms(tag, dt, x, w, **kw):
        N = w.shape[1]
        for name, kv in FORMS:
            if dt != "f32" and name.startswith(F32_ONLY):
                continue
            with knobs(**kv):
                emit(tag, name, lambda: ops.update_mm(x, w, **kw))
                if name in ("default", "rows", "ring_fr1", "wave_fr3", "split2_ring1", "split2_ring0"):
                    # "@ldo": out as a column slice, ldo = N + 3: rows not 16-B aligned, the per-element store
                    def sliced():
                        wide = torch.zeros(kw.get("row_idx", x).shape[0], N + 3, device=dev)
                        ops.update_mm(x, w, out=wide[:, :N], **kw)
                        return wide
                    emit(tag, f"{name}@ldo", sliced)

    old_form = ops.MM_FORM
    try:
        for dt in ("f32", "mixed", "bf16"):
            for M in SMALL_M:
                for N in SMALL_N:
                    for K in SMALL_K:
                        x, w = operands(dt, M, K, N, 1000003 * M + 1009 * K + N)
                        sf = {64: "RELU", 20: "ELU"}.get(N)
                        kw = {"sf": sf}
                        if N == 100:  # gathered rows, repeats included
                            kw["row_idx"] = torch.from_numpy(
                                np.random.default_rng(M + K).integers(0, M, M + 3).astype(np.int32)).to(dev)
                        tag = f"{dt} M={M} K={K} N={N} sf={sf}{' gathered' if 'row_idx' in kw else ''}"
                        ops.MM_FORM = "tile"
                        emit(tag, "tile", lambda: ops.update_mm(x, w, **kw))
                        ops.MM_FORM = "rows"
                        run_forms(tag, dt, x, w, **kw)
        # x a column window of a wider fp32 table: every row start 4-B aligned only
        for K, off in ((602, 1), (500, 3), (128, 1), (37, 1)):
            rng = np.random.default_rng(K + off)
            big = torch.from_numpy(rng.standard_normal((3001, K + 4 + off)).astype(np.float32)).to(dev)
            for dt in ("f32", "mixed"):
                w = torch.from_numpy((rng.standard_normal((K, 128)) / np.sqrt(K)).astype(np.float32)).to(dev)
                w = w if dt == "f32" else w.to(torch.bfloat16)
                run_forms(f"{dt} M=3001 K={K} N=128 x4B off={off}", dt, big[:, off:off + K], w)
        for dt, M, K, N in LARGE:
            x, w = operands(dt, M, K, N, M + K + N)
            run_forms(f"{dt} M={M} K={K} N={N}", dt, x, w)
        for M, K1, N1, N2, sf1, sf2 in MLP:
            rng = np.random.default_rng(M + K1 + N1 + N2)
            x = torch.from_numpy(rng.standard_normal((M, K1)).astype(np.float32)).to(dev)
            w1 = torch.from_numpy((rng.standard_normal((K1, N1)) / np.sqrt(K1)).astype(np.float32)).to(torch.bfloat16).to(dev)
            w2 = torch.from_numpy((rng.standard_normal((N1, N2)) / np.sqrt(N1)).astype(np.float32)).to(torch.bfloat16).to(dev)
            xb = torch.zeros(M, (K1 + 7) // 8 * 8, dtype=torch.bfloat16, device=dev)[:, :K1]  # rows padded to 16 B
            xb.copy_(x.to(torch.bfloat16))
            for xd, name in ((x, "fp32"), (xb, "bf16")):
                emit(f"mlp M={M} K1={K1} N1={N1} N2={N2} sf1={sf1} sf2={sf2} x={name}", "mlp",
                     lambda: ops.update_mlp(xd, w1, w2, sf1=sf1, sf2=sf2))
    finally:
        ops.MM_FORM = old_form
    full = [f"{tag} [{' '.join(forms)}] {d}" for tag, by_digest in cases.items() for d, forms in by_digest.items()]
    text = "\n".join(family_lines(full)) + "\n"
    if "--full" in sys.argv:
        write(sys.argv[sys.argv.index("--full") + 1], "\n".join(full) + "\n")
    if out_path:
        write(out_path, text)
        print(f"{sum(len(f) for c in cases.values() for f in c.values())} cases, {len(full)} full lines -> {out_path}")
    else:
        sys.stdout.write(text)
    refused = [ln for ln in full if "] refused: " in ln]
    if refused:  # every case here is one the entry points take: a refusal is a failure, in either build
        print(f"error: {len(refused)} full lines hold refused cases, the first: {refused[0]}", file=sys.stderr)
        return 1
    return 0


def family_lines(full):
    """The short listing: the full lines of one family (a shape tag with its K dropped: every K and
    every form of one dtype, M and N) hashed together, `<family> <cases> <sha256 of its full lines>`."""
    fam = {}
    for line in full:
        fam.setdefault(re.sub(r" K=\d+", "", line.split(" [")[0]), []).append(line)
    def forms(ls, refused):
        return sum(len(v.split("[")[1].split("]")[0].split()) for v in ls if ("] refused: " in v) == refused)
    return [f"{k} cases={forms(ls, False) + forms(ls, True)} "
            + (f"refused={forms(ls, True)} " if forms(ls, True) else "")
            + hashlib.sha256(chr(10).join(ls).encode()).hexdigest() for k, ls in fam.items()]


def write(path, text):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    sys.exit(main())
