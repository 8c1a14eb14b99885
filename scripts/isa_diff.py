"""Compare the gfx950 kernels of two libgta.so builds: python scripts/isa_diff.py OLD.so NEW.so [name ...]

Prints the kernels only one build has, then every common kernel whose per-mnemonic instruction
histogram or code-object resources (VGPRs, SGPRs, scratch) differ: total instructions, vector-memory
and LDS counts, the mnemonics that changed, and WAVES when the VGPR count crosses an occupancy step."""
import collections
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gta_graph_tensor_acclelrator_for_general_gnn_amd import asmcheck  # noqa: E402

VMEM = ("buffer_", "global_", "flat_", "scratch_")
_META = re.compile(r"\.(symbol|sgpr_count|vgpr_count|private_segment_fixed_size):\s+(\S+)")


def waves(vgprs):  # per SIMD on gfx950: 512 VGPRs, allocated in granules of 8, at most 8 waves
    return min(8, 512 // max(8, -(-vgprs // 8) * 8))


def kernels(so_path, names, arch="gfx950"):
    """{kernel: (mnemonic histogram, {vgpr_count, sgpr_count, private_segment_fixed_size})}."""
    with tempfile.TemporaryDirectory(prefix="gta_isa_diff_") as tmp:
        lib = os.path.join(tmp, "lib.so")
        os.symlink(os.path.abspath(so_path), lib)
        subprocess.run([asmcheck.objdump(), "--offloading", lib], check=True, cwd=tmp, capture_output=True)
        co, = [p for p in glob.glob(lib + ".*") if p.endswith(arch)]
        readelf = os.path.join(os.path.dirname(asmcheck.objdump()), "llvm-readelf")
        notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
    res = {}
    for block in notes.split("- .agpr_count:")[1:]:  # one block per kernel; only the kernel has a .symbol
        kv = dict(_META.findall(block))
        res[kv["symbol"][:-len(".kd")]] = {k: int(v) for k, v in kv.items() if k != "symbol"}
    return {f: (collections.Counter(i[1] for i in insns), res.get(f, {}))
            for f, insns in asmcheck.parse(asmcheck.disassemble(so_path, arch)).items()
            if not names or any(n in f for n in names)}


def demangle(symbols):
    """{symbol: 'name<template arguments>'} (the parameter list dropped); {} without a demangler."""
    symbols = list(symbols)
    cxxfilt = next((c for c in (os.path.join(os.path.dirname(asmcheck.objdump()), "llvm-cxxfilt"),
                                shutil.which("llvm-cxxfilt"), shutil.which("c++filt")) if c and os.path.exists(c)), None)
    if cxxfilt is None or not symbols:
        return {}
    out = subprocess.run([cxxfilt], input="\n".join(symbols), check=True, capture_output=True, text=True).stdout
    return {f: d.partition(">(")[0] for f, d in zip(symbols, out.splitlines())}


def pair_defaulted(old, new):
    """A kernel template that gained a trailing parameter defaulted to false (and perhaps an argument
    that instantiation never reads) changes its symbol: NEW's k<..., false> is OLD's k<...>.  Renames
    such NEW entries to OLD's symbol so the two are compared; returns how many were paired."""
    by_name = {d: f for f, d in demangle(old.keys() - new.keys()).items()}
    n = 0
    for f, d in demangle(new.keys() - old.keys()).items():
        if d.endswith(", false") and d[:-len(", false")] in by_name:
            new[by_name[d[:-len(", false")]]] = new.pop(f)
            n += 1
    return n


def main(argv):
    old, new = kernels(argv[1], argv[3:]), kernels(argv[2], argv[3:])
    paired = pair_defaulted(old, new)
    if paired:
        print(f"{paired} kernels of NEW paired with OLD's symbol (a trailing template parameter defaulted to false)")
    for f in sorted(old.keys() ^ new.keys()):
        print("only in OLD" if f in old else "only in NEW", f)
    differ = 0
    for f in sorted(old.keys() & new.keys()):
        (ho, ro), (hn, rn) = old[f], new[f]
        if ho == hn and ro == rn:
            continue
        differ += 1
        count = lambda h, *p: sum(n for m, n in h.items() if m.startswith(p))  # noqa: E731
        wo, wn = waves(ro.get("vgpr_count", 0)), waves(rn.get("vgpr_count", 0))
        print(f"{f}\n  total {sum(ho.values())} -> {sum(hn.values())}  vmem {count(ho, *VMEM)} -> {count(hn, *VMEM)}  "
              f"lds {count(ho, 'ds_')} -> {count(hn, 'ds_')}  resources {ro} -> {rn}"
              + (f"  WAVES {wo} -> {wn}" if wo != wn else ""))
        print(" ", {m: hn[m] - ho[m] for m in sorted(set(ho) | set(hn)) if hn[m] != ho[m]})
    print(f"{len(old)} / {len(new)} kernels, {len(old.keys() ^ new.keys())} unmatched, {differ} differ")


if __name__ == "__main__":
    sys.exit(main(sys.argv))
