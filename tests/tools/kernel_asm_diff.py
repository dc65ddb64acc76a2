#!/usr/bin/env python3
"""Compare the device code of two source trees kernel by kernel (CPU only: hipcc -S).

For a refactor that moves kernels between translation units without touching them:

    kernel_asm_diff.py --old OLD_CSRC ops.hip --new NEW_CSRC ops_bn.hip ops_pool.hip ...

compiles every listed file of either tree to gfx950 device assembly with the Makefile's flags
(EXTRA="..." adds to them, as ``make EXTRA=`` does) and compares the union of kernels by symbol:
each symbol must occur once on either side, with equal .vgpr_count, .sgpr_count,
.private_segment_fixed_size and .group_segment_fixed_size and equal instruction text once
comments and local labels are stripped.  Prints one line per difference and a summary; exit
status 1 if anything differs."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def assemble(tree, src, extra, tmp):
    out = os.path.join(tmp, f"{abs(hash(tree))}_{src}.s")
    inc = os.path.normpath(os.path.join(tree, "..", "..", "include"))
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{inc}", "-Wall", "-Wno-unused-function",
           *extra, "--cuda-device-only", "-S", "-o", out, os.path.join(tree, src)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(text):
    """{symbol: (metadata tuple, normalised instruction lines)} of one assembly file."""
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", blk).group(1)  # (four spaces: the kernel's, not an argument's)
        meta[name] = tuple(int(re.search(r"\n    " + re.escape(k) + r":\s+(\d+)", blk).group(1)) for k in META)
    out = {}
    for name, m in meta.items():
        start = text.index(f"\n{name}:") + len(name) + 2
        end = text.index(".Lfunc_end", start)
        lines = []
        for ln in text[start:end].splitlines():
            ln = ln.split(";")[0].strip()
            if not ln or re.fullmatch(r"\.L\w+:", ln):
                continue
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))  # a label's function number is its file position
        out[name] = (m, lines)
    return out


def side(tree, srcs, extra, tmp, pool):
    got, dup = {}, []
    for src, text in zip(srcs, pool.map(lambda s: assemble(tree, s, extra, tmp), srcs)):
        for name, v in kernels(text).items():
            if name in got:
                dup.append(f"{name}: in {got[name][0]} and {src}")
            got[name] = (src, *v)
    return got, dup


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True, metavar=("CSRC", "FILE"))
    ap.add_argument("--new", nargs="+", required=True, metavar=("CSRC", "FILE"))
    ap.add_argument("--extra", default="", help="appended to the compile flags of both sides")
    a = ap.parse_args()
    extra = a.extra.split()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(8) as pool:
        old, dup_old = side(a.old[0], a.old[1:], extra, tmp, pool)
        new, dup_new = side(a.new[0], a.new[1:], extra, tmp, pool)
    bad = [f"twice in the old tree: {d}" for d in dup_old] + [f"twice in the new tree: {d}" for d in dup_new]
    bad += [f"only in the old tree: {n} ({old[n][0]})" for n in sorted(set(old) - set(new))]
    bad += [f"only in the new tree: {n} ({new[n][0]})" for n in sorted(set(new) - set(old))]
    same = 0
    for n in sorted(set(old) & set(new)):
        (so, mo, to), (sn, mn, tn) = old[n], new[n]
        if mo != mn:
            bad.append(f"resources differ: {n}: {dict(zip(META, mo))} ({so}) vs {dict(zip(META, mn))} ({sn})")
        elif to != tn:
            at = next((i for i, (x, y) in enumerate(zip(to, tn)) if x != y), min(len(to), len(tn)))
            bad.append(f"text differs: {n}: {so} vs {sn}, {len(to)} vs {len(tn)} lines, first at line {at}")
        else:
            same += 1
    for b in bad:
        print(b)
    print(f"kernels: {len(old)} old, {len(new)} new, {same} identical, {len(bad)} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
