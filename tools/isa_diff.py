#!/usr/bin/env python3
"""Are the kernels of two source trees the same code?  usage: isa_diff.py OLD_TREE NEW_TREE [KERNEL-NAME REGEX [TRANSLATION UNIT]]

Compiles `#include "dsg_ppo.hpp"` (which includes dsg_mlp.hpp: the six k_mlp_* / k_ppo_* kernels) from each tree to gfx950 assembly
with the flags of _lib.build(), no GPU needed, and prints per kernel `identical` assembly, or else whether the listing of its `_f32` /
`_f64` opcodes agrees in program order with vector register numbers blanked, and the register, scratch and LDS
figures of both.  Exit status 1 unless every kernel is at least `fp-order-same` with equal figures.

With a TRANSLATION UNIT (a path below the tree, e.g. diffsg_amd/csrc/dsg_api.hip) that file is compiled instead of the baseline
headers and the kernels are keyed by their full demangled names (the library's kernels are templates: the short name is not unique);
`isa_diff.py OLD NEW . diffsg_amd/csrc/dsg_api.hip` is the check a host-side refactor runs: every kernel of the library `identical`.
Only a summary and the kernels that are not identical are printed then."""
import os
import re
import subprocess
import sys
import tempfile

FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -pragma-unroll-threshold=200000 -S --cuda-device-only".split()
FIGURES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize")


def kernels(tree, tmp, unit=None):
    """{kernel name: (instruction lines, {figure: value})} of the tree's baseline headers, or of its translation unit `unit`."""
    src, asm = os.path.join(tmp, "tu.hip"), os.path.join(tmp, "tu.s")
    with open(src, "w") as f:
        f.write('#include <hip/hip_runtime.h>\n#include "dsg_ppo.hpp"\n')
    inc = ["-I", os.path.join(tree, "diffsg_amd", "csrc"), "-I", os.path.join(tree, "include")]
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + inc + ["-o", asm, os.path.join(tree, unit) if unit else src], check=True)
    with open(asm) as f:
        txt = f.read()
    found = list(re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:.*?-- End function(.*?)(?=^\t\.text|^\t\.section\t\.text|\Z)", txt, re.M | re.S))
    full = {}
    if unit:        # demangled: a kernel of an unnamed namespace carries a per-compilation suffix in its mangled name only
        dem = subprocess.run(["c++filt"], input="\n".join(m.group(1) for m in found), capture_output=True, text=True, check=True).stdout.split("\n")
        full = {m.group(1): re.sub(r"^void ", "", d) for m, d in zip(found, dem)}
    out = {}
    for m in found:
        name = re.search(r"\d(k_[a-z0-9_]+)E", m.group(1))            # the kernels' names are lower case: the first E ends the name
        body = [ln.split(";")[0].strip() for ln in m.group(2).split("\n")]
        if unit:    # a basic-block label carries the function's ordinal in the module and a long branch's label a module-wide count:
            #         both follow the order of instantiation, which host code decides
            body = [re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", ln)) for ln in body]
        figures = re.search(r"; NumVgprs", m.group(3))
        if not figures:
            continue                                                 # a device function that is no kernel
        out[full.get(m.group(1)) or (name.group(1) if name else m.group(1))] = (
            [ln for ln in body if ln], {k: int(re.search(rf"; {k}: (\d+)", m.group(3)).group(1)) for k in FIGURES})
    return out


def fp_listing(lines):
    return [re.sub(r"\bv(\d+|\[\d+:\d+\])", "v", ln) for ln in lines if re.match(r"\w*_f(32|64)\b", ln)]


def main(old_tree, new_tree, want="k_(mlp|ppo)_", unit=None):
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(old_tree, tmp, unit), kernels(new_tree, tmp, unit)
    bad = sorted(k for k in set(old) ^ set(new) if re.search(want, k))
    count = {}
    for k in sorted(k for k in set(old) & set(new) if re.search(want, k)):
        (lo, fo), (ln, fn) = old[k], new[k]
        a, b = fp_listing(lo), fp_listing(ln)
        verdict = "identical" if lo == ln else "fp-order-same" if a == b else "fp-multiset-same" if sorted(a) == sorted(b) else "DIFFERENT"
        if verdict not in ("identical", "fp-order-same") or fo != fn or (unit and verdict != "identical"):
            bad.append(k)
        count[verdict] = count.get(verdict, 0) + 1
        if unit and verdict == "identical" and fo == fn:
            continue
        if unit and len(lo) == len(ln):
            print("    first difference:", next(f"{x!r} / {y!r}" for x, y in zip(lo, ln) if x != y))
        print(f"{k:16s} {verdict:16s} {len(lo)} / {len(ln)} lines, {len(a)} / {len(b)} fp   " + "  ".join(f"{f} {fo[f]} / {fn[f]}" for f in FIGURES))
    if unit:
        print(f"{unit}: {len(old)} / {len(new)} kernels, " + ", ".join(f"{n} {v}" for v, n in sorted(count.items())))
    if bad:
        sys.exit("NOT the same: " + ", ".join(bad))


if __name__ == "__main__":
    main(*sys.argv[1:5])
