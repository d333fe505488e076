#!/usr/bin/env python3
"""Compare the kernels of two device assembly files, kernel by kernel (CPU only, no GPU needed).

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -DRPT_PRODUCT_BUILD=1 -I include -I <pkg>/csrc \\
        --cuda-device-only -S <pkg>/csrc/rpt_gpu.hip -o A.s        (the same for B.s)
  tools/isa_compare.py A.s B.s

Prints one line per kernel: identical / different / only-in-A / only-in-B, with the VGPRs, SGPRs, LDS and
private-segment bytes of its .amdhsa_ block on each side. Kernels are matched by demangled name without the
parameter list (a kernel that gains or loses an argument is still the same kernel); without a demangler on
PATH, by symbol. Local labels and the comments that cite them lose their function ordinal first (.LBB<n>_,
.Lfunc_end<n>): it shifts when a kernel before them is added or removed, and with it the padding before a label's
comment, which is collapsed to one space. The text is compared as text: nothing
here reads instructions. Exit status 0; the verdict is the reader's.
"""
import re
import shutil
import subprocess
import sys

RES = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("lds", "group_segment_fixed_size"),
       ("priv", "private_segment_fixed_size"))


def demangle(symbols):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not symbols:
        return {s: s for s in symbols}
    out = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.split("\n")
    names = {}
    for sym, full in zip(symbols, out):
        full, depth = full.replace("(anonymous namespace)", "{anon}"), 0
        for i, ch in enumerate(full):  # cut the parameter list: the first '(' outside template brackets
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                full = full[:i]
                break
        names[sym] = full.replace("void ", "", 1) if full.startswith("void ") else full
    return names


def kernels(path):
    """{name: (normalised body text, {resource: value})} of every .amdhsa_kernel in the file."""
    lines = open(path).read().split("\n")
    syms, res = [], {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        syms.append(m.group(1))
        block = "\n".join(lines[i:lines.index("\t.end_amdhsa_kernel", i)])
        res[m.group(1)] = {k: int(re.search(r"\.amdhsa_" + d + r"\s+(\d+)", block).group(1)) for k, d in RES}
    names = demangle(syms)
    found = {}
    for sym in syms:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        end = next(i for i in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        body = "\n".join(lines[start + 1:end])
        body = re.sub(r"BB\d+_", "BB_", body).replace(sym, "<kernel>")
        body = re.sub(r"[ \t]+;", " ;", body)  # a label's comment is padded to a column: one space less per ordinal digit
        found[names[sym]] = (body, res[sym])
    return found


def fmt(r):
    return " ".join(f"{k}={r[k]}" for k, _ in RES) if r else "-"


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    count = {}
    for name in sorted(set(a) | set(b)):
        if name not in b:
            verdict = "only-in-A"
        elif name not in a:
            verdict = "only-in-B"
        else:
            verdict = "identical" if a[name][0] == b[name][0] else "different"
        count[verdict] = count.get(verdict, 0) + 1
        ra, rb = (a.get(name) or (None, None))[1], (b.get(name) or (None, None))[1]
        print(f"{verdict:9}  {name}\n           A: {fmt(ra)}\n           B: {fmt(rb)}")
    print("# " + ", ".join(f"{v} {k}" for k, v in sorted(count.items())), f"(A: {len(a)} kernels, B: {len(b)})")


if __name__ == "__main__":
    main()
