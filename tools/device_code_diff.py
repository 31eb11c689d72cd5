#!/usr/bin/env python3
"""Did a change move any kernel?  Compares two gfx950 device assembly files kernel by kernel (no GPU needed).

    hipcc <the flags of tensoir_amd/csrc/build.sh> --cuda-device-only -S tir_field.hip -o before.s     (parent commit)
    hipcc <the same flags>                         --cuda-device-only -S tir_field.hip -o after.s      (this tree)
    python tools/device_code_diff.py before.s after.s

A host-only change reorders the template instantiations, so the files differ as text while every kernel is the same.  Per
kernel symbol this compares (1) the instruction text between its label and its .Lfunc_end, comments stripped and the
function index of local labels (.LBB<i>_<n>) normalised, and (2) its .amdhsa_kernel ... .end_amdhsa_kernel block
(registers, scratch, LDS, kernarg size).  The sets of kernel symbols must be equal too.  Prints the verdict and the names
that differ; exit status 0 = identical, 1 = not.

Limit: only what lies between a kernel's label and its .Lfunc_end, and its descriptor, is compared.  A __device__ function that
is not inlined, or read-only data a kernel refers to (a jump table, a constant array), lies outside and could change unnoticed;
in this library every device function is inlined into its kernels."""
import re
import sys


def kernels(path):
    """{kernel symbol: (instruction lines, descriptor lines)}"""
    lines = open(path).read().split("\n")
    out = {}
    for i, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        start = max(j for j in range(i) if lines[j].split(";")[0].strip() == name + ":")
        stop = next(j for j in range(end, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[j]))
        body = lines[start + 1:i] + lines[end + 1:stop]
        out[name] = ([t for t in map(normalise, body) if t], [t for t in map(normalise, lines[i:end + 1]) if t])
    return out


def normalise(line):
    line = line.split(";")[0].strip()                         # comments carry block numbers and source positions
    return re.sub(r"\.L([A-Za-z_]+)\d+_(\d+)", r".L\1_\2", line)   # .LBB12_3 -> .LBB_3: the function index is emission order


def main(before, after):
    a, b = kernels(before), kernels(after)
    lost, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    code = sorted(k for k in set(a) & set(b) if a[k][0] != b[k][0])
    desc = sorted(k for k in set(a) & set(b) if a[k][1] != b[k][1])
    for title, names in (("lost", lost), ("new", new), ("instructions differ", code), ("descriptor differs", desc)):
        for k in names:
            print(f"{title}: {k}")
    same = not (lost or new or code or desc)
    print(f"{'IDENTICAL' if same else 'DIFFERENT'}: {len(a)} kernels before, {len(b)} after, "
          f"{sum(len(v[0]) for v in b.values())} instruction lines compared")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
