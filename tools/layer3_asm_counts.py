"""Static instruction counts of the layer-3 block of the decoder kernels in a gfx950 assembly listing of tir_mlp.hip
(hipcc with the flags of csrc/build.sh plus `--cuda-device-only -S`; no GPU needed).
Usage: python tools/layer3_asm_counts.py tir_mlp.s
Per kernel: the small matrix instructions (v_mfma_f32_4x4x1), the fp32 adds with an |abs| source, the v_max_i32, and, between
consecutive small matrix instructions, the s_nop instructions, the wait states they stand for (s_nop N = N + 1) and the VALU
instructions."""
import json
import re
import subprocess
import sys

KERNELS = ("k_indirect_fused_dense<12>", "k_indirect_fused<12, true>", "k_indirect_fused_hp<8>", "k_mlp_bf16_multi<3, false>")


def bodies(path):
    name, lines, out = None, [], {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, lines = m.group(1), []
        elif name and line.startswith("\t.end_amdhsa_kernel"):
            out[name] = lines
            name = None
        elif name:
            lines.append(line.strip())
    return out


def counts(lines):
    mf = [i for i, s in enumerate(lines) if s.startswith("v_mfma_f32_4x4x1")]
    c = {"mfma_4x4x1": len(mf), "v_add_f32_abs": sum(1 for s in lines if s.startswith("v_add_f32") and "|" in s),
         "v_max_i32": sum(1 for s in lines if s.startswith("v_max_i32"))}
    # a kernel may hold more than one layer-3 block (k_mlp_bf16_multi: one per decoder form): only the gaps between two small
    # matrix instructions fewer than 16 lines apart are layer 3
    block = [s for a, b in zip(mf, mf[1:]) if b - a < 16 for s in lines[a + 1:b]]
    nops = [int(s.split()[1]) + 1 for s in block if s.startswith("s_nop")]
    c["s_nop_in_block"], c["wait_states_in_block"] = len(nops), sum(nops)
    c["valu_in_block"] = sum(1 for s in block if s.startswith("v_") and not s.startswith("v_mfma"))
    return c


if __name__ == "__main__":
    res = {}
    for mangled, lines in bodies(sys.argv[1]).items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
        if name in KERNELS:
            res[name] = counts(lines)
    print(json.dumps(res, indent=1))
