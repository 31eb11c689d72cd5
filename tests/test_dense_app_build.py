"""Build-level checks of the dense appearance-volume route (no GPU): the register budget of the new kernels, the descriptor
mirror, and the host-side argument validation of the entries run as a stand-alone program under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensoir_amd", "csrc")


def test_dense_kernels_keep_their_register_budget():
    """k_indirect_fused_dense<12> runs three waves per SIMD like the kernel it stands in for (<= 168 VGPRs + AGPRs, nothing in
    scratch); the build kernel and the gather entry's lookup kernel hold no scratch object either."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from tensoir_amd import _lib
    ks = {k["name"]: k for k in kernel_resources.kernels(_lib.LIB_PATH)}
    k = ks["k_indirect_fused_dense<12>"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["vgpr"] + k["agpr"] <= 168, k
    for name in ("k_dense_app_build", "k_vm_app_dense"):
        assert ks[name]["scratch"] == 0 and ks[name]["vgpr_spill"] == 0, ks[name]
    old = ks["k_indirect_fused<12, true>"]                   # the shadow-tap kernel stays in the library, within its budget
    assert old["scratch"] == 0 and old["vgpr"] + old["agpr"] <= 168, old


def test_descriptor_mirror_agrees_with_the_header(tmp_path):
    """sizeof(TirField) and the offsets of the dense members: C header against the ctypes mirror."""
    from tensoir_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tensoir_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(TirField), offsetof(TirField, dense_sigma),\n'
                   '    offsetof(TirField, dense_pitch), offsetof(TirField, dense_app_pitch), offsetof(TirField, dense_app)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    F = _lib.TirField
    assert got == [C.sizeof(F), F.dense_sigma.offset, F.dense_pitch.offset, F.dense_app_pitch.offset, F.dense_app.offset]


def test_entry_validation_under_sanitizers(tmp_path):
    """tests/c/dense_app_validate.cpp: null volume, a pitch without a volume, n = 0, 4 GiB, several lights -> the -100x codes.
    The host code of tir_dense_app.hip / tir_field.hip / tir_mlp.hip is compiled with -fsanitize=address,undefined (device code
    as usual) and linked into a program with its own main; nothing sanitized is loaded into this interpreter, and the program needs no GPU."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    clangxx = "/opt/rocm/lib/llvm/bin/clang++"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    flags = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-Wno-unused-function"]
    for s in san:
        flags += ["-Xarch_host", s]
    procs, objs = [], []
    for stem in ("tir_dense_app", "tir_field", "tir_mlp"):
        objs.append(str(tmp_path / f"{stem}.o"))
        procs.append(subprocess.Popen([hipcc] + flags + ["-c", os.path.join(CSRC, f"{stem}.hip"), "-o", objs[-1]]))
    assert [p.wait() for p in procs] == [0, 0, 0]
    exe = str(tmp_path / "dense_app_validate")
    subprocess.check_call([clangxx, "-std=c++17", "-g"] + san + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "dense_app_validate.cpp")] + objs +
                          ["-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    assert run.returncode == 0 and "dense_app validation ok" in out, out
