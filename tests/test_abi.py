"""C-ABI checks that need no GPU: the library loads, exports every symbol include/tensoir_hip.h
declares, the binding derived from the header (signatures, struct layouts, constants) equals what the
host compiler makes of the same header, and argument validation works."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def declared_symbols():
    from tensoir_amd import _lib
    return sorted(_lib.SIGNATURES)       # test_binding_matches_the_compiler holds this set to the compiler's


def test_every_declared_symbol_is_exported(lib):
    syms = declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in tensoir_hip.h but not exported"


# ---- the derived binding (tensoir_amd/_lib.py parses the header) against what the host compiler makes of the same header ----
def _run(tmp, name, text, compiler, *flags):
    src = tmp / name
    src.write_text(text)
    exe = tmp / (name + ".exe")
    subprocess.check_call([compiler, *flags, "-I", INCLUDE, str(src), "-o", str(exe)])
    return subprocess.check_output([str(exe)]).decode().splitlines()


_TRAITS = r"""
#include <cstdio>
#include <type_traits>
#include "tensoir_hip.h"
template <class T> void kind() {
  if constexpr (std::is_void_v<T>) std::printf(" v");
  else if constexpr (std::is_pointer_v<T>) std::printf(" p");
  else if constexpr (std::is_floating_point_v<T>) std::printf(" f%zu", sizeof(T));
  else if constexpr (std::is_integral_v<T>) std::printf(" %c%zu", std::is_signed_v<T> ? 'i' : 'u', sizeof(T));
  else static_assert(!sizeof(T), "a parameter that is neither a pointer nor a number");
}
template <class F> struct sig;
template <class R, class... A> struct sig<R (*)(A...)> {
  static void print(const char* name) { std::printf("%s", name); kind<R>(); (kind<A>(), ...); std::printf("\n"); }
};
int main() {
ENTRIES  return 0; }
"""


@pytest.fixture(scope="module")
def compiler_kinds(tmp_path_factory):
    """name -> [return kind, parameter kinds ...] of every bound entry as g++ sees its prototype: p = any pointer, i4 / i8 / u8 =
    integral by size and signedness, f4 / f8 = floating, v = void."""
    from tensoir_amd import _lib
    body = "".join(f'  sig<decltype(&{n})>::print("{n}");\n' for n in _lib.SIGNATURES)
    out = _run(tmp_path_factory.mktemp("sig"), "sig.cpp", _TRAITS.replace("ENTRIES", body), "g++", "-std=c++17")
    return {line.split()[0]: line.split()[1:] for line in out}


def _kind(t):
    if t is None:
        return "v"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "p"
    if t in (C.c_float, C.c_double):
        return f"f{C.sizeof(t)}"
    assert isinstance(t(0).value, int), t
    return f"{'i' if t(-1).value < 0 else 'u'}{C.sizeof(t)}"


def signature_mismatches(signatures, kinds):
    """[(entry, position, binding's kind, compiler's kind)]: position is 'ret', a parameter index or 'arity' (then the counts)."""
    bad = []
    for name, (res, args) in signatures.items():
        want = kinds[name]
        if _kind(res) != want[0]:
            bad.append((name, "ret", _kind(res), want[0]))
        if len(args) != len(want) - 1:
            bad.append((name, "arity", len(args), len(want) - 1))
        bad += [(name, i, _kind(a), w) for i, (a, w) in enumerate(zip(args, want[1:])) if _kind(a) != w]
    return bad


def test_binding_matches_the_compiler(tmp_path, compiler_kinds):
    """Every entry of SIGNATURES: arity, class and width of each parameter and the return type equal the compiler's; and the bound
    names are exactly the functions the compiler finds declared in the header (gcc -aux-info lists them)."""
    from tensoir_amd import _lib
    assert set(compiler_kinds) == set(_lib.SIGNATURES)
    assert signature_mismatches(_lib.SIGNATURES, compiler_kinds) == []
    unit = tmp_path / "unit.c"
    unit.write_text('#include "tensoir_hip.h"\n')
    subprocess.check_call(["gcc", "-I", INCLUDE, "-fsyntax-only", "-aux-info", str(tmp_path / "protos.txt"), str(unit)])
    protos = [ln for ln in (tmp_path / "protos.txt").read_text().splitlines() if "tensoir_hip.h:" in ln]
    declared = [re.search(r"(\w+) \(", ln.split("*/", 1)[1]).group(1) for ln in protos]
    assert sorted(declared) == sorted(_lib.SIGNATURES) and len(declared) >= 138


def test_signature_check_reports_every_kind_of_mistake(compiler_kinds):
    """The comparison above is not vacuous: a widened integer, a double for a float, an integer for a pointer, a dropped argument
    and a changed return type are each reported, by entry and by position."""
    from tensoir_amd import _lib

    def first(pred):
        return next((n, i) for n, (_, args) in _lib.SIGNATURES.items() for i, a in enumerate(args) if pred(a))

    def perturbed(name, res=..., args=None):
        sigs = dict(_lib.SIGNATURES)
        sigs[name] = (sigs[name][0] if res is ... else res, list(sigs[name][1]) if args is None else args)
        return sigs

    def swap(where, t):
        name, i = where
        args = list(_lib.SIGNATURES[name][1])
        args[i] = t
        return signature_mismatches(perturbed(name, args=args), compiler_kinds)

    n, i = where = first(lambda a: a is C.c_int32)
    assert swap(where, C.c_int64) == [(n, i, "i8", "i4")]
    n, i = where = first(lambda a: a is C.c_float)
    assert swap(where, C.c_double) == [(n, i, "f8", "f4")]
    n, i = where = first(lambda a: a is C.c_void_p)
    assert swap(where, C.c_int64) == [(n, i, "i8", "p")]
    n, i = where = first(lambda a: issubclass(a, C._Pointer))
    assert swap(where, C.c_int64) == [(n, i, "i8", "p")]
    args = _lib.SIGNATURES["tir_exclusive_scan"][1]
    assert signature_mismatches(perturbed("tir_exclusive_scan", args=args[:-1]), compiler_kinds) == [("tir_exclusive_scan", "arity", 3, 4)]
    got = signature_mismatches(perturbed("tir_exclusive_scan", args=args[:1] + args[2:]), compiler_kinds)   # dropped in the middle
    assert ("tir_exclusive_scan", "arity", 3, 4) in got and ("tir_exclusive_scan", 1, "i4", "p") in got
    assert signature_mismatches(perturbed("tir_mlp_packed_floats", res=C.c_int), compiler_kinds) == [("tir_mlp_packed_floats", "ret", "i4", "i8")]
    assert signature_mismatches(perturbed("tir_version", res=C.c_char_p), compiler_kinds) == [("tir_version", "ret", "p", "i4")]


def test_struct_layout_matches_c(tmp_path):
    """sizeof of every struct the binding derived, offsetof and size of every field: the C compiler's against ctypes'."""
    from tensoir_amd import _lib
    assert {"TirField", "TirFieldHalf", "TirFieldGrad", "TirMlp", "TirEnvSG", "TirHalfJob", "TirHalfJobs"} <= set(_lib.STRUCTS)
    lines, want = [], []
    for name, S in _lib.STRUCTS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {C.sizeof(S)}")
        for f, _ in S._fields_:
            lines.append(f'  printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));')
            want.append(f"{name}.{f} {getattr(S, f).offset} {getattr(S, f).size}")
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tensoir_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0; }\n"
    assert _run(tmp_path, "layout.c", prog, "gcc") == want
    assert len(_lib.TirField._fields_) == 34 and _lib.TirField._fields_[-1][0] == "dense_app"


def test_constants_match_c(tmp_path):
    """Every #define the binding published: the C compiler's value, exactly (integers as long long, floating values in hex), and
    its class; and no TIR_* macro is missing but the brace list, which the parser must skip."""
    from tensoir_amd import _lib
    lines = []
    for name, v in _lib.CONST.items():
        cls = f'_Generic(({name}), float: "f", double: "f", default: "i")'
        lines.append(f'  printf("{name} %s %lld\\n", {cls}, (long long)({name}));' if isinstance(v, int) else
                     f'  printf("{name} %s %a\\n", {cls}, (double)({name}));')
    prog = '#include <stdio.h>\n#include "tensoir_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0; }\n"
    got = {}
    for line in _run(tmp_path, "const.c", prog, "gcc", "-std=c11"):
        name, cls, text = line.split()
        got[name] = int(text) if cls == "i" else float.fromhex(text)
    assert got.keys() == _lib.CONST.keys()
    for name, v in _lib.CONST.items():
        assert type(got[name]) is type(v) and got[name] == v, (name, v, got[name])
    assert _lib.CONST["TIR_ERR_ARG"] == -1001 and _lib.CONST["TIR_DISTANCE_SLACK"] == 2.0 ** -13 and _lib.CONST["TIR_MAP_STRIDE"] == 20
    macros = subprocess.check_output(["gcc", "-dM", "-E", "-I", INCLUDE, os.path.join(INCLUDE, "tensoir_hip.h")]).decode()
    assert set(re.findall(r"^#define (TIR_\w+)", macros, flags=re.M)) == set(_lib.CONST) | {"TIR_RAY_INSIDE_DIRECTIONS"}


@pytest.mark.parametrize("text, names", [
    ("int tir_f(size_t n);", "size_t n"),                                                # an unknown type
    ("typedef struct TirA { quad q; } TirA;", "quad q"),
    ("typedef struct TirA { float v[TIR_N]; } TirA;", "float v[TIR_N]"),                 # a length that is no number and no macro
    ("#define TIR_N 1.5\ntypedef struct TirA { float v[TIR_N]; } TirA;", "float v[TIR_N]"),
    ("int tir_f(int32_t n, void (*)(int));", "tir_f"),                                   # an unnamed function-pointer parameter
    ("int tir_f(int32_t);", "int32_t"),                                                  # an unnamed parameter
    ("int tir_f(int32_t n[3]);", "int32_t n[3]"),
    ("int tir_f(TirA a);", "TirA a"),
    ("#if TIR_X\nint tir_f(void);\n#endif", "#if TIR_X"),                                # conditional text would be a guess
])
def test_parser_refuses_what_it_cannot_read(text, names):
    from tensoir_amd import _lib
    with pytest.raises(_lib.TensoirHipError, match=re.escape(names)):
        _lib.parse_header(text)


def test_parser_reads_the_subset():
    from tensoir_amd import _lib
    const, structs, sigs = _lib.parse_header("""/* a comment; with, punctuation ( */
#define TIR_N 2
#define TIR_Q (1.0 / 4.0)
#define TIR_LIST {1, 2}
typedef struct TirA { const float* p[TIR_N]; float near_, far_; unsigned* u; } TirA;
typedef struct TirB { TirA a[3]; int64_t n; } TirB;
const char* tir_name(int code);
int64_t tir_f(const TirA* a, const TirB* const* bs, unsigned long long* stats,
              double x, uint64_t seed, void* stream);
void tir_g(void);
""")
    assert const == {"TIR_N": 2, "TIR_Q": 0.25}
    A, B = structs["TirA"], structs["TirB"]
    assert [(n, t) for n, t in A._fields_] == [("p", C.c_void_p * 2), ("near_", C.c_float), ("far_", C.c_float), ("u", C.c_void_p)]
    assert B._fields_ == [("a", A * 3), ("n", C.c_int64)] and C.sizeof(B) == 3 * C.sizeof(A) + 8
    assert sigs == {"tir_name": (C.c_char_p, [C.c_int]),
                    "tir_f": (C.c_int64, [C.POINTER(A), C.c_void_p, C.c_void_p, C.c_double, C.c_uint64, C.c_void_p]),
                    "tir_g": (None, [])}


def test_missing_header_is_named():
    """TENSOIR_HIP_HEADER overrides the path; a header that is not there raises at import, naming the path."""
    env = dict(os.environ, TENSOIR_HIP_HEADER="/nonexistent/tensoir_hip.h")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tensoir_amd", "_lib.py")], env=env, capture_output=True, text=True)   # _lib alone
    assert p.returncode != 0 and "TensoirHipError" in p.stderr and "/nonexistent/tensoir_hip.h" in p.stderr, p.stderr


def test_version_and_errors(lib):
    assert lib.tir_version() == 100
    assert b"invalid argument" in lib.tir_error_string(-1001)
    assert b"not supported" in lib.tir_error_string(-1002)
    # argument validation happens before any device work, so it is testable without a GPU
    assert lib.tir_pack_plane(None, None, 16, 8, 8, None) == -1001
    assert lib.tir_vm_density_fwd(None, None, None, None, 10, None) == -1001
    assert lib.tir_exclusive_scan(None, None, 4, None) == -1001
    assert lib.tir_exclusive_scan(None, None, 0, None) == -1001   # offsets is always required
    assert lib.tir_mlp_packed_floats(27, 2, 128, 4) > 36000
    assert lib.tir_mlp_packed_floats(27, 6, 128, 4) == -1002      # only pe=2 / 27 / 128 are built
    assert lib.tir_mlp_packed_floats(27, 2, 64, 3) == -1002


def test_round5_entry_points_validate_before_any_device_work(lib):
    """The entries added in round 5 (and the guards ADVICE r4 asked for) reject bad arguments on the host: plane element
    offsets of the fp16 gathers (32-bit, 24-bit index multiplies), tir_pack_half_checked's report buffer, the device-bounded C5
    entries and the compaction / compose kernels."""
    from tensoir_amd import _lib
    import torch
    # a field whose plane would need > 2^31 element offsets / a row pitch beyond the 24-bit multiplier: UNSUPPORTED, not garbage
    keep = torch.zeros(64, dtype=torch.float32)                       # any non-null, 16-byte aligned host address: never dereferenced
    ptr = keep.data_ptr()
    assert ptr % 16 == 0
    m = _lib.TirMlp(ptr, 27, 2, 128, 3, 0, 0)
    for grid, want in (((70000, 70000, 8), -1002), ((400000, 8, 8), -1002)):
        f = _lib.TirField()
        f.grid[:] = grid
        f.n_dcomp, f.n_acomp, f.app_dim, f.n_lights = 16, 48, 27, 1
        f.basis_t = f.light_line = f.light_mean = ptr
        fh = _lib.TirFieldHalf()
        for i in range(3):
            fh.aplane[i] = fh.aline[i] = ptr
        assert lib.tir_vm_app_fwd_h16(C.byref(f), C.byref(fh), ptr, ptr, None, ptr, 32, 0, 10, None, None) == want, grid
        assert lib.tir_indirect_fused_fwd(C.byref(f), C.byref(fh), C.byref(m), ptr, ptr, None, 1, 1, ptr, ptr, 10, None, None) == want, grid
    # tir_pack_half_checked: the report buffer is mandatory, a scan-only table needs it, at most TIR_HALF_MAX_JOBS tables
    one = (C.c_void_p * 1)(ptr)
    none = (C.c_void_p * 1)(None)
    cnt = (C.c_int64 * 1)(8)
    assert lib.tir_pack_half_checked(one, one, cnt, 1, None, None) == -1001
    assert lib.tir_pack_half(one, none, cnt, 1, None) == -1001                    # nothing to write, nowhere to report
    nine = (C.c_void_p * 9)(*([ptr] * 9))
    assert lib.tir_pack_half_checked(nine, nine, (C.c_int64 * 9)(*([8] * 9)), 9, ptr, None) == -1001
    assert lib.tir_pack_half_checked(one, one, (C.c_int64 * 1)(0), 1, ptr, None) == 0          # empty tables: nothing to do
    # C5 chunk entries
    assert lib.tir_surface_compact(None, None, 4, 0.5, None, None, None, None, None, None, None, None, None) == -1001
    assert lib.tir_surface_compact(ptr, ptr, -1, 0.5, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None) == -1001
    assert lib.tir_env_compose(ptr, 8, 16, ptr, 2, 4, ptr, ptr, ptr, 3, None) == -1001        # dir_stride < 3
    assert lib.tir_env_compose(ptr, 8, 16, ptr, 6, 4, None, ptr, ptr, 3, None) == -1001       # no slot map
    assert lib.tir_env_compose(ptr, 8, 16, ptr, 6, 0, ptr, ptr, ptr, 3, None) == 0            # n = 0
    assert lib.tir_relight_importance_cells_packed_n(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 0, 512, ptr, None, None) == 0
    assert lib.tir_relight_importance_cells_packed_n(ptr, ptr, ptr, ptr, ptr, ptr, None, ptr, 4, 512, ptr, None, None) == -1001
    assert lib.tir_env_sample_setup_list_n(ptr, ptr, 8, 16, ptr, 8, ptr, 4, 512, 1, 1, 16, 17, 512, None, None, 0, 0, ptr, ptr, ptr, ptr,
                                           None, None) == -1002                                # 16 x 17 = 272 bins > 255


def test_no_gpu_no_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tensoir_amd import _lib, ops
    assert lib.tir_device_check() == -1003
    with pytest.raises(_lib.TensoirHipError):
        ops.pack_plane(torch.zeros(1, 16, 8, 8))


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under tensoir_amd/ (or bench's product leg) may import it."""
    bad = []
    for dp, _, fs in os.walk(os.path.join(ROOT, "tensoir_amd")):
        for f in fs:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M) or "tensoir_oracle" in txt:
                    bad.append(f)
    assert not bad, bad


def test_hot_kernels_keep_their_register_budget(lib):
    """DESIGN 4.1's occupancy statements as a build check (no GPU): the kernels of the bench step hold no scratch object and fit the
    VGPR budget their waves-per-SIMD figure needs (tools/kernel_resources.py reads the gfx950 code object's metadata).  A PE array
    that became a scratch object cost round 4 0.4 GB of scratch writes per launch; the 1024-thread march spilled one register in
    the first tap-record version of round 6."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from tensoir_amd import _lib
    ks = {k["name"]: k for k in kernel_resources.kernels(_lib.LIB_PATH)}
    budget = {"k_march_secondary_lds<4, 3, 512, true>": 128, "k_march_secondary_lds<4, 3, 1024, true>": 128,      # 4 waves per SIMD
              "k_march_secondary_lds<4, 3, 512, false>": 128, "k_march_secondary_lds<4, 3, 1024, false>": 128,  # (visibility only)
              "k_indirect_fused<12, true>": 168,                                                         # 3 waves per SIMD
              "k_indirect_fused_hp<8>": 256, "k_mlp_bf16_multi<3, false>": 256, "k_vm_app_primary<12, false>": 256,
              "k_march_primary": 256, "k_shade_integrate": 256}
    for name, vgpr in budget.items():
        assert name in ks, (name, sorted(ks)[:5])
        k = ks[name]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert k["vgpr"] + k["agpr"] <= vgpr, k
    # the only kernels allowed a scratch object: the fp32 VALU fallback decoder, the backward decoders (4 spilled registers), the
    # rarely used hidden-saving aux-table decoder and the 16-lane scatter of the wide (24 / 96-channel) appearance grids
    allowed = ("k_mlp_valu", "k_mlp_bwd_bf16", "k_mlp_bf16_auxt<false, true>", "k_mlp_bf16_auxt<true, true>", "k_vm_app_bwd<")
    bad = [k for k in ks.values() if k["scratch"] and not k["name"].startswith(allowed)]
    assert not bad, bad


# ---- the configuration matrix (tests/config_scenes.py): what needs no GPU -----------------------------------------------------
def _host_packing(monkeypatch):
    """packed_field() fills the descriptor's scalars on the host; its derived tables (basis_mat^T, mean light row) are device
    kernels, replaced here by host stand-ins that are never read."""
    from tensoir_amd import ops
    monkeypatch.setattr(ops, "pack_basis", lambda w: w.detach().t().contiguous())
    monkeypatch.setattr(ops, "light_mean", lambda ll: ll.mean(0))


def _matrix_rows():
    from tests import config_scenes as CS
    return [r.name for r in CS.ROWS]


@pytest.mark.parametrize("name", _matrix_rows())
def test_packed_field_scalars_per_configuration(monkeypatch, name):
    import tensoir_amd
    from tests import config_scenes as CS
    row = CS.ROW[name]
    m = tensoir_amd.model_from_checkpoint(CS.checkpoint(row), "cpu", envmap_h=CS.ENVMAP_HW[0], envmap_w=CS.ENVMAP_HW[1])
    _host_packing(monkeypatch)
    f = m.packed_field()
    assert (int(f.n_dcomp), int(f.n_acomp), int(f.n_lights), int(f.app_dim)) == (row.n_dcomp, row.n_acomp, row.n_lights, 27)
    assert int(f.act) == {"softplus": 0, "relu": 1}[row.act]
    assert [int(g) for g in f.grid] == CS.GRID
    assert float(f.density_shift) == -10.0 and float(f.distance_scale) == 25.0
    assert all(int(f.dplane[i]) and int(f.dline[i]) and int(f.aplane[i]) and int(f.aline[i]) for i in range(3))
    for i in range(3):                      # the planes are gathered in place, channel-last: component stride 1
        assert m.density_plane[i].shape[1] == row.n_dcomp and m.density_plane[i].stride(1) == 1
        assert m.app_plane[i].shape[1] == row.n_acomp and m.app_plane[i].stride(1) == 1
        assert int(f.dplane[i]) == m.density_plane[i].data_ptr() and int(f.aplane[i]) == m.app_plane[i].data_ptr()


@pytest.mark.parametrize("which", ["density", "appearance"])
def test_packed_field_refuses_unequal_per_plane_counts(monkeypatch, which):
    import torch
    import tensoir_amd
    from tensoir_amd._lib import TensoirHipError
    from tests import config_scenes as CS
    kw = dict(density_n_comp=[16, 16, 16], appearance_n_comp=[48, 48, 48], shadingMode="MLP_Fea")
    kw["density_n_comp" if which == "density" else "appearance_n_comp"] = [16, 8, 16] if which == "density" else [48, 24, 48]
    m = tensoir_amd.TensorVMSplit(torch.tensor(CS.AABB), CS.GRID, "cpu", **kw)
    _host_packing(monkeypatch)
    with pytest.raises(TensoirHipError, match="per-plane component counts"):
        m.packed_field()


def test_constructor_default_configuration_round_trips():
    """TensorVMSplit's own defaults are 8 density / 24 appearance components per plane: the model builds on the host, and its
    kwargs + state_dict rebuild the same model."""
    import torch
    import tensoir_amd
    from tests import config_scenes as CS
    torch.manual_seed(5)
    m = tensoir_amd.TensorVMSplit(torch.tensor(CS.AABB), CS.GRID, "cpu", shadingMode="MLP_Fea")
    assert list(m.density_n_comp) == [8, 8, 8] and list(m.app_n_comp) == [24, 24, 24] and m.fea2denseAct == "softplus"
    kw = m.get_kwargs()
    assert list(kw["density_n_comp"]) == [8, 8, 8] and list(kw["appearance_n_comp"]) == [24, 24, 24]
    m2 = tensoir_amd.model_from_checkpoint({"kwargs": kw, "state_dict": m.state_dict()}, "cpu")
    assert m2.get_kwargs().keys() == kw.keys()
    for k, v in kw.items():
        w = m2.get_kwargs()[k]
        assert (torch.equal(torch.as_tensor(v), torch.as_tensor(w)) if not isinstance(v, str) else v == w), k
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert sd["density_plane.0"].shape[1] == 8 and sd["app_plane.0"].shape[1] == 24 and sd["basis_mat.weight"].shape == (27, 72)


def test_launchers_refuse_unlisted_component_counts(lib):
    """No entry runs another width's kernel for a count it has no instantiation for: the density entries refuse anything but
    4 / 8 / 16 / 32, the appearance gathers anything but their own list (96 has only the fp32 gather), the merged / fp16 / fused
    entries anything but 48 -- all on the host, before any device work."""
    import torch
    from tensoir_amd import _lib
    # The pointers are HOST addresses and n > 0 (n = 0 returns OK before the checks): every call below must be refused on the host.
    # Only counts the launchers REFUSE belong in these loops -- an accepted count would launch a kernel on host memory where a GPU
    # is present.
    keep = torch.zeros(64, dtype=torch.float32)
    ptr = keep.data_ptr()

    def field(n_dcomp, n_acomp):
        f = _lib.TirField()
        f.grid[:] = (20, 24, 28)
        f.n_dcomp, f.n_acomp, f.app_dim, f.n_lights = n_dcomp, n_acomp, 27, 3
        f.basis_t = f.light_line = f.light_mean = ptr
        for i in range(3):
            f.dplane[i] = f.dline[i] = f.aplane[i] = f.aline[i] = ptr
        return f
    g = _lib.TirFieldGrad()
    for i in range(3):
        g.dplane[i] = g.dline[i] = g.aplane[i] = g.aline[i] = ptr
    for nd in (1, 2, 12, 24, 64):
        f = field(nd, 48)
        assert lib.tir_vm_density_fwd(C.byref(f), ptr, ptr, ptr, 8, None) == -1002, nd
        assert lib.tir_density_grad_fwd(C.byref(f), ptr, ptr, ptr, ptr, 8, None, None) == -1002, nd
        assert lib.tir_density_feat_grad_fwd(C.byref(f), ptr, ptr, ptr, 8, None) == -1002, nd
        assert lib.tir_density_grad_bwd(C.byref(f), C.byref(g), ptr, ptr, 8, None) == -1002, nd
        assert lib.tir_vm_density_bwd(C.byref(f), C.byref(g), ptr, ptr, 8, None) == -1002, nd
    accepted = {"tir_vm_app_fwd": (16, 24, 48, 96), "tir_vm_app_fwd_valu": (16, 24, 48, 96), "tir_vm_app_fwd_bf16x3": (16, 24, 48),
                "tir_vm_app_fwd_x3": (16, 24, 48)}
    for entry, ok in accepted.items():
        for na in (8, 12, 32, 64, 96, 192):
            if na in ok:
                continue
            f = field(16, na)
            assert getattr(lib, entry)(C.byref(f), ptr, ptr, None, ptr, ptr, 32, 0, 8, None, None) == -1002, (entry, na)
    fh = _lib.TirFieldHalf()
    for i in range(3):
        fh.aplane[i] = fh.aline[i] = ptr
    mlp = _lib.TirMlp(ptr, 27, 2, 128, 3, 0, 0)
    for na in (16, 24, 96):
        f = field(16, na)
        assert lib.tir_vm_app_fwd_h16(C.byref(f), C.byref(fh), ptr, ptr, None, ptr, 32, 0, 8, None, None) == -1002, na
        assert lib.tir_indirect_fused_fwd(C.byref(f), C.byref(fh), C.byref(mlp), ptr, ptr, None, 1, 1, ptr, ptr, 8, None, None) == -1002, na
        assert lib.tir_vm_app_primary_fwd(C.byref(f), ptr, ptr, None, ptr, ptr, 32, 8, None, 0.01, 0, 0, None, ptr, ptr, None) == -1002, na
        assert lib.tir_vm_app_primary_x3_fwd(C.byref(f), ptr, ptr, None, ptr, ptr, 32, 8, None, 0.01, 0, 0, None, ptr, ptr, None) == -1002, na
