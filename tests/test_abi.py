"""C-ABI checks that need no GPU: the library loads, exports every symbol include/tensoir_hip.h
declares, the ctypes mirror matches the C struct layout, and argument validation works."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tensoir_hip.h")


@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tir_\w+)\s*\(", src)))


def test_every_declared_symbol_is_exported(lib):
    syms = declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in tensoir_hip.h but not exported"


def test_binding_table_matches_header(lib):
    from tensoir_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    # arity of every prototype
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (_, args) in _lib.SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert m, name
        params = m.group(1).strip()
        n = 0 if params in ("", "void") else params.count(",") + 1
        assert n == len(args), f"{name}: header has {n} parameters, binding {len(args)}"


def test_struct_layout_matches_c(tmp_path, lib):
    from tensoir_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "tensoir_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(TirField), offsetof(TirField, grid), offsetof(TirField, dplane),
         offsetof(TirField, basis_t), offsetof(TirField, occ_nbr), offsetof(TirField, occ_dim), offsetof(TirField, occ_inv),
         offsetof(TirField, occ_hi));
  printf("%zu %zu %zu\n", sizeof(TirMlp), offsetof(TirMlp, feat_dim), offsetof(TirMlp, act));
  printf("%zu %zu\n", sizeof(TirEnvSG), offsetof(TirEnvSG, n_sg));
  return 0; }''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    F, M, E = _lib.TirField, _lib.TirMlp, _lib.TirEnvSG
    assert [int(x) for x in out[0].split()] == [C.sizeof(F), F.grid.offset, F.dplane.offset, F.basis_t.offset,
                                                F.occ_nbr.offset, F.occ_dim.offset, F.occ_inv.offset, F.occ_hi.offset]
    assert [int(x) for x in out[1].split()] == [C.sizeof(M), M.feat_dim.offset, M.act.offset]
    assert [int(x) for x in out[2].split()] == [C.sizeof(E), E.n_sg.offset]


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
