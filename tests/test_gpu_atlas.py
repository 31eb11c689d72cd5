"""The texture atlas on the GPU (tir_atlas_corners / _texels / _pack, ops.atlas_*, mesh.bake_atlas / export_textured, the bake
command line with --texture-size) against the numpy restatement (tests/atlas_reference.py).

Comparison rules.  face, uv and the copied pos / nrm are discrete or copies and must be equal bit for bit.  point, outward and the
tangent must agree with the float64 restatement within ten times the distance of the restatement run wholly in float32 from its
float64 self over the same meshes and sizes (tests/test_atlas_cpu.py measures it: 1.16e-7 of the largest |coordinate| for point,
1.20e-7 per component for outward, 3.52e-7 for the tangent): POINT_TOL = 1.2e-6, OUTWARD_TOL = 1.2e-6, TAN_TOL = 3.6e-6 -- the
device may contract the three-term sums into fused multiply-adds and associate them differently.  The packed images are bytes:
within 0.5 + 1e-3 of 255 x the float64 value, and equal to its rounding on inputs that keep 1e-2 from every rounding boundary."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import atlas_reference as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_TOL, OUTWARD_TOL, TAN_TOL = A.POINT_TOL, A.OUTWARD_TOL, A.TAN_TOL


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def device_mesh(v, n, f):
    return dev(v, np.float32).reshape(-1, 3), dev(n, np.float32).reshape(-1, 3), dev(f, np.int32).reshape(-1, 3)


def bits(t):
    return t.contiguous().view(torch.int32)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


CASES = [(name, size) for name, c in A.layout_cases().items() for size in c[3]]


@pytest.mark.parametrize("name, size", CASES)
def test_layout_kernels_equal_restatement_and_repeat(name, size):
    from tensoir_amd import ops
    v, n, f, _ = A.layout_cases()[name]
    F = len(f)
    cols, T = ops.atlas_layout(F, size)
    assert (cols, T) == A.layout(F, size)
    dv, dn, df = device_mesh(v, n, f)
    got_c = ops.atlas_corners(dv, dn, df, size, cols, T)
    got_t = ops.atlas_texels(dv, dn, df, size, cols, T)
    again_c = ops.atlas_corners(dv, dn, df, size, cols, T)
    again_t = ops.atlas_texels(dv, dn, df, size, cols, T)
    torch.cuda.synchronize()
    N = ((F + 1) // 2) * T * T
    assert [tuple(t.shape) for t in got_c] == [(3 * F, 3), (3 * F, 3), (3 * F, 4), (3 * F, 2)]
    assert [tuple(t.shape) for t in got_t] == [(N, 3), (N, 3), (N,)] and got_t[2].dtype == torch.int32
    for a, b in zip(got_c + got_t, again_c + again_t):
        assert torch.equal(bits(a), bits(b))
    pos, nrm, tan, uv = (t.cpu().numpy() for t in got_c)
    point, outward, face = (t.cpu().numpy() for t in got_t)
    rpos, rnrm, rtan, ruv = A.corners(v, n, f, size, cols, T)
    rpoint, routward, rface, _ = A.texels(v, n, f, cols, T)
    assert np.array_equal(face, rface)
    assert np.array_equal(u32(uv), u32(ruv)) and np.array_equal(u32(pos), u32(rpos)) and np.array_equal(u32(nrm), u32(rnrm))
    dp = np.abs(point - rpoint).max() / np.abs(v).max()
    do = np.abs(outward - routward).max()
    dt = np.abs(tan - rtan).max()
    print(f"\n[atlas {name} size {size}] F {F} cols {cols} T {T} texels {N}: point {dp:.2e} of the largest coordinate, outward "
          f"{do:.2e}, tangent {dt:.2e}")
    assert dp <= POINT_TOL and do <= OUTWARD_TOL and dt <= TAN_TOL
    assert (tan[:, 3] == 1).all()
    if name == "sphere":
        assert F > 3000 and N > 20 * 256                       # many blocks, and a last one that is not full
        assert N % 256 != 0


def test_unaligned_outputs_take_the_scalar_route():
    """The 16-byte stores need 16-byte aligned outputs; a caller's odd view gets the 4-byte route and the same values."""
    from tensoir_amd import _lib, ops
    v, n, f, _ = A.layout_cases()["F7"]
    dv, dn, df = device_mesh(v, n, f)
    cols, T = ops.atlas_layout(7, 27)
    point, outward, face = ops.atlas_texels(dv, dn, df, 27, cols, T)
    N = point.shape[0]
    buf = torch.zeros((2, 3 * N + 1), dtype=torch.float32, device="cuda")
    status = torch.zeros((1,), dtype=torch.int32, device="cuda")
    face2 = torch.empty_like(face)
    p2, o2 = buf[0, 1:], buf[1, 1:]
    assert p2.data_ptr() % 16 == 4
    _lib.check(_lib.lib().tir_atlas_texels(dv.data_ptr(), 9, dn.data_ptr(), df.data_ptr(), 7, 27, cols, T, p2.data_ptr(), o2.data_ptr(),
                                           face2.data_ptr(), status.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(bits(p2), bits(point.view(-1))) and torch.equal(bits(o2), bits(outward.view(-1))) and torch.equal(face, face2)
    assert int(status.item()) == 0 and float(buf[:, 0].abs().max()) == 0.0


def test_no_faces_and_bad_face_indices():
    from tensoir_amd import ops
    from tensoir_amd._lib import TensoirHipError
    v, n, f, _ = A.layout_cases()["F2"]
    dv, dn, df = device_mesh(v, n, f)
    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    cols, T = ops.atlas_layout(0, 12)
    assert [tuple(t.shape) for t in ops.atlas_corners(dv, dn, none, 12, cols, T)] == [(0, 3), (0, 3), (0, 4), (0, 2)]
    assert [tuple(t.shape) for t in ops.atlas_texels(dv, dn, none, 12, cols, T)] == [(0, 3), (0, 3), (0,)]
    z3, z1 = torch.zeros((0, 3), device="cuda"), torch.zeros((0,), device="cuda")
    base, orm, normal = ops.atlas_pack(dv, dn, none, 12, cols, T, z3, z1, z3, z1)
    for img, key in ((base, "base"), (orm, "orm"), (normal, "normal")):
        assert img.shape == (12, 12, 4) and img.dtype == torch.uint8 and (img.cpu().numpy() == A.UNOWNED[key]).all()
    for bad in ([[0, 1, 4], [1, 2, 3]], [[0, 1, 2], [1, -1, 3]]):
        dbad = dev(np.int32(bad), np.int32)
        with pytest.raises(TensoirHipError, match="face index"):
            ops.atlas_corners(dv, dn, dbad, 12, 1, 12)
        with pytest.raises(TensoirHipError, match="face index"):
            ops.atlas_texels(dv, dn, dbad, 12, 1, 12)
        ones3, ones1 = torch.ones((144, 3), device="cuda"), torch.ones((144,), device="cuda")
        with pytest.raises(TensoirHipError, match="face index"):
            ops.atlas_pack(dv, dn, dbad, 12, 1, 12, ones3, ones1, ones3, ones1)
    with pytest.raises(TensoirHipError):                                       # the library's own refusal: cols * T > size
        ops.atlas_texels(dv, dn, df, 12, 2, 7)
    with pytest.raises(ValueError, match="rows"):
        ops.atlas_pack(dv, dn, df, 12, 1, 12, torch.ones((5, 3), device="cuda"), torch.ones((144,), device="cuda"),
                       torch.ones((144, 3), device="cuda"), torch.ones((144,), device="cuda"))
    with pytest.raises(TensoirHipError):                                       # host tensors: no fallback
        ops.atlas_texels(dv.cpu(), dn.cpu(), df.cpu(), 12, 1, 12)


@pytest.mark.parametrize("variant", list(A.PACK_VARIANTS))
def test_pack_kernel_writes_the_rounded_float64_values(variant):
    """Size 27, five faces (T = 13, an odd last face, an unused cell, an unused last row and column), per-texel inputs that keep
    every channel's float64 value at least 1e-2 / 255 from a rounding boundary: the bytes must equal the rounded float64 values,
    every one; unowned texels hold their constants; a second call gives the same bytes."""
    from tensoir_amd import ops
    case = A.pack_case()
    opt = A.PACK_VARIANTS[variant]
    dv, dn, df = device_mesh(case["verts"], case["normals"], case["faces"])
    t = {k: dev(case[k], np.float32) for k in ("albedo", "irradiance", "roughness", "ao", "normal", "coverage")}
    call = lambda: ops.atlas_pack(dv, dn, df, A.PACK_SIZE, case["cols"], case["T"], t["albedo"], t["roughness"], t["normal"], t["coverage"],
                                  irradiance=t["irradiance"] if opt["diffuse"] else None, ao=t["ao"] if opt["ao"] else None)
    got, again = call(), call()
    torch.cuda.synchronize()
    want, owned = A.pack_variant(case, variant)
    for img, img2, key in zip(got, again, ("base", "orm", "normal")):
        assert img.shape == (27, 27, 4) and img.dtype == torch.uint8 and torch.equal(img, img2)
        a = img.cpu().numpy()
        err = np.abs(a.astype(np.float64) - want[key])
        print(f"\n[atlas pack {variant}] {key}: max |byte - 255 x float64 value| {err.max():.4f}, owned texels {int(owned.sum())}")
        assert err.max() <= 0.5 + 1e-3
        assert np.array_equal(a, np.clip(np.rint(want[key]), 0, 255).astype(np.uint8)), key
        assert (a[~owned] == A.UNOWNED[key]).all() and (a[..., 3] == 255).all()
    if not opt["ao"]:
        assert (got[1].cpu().numpy()[owned][:, 0] == 255).all()
    dark = np.zeros((27, 27), bool)
    c, j, i, _, _ = A.texel_index(5, case["cols"], case["T"])
    dark[(c // 2) * 13 + j, (c % 2) * 13 + i] = case["coverage"] <= 0.5
    assert dark.sum() > 20 and (got[2].cpu().numpy()[dark] == (128, 128, 255, 255)).all()


# ---- end to end on a trained field ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    from tests.train_sequence import reconstruct
    return reconstruct()


def bilinear(img, u, v):
    """A LINEAR / CLAMP_TO_EDGE lookup of an [S, S, C] image at glTF uv -> ([C] float64, the four taps (i, j))."""
    S = img.shape[0]
    x, y = u * S - 0.5, v * S - 0.5
    i0, j0 = int(np.floor(x)), int(np.floor(y))
    fx, fy = x - i0, y - j0
    out, taps = np.zeros(img.shape[2]), []
    for dj, wy in ((0, 1 - fy), (1, fy)):
        for di, wx in ((0, 1 - fx), (1, fx)):
            i, j = min(max(i0 + di, 0), S - 1), min(max(j0 + dj, 0), S - 1)
            out += wx * wy * img[j, i]
            taps.append((i, j))
    return out, taps


def test_export_textured_on_trained_field(trained, tmp_path):
    """export_textured(simplify=3, size=256): the file's positions are the simplified mesh's corners bit for bit; its images
    are ops.atlas_pack of bake_points at field_positions of ops.atlas_texels' output, byte for byte; bilinear lookups at the UV
    corners read the texels the restatement assigns to the face; the command line writes the same file; the PLY export is
    untouched.  Printed, not asserted: T and the share of covered texels."""
    from tensoir_amd import bake, mesh, ops
    m = trained.model
    ply_before, ply_after, glb, cli = (str(tmp_path / n) for n in ("before.ply", "after.ply", "scene.glb", "cli.glb"))
    mesh.export_mesh(m, ply_before, simplify=3, attributes=True)
    size = 256
    corners, nf = mesh.export_textured(m, glb, simplify=3, size=size)
    verts, faces, normals = mesh.extract_mesh(m, simplify=3)
    F = faces.shape[0]
    assert (corners, nf) == (3 * F, F) and F > 0
    cols, T = ops.atlas_layout(F, size)
    file = mesh.read_glb(glb)
    assert np.array_equal(u32(file["pos"]), u32(verts[faces.long()].reshape(-1, 3).cpu().numpy()))
    assert np.array_equal(u32(file["nrm"]), u32(normals[faces.long()].reshape(-1, 3).cpu().numpy()))
    ex = file["json"]["extras"]["tensoir_amd"]
    assert ex == {"size": size, "cols": cols, "T": T, "faces": F, "level": 0.005, "simplify": 3, "color": "albedo", "light_idx": 0}
    assert "occlusionTexture" in file["json"]["materials"][0]
    # the same kernels on the same inputs
    grid = [int(g) for g in m.gridSize]
    point, outward, face = ops.atlas_texels(verts, normals, faces, size, cols, T)
    p, d = mesh.field_positions(m.aabb, grid, point, outward)
    b = bake.bake_points(m, p.contiguous(), d.contiguous())
    images = ops.atlas_pack(verts, normals, faces, size, cols, T, b["albedo"], b["roughness"], b["normal"], b["coverage"], ao=b["ao"])
    torch.cuda.synchronize()
    for img, key in zip(images, mesh.IMAGE_NAMES):
        assert np.array_equal(file["images"][key], img.cpu().numpy()), key
    covered = float((b["coverage"] > 0.5).float().mean())
    print(f"\n[atlas export] grid {grid}: {F} faces, size {size}, cols {cols}, T {T}; coverage > 0.5 on {covered:.3f} of the "
          f"{point.shape[0]} texels")
    # uv, tangents and the bilinear footprint against the restatement
    hv, hn, hf = verts.cpu().numpy(), normals.cpu().numpy(), faces.cpu().numpy()
    _, _, rtan, ruv = A.corners(hv, hn, hf, size, cols, T)
    tan32 = np.abs(A.corners(hv, hn, hf, size, cols, T, np.float32)[2] - rtan).max()
    print(f"[atlas export] tangent: device {np.abs(file['tan'] - rtan).max():.2e}, float32 restatement on this mesh {tan32:.2e}")
    assert np.array_equal(u32(file["uv"]), u32(ruv)) and np.abs(file["tan"] - rtan).max() <= TAN_TOL
    base = file["images"]["base"].astype(np.float64)
    lo, hi = A.corner_uv_local(T)
    up = A.upper_owned(T)
    tol = 255 * 2 * size * 2.0 ** -24               # uv is a rounded float32: the lookup lands within size * 2^-24 texels of the corner
    for fi in np.linspace(0, F - 1, 200).astype(np.int64):
        c, upper = fi // 2, bool(fi % 2)
        ox, oy = (c % cols) * T, (c // cols) * T
        for k in range(3):
            val, taps = bilinear(base, *file["uv"][3 * fi + k].astype(np.float64))
            cx, cy = (hi if upper else lo)[k]
            want_taps = [(ox + cx - 1 + di, oy + cy - 1 + dj) for dj in (0, 1) for di in (0, 1)]
            assert taps == want_taps
            whole = fi == F - 1 and not upper
            assert all(whole or up[j - oy, i - ox] == upper for i, j in taps)          # every tap is a texel of this face
            assert np.abs(val - np.mean([base[j, i] for i, j in want_taps], axis=0)).max() <= tol
    # the command line, as a fresh child process on the saved checkpoint
    ckpt = str(tmp_path / "trained.th")
    m.save(ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tensoir_amd.bake", ckpt, cli, "--simplify", "3", "--texture-size", str(size)], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"{3 * F} vertices, {F} faces" in r.stdout, r.stdout
    assert open(cli, "rb").read() == open(glb, "rb").read()
    # the PLY export is what it was
    mesh.export_mesh(m, ply_after, simplify=3, attributes=True)
    assert open(ply_after, "rb").read() == open(ply_before, "rb").read()


def test_bake_atlas_options(trained):
    """color="diffuse" changes the base image only; lighting=False leaves the occlusion channel at 255 and the other images as
    they are; a size too small for the faces is refused with the size that works."""
    from tensoir_amd import mesh
    m = trained.model
    grid = [int(g) for g in m.gridSize]
    from tensoir_amd import ops
    verts, faces, normals = mesh.extract_mesh(m, simplify=4)
    size = 6 * ops.atlas_layout(faces.shape[0], 8192)[0] + 5                 # the smallest cells, and a size cols does not divide
    a = mesh.bake_atlas(m, verts, faces, normals, grid, size=size)
    d = mesh.bake_atlas(m, verts, faces, normals, grid, size=size, color="diffuse")
    u = mesh.bake_atlas(m, verts, faces, normals, grid, size=size, lighting=False)
    torch.cuda.synchronize()
    print(f"\n[atlas options] {faces.shape[0]} faces, size {size}, cols {a['cols']}, T {a['T']}")
    assert a["T"] == 6 and a["base"].shape == (size, size, 4)
    assert not torch.equal(a["base"], d["base"]) and torch.equal(a["orm"], d["orm"]) and torch.equal(a["normal"], d["normal"])
    assert torch.equal(a["base"], u["base"]) and torch.equal(a["normal"], u["normal"])
    owned = (u["orm"][..., 0] == 255)
    assert torch.equal(a["orm"][..., 1:], u["orm"][..., 1:]) and bool(owned.any()) and bool((u["orm"][..., 0][~owned] == 0).all())
    for k in ("pos", "nrm", "tan", "uv"):
        assert torch.equal(bits(a[k]), bits(d[k])) and torch.equal(bits(a[k]), bits(u[k]))
    cols = a["cols"]
    with pytest.raises(ValueError, match=f"at least {6 * cols}"):
        mesh.bake_atlas(m, verts, faces, normals, grid, size=6 * cols - 1)
