"""The texture atlas without a GPU: the layout's ownership property by brute force on the numpy restatement
(tests/atlas_reference.py), ops.atlas_layout, the PNG and GLB writers against their readers (and PIL, where installed), the host
validation of the tir_atlas_* entries, and where the GPU test's bounds come from."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

from tests import atlas_reference as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_TOL, OUTWARD_TOL, TAN_TOL = A.POINT_TOL, A.OUTWARD_TOL, A.TAN_TOL


# ---- the layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", range(6, 20))
def test_bilinear_lookups_inside_a_face_read_only_its_own_texels(T):
    """Every texel of a used cell has exactly one owner; the UV corners lie in the cell; all four taps of a bilinear lookup at
    2 x 10^5 random points of each UV triangle, at its corners and at its edge midpoints are texels the face owns."""
    up = A.upper_owned(T)
    j, i = np.mgrid[0:T, 0:T]
    assert np.array_equal(~up, i + j <= T - 1) and up.sum() + (~up).sum() == T * T      # one owner each: the two sets are complements
    c, jj, ii, face, upper = A.texel_index(2, 1, T)
    assert np.array_equal(upper.reshape(T, T), up) and np.array_equal(face, upper.astype(np.int64))
    assert not A.texel_index(1, 1, T)[4].any()                                          # an odd last face owns its whole cell
    rng = np.random.default_rng(T)
    for tri, owned in zip(A.corner_uv_local(T), (~up, up)):
        assert (tri >= 0).all() and (tri <= T).all()
        r = rng.random((200000, 2))
        flip = r.sum(1) > 1
        r[flip] = 1 - r[flip]
        w = np.concatenate([np.stack([1 - r.sum(1), r[:, 0], r[:, 1]], 1), np.eye(3),
                            [[0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]]])
        p = w @ tri.astype(np.float64)
        taps = A.bilinear_taps(p[:, 0], p[:, 1]).reshape(-1, 2)
        assert (taps >= 0).all() and (taps < T).all()
        assert owned[taps[:, 1], taps[:, 0]].all()
    # the upper triangle is the lower one turned by 180 degrees about the cell centre
    lo, hi = A.corner_uv_local(T)
    assert np.array_equal(hi, T - lo) and np.array_equal(up[::-1, ::-1], i + j <= T - 2)


@pytest.mark.parametrize("T", [6, 7, 13, 19])
def test_clamped_barycentrics(T):
    """Texel centres inside the UV triangle keep their own barycentrics; the others take those of the nearest point of the
    triangle (checked against a dense search along its boundary): all in [0, 1] and summing to 1."""
    bl, bu = A.cell_barycentrics(T)
    lo, hi = A.corner_uv_local(T)
    j, i = np.mgrid[0:T, 0:T]
    centre = np.stack([i + 0.5, j + 0.5], -1)
    s = np.linspace(0, 1, 4001)[:, None]
    for b, tri in ((bl, lo.astype(np.float64)), (bu, hi.astype(np.float64))):
        assert (b >= 0).all() and (b <= 1).all() and np.abs(b.sum(-1) - 1).max() < 1e-15
        q = b @ tri
        edge = np.concatenate([tri[k] + s * (tri[(k + 1) % 3] - tri[k]) for k in range(3)])
        best = np.sqrt(((centre[:, :, None] - edge) ** 2).sum(-1)).min(-1)
        dist = np.sqrt(((centre - q) ** 2).sum(-1))
        M = np.linalg.inv(np.concatenate([tri, np.ones((3, 1))], 1))
        own = np.concatenate([centre, np.ones((T, T, 1))], -1) @ M
        inside = (own >= -1e-12).all(-1)
        assert np.abs(b[inside] - own[inside]).max() < 1e-12 and dist[inside].max() < 1e-12
        assert (dist[~inside] <= best[~inside] + 1e-12).all() and inside.sum() > 0
    assert np.array_equal(bu, bl[::-1, ::-1])


@pytest.mark.parametrize("F, size, want", [(1, 2048, (1, 2048)), (2, 2048, (1, 2048)), (7, 2048, (2, 1024)), (8, 27, (2, 13)),
                                           (9, 2048, (3, 682)), (5000, 2048, (50, 40)), (5000, 300, (50, 6)), (0, 6, (1, 6))])
def test_atlas_layout(F, size, want):
    from tensoir_amd import ops
    assert ops.atlas_layout(F, size) == want == A.layout(F, size)
    cols, T = want
    assert cols * cols >= (F + 1) // 2 and (cols - 1) ** 2 < max((F + 1) // 2, 1) and cols * T <= size


def test_atlas_layout_refuses_a_size_too_small_for_the_faces():
    from tensoir_amd import ops
    with pytest.raises(ValueError, match="at least 300"):
        ops.atlas_layout(5000, 299)
    with pytest.raises(ValueError, match="at least 12"):
        ops.atlas_layout(7, 11)
    for bad in (5, 8193, 64.0, True, "64", None):
        with pytest.raises(ValueError, match="size"):
            ops.atlas_layout(4, bad)
    with pytest.raises(ValueError):
        A.layout(5000, 299)


def test_float32_restatement_stays_inside_the_gpu_tolerance():
    """Where the GPU test's bounds on point, outward and tangent come from: the restatement run wholly in float32 against its
    float64 self over the same meshes and sizes (1.16e-7 / 1.20e-7 / 3.52e-7 when the bounds were set, ten times below them).
    face, uv and the copied attributes are the same arrays in both."""
    worst = np.zeros(3)
    for name, (v, n, f, sizes) in A.layout_cases().items():
        for size in sizes:
            cols, T = A.layout(len(f), size)
            p64, o64, f64, _ = A.texels(v, n, f, cols, T)
            p32, o32, f32, _ = A.texels(v, n, f, cols, T, np.float32)
            c64, c32 = A.corners(v, n, f, size, cols, T), A.corners(v, n, f, size, cols, T, np.float32)
            assert p32.dtype == o32.dtype == c32[2].dtype == np.float32 and np.array_equal(f32, f64)
            assert np.array_equal(c32[3], c64[3]) and c64[3].dtype == np.float32
            assert np.abs(np.linalg.norm(o64, axis=1) - 1).max() < 1e-12 and np.abs(np.linalg.norm(c64[2][:, :3], axis=1) - 1).max() < 1e-12
            k, rep = np.tile(np.arange(3), len(f)), np.repeat(np.arange(len(f)), 3)
            unit = A.unit_normals(np.eye(3)[k], v.astype(np.float64)[f][rep], n.astype(np.float64)[f][rep])
            assert np.abs((c64[2][:, :3] * unit).sum(1)).max() < 1e-12                     # the tangent is orthogonal to the normal
            worst = np.maximum(worst, [np.abs(p32 - p64).max() / np.abs(v).max(), np.abs(o32 - o64).max(), np.abs(c32[2] - c64[2]).max()])
    print(f"\n[float32 restatement] point {worst[0]:.2e} of the largest coordinate, outward {worst[1]:.2e}, tangent {worst[2]:.2e}")
    assert worst[0] <= POINT_TOL / 5 and worst[1] <= OUTWARD_TOL / 5 and worst[2] <= TAN_TOL / 5


def test_the_fallbacks_of_the_degenerate_mesh():
    v, n, f = A.degenerate_mesh()
    cols, T = A.layout(len(f), 12)
    _, out, face, _ = A.texels(v, n, f, cols, T)
    pos, nrm, tan, uv = A.corners(v, n, f, 12, cols, T)
    assert (out[face == 1] == (0, 0, 1)).all()                                   # a point with zero normals
    fn = np.cross(v[4].astype(np.float64) - v[3], v[5].astype(np.float64) - v[3])
    assert np.allclose(out[face == 2], fn / np.linalg.norm(fn), atol=1e-15)      # zero normals on a proper face: its own normal
    # face 0 has v0 = v1: the tangent is built from the axis of the normal's smallest component; n = (0, 0.6, 0.8) -> axis x
    assert np.allclose(tan[0], (1, 0, 0, 1)) and np.allclose(tan[2], (0, 1, 0, 1)) and np.allclose(tan[3:6, :3], (1, 0, 0))
    assert (tan[:, 3] == 1).all() and np.array_equal(pos, v[f.reshape(-1)]) and np.array_equal(nrm, n[f.reshape(-1)])


def test_pack_case_keeps_clear_of_the_rounding_boundaries():
    """The pack kernel's test inputs qualify: in every variant every channel of every owned texel is at least PACK_MARGIN (in
    units of 1 / 255) from a rounding boundary, so float32 arithmetic cannot change a byte; all three variants differ."""
    case = A.pack_case()
    assert (case["cols"], case["T"]) == (2, 13) and len(case["faces"]) == 5
    seen = {}
    for name in A.PACK_VARIANTS:
        imgs, owned = A.pack_variant(case, name)
        assert owned.sum() == 3 * 13 * 13 and not owned[:, 26].any() and not owned[26].any() and not owned[13:, 13:].any()
        for key, img in imgs.items():
            assert A.rounding_margin(img[owned]).min() >= A.PACK_MARGIN, (name, key)
            assert (img[~owned] == A.UNOWNED[key]).all() and img.min() >= 0 and img.max() < 255.4      # srgb(1) = 1 + 4e-7
        seen[name] = imgs
    assert np.abs(seen["albedo"]["base"] - seen["diffuse"]["base"]).max() > 1
    assert (seen["no-lighting"]["orm"][..., 0][owned] == 255).all() and seen["albedo"]["orm"][..., 0][owned].min() < 250
    cov = case["coverage"]
    assert 0 < (cov <= 0.5).sum() < len(cov) and np.abs(cov - 0.5).min() > 1e-3


# ---- PNG -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7), (64, 64)])
def test_png_round_trip(shape):
    from tensoir_amd import mesh
    a = np.random.default_rng(shape[0]).integers(0, 256, shape + (4,), dtype=np.uint8)
    for level in (0, 6, 9):
        data = mesh.write_png(a, level)
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[-8:-4] == b"IEND"
        assert struct.unpack(">II", data[16:24]) == (shape[1], shape[0])
        assert np.array_equal(mesh.read_png(data), a)
    bad = bytearray(data)
    bad[40] ^= 1
    with pytest.raises(Exception):
        mesh.read_png(bytes(bad))
    with pytest.raises(ValueError):
        mesh.write_png(a[..., :3])


@pytest.mark.parametrize("shape", [(5, 7), (64, 64)])
def test_png_is_read_by_pil(shape):
    Image = pytest.importorskip("PIL.Image")
    import io
    from tensoir_amd import mesh
    a = np.random.default_rng(shape[1]).integers(0, 256, shape + (4,), dtype=np.uint8)
    im = Image.open(io.BytesIO(mesh.write_png(a)))
    assert im.mode == "RGBA" and im.size == (shape[1], shape[0]) and np.array_equal(np.asarray(im), a)


# ---- GLB -----------------------------------------------------------------------------------------------------------------------
def _two_triangles():
    v, n, f = A.random_mesh(2, 12)
    cols, T = A.layout(2, 12)
    pos, nrm, tan, uv = A.corners(v, n, f, 12, cols, T, np.float32)
    rng = np.random.default_rng(3)
    images = {k: rng.integers(0, 256, (12, 12, 4), dtype=np.uint8) for k in ("base", "orm", "normal")}
    return pos, nrm, tan.astype(np.float32), uv, images


@pytest.mark.parametrize("occlusion", [True, False])
def test_glb_structure_and_round_trip(tmp_path, occlusion):
    from tensoir_amd import mesh
    pos, nrm, tan, uv, images = _two_triangles()
    extras = {"size": 12, "cols": 1, "T": 12, "faces": 2, "level": 0.005, "simplify": 3, "color": "albedo", "light_idx": 0}
    path = str(tmp_path / "two.glb")
    mesh.write_glb(path, pos, nrm, tan, uv, images, extras, occlusion=occlusion)
    data = open(path, "rb").read()
    assert data[:4] == b"glTF" and struct.unpack("<II", data[4:12]) == (2, len(data)) and len(data) % 4 == 0
    n_json, kind = struct.unpack("<II", data[12:20])
    assert kind == 0x4E4F534A and n_json % 4 == 0
    doc = json.loads(data[20:20 + n_json])
    assert data[20:20 + n_json].rstrip(b" ") == json.dumps(doc, separators=(",", ":")).encode()      # padded with spaces only
    n_bin, kind = struct.unpack("<II", data[20 + n_json:28 + n_json])
    assert kind == 0x004E4942 and n_bin % 4 == 0 and 28 + n_json + n_bin == len(data)
    assert doc["asset"]["version"] == "2.0" and len(doc["buffers"]) == 1 and "uri" not in doc["buffers"][0]
    size = doc["buffers"][0]["byteLength"]
    assert size <= n_bin < size + 4 and not any(data[28 + n_json + size:])
    for v in doc["bufferViews"]:
        assert v["buffer"] == 0 and v["byteOffset"] % 4 == 0 and v["byteOffset"] + v["byteLength"] <= size
    prim, = doc["meshes"][0]["primitives"]
    assert prim["mode"] == 4 and "indices" not in prim and sorted(prim["attributes"]) == ["NORMAL", "POSITION", "TANGENT", "TEXCOORD_0"]
    kinds = {"POSITION": "VEC3", "NORMAL": "VEC3", "TANGENT": "VEC4", "TEXCOORD_0": "VEC2"}
    for name, k in kinds.items():
        acc = doc["accessors"][prim["attributes"][name]]
        assert acc["count"] == 6 and acc["componentType"] == 5126 and acc["type"] == k
    acc = doc["accessors"][prim["attributes"]["POSITION"]]
    assert np.array_equal(np.float32(acc["min"]), pos.min(0)) and np.array_equal(np.float32(acc["max"]), pos.max(0))
    mat, = doc["materials"]
    pbr = mat["pbrMetallicRoughness"]
    assert pbr["metallicFactor"] == 1 and pbr["roughnessFactor"] == 1
    tex = lambda t: doc["images"][doc["textures"][t["index"]]["source"]]["name"]
    assert tex(pbr["baseColorTexture"]) == "base" and tex(pbr["metallicRoughnessTexture"]) == "orm" and tex(mat["normalTexture"]) == "normal"
    assert ("occlusionTexture" in mat) == occlusion and (not occlusion or tex(mat["occlusionTexture"]) == "orm")
    assert doc["samplers"] == [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
    assert all(t["sampler"] == 0 for t in doc["textures"])
    assert all(im["mimeType"] == "image/png" and "bufferView" in im and "uri" not in im for im in doc["images"])
    assert doc["extras"]["tensoir_amd"] == extras
    back = mesh.read_glb(path)
    for key, want in (("pos", pos), ("nrm", nrm), ("tan", tan), ("uv", uv)):
        assert back[key].dtype == np.float32 and np.array_equal(back[key].view(np.uint32), want.view(np.uint32)), key
    assert sorted(back["images"]) == sorted(images) and all(np.array_equal(back["images"][k], images[k]) for k in images)
    assert back["json"] == doc


def test_glb_refuses_mismatched_input(tmp_path):
    from tensoir_amd import mesh
    pos, nrm, tan, uv, images = _two_triangles()
    with pytest.raises(ValueError):
        mesh.write_glb(str(tmp_path / "a.glb"), pos[:5], nrm[:5], tan[:5], uv[:5], images)
    with pytest.raises(ValueError):
        mesh.write_glb(str(tmp_path / "a.glb"), pos, nrm, tan, uv, {"base": images["base"]})
    assert not os.path.exists(str(tmp_path / "a.glb"))


# ---- the library and the options, on the host ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_entries_validate_before_any_device_work(lib):
    import torch
    keep = torch.zeros(64, dtype=torch.float32)                        # a non-null, 16-byte aligned host address: never dereferenced
    p = keep.data_ptr()
    assert p % 16 == 0
    corners = lambda V, F, size, cols, T, *b: lib.tir_atlas_corners(p, V, p, p, F, size, cols, T, *b, None)
    texels = lambda V, F, size, cols, T, *b: lib.tir_atlas_texels(p, V, p, p, F, size, cols, T, *b, None)
    pack = lambda V, F, size, cols, T, *b: lib.tir_atlas_pack(p, V, p, p, F, size, cols, T, *b, None)
    ok_c, ok_t, ok_p = (p, p, p, p, p), (p, p, p, p), (p, None, p, None, p, p, p, p, p, p)
    for entry, ok in ((corners, ok_c), (texels, ok_t), (pack, ok_p)):
        assert entry(8, 7, 5, 1, 6, *ok) == -1001                      # size < 6
        assert entry(8, 7, 12, 0, 6, *ok) == -1001                     # cols < 1
        assert entry(8, 7, 12, 2, 7, *ok) == -1001                     # cols * T > size
        assert entry(8, 7, 24, 1, 12, *ok) == -1001                    # four cells in one column: more rows than fit
        assert entry(-1, 7, 12, 2, 6, *ok) == -1001 and entry(8, -7, 12, 2, 6, *ok) == -1001
        assert entry(8, 7, 12, 2, 6, *ok[:-1], None) == -1001          # the error word
        assert entry(8, 7, 12, 2, 6, None, *ok[1:]) == -1001           # an output (pack: the albedo)
        assert entry(8, 7, 12, 2, 5, *ok) == -1002                     # T < 6
        assert entry(8, 7, 8200, 2, 6, *ok) == -1002                   # size > 8192
        assert entry(8, 0, 12, 2, 6, *ok) == 0                         # no faces: nothing to do
    assert lib.tir_atlas_corners(None, 8, p, p, 7, 12, 2, 6, p, p, p, p, p, None) == -1001
    assert lib.tir_atlas_texels(p, 8, None, p, 7, 12, 2, 6, p, p, p, p, None) == -1001
    assert lib.tir_atlas_pack(p, 8, p, None, 7, 12, 2, 6, *ok_p, None) == -1001
    assert lib.tir_atlas_corners(p, 8, p, p, 7, 12, 2, 6, p, p, p + 4, p, p, None) == -1001       # tan: 16-byte stores
    assert lib.tir_atlas_pack(p, 8, p, p, 7, 12, 2, 6, p, None, p, None, p, p, p + 1, p, p, p, None) == -1001
    assert lib.tir_atlas_corners(None, 0, None, None, 0, 12, 1, 12, None, None, None, None, p, None) == 0
    assert lib.tir_atlas_texels(None, 0, None, None, 0, 12, 1, 12, None, None, None, p, None) == 0
    assert lib.tir_version() == 100


def test_atlas_kernels_hold_no_scratch(lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from tensoir_amd import _lib
    ks = [k for k in kernel_resources.kernels(_lib.LIB_PATH) if k["name"].startswith("k_atlas_")]
    assert sorted(k["name"] for k in ks) == ["k_atlas_corners", "k_atlas_pack", "k_atlas_texels<false>", "k_atlas_texels<true>"]
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgpr"] + k["agpr"] <= 128, k


@pytest.mark.parametrize("kw", [dict(size=5), dict(size=8193), dict(size=64.0), dict(size=True), dict(color="specular"),
                                dict(color="diffuse", lighting=False), dict(simplify=1), dict(connectivity=18),
                                dict(keep_largest=-1), dict(compress_level=10), dict(compress_level=1.5)])
def test_export_textured_refuses_bad_arguments_before_touching_the_device(kw, tmp_path):
    import torch
    import tensoir_amd
    from tensoir_amd import mesh
    from tests import config_scenes as CS
    m = tensoir_amd.TensorVMSplit(torch.tensor(CS.AABB), CS.GRID, "cpu", shadingMode="MLP_Fea")       # a host-built model
    path = str(tmp_path / "never.glb")
    with pytest.raises(ValueError):
        mesh.export_textured(m, path, **kw)
    assert not os.path.exists(path)
