"""Traced shadows of the exported asset on the GPU (tir_shadow_trace, tir_light_gbuffer_occluded, their ops wrappers,
raster.relight_mesh(shadows="traced") / shadow_grid_for / compare_asset(shadows="traced" | "both"), the bake command line with
--shadow-method) against the ray query (ops.ray_mesh) and the numpy restatement (tests/shadowtrace_reference.py).

Comparison rule: a bit is exact -- every pair equals the ray query's any-hit answer and the brute-force restatement's, nothing
excluded; lighting follows DESIGN 4.8's rule (the device within ten times the float32 restatement's own distance from the float64
one).  Everything repeats bit for bit.

Measured on an MI355X: see DESIGN 4.17."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import light_reference as L
from tests import raster_reference as R
from tests import shadow_reference as SR
from tests import shadowtrace_reference as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIAS = (0.5, 1.0)
INF = float("inf")


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def words(occl):
    return occl.cpu().numpy().view(np.uint64)


def trace(pts, nrm, cells, pos, t0, grid=None, faces=None):
    from tensoir_amd import ops
    faces = ST.unwelded_faces(pos) if faces is None else faces
    return ops.shadow_trace(dev(pts), dev(nrm), dev(cells), dev(pos), dev(faces, np.int32), grid, t0)


# ---- the bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ST.TRACE_D)
@pytest.mark.parametrize("M", ST.TRACE_M)
def test_bits_equal_the_ray_query_and_the_restatement(M, D):
    """Ground, quad and fan (11 faces), M ground points with up normals, D of SR.cell_dirs, rays from t0 = 0 (every point lies on
    the ground's own faces) and from SHADOW_EPS x the radius: every bit equals ops.ray_mesh(mode="any") on the explicitly built
    ray, gated by the contribution test, and the brute-force restatement; the bits of rows beyond M are 0.  With up normals c =
    L_z: the nearest to the 1e-6 threshold is exactly 0 (e_x), the next is more than 0.01 away, so no rounding decides a pair."""
    from tensoir_amd import ops, raster
    pos = SR.scene()
    faces = ST.unwelded_faces(pos)
    pts, nrm = ST.ground_rows(M)
    cells = SR.cells_of(SR.cell_dirs(D))
    on, c = ST.contributing(nrm, cells)
    assert (np.abs(c[np.abs(c) > 0]) > 0.01).all()
    grid = ops.face_grid(dev(pos), dev(faces, np.int32))
    for t0 in (0.0, raster.SHADOW_EPS * SR.mesh_bounds(pos)[1]):
        occl = trace(pts, nrm, cells, pos, t0, grid)
        assert occl.shape == (D, (M + 63) // 64) and occl.dtype == torch.int64
        got = ops.occlusion_bits(occl, M).cpu().numpy()
        assert np.array_equal(got, ST.unpack(words(occl), M))
        o = np.repeat(pts, D, 0)
        d = np.tile(cells[:, 0:3], (M, 1))
        tr = np.tile(np.float32([[t0, INF]]), (M * D, 1))
        hit = ops.ray_mesh(dev(o), dev(d), dev(pos), dev(faces, np.int32), grid, mode="any", trange=dev(tr))[0].cpu().numpy().reshape(M, D)
        assert np.array_equal(got, hit & on)
        want = ST.shadow_trace(pts, nrm, cells, pos, faces, t0)
        assert np.array_equal(got, want)
        assert np.array_equal(words(occl), ST.pack(want))                 # the bits beyond M included: they are 0
        assert np.array_equal(words(ops.pack_occlusion(dev(want, bool))), ST.pack(want))
        if t0 == 0.0:
            assert np.array_equal(got, on)                                   # the ground meets its own points at t = 0
        elif M >= 63 and D >= 17:
            assert got.any() and (on & ~got).any()
        print(f"\n[shadow trace M {M} D {D} t0 {t0:.2e}] contributing {int(on.sum())}, occluded {int(got.sum())}")


def test_bits_do_not_depend_on_the_grid():
    """257 points of the 4008-face sphere with its smooth normals under 33 cells: the default grid, a 1 x 1 x 1 grid, dims (3, 5,
    2), a permutation of the faces and a second call give identical words, equal to the brute-force restatement's.  From t0 = 0,
    where the rounding of a point to float32 decides whether it meets its own face (the case in which a grid could matter most),
    and from SHADOW_EPS x the radius, where the convex sphere occludes nothing.  No pair of the fixture has a cosine within 1e-5
    of the threshold."""
    from tensoir_amd import ops, raster
    pts, nrm, pos = ST.sphere_rows(257)
    cells = SR.cells_of(SR.cell_dirs(33))
    on, c = ST.contributing(nrm, cells)
    assert (np.abs(c - L.THRESHOLD) > 1e-5).all()
    faces = ST.unwelded_faces(pos)
    v, f = dev(pos), dev(faces, np.int32)
    perm = np.random.default_rng(9).permutation(len(faces))
    for t0 in (0.0, raster.SHADOW_EPS * SR.mesh_bounds(pos)[1]):
        base = words(trace(pts, nrm, cells, pos, t0))
        for kw in (dict(dims=[1, 1, 1]), dict(dims=[3, 5, 2])):
            assert np.array_equal(words(trace(pts, nrm, cells, pos, t0, ops.face_grid(v, f, **kw))), base), kw
        assert np.array_equal(words(trace(pts, nrm, cells, pos, t0, faces=faces[perm])), base)
        assert np.array_equal(words(trace(pts, nrm, cells, pos, t0)), base)
        want = ST.shadow_trace(pts, nrm, cells, pos, faces, t0)
        print(f"\n[shadow trace grids t0 {t0:.2e}] contributing {int(on.sum())} of {on.size}, occluded {int(want.sum())}")
        assert np.array_equal(base, ST.pack(want)) and (on & ~want).sum() > 100
        assert t0 != 0.0 or want.sum() > 100


# ---- lighting ---------------------------------------------------------------------------------------------------------------------------
def _light(g, v, cells, occl, flags):
    from tensoir_amd import ops
    return ops.light_gbuffer_occluded(dev(g), dev(v), dev(cells), occl, 0.04, bool(flags & L.OCCLUSION), bool(flags & L.SRGB)).cpu().numpy()


@pytest.mark.parametrize("D", [1, 33, 67])
@pytest.mark.parametrize("M", L.M_CASES)
def test_no_bits_give_the_unshadowed_bits(M, D):
    from tensoir_amd import ops
    g, v, cells = L.surface_rows(M, D)
    zero = torch.zeros((D, (M + 63) // 64), dtype=torch.int64, device="cuda")
    for flags in range(4):
        want = ops.light_gbuffer(dev(g), dev(v), dev(cells), 0.04, bool(flags & 1), bool(flags & 2)).cpu().numpy()
        assert np.array_equal(_light(g, v, cells, zero, flags), want), (M, D, flags)
    full = torch.full_like(zero, -1)
    dark = _light(g, v, cells, full, 0)
    assert (dark[:, 0:3] == 0).all() and np.array_equal(dark[:, 3], g[:, 8])


def test_occluded_lighting_is_the_map_paths_lighting():
    """The M = 257, D = 33 fixture of the shadow-map tests.  With the bits packed from shadow_lookup's codes (== 1) the occluded
    kernel equals the shadowed one bit for bit, for every flag combination, also with a wider row stride.  With the traced bits it
    lies within the bound of the float64 restatement fed with the same bits; two calls and a permutation of the rows give the same
    bits."""
    from tensoir_amd import ops, raster
    M, D, S = 257, 33, 64
    g, v, cells = L.surface_rows(M, D)
    pos = SR.scene()
    fr = SR.frames(cells[:, 0:3], *SR.SCENE_BOUNDS, S).astype(np.float32)
    pts = SR.ground_grid()[0][np.random.default_rng(2).permutation(SR.GRID_N ** 2)[:M]]
    maps, _ = ops.shadow_maps(dev(pos), dev(fr), S)
    codes = ops.shadow_lookup(dev(pts), dev(g[:, 5:8]), dev(cells), dev(fr), maps, BIAS)
    packed = ops.pack_occlusion(codes == 1)
    wide = torch.zeros((D, packed.shape[1] + 3), dtype=torch.int64, device="cuda")
    wide[:, :packed.shape[1]] = packed
    for flags in range(4):
        want = ops.light_gbuffer_shadowed(dev(g), dev(v), dev(cells), dev(pts), dev(fr), maps, BIAS, 0.04, bool(flags & 1),
                                          bool(flags & 2)).cpu().numpy()
        assert np.array_equal(_light(g, v, cells, packed, flags), want), flags
        assert np.array_equal(_light(g, v, cells, wide, flags), want), flags
    t0 = raster.SHADOW_EPS * SR.mesh_bounds(pos)[1]
    occl = trace(pts, g[:, 5:8], cells, pos, t0)
    occ = ops.occlusion_bits(occl, M).cpu().numpy()
    on = (codes != 0).cpu().numpy()
    assert not (occ & ~on).any() and (occ & on).sum() > 200 and (on & ~occ).sum() > 200
    for flags in (0, 3):
        ref = ST.light_gbuffer_occluded(g, v, cells, 0.04, flags, occ)
        bound = 10 * L.distance(ST.light_gbuffer_occluded(g, v, cells, 0.04, flags, occ, np.float32), ref)
        got = _light(g, v, cells, occl, flags)
        d = L.distance(got, ref)
        print(f"\n[shadow trace lighting M {M} D {D} flags {flags}] device {d:.2e} (bound {bound:.2e}), pairs occluded {int(occ.sum())}, "
              f"lit {int((on & ~occ).sum())}; occluded by the maps {int((codes == 1).sum())}")
        assert d <= bound and np.array_equal(got[:, 3], g[:, 8])
    a = _light(g, v, cells, occl, 3)
    assert np.array_equal(a, _light(g, v, cells, occl, 3))
    perm = np.random.default_rng(0).permutation(M)
    c = _light(g[perm], v[perm], cells, trace(pts[perm], g[perm, 5:8], cells, pos, t0), 3)
    undone = np.empty_like(c)
    undone[perm] = c
    assert np.array_equal(undone, a)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _flat_images(size=4):
    base = np.tile(np.uint8([200, 180, 160, 255]), (size, size, 1))
    orm = np.tile(np.uint8([255, 128, 0, 255]), (size, size, 1))
    normal = np.tile(np.uint8([128, 128, 255, 255]), (size, size, 1))
    return base, orm, normal


def test_relight_mesh_traces_the_quads_shadow():
    """Ground and quad from obliquely above, one bright cell at e_z (two dark ones beside it), 128 x 128: ground pixels whose point
    lies more than 1e-3 inside the quad's analytic shadow are black, those more than 1e-3 outside it and the quad's own pixels
    equal the unshadowed image bit for bit.  A grid handed in gives the same image; "maps" is True."""
    from tensoir_amd import raster
    h, W = 0.25, 128
    pos = SR.ground_quad(h)
    n = len(pos)
    nrm = np.tile(np.float32([[0, 0, 1]]), (n, 1))
    tan = np.tile(np.float32([[1, 0, 0, 1]]), (n, 1))
    uv = np.full((n, 2), 0.5, np.float32)
    mesh = (dev(pos), dev(nrm), dev(tan), dev(uv), dict(zip(raster.IMAGE_NAMES, _flat_images())))
    cells = SR.cells_of(SR.cell_dirs(3), rgb=(3.0, 2.0, 1.0), omega=0.5)
    cells[1:, 4:7] = 0
    c2w = R.look_at((0.0, -4.0, 1.5), (0.0, 0.0, 0.0)).astype(np.float32)
    kw = dict(cull=False, srgb=False)
    plain = raster.relight_mesh(*mesh, dev(cells), c2w, 200.0, W, W, **kw)
    traced = raster.relight_mesh(*mesh, dev(cells), c2w, 200.0, W, W, shadows="traced", **kw)
    again = raster.relight_mesh(*mesh, dev(cells), c2w, 200.0, W, W, shadows="traced", shadow_eps=raster.SHADOW_EPS,
                                shadow_grid=raster.shadow_grid_for(mesh[0]), **kw)
    assert torch.equal(traced["rgb"], again["rgb"]) and all(torch.equal(plain[k], traced[k]) for k in plain if k not in ("rgb", "drops"))
    by_maps = raster.relight_mesh(*mesh, dev(cells), c2w, 200.0, W, W, shadows="maps", shadow_size=64, **kw)
    assert torch.equal(by_maps["rgb"], raster.relight_mesh(*mesh, dev(cells), c2w, 200.0, W, W, shadows=True, shadow_size=64, **kw)["rgb"])
    with pytest.raises(ValueError, match="shadows"):
        raster.relight_mesh(*mesh, dev(cells), c2w, 200.0, W, W, shadows="both", **kw)
    rays = raster.camera_rays(c2w, 200.0, W, W, "cuda")
    pts = (rays[:, 0:3] + plain["depth"].reshape(-1, 1) * rays[:, 3:6]).cpu().numpy()
    face = plain["face"].reshape(-1).cpu().numpy()
    a, b = plain["rgb"].reshape(-1, 3).cpu().numpy(), traced["rgb"].reshape(-1, 3).cpu().numpy()
    ground, quad = (face == 0) | (face == 1), (face == 2) | (face == 3)
    inset = SR.shadow_inset(pts, SR.LIGHTS["overhead"], h, 0.0, 2, 1.0)          # 2 r / S = 1: the inset in world units
    deep, clear = ground & (inset > 1e-3), ground & (inset < -1e-3)
    print(f"\n[shadow trace relight_mesh] ground pixels {int(ground.sum())}: in shadow {int(deep.sum())}, clear {int(clear.sum())}, within "
          f"1e-3 of the border {int((ground & ~deep & ~clear).sum())}; quad pixels {int(quad.sum())}; black ground pixels "
          f"{int((ground & (b == 0).all(1)).sum())}")
    assert deep.sum() > 100 and clear.sum() > 1000 and quad.sum() > 300
    assert (a[ground | quad] > 0).all()
    assert (b[deep] == 0).all()
    assert np.array_equal(b[clear], a[clear]) and np.array_equal(b[quad], a[quad]) and np.array_equal(b[face < 0], a[face < 0])


@pytest.mark.parametrize("rows", [4, 1])
def test_the_sphere_does_not_shadow_itself(rows):
    """The sphere view of the lighting tests under rows x 2 rows cells with the default shadow_eps: pair by pair, at the pixels' own
    rasterised points and shading normals, no pair with c >= 0.25 is occluded; every pixel all of whose contributing pairs have
    c >= 0.25 equals the unshadowed image bit for bit.  (At shadow_eps = 1e-5, the value the face points alone would give, 4 473
    of the 18 740 pairs with c >= 0.25 under 4 x 8 cells were occluded on an MI355X: the rasterised points lie up to 1.1e-4 of the
    radius off their faces.  The rule of DESIGN 4.17 therefore counts them as a third point set, and the default is 1e-2.)"""
    from tensoir_amd import ops, raster
    pos, nrm, c2w, focal, W, H = R.sphere_case("sphere-64")
    tan, uv, _ = R.shade_inputs(13)
    mesh = (dev(pos), dev(nrm), dev(tan), dev(uv), dict(zip(raster.IMAGE_NAMES, _flat_images())))
    cells = raster.environment_cells(dev(L.hdr_map(16, 32, 21) * np.float32(0.05)), rows=rows)
    plain = raster.relight_mesh(*mesh, cells, c2w, float(focal), H, W)
    traced = raster.relight_mesh(*mesh, cells, c2w, float(focal), H, W, shadows="traced")
    m = plain["coverage"].reshape(-1).cpu().numpy() > 0
    c = L._dot(plain["normal"].reshape(-1, 1, 3).cpu().numpy().astype(np.float64), cells[:, 0:3].cpu().numpy().astype(np.float64)[None])
    safe = m & ~((c > 0) & (c < 0.25)).any(1)
    a, b = plain["rgb"].reshape(-1, 3).cpu().numpy(), traced["rgb"].reshape(-1, 3).cpu().numpy()
    rays = raster.camera_rays(c2w, float(focal), H, W, "cuda")
    pts = rays[:, 0:3] + plain["depth"].reshape(-1, 1) * rays[:, 3:6]
    occl = ops.shadow_trace(pts, plain["normal"].reshape(-1, 3), cells, *raster.shadow_grid_for(mesh[0]),
                            raster.SHADOW_EPS * raster.mesh_bounds(mesh[0])[1])
    occ = ops.occlusion_bits(occl, H * W).cpu().numpy()
    facing = m[:, None] & (c >= 0.25)
    print(f"\n[shadow trace sphere {rows} x {2 * rows}] covered {int(m.sum())}, pixels with every pair at c >= 0.25: {int(safe.sum())}, pixels "
          f"the shadows change {int((a != b).any(1).sum())}; pairs with c >= 0.25: {int(facing.sum())}, occluded among them "
          f"{int(occ[facing].sum())}; occluded pairs below 0.25: {int(occ[m[:, None] & (c < 0.25)].sum())}")
    assert int(m.sum()) == R.SPHERE_VIEWS["sphere-64"][4] and facing.sum() > 1000 and (rows != 1 or safe.sum() > 500)
    assert not occ[facing].any()
    assert np.array_equal(a[safe], b[safe]) and np.array_equal(a[~m], b[~m])


# ---- validation -----------------------------------------------------------------------------------------------------------------------------
def test_entries_validate_before_any_device_work():
    """Host addresses throughout: every call below must be refused on the host (an accepted one would launch on host memory), and
    the sentinels in occl / out stay as they are."""
    import ctypes as C
    from tensoir_amd import _lib
    lib = _lib.lib()
    keep = torch.zeros(64, dtype=torch.float32)
    sentinel = torch.full((64,), 12345.0, dtype=torch.float32)
    ptr, out = keep.data_ptr(), sentinel.data_ptr()
    assert ptr % 16 == 0 and out % 16 == 0
    ARG, UNSUPPORTED = -1001, -1002
    cell, org, dims = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2)

    def t(pts=ptr, nrm=ptr, cells=ptr, M=4, D=3, verts=ptr, V=12, faces=ptr, F=4, cell=cell, org=org, dims=dims, cursor=ptr, pairs=ptr,
          n_pairs=8, bounds=ptr, t0=0.0, occl=out):
        return lib.tir_shadow_trace(pts, nrm, cells, M, D, verts, V, faces, F, cell, org, dims, cursor, pairs, n_pairs, bounds, t0, occl, None)
    for name in ("pts", "nrm", "cells", "verts", "faces", "cell", "org", "dims", "cursor", "pairs", "bounds", "occl"):
        assert t(**{name: None}) == ARG, name
    assert t(M=-1) == ARG and t(D=0) == ARG and t(V=-1) == ARG and t(F=-1) == ARG and t(n_pairs=-1) == ARG
    assert t(t0=-1.0) == ARG and t(t0=float("nan")) == ARG and t(t0=INF) == ARG
    assert t(cell=(C.c_float * 3)(1, 0, 1)) == ARG and t(cell=(C.c_float * 3)(1, INF, 1)) == ARG
    assert t(org=(C.c_float * 3)(0, float("nan"), 0)) == ARG and t(dims=(C.c_int32 * 3)(2, 0, 2)) == ARG
    assert t(occl=out + 4) == ARG and t(cells=ptr + 8) == ARG
    assert t(D=(1 << 20) + 1) == UNSUPPORTED and t(M=1 << 31) == UNSUPPORTED and t(n_pairs=1 << 31) == UNSUPPORTED
    assert t(dims=(C.c_int32 * 3)(2, 257, 2)) == UNSUPPORTED
    assert t(pts=None, nrm=None, cells=None, cursor=None, bounds=None, occl=None, M=0) == 0             # M = 0: nothing to do
    # gbuf, view, cells, occl, occl_stride, M, D, fresnel, flags, out, stream
    s = lib.tir_light_gbuffer_occluded
    for bad in range(4):
        a = [ptr] * 4
        a[bad] = None
        assert s(*a, 1, 4, 8, 0.04, 0, out, None) == ARG
    four = [ptr] * 4
    assert s(*four, 1, 4, 8, 0.04, 0, None, None) == ARG
    assert s(*four, 1, -1, 8, 0.04, 0, out, None) == ARG
    assert s(*four, 1, 4, 0, 0.04, 0, out, None) == ARG
    assert s(*four, 1, 4, 8, 0.04, 4, out, None) == ARG                         # an unknown flag bit
    assert s(*four, 0, 4, 8, 0.04, 0, out, None) == ARG                         # a stride below ceil(M / 64)
    assert s(*four, 1, 65, 8, 0.04, 0, out, None) == ARG
    assert s(ptr + 4, ptr, ptr, ptr, 1, 4, 8, 0.04, 0, out, None) == ARG
    assert s(ptr, ptr, ptr + 8, ptr, 1, 4, 8, 0.04, 0, out, None) == ARG
    assert s(ptr, ptr, ptr, ptr + 4, 1, 4, 8, 0.04, 0, out, None) == ARG        # occl: 8 bytes
    assert s(*four, 1, 4, 8, 0.04, 0, out + 4, None) == ARG
    assert s(*four, 1, 4, (1 << 20) + 1, 0.04, 0, out, None) == UNSUPPORTED
    assert s(None, None, None, None, 0, 0, 8, 0.04, 3, None, None) == 0        # M = 0: nothing to do
    assert (sentinel == 12345.0).all() and (keep == 0).all()


# ---- a real asset ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    from tests.train_sequence import reconstruct
    return reconstruct()


def test_compare_asset_with_both_shadow_methods(trained, tmp_path):
    """The fixture of test_compare_asset_with_shadows (export_textured(simplify=3, size=256), 4 views at 64 x 64, light_rows=8,
    shadow_size=128): with shadows="both", shadow_agreement and every other number equal the shadows=True report; the two new
    numbers lie in [0, 1] and repeat exactly; shadows="traced" reports the traced agreement as shadow_agreement; the command line
    prints the same report.  The values are printed, not judged (DESIGN 4.17 records them)."""
    from tensoir_amd import mesh, raster
    m = trained.model
    glb, cli = str(tmp_path / "scene.glb"), str(tmp_path / "cli.glb")
    mesh.export_textured(m, glb, simplify=3, size=256)
    light = L.hdr_map(16, 32, 33) * np.float32(0.05)
    npy = str(tmp_path / "light.npy")
    np.save(npy, light)
    kw = dict(H=64, W=64, n_views=4, light_rows=8, shadow_size=128)
    base = raster.compare_asset(m, glb, light=light, shadows=True, **kw)
    report = raster.compare_asset(m, glb, light=light, shadows="both", **kw)
    print("\n[shadow trace compare_asset] " + json.dumps(report))
    new = ["shadow_agreement_traced", "shadow_map_agreement"]
    for v, b in zip(report["views"] + [report["mean"]], base["views"] + [base["mean"]]):
        assert sorted(v) == sorted(list(b) + new)
        assert all(np.isfinite(v[k]) and 0.0 <= v[k] <= 1.0 for k in new)
        assert {k: v[k] for k in b} == b
    assert {k: report[k] for k in report if k not in ("views", "mean")} == {k: base[k] for k in base if k not in ("views", "mean")}
    views = str(tmp_path / "views")
    assert raster.compare_asset(m, glb, light=npy, shadows="both", write_views=views, **kw) == report
    assert sorted(os.listdir(views)) == sorted(f"view_{k:02d}_{s}.png" for k in range(4)
                                               for s in ("field", "asset", "asset_shadowed", "asset_traced"))
    assert mesh.read_png(open(os.path.join(views, "view_00_asset_traced.png"), "rb").read()).shape == (64, 64, 4)
    only = raster.compare_asset(m, glb, light=light, shadows="traced", **kw)
    for v, r in zip(only["views"] + [only["mean"]], report["views"] + [report["mean"]]):
        assert sorted(v) == sorted(k for k in r if k not in new)
        assert v["shadow_agreement"] == r["shadow_agreement_traced"]
        assert {k: v[k] for k in v if k != "shadow_agreement"} == {k: r[k] for k in v if k != "shadow_agreement"}
    with pytest.raises(ValueError):
        raster.compare_asset(m, glb, H=64, W=64, n_views=1, shadows="both")
    ckpt = str(tmp_path / "trained.th")
    m.save(ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tensoir_amd.bake", ckpt, cli, "--simplify", "3", "--texture-size", "256", "--check-views", "4",
                        "--check-size", "64", "--check-light", npy, "--check-light-rows", "8", "--check-shadows", "--shadow-size", "128",
                        "--shadow-method", "both", "--shadow-eps", str(raster.SHADOW_EPS)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == report
