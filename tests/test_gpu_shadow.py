"""The shadow maps of the exported asset on the GPU (tir_shadow_maps, tir_shadow_lookup, tir_light_gbuffer_shadowed, their ops
wrappers, raster.relight_mesh(shadows=True) / shadow_maps_for / compare_asset(shadows=True), the bake command line with
--check-shadows) against the numpy restatement (tests/shadow_reference.py).

Comparison rule (DESIGN 4.8's): a continuous quantity of the device lies within ten times the float32 restatement's own distance
from the float64 restatement on the same fixture (a distance of 0 asks for equal numbers); coverage is integer and exact; a
visibility code is compared outside the margins the restatement flags (tests/test_shadow_cpu.py keeps their share under 1 %).
Everything repeats bit for bit.

Measured on an MI355X: see DESIGN 4.10."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIAS = (0.5, 1.0)


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def device_maps(pos, fr, S, **kw):
    """-> (depth [D, S, S] float32 view of the map bits, the bits as uint32, drops)."""
    from tensoir_amd import ops
    faces = kw.pop("faces", None)
    maps, drops = ops.shadow_maps(dev(pos), dev(fr), S, faces=None if faces is None else dev(faces, np.int32), **kw)
    bits = maps.cpu().numpy().view(np.uint32)
    return bits.view(np.float32), bits, drops


# ---- maps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 61, 64])
@pytest.mark.parametrize("D", [1, 3, 33])
def test_maps_against_the_restatement(D, S):
    """Ground, quad and the fan on texel centres under e_z, -e_z, a grazing axis and seeded directions: occupancy equals the float32
    restatement at every texel, depth is within the bound, and a face permutation, the indexed form and a second call give the
    same bits.  ops.shadow_frames makes the frames the restatement makes."""
    from tensoir_amd import ops
    pos, dirs = SR.scene(), SR.cell_dirs(D)
    fr = SR.scene_frames(pos, dirs, S, SR.SCENE_BOUNDS)
    got_fr = ops.shadow_frames(dev(SR.cells_of(dirs)), *SR.SCENE_BOUNDS, S)
    assert got_fr.dtype == torch.float32 and np.abs(got_fr.cpu().numpy().astype(np.float64) - fr).max() <= 1e-6 * np.abs(fr).max()
    f32, counts = SR.maps(pos, fr, S, dtype=np.float32)
    f64 = SR.maps(pos, fr, S)[0]
    depth, bits, drops = device_maps(pos, fr, S)
    assert depth.shape == (D, S, S) and drops == counts == dict.fromkeys(R.DROPS, 0)
    assert np.array_equal(bits != 0, f32 != 0) and (bits != 0).any()
    both = (f32 != 0) & (f64 != 0)
    bound = 10 * L.distance(f32[both], f64[both])
    d = L.distance(depth[both], f64[both])
    print(f"\n[shadow maps D {D} S {S}] device {d:.2e} (bound {bound:.2e}), bits equal the float32 restatement's: "
          f"{np.array_equal(bits, f32.view(np.uint32))}, occupied {int((bits != 0).sum())} of {bits.size}")
    assert d <= bound
    assert (depth[bits != 0] > 0.2).all() and (depth[bits != 0] < 0.8).all()
    F = len(pos) // 3
    perm = np.random.default_rng(D + S).permutation(F)
    assert np.array_equal(device_maps(pos.reshape(F, 3, 3)[perm].reshape(-1, 3), fr, S)[1], bits)
    assert np.array_equal(device_maps(pos, fr, S)[1], bits)
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)[perm]
    assert np.array_equal(device_maps(pos, fr, S, faces=faces)[1], bits)


@pytest.mark.parametrize("S", [64, 97])
def test_whole_map_triangle_for_every_capacity(S):
    """A triangle over the whole map and a small one in front: the workgroup pass (large capacity), a list of one, and no list at
    all (the thread walks its own face) give identical bits, equal to the restatement's occupancy."""
    pos = SR.whole_map_triangle()
    dirs = SR.cell_dirs(3)
    fr = SR.scene_frames(pos, dirs, S, ((0.0, 0.0, 0.25), 1.0))
    f32, _ = SR.maps(pos, fr, S, dtype=np.float32)
    results = [device_maps(pos, fr, S, work_cap=cap)[1] for cap in (0, 1, 1 << 16)]
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
    assert np.array_equal(results[0] != 0, f32 != 0) and (results[0][0] != 0).all()
    both = f32 != 0
    f64 = SR.maps(pos, fr, S)[0]
    both &= f64 != 0
    bound = 10 * L.distance(f32[both], f64[both])
    d = L.distance(results[0].view(np.float32)[both], f64[both])
    print(f"\n[shadow maps whole-map S {S}] device {d:.2e} (bound {bound:.2e}), bits equal: {np.array_equal(results[0], f32.view(np.uint32))}")
    assert d <= bound


def test_no_faces_and_dropped_pairs():
    from tensoir_amd import ops
    fr = SR.scene_frames(SR.scene(), SR.cell_dirs(3), 16, SR.SCENE_BOUNDS)
    maps, drops = ops.shadow_maps(torch.zeros((0, 3), device="cuda"), dev(fr), 16)
    assert maps.shape == (3, 16, 16) and int(maps.abs().max()) == 0 and drops == dict.fromkeys(R.DROPS, 0)
    pos = SR.scene().copy()
    pos[3 * 2 + 1, 1] = np.nan                               # a corner of the occluder's first triangle
    F = len(pos) // 3
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    faces[5, 2] = 3 * F                                      # one index past the end
    faces[7, 0] = -1
    f32, counts = SR.maps(pos, fr, 16, faces=faces, dtype=np.float32)
    depth, bits, drops = device_maps(pos, fr, 16, faces=faces)
    assert counts == {"index": 6, "near": 0, "guard": 0, "nonfinite": 3} and drops == counts
    assert np.array_equal(bits != 0, f32 != 0)
    far = SR.scene().copy()
    far[0, 0] = 1.0e6                                        # x_px far beyond the guard band under e_z; edge-on cells see it too
    f32, counts = SR.maps(far, fr, 16, dtype=np.float32)
    assert counts["guard"] >= 1 and device_maps(far, fr, 16)[2] == counts


# ---- lookup -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", list(SR.LIGHTS))
def test_lookup_against_float64(light):
    """41 x 41 ground points with up normals: every code equals the float64 restatement's (which reads its own float64 maps),
    outside the pairs it flags; points beyond the map are lit, pairs below the horizon are 0."""
    from tensoir_amd import ops
    pos, dirs = SR.scene(), [SR.LIGHTS[light]]
    cells = SR.cells_of(dirs)
    fr = SR.scene_frames(pos, dirs, 64, SR.SCENE_BOUNDS)
    pts, nrm = SR.ground_grid()
    extra_p = np.float32([(100, 0, 0), (0, -100, 0), (0.1, 0.1, 0), (0.1, 0.1, 0)])
    extra_n = np.float32([(0, 0, 1), (0, 0, 1), (0, 0, -1), (0, 1, 0)])
    pts, nrm = np.concatenate([pts, extra_p]), np.concatenate([nrm, extra_n])
    near = {}
    ref = SR.lookup(pts, nrm, cells, fr, SR.maps(pos, fr, 64)[0], BIAS, np.float64, near)
    excluded = near["depth"] | near["texel"]
    maps, _ = ops.shadow_maps(dev(pos), dev(fr), 64)
    got = ops.shadow_lookup(dev(pts), dev(nrm), dev(cells), dev(fr), maps, BIAS).cpu().numpy()
    n = SR.GRID_N ** 2
    print(f"\n[shadow lookup {light}] excluded {int(excluded.sum())} of {excluded.size}, codes 0 / 1 / 2: "
          f"{[int((got == k).sum()) for k in range(3)]}, disagreeing among the excluded {int((got != ref)[excluded].sum())}")
    assert got.shape == ref.shape and got.dtype == np.uint8 and excluded.mean() <= 0.01
    assert np.array_equal(got[~excluded], ref[~excluded])
    assert (got[:n] == 1).sum() > 100 and (got[:n] == 2).sum() > 100
    assert got[n:, 0].tolist() == [2, 2, 0, 0]              # beyond the map: lit; n.L < 0 and n.L = 0 <= 1e-6: no contribution


# ---- fused lighting -------------------------------------------------------------------------------------------------------------------------
def _light(g, v, cells, pts, fr, maps, flags, bias=BIAS):
    from tensoir_amd import ops
    return ops.light_gbuffer_shadowed(dev(g), dev(v), dev(cells), dev(pts), dev(fr), maps, bias, 0.04, bool(flags & L.OCCLUSION),
                                      bool(flags & L.SRGB)).cpu().numpy()


@pytest.mark.parametrize("D", [1, 33, 67])
@pytest.mark.parametrize("M", L.M_CASES)
def test_empty_maps_give_the_unshadowed_bits(M, D):
    from tensoir_amd import ops
    g, v, cells = L.surface_rows(M, D)
    fr = SR.frames(cells[:, 0:3], (0, 0, 0), 2.0, 8).astype(np.float32)
    maps, _ = ops.shadow_maps(torch.zeros((0, 3), device="cuda"), dev(fr), 8)
    pts = np.random.default_rng(M + D).uniform(-1, 1, (M, 3)).astype(np.float32)
    for flags in range(4):
        want = ops.light_gbuffer(dev(g), dev(v), dev(cells), 0.04, bool(flags & 1), bool(flags & 2)).cpu().numpy()
        assert np.array_equal(_light(g, v, cells, pts, fr, maps, flags), want), (M, D, flags)


def test_shadowed_lighting_against_float64():
    """257 rows of light_reference.surface_rows standing on the ground grid, 33 cells over the sphere, the maps of the scene: within
    the bound of the float64 restatement fed with the device's own visibility codes (the rule is one function: nothing is
    excluded); two calls and a permutation of the rows give the same bits."""
    from tensoir_amd import ops
    M, D, S = 257, 33, 64
    g, v, cells = L.surface_rows(M, D)
    pos = SR.scene()
    fr = SR.frames(cells[:, 0:3], *SR.SCENE_BOUNDS, S).astype(np.float32)
    pts = SR.ground_grid()[0][np.random.default_rng(2).permutation(SR.GRID_N ** 2)[:M]]
    maps, _ = ops.shadow_maps(dev(pos), dev(fr), S)
    codes = ops.shadow_lookup(dev(pts), dev(g[:, 5:8]), dev(cells), dev(fr), maps, BIAS).cpu().numpy()
    assert (codes == 1).sum() > 200 and (codes == 2).sum() > 200 and (codes == 0).sum() > 200
    for flags in (0, 3):
        ref = SR.light_gbuffer_shadowed(g, v, cells, 0.04, flags, codes)
        bound = 10 * L.distance(SR.light_gbuffer_shadowed(g, v, cells, 0.04, flags, codes, np.float32), ref)
        got = _light(g, v, cells, pts, fr, maps, flags)
        d = L.distance(got, ref)
        print(f"\n[shadow lighting M {M} D {D} flags {flags}] device {d:.2e} (bound {bound:.2e}), pairs shadowed {int((codes == 1).sum())}, "
              f"lit {int((codes == 2).sum())}")
        assert d <= bound and np.array_equal(got[:, 3], g[:, 8])
        assert L.distance(ops.light_gbuffer(dev(g), dev(v), dev(cells), 0.04, bool(flags & 1), bool(flags & 2)).cpu().numpy(), ref) > 100 * bound
    a = _light(g, v, cells, pts, fr, maps, 3)
    assert np.array_equal(a, _light(g, v, cells, pts, fr, maps, 3))
    perm = np.random.default_rng(0).permutation(M)
    c = _light(g[perm], v[perm], cells, pts[perm], fr, maps, 3)
    undone = np.empty_like(c)
    undone[perm] = c
    assert np.array_equal(undone, a)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _flat_images(size=4):
    base = np.tile(np.uint8([200, 180, 160, 255]), (size, size, 1))
    orm = np.tile(np.uint8([255, 128, 0, 255]), (size, size, 1))
    normal = np.tile(np.uint8([128, 128, 255, 255]), (size, size, 1))
    return base, orm, normal


def test_relight_mesh_casts_the_quads_shadow():
    """From obliquely above (straight down the quad would hide its own shadow), one bright cell at e_z (two dark ones beside it),
    S = 64: ground pixels more than two texels inside the quad's shadow are black, those more than two texels outside it and the
    quad's own pixels equal the unshadowed image bit for bit."""
    from tensoir_amd import raster
    h, S, W = 0.25, 64, 128
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
    shadowed = raster.relight_mesh(*mesh, dev(cells), c2w, 200.0, W, W, shadows=True, shadow_size=S, **kw)
    again = raster.relight_mesh(*mesh, dev(cells), c2w, 200.0, W, W, shadows=True, shadow_bias=raster.SHADOW_BIAS,
                                shadow_maps=raster.shadow_maps_for(mesh[0], dev(cells), S), **kw)
    assert torch.equal(shadowed["rgb"], again["rgb"]) and all(torch.equal(plain[k], shadowed[k]) for k in plain if k not in ("rgb", "drops"))
    centre, r = raster.mesh_bounds(mesh[0])
    want_c, want_r = SR.mesh_bounds(pos)
    assert np.allclose(centre, want_c, atol=1e-7) and abs(r - want_r) < 1e-6 * want_r
    rays = raster.camera_rays(c2w, 200.0, W, W, "cuda")
    pts = (rays[:, 0:3] + plain["depth"].reshape(-1, 1) * rays[:, 3:6]).cpu().numpy()
    face = plain["face"].reshape(-1).cpu().numpy()
    a, b = plain["rgb"].reshape(-1, 3).cpu().numpy(), shadowed["rgb"].reshape(-1, 3).cpu().numpy()
    ground, quad = (face == 0) | (face == 1), (face == 2) | (face == 3)
    inset = SR.shadow_inset(pts, SR.LIGHTS["overhead"], h, 0.0, S, r)
    deep, clear = ground & (inset > 2), ground & (inset < -2)
    print(f"\n[shadow relight_mesh] ground pixels {int(ground.sum())}: in shadow {int(deep.sum())}, clear {int(clear.sum())}; quad pixels "
          f"{int(quad.sum())}; black ground pixels {int((ground & (b == 0).all(1)).sum())}")
    assert deep.sum() > 100 and clear.sum() > 1000 and quad.sum() > 300
    assert (a[ground | quad] > 0).all()
    assert (b[deep] == 0).all()
    assert np.array_equal(b[clear], a[clear]) and np.array_equal(b[quad], a[quad]) and np.array_equal(b[face < 0], a[face < 0])
    with pytest.raises(ValueError, match="shadow_size.*rows"):
        raster.shadow_maps_for(mesh[0], torch.zeros((2048, 8), device="cuda"), 1024)


@pytest.mark.parametrize("rows", [4, 1])
def test_the_sphere_does_not_shadow_itself(rows):
    """The sphere view of the lighting tests under rows x 2 rows cells with the default map size and bias: every pixel all of whose
    contributing pairs have c >= 0.25 equals the unshadowed image bit for bit (with 4 x 8 cells nearly every pixel has a grazing
    cell and few qualify; with 1 x 2 most do), and pair by pair, at the pixels' own points and shading normals, no pair with
    c >= 0.25 is shadowed."""
    from tensoir_amd import ops, raster
    pos, nrm, c2w, focal, W, H = R.sphere_case("sphere-64")
    tan, uv, _ = R.shade_inputs(13)
    mesh = (dev(pos), dev(nrm), dev(tan), dev(uv), dict(zip(raster.IMAGE_NAMES, _flat_images())))
    cells = raster.environment_cells(dev(L.hdr_map(16, 32, 21) * np.float32(0.05)), rows=rows)
    plain = raster.relight_mesh(*mesh, cells, c2w, float(focal), H, W)
    shadowed = raster.relight_mesh(*mesh, cells, c2w, float(focal), H, W, shadows=True)
    m = plain["coverage"].reshape(-1).cpu().numpy() > 0
    c = L._dot(plain["normal"].reshape(-1, 1, 3).cpu().numpy().astype(np.float64), cells[:, 0:3].cpu().numpy().astype(np.float64)[None])
    safe = m & ~((c > 0) & (c < 0.25)).any(1)
    a, b = plain["rgb"].reshape(-1, 3).cpu().numpy(), shadowed["rgb"].reshape(-1, 3).cpu().numpy()
    changed = (a != b).any(1)
    rays = raster.camera_rays(c2w, float(focal), H, W, "cuda")
    pts = rays[:, 0:3] + plain["depth"].reshape(-1, 1) * rays[:, 3:6]
    codes = ops.shadow_lookup(pts, plain["normal"].reshape(-1, 3), cells, *raster.shadow_maps_for(mesh[0], cells), raster.SHADOW_BIAS).cpu().numpy()
    facing = m[:, None] & (c >= 0.25)
    print(f"\n[shadow sphere {rows} x {2 * rows}] covered {int(m.sum())}, pixels with every pair at c >= 0.25: {int(safe.sum())}, pixels the "
          f"shadows change {int(changed.sum())} (among those {int((changed & safe).sum())}); pairs with c >= 0.25: {int(facing.sum())}, "
          f"shadowed among them {int((codes[facing] == 1).sum())}; shadowed pairs below 0.25: {int((codes[m[:, None] & (c < 0.25)] == 1).sum())}")
    assert int(m.sum()) == R.SPHERE_VIEWS["sphere-64"][4] and facing.sum() > 1000 and (rows != 1 or safe.sum() > 500)
    assert np.array_equal(a[safe], b[safe]) and np.array_equal(a[~m], b[~m])
    assert (codes[facing] == 2).all()


# ---- validation -----------------------------------------------------------------------------------------------------------------------------
def test_entries_validate_before_any_device_work():
    """Host addresses throughout: every call below must be refused on the host (an accepted one would launch on host memory)."""
    from tensoir_amd import _lib
    lib = _lib.lib()
    keep = torch.zeros(64, dtype=torch.float32)
    ptr = keep.data_ptr()
    assert ptr % 16 == 0
    ARG, UNSUPPORTED = -1001, -1002
    f = lib.tir_shadow_maps                                  # pos, V, faces, F, frames, D, S, maps, work, work_cap, status, stream
    assert f(None, 12, None, 4, ptr, 3, 8, ptr, ptr, 4, ptr, None) == ARG
    assert f(ptr, 12, None, 4, None, 3, 8, ptr, ptr, 4, ptr, None) == ARG
    assert f(ptr, 12, None, 4, ptr, 3, 8, None, ptr, 4, ptr, None) == ARG
    assert f(ptr, 12, None, 4, ptr, 3, 8, ptr, None, 4, ptr, None) == ARG
    assert f(ptr, 12, None, 4, ptr, 3, 8, ptr, ptr, 4, None, None) == ARG
    assert f(ptr, 12, None, 4, ptr, 0, 8, ptr, ptr, 4, ptr, None) == ARG
    assert f(ptr, 12, None, 4, ptr, 3, 0, ptr, ptr, 4, ptr, None) == ARG
    assert f(ptr, -1, None, 4, ptr, 3, 8, ptr, ptr, 4, ptr, None) == ARG
    assert f(ptr, 12, None, -1, ptr, 3, 8, ptr, ptr, 4, ptr, None) == ARG
    assert f(ptr, 12, None, 4, ptr, 3, 8, ptr, ptr, -1, ptr, None) == ARG
    assert f(ptr, 11, None, 4, ptr, 3, 8, ptr, ptr, 4, ptr, None) == ARG          # unwelded: V >= 3 F
    assert f(ptr, 12, None, 4, ptr + 4, 3, 8, ptr, ptr, 4, ptr, None) == ARG      # frames: 16 bytes
    assert f(ptr, 12, None, 4, ptr, 3, 8, ptr + 2, ptr, 4, ptr, None) == ARG      # maps, work: 4 bytes
    assert f(ptr, 12, None, 4, ptr, 3, 8, ptr, ptr + 2, 4, ptr, None) == ARG
    assert f(ptr, 12, None, 4, ptr, 3, 8, ptr, ptr, 4, ptr + 4, None) == ARG      # status: 8 bytes
    assert f(ptr, 12, None, 4, ptr, 3, 4097, ptr, ptr, 4, ptr, None) == UNSUPPORTED
    assert f(ptr, 12, None, 4, ptr, (1 << 20) + 1, 8, ptr, ptr, 4, ptr, None) == UNSUPPORTED
    assert f(ptr, 12, ptr, 715827883, ptr, 3, 8, ptr, ptr, 4, ptr, None) == UNSUPPORTED
    k = lib.tir_shadow_lookup                                # pts, nrm, cells, frames, maps, M, D, S, bias_const, bias_slope, vis, stream
    for bad in range(5):
        a = [ptr] * 5
        a[bad] = None
        assert k(*a, 4, 3, 8, 0.5, 1.0, ptr, None) == ARG
    assert k(ptr, ptr, ptr, ptr, ptr, 4, 3, 8, 0.5, 1.0, None, None) == ARG
    assert k(ptr, ptr, ptr, ptr, ptr, -1, 3, 8, 0.5, 1.0, ptr, None) == ARG
    assert k(ptr, ptr, ptr, ptr, ptr, 4, 0, 8, 0.5, 1.0, ptr, None) == ARG
    assert k(ptr, ptr, ptr, ptr, ptr, 4, 3, 0, 0.5, 1.0, ptr, None) == ARG
    assert k(ptr, ptr, ptr, ptr, ptr, 4, 3, 8, -0.5, 1.0, ptr, None) == ARG
    assert k(ptr, ptr, ptr, ptr, ptr, 4, 3, 8, 0.5, float("nan"), ptr, None) == ARG
    assert k(ptr, ptr, ptr + 8, ptr, ptr, 4, 3, 8, 0.5, 1.0, ptr, None) == ARG
    assert k(ptr, ptr, ptr, ptr + 8, ptr, 4, 3, 8, 0.5, 1.0, ptr, None) == ARG
    assert k(ptr, ptr, ptr, ptr, ptr + 2, 4, 3, 8, 0.5, 1.0, ptr, None) == ARG
    assert k(ptr, ptr, ptr, ptr, ptr, 4, 3, 4097, 0.5, 1.0, ptr, None) == UNSUPPORTED
    assert k(ptr, ptr, ptr, ptr, ptr, 4, (1 << 20) + 1, 8, 0.5, 1.0, ptr, None) == UNSUPPORTED
    assert k(None, None, None, None, None, 0, 3, 8, 0.5, 1.0, None, None) == 0   # M = 0: nothing to do
    # gbuf, view, cells, pts, frames, maps, M, D, S, bias_const, bias_slope, fresnel, flags, out, stream
    s = lib.tir_light_gbuffer_shadowed
    for bad in range(6):
        a = [ptr] * 6
        a[bad] = None
        assert s(*a, 4, 8, 8, 0.5, 1.0, 0.04, 0, ptr, None) == ARG
    six = [ptr] * 6
    assert s(*six, 4, 8, 8, 0.5, 1.0, 0.04, 0, None, None) == ARG
    assert s(*six, -1, 8, 8, 0.5, 1.0, 0.04, 0, ptr, None) == ARG
    assert s(*six, 4, 0, 8, 0.5, 1.0, 0.04, 0, ptr, None) == ARG
    assert s(*six, 4, 8, 0, 0.5, 1.0, 0.04, 0, ptr, None) == ARG
    assert s(*six, 4, 8, 8, 0.5, 1.0, 0.04, 4, ptr, None) == ARG                  # an unknown flag bit
    assert s(*six, 4, 8, 8, -1.0, 1.0, 0.04, 0, ptr, None) == ARG
    assert s(*six, 4, 8, 8, 0.5, float("inf"), 0.04, 0, ptr, None) == ARG
    assert s(ptr + 4, ptr, ptr, ptr, ptr, ptr, 4, 8, 8, 0.5, 1.0, 0.04, 0, ptr, None) == ARG
    assert s(ptr, ptr, ptr + 8, ptr, ptr, ptr, 4, 8, 8, 0.5, 1.0, 0.04, 0, ptr, None) == ARG
    assert s(ptr, ptr, ptr, ptr, ptr + 8, ptr, 4, 8, 8, 0.5, 1.0, 0.04, 0, ptr, None) == ARG
    assert s(ptr, ptr, ptr, ptr, ptr, ptr + 2, 4, 8, 8, 0.5, 1.0, 0.04, 0, ptr, None) == ARG
    assert s(*six, 4, 8, 8, 0.5, 1.0, 0.04, 0, ptr + 4, None) == ARG
    assert s(*six, 4, (1 << 20) + 1, 8, 0.5, 1.0, 0.04, 0, ptr, None) == UNSUPPORTED
    assert s(*six, 4, 8, 4097, 0.5, 1.0, 0.04, 0, ptr, None) == UNSUPPORTED
    assert s(None, None, None, None, None, None, 0, 8, 8, 0.5, 1.0, 0.04, 3, None, None) == 0


# ---- a real asset ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    from tests.train_sequence import reconstruct
    return reconstruct()


def test_compare_asset_with_shadows(trained, tmp_path):
    """export_textured(simplify=3, size=256), 4 views at 64 x 64, light_rows=8, shadow_size=128: shadow_agreement lies in [0, 1]
    in every view and repeats exactly, every other number equals the report without shadows, the command line prints the same
    report.  The value is printed, not judged: it is the first number that compares the mesh's occlusion with the field's; on an
    MI355X it is recorded in DESIGN 4.10."""
    from tensoir_amd import mesh, raster
    m = trained.model
    glb, cli = str(tmp_path / "scene.glb"), str(tmp_path / "cli.glb")
    mesh.export_textured(m, glb, simplify=3, size=256)
    light = L.hdr_map(16, 32, 33) * np.float32(0.05)
    npy = str(tmp_path / "light.npy")
    np.save(npy, light)
    base = raster.compare_asset(m, glb, H=64, W=64, n_views=4, light=light, light_rows=8)
    report = raster.compare_asset(m, glb, H=64, W=64, n_views=4, light=light, light_rows=8, shadows=True, shadow_size=128)
    print("\n[shadow compare_asset] " + json.dumps(report))
    for v, b in zip(report["views"] + [report["mean"]], base["views"] + [base["mean"]]):
        assert sorted(v) == sorted(list(b) + ["shadow_agreement"])
        assert np.isfinite(v["shadow_agreement"]) and 0.0 <= v["shadow_agreement"] <= 1.0
        assert {k: v[k] for k in b} == b
    assert {k: report[k] for k in report if k not in ("views", "mean")} == {k: base[k] for k in base if k not in ("views", "mean")}
    views = str(tmp_path / "views")
    assert raster.compare_asset(m, glb, H=64, W=64, n_views=4, light=npy, light_rows=8, shadows=True, shadow_size=128,
                                write_views=views) == report
    assert sorted(os.listdir(views)) == sorted(f"view_{k:02d}_{s}.png" for k in range(4) for s in ("field", "asset", "asset_shadowed"))
    assert mesh.read_png(open(os.path.join(views, "view_00_asset_shadowed.png"), "rb").read()).shape == (64, 64, 4)
    with pytest.raises(ValueError):
        raster.compare_asset(m, glb, H=64, W=64, n_views=1, shadows=True)
    ckpt = str(tmp_path / "trained.th")
    m.save(ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tensoir_amd.bake", ckpt, cli, "--simplify", "3", "--texture-size", "256", "--check-views", "4",
                        "--check-size", "64", "--check-light", npy, "--check-light-rows", "8", "--check-shadows", "--shadow-size", "128"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == report
