"""What the rasteriser (include/tensoir_hip.h, tir_raster_*; tensoir_amd/raster.py) promises without a GPU: the entries refuse
bad arguments on the host, the restatement's fill rule (tests/raster_reference.py) partitions the plane, the camera helpers
follow the datasets' convention, and the distance between the restatement's float32 and float64 modes -- the yardstick of the
GPU tests' bounds -- is what raster_reference.py's constants say."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import raster_reference as R

ARG, UNSUPPORTED = -1001, -1002


@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    return _lib.lib()


def test_raster_entries_validate_before_any_device_work(lib):
    """Every call below must be refused on the host: the pointers are HOST addresses, never dereferenced."""
    keep = torch.zeros(64, dtype=torch.float32)
    p = keep.data_ptr()
    assert p % 16 == 0
    cam = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    nan = float("nan")
    proj = lambda pos=p, V=3, faces=None, F=1, c=cam, f=8.0, W=16, H=16, near=0.1, rows=p, status=p: \
        lib.tir_raster_project(pos, V, faces, F, c, f, W, H, near, rows, status, None)
    for kw in (dict(pos=None), dict(rows=None), dict(status=None), dict(c=None), dict(W=0), dict(H=-1), dict(f=0.0), dict(f=-1.0),
               dict(f=nan), dict(near=nan), dict(near=-1.0), dict(F=-1), dict(V=-1), dict(V=2), dict(rows=p + 4)):
        assert proj(**kw) == ARG, kw
    for kw in (dict(W=8193), dict(H=8193), dict(F=715827883, V=3 * 715827883)):
        assert proj(**kw) == UNSUPPORTED, kw
    cover = lambda rows=p, F=1, W=16, H=16, cull=1, keys=p, work=p: lib.tir_raster_cover(rows, F, W, H, cull, keys, work, None)
    for kw in (dict(rows=None), dict(keys=None), dict(work=None), dict(W=0), dict(H=0), dict(F=-1), dict(keys=p + 4), dict(rows=p + 8)):
        assert cover(**kw) == ARG, kw
    for kw in (dict(W=8193), dict(H=8193), dict(F=715827883)):
        assert cover(**kw) == UNSUPPORTED, kw
    resolve = lambda rows=p, F=1, keys=p, W=16, H=16, out=p: lib.tir_raster_resolve(rows, F, keys, W, H, out, None)
    for kw in (dict(rows=None), dict(keys=None), dict(out=None), dict(W=0), dict(H=0), dict(F=-1), dict(out=p + 4)):
        assert resolve(**kw) == ARG, kw
    for kw in (dict(W=8193), dict(H=8193), dict(F=715827883)):
        assert resolve(**kw) == UNSUPPORTED, kw
    shade = lambda pix=p, F=1, nrm=p, tan=p, uv=p, base=p, orm=p, normal=p, size=8, raw=0, W=16, H=16, out=p: \
        lib.tir_raster_shade(pix, F, nrm, tan, uv, base, orm, normal, size, raw, W, H, out, None)
    for kw in (dict(pix=None), dict(out=None), dict(nrm=None), dict(tan=None), dict(uv=None), dict(base=None), dict(orm=None),
               dict(normal=None), dict(size=0), dict(W=0), dict(H=0), dict(F=-1), dict(out=p + 4), dict(base=p + 1)):
        assert shade(**kw) == ARG, kw
    for kw in (dict(W=8193), dict(H=8193), dict(size=8193), dict(F=715827883)):
        assert shade(**kw) == UNSUPPORTED, kw


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    from tensoir_amd import ops
    from tensoir_amd._lib import TensoirHipError
    with pytest.raises(TensoirHipError):                                   # no CPU path
        ops.raster_project(torch.zeros(3, 3), R.IDENTITY, 8.0, 16, 16)
    with pytest.raises(TensoirHipError):
        ops.raster_cover(torch.zeros(3, 4, dtype=torch.int32), 16, 16)


def _random_quads(rng, n):
    """n random convex quads on the half-pixel grid (corners on pixel centres), each split along a diagonal into two triangles
    with random winding -> (sx, sy) int64 [6 n] and the quads' corner lists."""
    sx, sy, quads = [], [], []
    while len(quads) < n:
        q = rng.integers(0, 20, (4, 2))
        c = q.mean(0)
        q = q[np.argsort(np.arctan2(q[:, 1] - c[1], q[:, 0] - c[0]))]
        e = [q[(k + 1) % 4] - q[k] for k in range(4)]
        cr = [e[k][0] * e[(k + 1) % 4][1] - e[k][1] * e[(k + 1) % 4][0] for k in range(4)]
        if not (np.all(np.array(cr) > 0)):
            continue                                                        # strictly convex, counter-clockwise in (x, y)
        quads.append(q)
        for tri in ((0, 1, 2), (0, 2, 3)):
            tri = list(tri)
            if rng.random() < 0.5:
                tri = tri[::-1]
            k = rng.integers(0, 3)
            tri = tri[k:] + tri[:k]
            sx += [256 * int(q[t, 0]) + 128 for t in tri]
            sy += [256 * int(q[t, 1]) + 128 for t in tri]
    return np.int64(sx), np.int64(sy), quads


def _in_quad(q, px, py):
    """Exact: strictly inside / on the border / outside the convex counter-clockwise polygon q for integer points (in pixels)."""
    inside, border = np.ones(px.shape, bool), np.zeros(px.shape, bool)
    for k in range(4):
        a, b = q[k], q[(k + 1) % 4]
        s = (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
        inside &= s >= 0
        border |= s == 0
    return inside & ~border, inside & border


def test_fill_rule_partitions_the_plane():
    """Triangulated quads with every corner on a pixel centre, so that edges, diagonals and vertices pass through centres: a centre
    strictly inside a quad is owned by exactly one of its two triangles, a centre outside by none, a centre on the quad's border by
    at most one; and in a strip of quads sharing edges, a centre on a shared edge is owned by exactly one of the two neighbours."""
    rng = np.random.default_rng(7)
    W = H = 20
    jj, ii = np.mgrid[0:H, 0:W]
    sx, sy, quads = _random_quads(rng, 60)
    on_centres = 0
    for k, q in enumerate(quads):
        s = slice(6 * k, 6 * k + 6)
        c = R.cover(sx[s], sy[s], np.ones(6), np.zeros(6, int), W, H, cull=False)
        strictly, border = _in_quad(q, ii, jj)
        assert (c["layers"][strictly] == 1).all() and (c["layers"][~strictly & ~border] == 0).all() and (c["layers"] <= 1).all()
        on_centres += int(border.sum()) + int((c["layers"][strictly] == 1).sum())
    assert on_centres > 2000
    # a strip of quads sharing vertical, horizontal and slanted edges through centres tiles a polygon: every centre strictly inside
    # the union is owned exactly once
    xs, tris = [2, 5, 9, 12, 17], []
    top, bot = [3, 1, 4, 2, 6], [15, 18, 14, 17, 13]
    for k in range(4):
        a, b, c, d = (xs[k], top[k]), (xs[k + 1], top[k + 1]), (xs[k + 1], bot[k + 1]), (xs[k], bot[k])
        tris += [(a, b, c), (c, a, d)] if k % 2 else [(b, d, a), (d, b, c)]
    px = np.int64([[256 * p[0] + 128 for p in t] for t in tris]).reshape(-1)
    py = np.int64([[256 * p[1] + 128 for p in t] for t in tris]).reshape(-1)
    c = R.cover(px, py, np.ones(len(px)), np.zeros(len(px), int), W, H, cull=False)
    union = np.zeros((H, W), bool)
    outside = np.ones((H, W), bool)
    for k in range(4):
        q = np.array([(xs[k], top[k]), (xs[k + 1], top[k + 1]), (xs[k + 1], bot[k + 1]), (xs[k], bot[k])])
        s, b = _in_quad(q, ii, jj)
        union |= s
        outside &= ~s & ~b
    inner_edges = np.zeros((H, W), bool)                                 # centres on the three shared vertical edges, ends excluded
    for k in (1, 2, 3):
        inner_edges |= (ii == xs[k]) & (jj > top[k]) & (jj < bot[k])
    assert inner_edges.sum() > 30
    assert (c["layers"][union | inner_edges] == 1).all() and (c["layers"][outside] == 0).all() and (c["layers"] <= 1).all()


def test_exact_cases_snap_where_they_were_placed():
    """The scenes of the GPU coverage test put their corners on dyadic pixel coordinates: both modes of the restatement snap them
    to exactly 256 x that coordinate, and every named case draws something with culling on."""
    for name, (pos, W, H) in R.exact_cases().items():
        a = R.project(pos, R.IDENTITY, R.FOCAL, W, H, R.NEAR, dtype=np.float32)
        b = R.project(pos, R.IDENTITY, R.FOCAL, W, H, R.NEAR)
        assert np.array_equal(a["sx"], b["sx"]) and np.array_equal(a["sy"], b["sy"]) and not a["flags"].any(), name
        assert np.array_equal(b["sx"], b["x256"]) and np.array_equal(b["sy"], b["y256"]), name
        c = R.cover(b["sx"], b["sy"], b["invz"], b["flags"], W, H, cull=True)
        assert c["drawn"] > 0 and (name in ("degenerate", "outside") or (c["face"] >= 0).any()), name
    c = R.exact_cases()
    for a, b in (("near-first", "far-first"),):
        pa, pb = (R.project(c[k][0], R.IDENTITY, R.FOCAL, 16, 16, R.NEAR) for k in (a, b))
        fa, fb = (R.cover(p["sx"], p["sy"], p["invz"], p["flags"], 16, 16, cull=False) for p in (pa, pb))
        assert np.array_equal(fa["invz"], fb["invz"]) and np.array_equal(fa["face"] >= 0, fb["face"] >= 0)
        assert np.array_equal(np.where(fa["face"] >= 0, fa["face"] // 2, -1), np.where(fb["face"] >= 0, 1 - fb["face"] // 2, -1))
    pos, W, H, counts = R.dropped_case()
    assert R.project(pos, R.IDENTITY, R.FOCAL, W, H, R.NEAR)["counts"] == counts
    assert R.project(pos, R.IDENTITY, R.FOCAL, W, H, R.NEAR, dtype=np.float32)["counts"] == counts


@pytest.mark.parametrize("name", list(R.SPHERE_VIEWS))
def test_sphere_views_have_one_front_layer(name):
    """The two sphere views: with culling, the number of front faces (A < 0) and of covered pixels that were computed
    independently in float64, and no pixel covered by two front faces -- which also fixes A < 0 as the front of the project's
    outward-oriented meshes."""
    pos, _, c2w, focal, W, H = R.sphere_case(name)
    _, _, _, front, covered = R.SPHERE_VIEWS[name]
    p = R.project(pos, c2w, focal, W, H, 1e-3)
    assert not p["flags"].any()
    c = R.cover(p["sx"], p["sy"], p["invz"], p["flags"], W, H, cull=True)
    assert c["drawn"] == front and int((c["face"] >= 0).sum()) == covered and c["layers"].max() == 1


def test_camera_rays_follow_the_dataset_convention():
    from tensoir_amd import raster
    c2w = torch.from_numpy(R.look_at((3.0, -2.0, 1.5), (0.2, 0.1, -0.3))).to(torch.float32)
    H, W, f = 5, 7, 6.5
    rays = raster.camera_rays(c2w, f, H, W)
    assert rays.shape == (H * W, 6) and rays.dtype == torch.float32
    for j in range(H):
        for i in range(W):
            d = np.array([(i + 0.5 - W / 2) / f, (j + 0.5 - H / 2) / f, 1.0])
            world = c2w[:, :3].double().numpy() @ d
            world /= np.linalg.norm(world)
            r = rays[j * W + i].double().numpy()
            assert np.abs(r[:3] - c2w[:, 3].double().numpy()).max() == 0 and np.abs(r[3:] - world).max() < 1e-6
    # the pixel a point projects to is the pixel whose ray passes through it
    p = c2w[:, 3].double().numpy() + 4.0 * rays[3 * W + 5, 3:].double().numpy()
    pr = R.project(np.float32([p, p, p]), c2w.numpy(), f, W, H, 1e-3)
    assert abs(pr["x256"][0] / 256 - 5.5) < 1e-4 and abs(pr["y256"][0] / 256 - 3.5) < 1e-4


def test_orbit_cameras_look_at_the_box_centre():
    from tensoir_amd import raster
    aabb = torch.tensor([[-1.0, -2.0, 0.5], [2.0, 1.0, 3.5]])
    centre = aabb.mean(0).double()
    for n, el, dist in ((1, 20, None), (6, 35, 4.0), (8, -10, 7.5)):
        cams = raster.orbit_cameras(aabb, n, elevation_deg=el, distance=dist)
        assert cams.shape == (n, 3, 4) and cams.dtype == torch.float32
        want = 2 * float(torch.linalg.norm(aabb[1] - aabb[0])) if dist is None else dist
        for c in cams.double():
            Rm, eye = c[:, :3], c[:, 3]
            assert torch.allclose(Rm.T @ Rm, torch.eye(3, dtype=torch.float64), atol=1e-6) and float(torch.linalg.det(Rm)) > 0.999
            to = centre - eye
            assert abs(float(torch.linalg.norm(to)) - want) < 1e-5 * want
            assert torch.allclose(Rm[:, 2], to / torch.linalg.norm(to), atol=1e-6)               # z looks at the centre
            assert abs(float(Rm[2, 0])) < 1e-6 and float(Rm[2, 1]) < 0                             # x level, y down (world up +z)
            assert abs(float(torch.asin(-Rm[2, 2])) - np.radians(el)) < 1e-5
        assert len({tuple(np.round(c[:, 3].numpy(), 4)) for c in cams}) == n
    with pytest.raises(ValueError):
        raster.orbit_cameras(aabb, 0)


def float32_distances():
    """The restatement's float32 mode against its float64 self on the GPU tests' resolve / shade cases -> {quantity: distance}."""
    d = {k: 0.0 for k in ("x256", "invz", "bary", "zc", "albedo", "orm", "normal")}
    for name in R.SPHERE_VIEWS:
        pos, nrm, c2w, focal, W, H = R.sphere_case(name)
        p64, p32 = R.project(pos, c2w, focal, W, H, 1e-3), R.project(pos, c2w, focal, W, H, 1e-3, dtype=np.float32)
        d["x256"] = max(d["x256"], np.abs(p32["x256"] - p64["x256"]).max(), np.abs(p32["y256"] - p64["y256"]).max())
        # one set of snapped corners (the float32 mode's, as a device would hand them on) and one face image for both modes
        cov = R.cover(p32["sx"], p32["sy"], p32["invz"], p32["flags"], W, H, cull=True)
        face = cov["face"]
        m = face >= 0
        r64, r32 = R.resolve(face, p32["sx"], p32["sy"], p32["invz"]), R.resolve(face, p32["sx"], p32["sy"], p32["invz"], dtype=np.float32)
        d["bary"] = max(d["bary"], np.abs(r32[0] - r64[0]).max(), np.abs(r32[1] - r64[1]).max())
        d["zc"] = max(d["zc"], (np.abs(r32[2] - r64[2])[m] / r64[2][m]).max())
        d["invz"] = max(d["invz"], (np.abs(r32[3] - r64[3])[m] / r64[3][m]).max())
        for size in R.SHADE_SIZES:
            tan, uv, images = R.shade_inputs(size)
            for raw in (False, True):
                # both modes start from the float32 barycentrics a device resolve would hand to shade
                s64 = R.shade(face, r32[0], r32[1], nrm, tan, uv, images, raw)
                s32 = R.shade(face, r32[0], r32[1], nrm, tan, uv, images, raw, dtype=np.float32)
                d["albedo"] = max(d["albedo"], np.abs(s32[..., 0:3] - s64[..., 0:3]).max())
                d["orm"] = max(d["orm"], np.abs(s32[..., 3:5] - s64[..., 3:5]).max())
                d["normal"] = max(d["normal"], np.abs(s32[..., 5:8] - s64[..., 5:8]).max())
        g64, g32 = R.shade(face, r32[0], r32[1], nrm), R.shade(face, r32[0], r32[1], nrm, dtype=np.float32)
        d["normal"] = max(d["normal"], np.abs(g32[..., 5:8] - g64[..., 5:8]).max())
    return {k: float(v) for k, v in d.items()}


def test_float32_mode_distances_set_the_gpu_bounds():
    """The GPU bounds are ten times these distances; the constants in raster_reference.py must say so (rounded up, by at most a
    fifth).  Printed for DESIGN 4.8."""
    d = float32_distances()
    print("\n[raster float32 mode vs float64] " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
    for key, tol in (("invz", R.INVZ_TOL), ("bary", R.BARY_TOL), ("zc", R.ZC_TOL), ("albedo", R.ALBEDO_TOL), ("orm", R.ORM_TOL),
                     ("normal", R.NORMAL_TOL)):
        assert 10 * d[key] <= tol <= 12 * d[key], (key, d[key], tol)
