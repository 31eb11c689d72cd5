"""numpy restatement of the traced-shadow contract of include/tensoir_hip.h (tir_shadow_trace, tir_light_gbuffer_occluded; DESIGN
4.17), brute force: pair (m, d) is occluded iff it contributes (n.L > 1e-6) and raymesh_reference.ray_mesh finds an accepted hit
of the ray from pts[m] along cells[d]'s direction over [t0, +inf].  Also the packing of the answers, the rule that chooses
raster.SHADOW_EPS, and the fixtures the CPU and the GPU tests share."""
import functools

import numpy as np

from tests import light_reference as L
from tests import raster_reference as R
from tests import raymesh_reference as RM
from tests import shadow_reference as SR


def contributing(nrm, cells, dtype=np.float64):
    """nrm [M, 3], cells [D, 8] (float32 inputs) -> (on [M, D] bool: c = n.L > 1e-6 in dtype, c [M, D])."""
    n = np.asarray(nrm, np.float32).reshape(-1, 3).astype(dtype)
    l = np.asarray(cells, np.float32).reshape(-1, 8)[:, 0:3].astype(dtype)
    with np.errstate(invalid="ignore"):
        c = L._dot(n[:, None, :], l[None, :, :])
        return c > dtype(L.THRESHOLD), c


def shadow_trace(pts, nrm, cells, verts, faces, t0=0.0):
    """-> occluded [M, D] bool.  An invalid ray (a non-finite point, a non-finite or zero direction) and a pair that does not
    contribute give False."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    cells = np.asarray(cells, np.float32).reshape(-1, 8)
    on, _ = contributing(nrm, cells)
    out = np.zeros(on.shape, bool)
    tr = np.empty((len(pts), 2), np.float32)
    tr[:, 0], tr[:, 1] = np.float32(t0), np.inf
    for d in range(len(cells)):
        rows = np.nonzero(on[:, d])[0]
        if len(rows):
            r = RM.ray_mesh(pts[rows], np.broadcast_to(cells[d, 0:3], (len(rows), 3)), verts, faces, tr[rows])
            out[rows, d] = r["count"] > 0
    return out


def pack(mask):
    """bool [M, D] -> uint64 [D, ceil(M / 64)]: bit m & 63 of word [d, m >> 6]; rows beyond M are 0."""
    mask = np.asarray(mask, bool)
    M, D = mask.shape
    W = (M + 63) // 64
    b = np.zeros((D, W * 64), np.uint64)
    b[:, :M] = mask.T
    return (b.reshape(D, W, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def unpack(occl, M):
    """uint64 (or int64 bits) [D, ceil(M / 64)] -> bool [M, D]."""
    w = np.ascontiguousarray(occl).view(np.uint64)
    bits = (w[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(w.shape[0], -1)[:, :M].T.astype(bool)


def light_gbuffer_occluded(gbuf, view, cells, fresnel, flags, occluded, dtype=np.float64):
    """light_reference.light_gbuffer with the pairs' occlusion [M, D] bool: a contributing pair is added iff its bit is 0."""
    return SR.light_gbuffer_shadowed(gbuf, view, cells, fresnel, flags, np.where(np.asarray(occluded, bool), 1, 2), dtype)


def unwelded_faces(pos):
    return np.arange(len(pos), dtype=np.int32).reshape(-1, 3)


# ---- the rule of raster.SHADOW_EPS -------------------------------------------------------------------------------------
EPS_EXPONENTS = (-7, -6, -5, -4, -3, -2)
EPS_CANDIDATES = tuple(float(f"1e{k}") for k in EPS_EXPONENTS)
SPHERE_STRIDE = 100              # the CPU test's subset of condition (i): every 100th point (the table over all points: DESIGN 4.17)


def farthest_meeting(origins, dirs, verts, faces, chunk=2000000):
    """Per ray the largest t at which its LINE meets a listed face under the ray-triangle rule (-inf: none).  Over [t0, +inf] a ray
    has an accepted hit iff this is >= t0: one pass serves every t0."""
    o32, d32 = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    v, f = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    keep, _ = RM.D.listed_faces(v, f)
    tri = v[f[keep]].astype(np.float64)
    out = np.full(len(o32), -np.inf)
    step = max(1, chunk // max(len(keep), 1))
    for s in range(0, len(o32) if len(keep) else 0, step):
        o, d = o32[s:s + step].astype(np.float64)[:, None, :], d32[s:s + step].astype(np.float64)[:, None, :]
        meets, t, _, _, _ = RM.ray_triangle(o, d, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        with np.errstate(invalid="ignore"):
            out[s:s + step] = np.where(meets & ~np.isnan(t), t, -np.inf).max(1)
    return out


@functools.lru_cache(maxsize=None)
def sphere_points():
    """SR._sphere_setup's points, normals and cells without its shadow maps: the corners, edge midpoints and centroid of every
    face of the 4008-face sphere (float32) with normalised smooth normals, under the 4 x 8 cells of a constant map."""
    pos, nrm = R.sphere_case("sphere-64")[0:2]
    cells = L.env_cells(np.ones((4, 8, 3), np.float32), 4, 8).astype(np.float32)
    P, N = pos.reshape(-1, 3, 3).astype(np.float64), nrm.reshape(-1, 3, 3).astype(np.float64)
    wts = np.float64([(1, 0, 0), (0, 1, 0), (0, 0, 1), (.5, .5, 0), (0, .5, .5), (.5, 0, .5), (1 / 3, 1 / 3, 1 / 3)])
    pts = np.einsum("qk,fkc->fqc", wts, P).reshape(-1, 3)
    n = np.einsum("qk,fkc->fqc", wts, N).reshape(-1, 3)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return pts.astype(np.float32), n.astype(np.float32), cells, pos


@functools.lru_cache(maxsize=None)
def sphere_pairs(stride=SPHERE_STRIDE):
    """Condition (i): the 4008-face sphere under 4 x 8 cells, every stride-th of the corners, edge midpoints and centroids of its
    faces (sphere_points) -> (farthest meeting t of every pair with c >= 0.25, the radius)."""
    pts, n, cells, pos = sphere_points()
    pts, n = pts[::stride], n[::stride]
    _, c = contributing(n, cells)
    m, d = np.nonzero(c >= 0.25)
    return farthest_meeting(pts[m], cells[d, 0:3], pos, unwelded_faces(pos)), SR.mesh_bounds(pos)[1]


@functools.lru_cache(maxsize=None)
def contact_pairs():
    """Condition (ii): ground + quad at CONTACT_HEIGHT under e_z and normalize(1, 0, 1), the ground points inside the analytic
    shadow -> (farthest meeting t of each, the radius)."""
    pos, r, dirs, _, _, pts, _ = SR._contact_setup()
    cells = SR.cells_of(dirs)
    far = []
    for d, l in enumerate(dirs):
        inside = SR.shadow_inset(pts, l, SR.CONTACT_HEIGHT, 0.0, 256, r) > 0
        far.append(farthest_meeting(pts[inside], np.broadcast_to(cells[d, 0:3], (int(inside.sum()), 3)), pos, unwelded_faces(pos)))
    return np.concatenate(far), r


@functools.lru_cache(maxsize=None)
def raster_points():
    """The third point set: the G-buffer points of the sphere's 64 x 64 view as raster.relight_mesh forms them, restated in float32
    with tests/raster_reference.py (corners snapped to 1 / 256 pixel, depth interpolated over the snapped face, point = eye + depth
    x unit ray) -> (pts, interpolated unit normals) float32 of the covered pixels, row-major.  These points lie off their faces by
    far more than a face point's rounding: the snapping moves a face by up to 1 / 256 pixel."""
    T = np.float32
    pos, nrm, c2w, focal, W, H = R.sphere_case("sphere-64")
    pr = R.project(pos, c2w, focal, W, H, 1e-3, dtype=T)
    cv = R.cover(pr["sx"], pr["sy"], pr["invz"], pr["flags"], W, H, True, T)
    b1, b2, zc, _ = R.resolve(cv["face"], pr["sx"], pr["sy"], pr["invz"], T)
    normal = R.shade(cv["face"], b1, b2, nrm, dtype=T)[..., 5:8]
    j, i = np.meshgrid(np.arange(H, dtype=T), np.arange(W, dtype=T), indexing="ij")
    cam = np.stack([(i + T(0.5) - T(W / 2)) / T(focal), (j + T(0.5) - T(H / 2)) / T(focal), np.ones_like(i)], -1).astype(T)
    d = (cam.reshape(-1, 3) @ c2w[:, :3].T.astype(T)).astype(T)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(T)
    depth = (zc.astype(T) * np.linalg.norm(cam, axis=-1).astype(T)).reshape(-1, 1)
    pts = (c2w[:, 3].astype(T)[None, :] + depth * d).astype(T)
    covered = cv["face"].reshape(-1) >= 0
    return pts[covered], normal.reshape(-1, 3)[covered].astype(T)


# the CPU test's subset of the third point set: every 7th covered pixel.  It holds covered pixel 1505, one of the three pixels of
# the full set (2, 1505, 1516) with a pair that is still occluded at 1e-4: the subset decides as the full set does
RASTER_STRIDE = 7


@functools.lru_cache(maxsize=None)
def raster_pairs(stride=RASTER_STRIDE):
    """Condition (iii): raster_points under 4 x 8 and 1 x 2 cells -> (farthest meeting t of every pair with c >= 0.25, the radius)."""
    pos = R.sphere_case("sphere-64")[0]
    pts, n = raster_points()
    pts, n = pts[::stride], n[::stride]
    far = []
    for rows in (4, 1):
        cells = L.env_cells(np.ones((rows, 2 * rows, 3), np.float32), rows, 2 * rows).astype(np.float32)
        _, c = contributing(n, cells)
        m, d = np.nonzero(c >= 0.25)
        far.append(farthest_meeting(pts[m], cells[d, 0:3], pos, unwelded_faces(pos)))
    return np.concatenate(far), SR.mesh_bounds(pos)[1]


def eps_criteria(eps, stride=SPHERE_STRIDE, raster_stride=RASTER_STRIDE):
    """-> (self-shadowed pairs of (i), pairs of (i), contact points of (ii) that came out lit, points of (ii), self-shadowed pairs
    of (iii), pairs of (iii)) at shadow_eps = eps: t0 = fp32(eps r), as the wrapper hands it to the kernel."""
    far_i, r_i = sphere_pairs(stride)
    far_ii, r_ii = contact_pairs()
    far_iii, r_iii = raster_pairs(raster_stride)
    return (int((far_i >= np.float64(np.float32(eps * r_i))).sum()), len(far_i),
            int((far_ii < np.float64(np.float32(eps * r_ii))).sum()), len(far_ii),
            int((far_iii >= np.float64(np.float32(eps * r_iii))).sum()), len(far_iii))


def eps_rule(stride=SPHERE_STRIDE, raster_stride=RASTER_STRIDE):
    """Ten times the smallest candidate that meets the three conditions (as the decimal literal of the next decade)."""
    for k in EPS_EXPONENTS:
        a, _, b, _, c, _ = eps_criteria(float(f"1e{k}"), stride, raster_stride)
        if a == 0 and b == 0 and c == 0:
            return float(f"1e{k + 1}")
    raise RuntimeError("no candidate meets the conditions")


# ---- fixtures of the GPU tests ---------------------------------------------------------------------------------------------------------
TRACE_M, TRACE_D = (1, 63, 64, 65, 257), (1, 17, 33)


def ground_rows(M):
    """The first M of SR.ground_grid()'s points in a seeded order, with up normals."""
    pts, nrm = SR.ground_grid()
    idx = np.random.default_rng(17).permutation(len(pts))[:M]
    return pts[idx], nrm[idx]


def sphere_rows(M=257, seed=5):
    """M points on the 4008-face sphere (face centroids, float32) with their smooth normals -> (pts, nrm, pos)."""
    pts, n, _, pos = sphere_points()
    idx = np.random.default_rng(seed).permutation(len(pts) // 7)[:M] * 7 + 6
    return pts[idx], n[idx], pos
