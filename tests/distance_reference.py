"""Numpy restatement of the surface-distance contract of include/tensoir_hip.h (tir_mesh_sample*, tir_face_grid_*,
tir_point_mesh_distance) and of mesh.distance_summary.

    weights      w_f = sqrt(|(v1 - v0) x (v2 - v0)|^2) in float64 from the float32 corners (not finite -> 0); q_f = trunc(w_f / w_max
                 * 2^s), s = the largest integer <= 52 with F * 2^s <= 2^52; cdf = the inclusive integer sums, T their total
    uniforms     x = seed + 0x9E3779B97F4A7C15 * (3 i + ch + 1); x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
                 x *= 0x94D049BB133111EB; x ^= x >> 31; u = x >> 40; xi = u * 2^-24          (uint64, wrapping)
    sample i     k = min(trunc(((i + xi_0) / n) * T), T - 1), face = the first f with cdf[f] > k;
                 s = sqrt(xi_1), point = ((1 - s) v0 + s (1 - xi_2) v1) + s xi_2 v2
    distance     brute force over every non-degenerate face (|cross|^2 == 0 in float64, or a non-finite corner: skipped and
                 counted), the seven regions of the closest point in coordinates relative to corner a; ties -> the smaller index

The discrete parts (weights, cdf, the face of a sample, the degenerate rule) are float64 / integer whatever `dtype` says; `dtype`
switches the arithmetic that the GPU tolerances rest on (the point of a sample, the closest point and the distance) to float32.
Also the cases the CPU and the GPU tests share.
"""
import functools

import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the hash, the integer cdf, the samples ----------------------------------------------------------------------------------------
def hash24(seed, i, channel):
    """-> the 24-bit integers u of samples i (an int array) on `channel`, as uint64."""
    with np.errstate(over="ignore"):
        i = np.asarray(i, np.uint64)
        x = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64(3) * i + np.uint64(channel + 1))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x >> np.uint64(40)


def _valid(faces, V):
    return ((faces >= 0) & (faces < V)).all(1)


def cross2(verts, faces):
    """|(v1 - v0) x (v2 - v0)|^2 in float64 per face (NaN for a face with an index outside [0, V))."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = _valid(f, len(v))
    out = np.full(len(f), np.nan)
    with np.errstate(all="ignore"):
        p = v[f[ok]]
        u, w = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        out[ok] = (nx * nx + ny * ny) + nz * nz
    return out


def integer_cdf(verts, faces):
    """-> (q [F] int64 integer weights, cdf [F] int64 inclusive sums, total)."""
    F = len(np.asarray(faces).reshape(-1, 3))
    with np.errstate(all="ignore"):
        w = np.sqrt(cross2(verts, faces))
    w = np.where(np.isfinite(w), w, 0.0)
    wmax = w.max() if F else 0.0
    s = 52
    while s > 0 and (1 << (52 - s)) < F:
        s -= 1
    q = np.zeros(F, np.int64)
    if wmax > 0:
        q = np.where(w > 0, np.trunc((w / wmax) * float(2 ** s)), 0.0).astype(np.int64)
    cdf = np.cumsum(q)
    return q, cdf, int(cdf[-1]) if F else 0


def sample(verts, faces, n, seed=0, dtype=np.float64):
    """-> (points [n, 3] dtype, face [n] int32)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    _, cdf, total = integer_cdf(v, f)
    assert total > 0
    i = np.arange(n, dtype=np.int64)
    u0, u1, u2 = (hash24(seed, i, c).astype(np.float64) for c in range(3))
    pos = ((i.astype(np.float64) + u0 * 2.0 ** -24) / float(n)) * float(total)
    k = np.minimum(np.trunc(pos).astype(np.int64), total - 1)
    face = np.searchsorted(cdf, k, side="right")
    x1, x2 = (u1 * 2.0 ** -24).astype(dtype), (u2 * 2.0 ** -24).astype(dtype)
    s = np.sqrt(x1)
    b0, b1, b2 = dtype(1) - s, s * (dtype(1) - x2), s * x2
    p = v[f[face]].astype(dtype)
    pts = (b0[:, None] * p[:, 0] + b1[:, None] * p[:, 1]) + b2[:, None] * p[:, 2]
    assert pts.dtype == dtype
    return pts, face.astype(np.int32)


# ---- point to triangle ----------------------------------------------------------------------------------------------------------------
REGIONS = ("a", "b", "ab", "c", "ac", "bc", "interior")


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def closest_on_triangle(p, a, b, c):
    """Broadcasting [..., 3] arrays of one dtype -> (D = squared distance, closest point, region index into REGIONS)."""
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = ap - ab
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = ap - ac
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        w5 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = (va + vb) + vc
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        v = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, one - w5], vb / den)
        w = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), w5], vc / den)
        region = np.select(conds, [0, 1, 2, 3, 4, 5], 6)
        rel = ab * v[..., None] + ac * w[..., None]
        e = ap - rel
        D = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return D, a + rel, region


def listed_faces(verts, faces):
    """-> (indices of the faces a grid lists, number of degenerate / non-finite faces); an index outside [0, V) raises."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not _valid(f, len(v)).all():
        raise ValueError("face index")
    c2 = cross2(v, f)
    finite = np.isfinite(v[f].astype(np.float64)).all((1, 2)) if len(f) else np.zeros(0, bool)
    ok = finite & (c2 != 0)
    return np.nonzero(ok)[0], int((~ok).sum())


def point_mesh(points, verts, faces, dtype=np.float64, chunk=400000):
    """Brute force -> (dist [n] dtype, face [n] int32, closest [n, 3] dtype).  No listed face: +inf / -1 / NaN; a non-finite
    point: NaN / -1 / NaN."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    keep, _ = listed_faces(v, f)
    n = len(pts)
    dist, face, close = np.full(n, np.inf, dtype), np.full(n, -1, np.int32), np.full((n, 3), np.nan, dtype)
    bad = ~np.isfinite(pts).all(1)
    dist[bad] = np.nan
    good = np.nonzero(~bad)[0]
    if len(keep) == 0 or len(good) == 0:
        return dist, face, close
    tri = v[f[keep]].astype(dtype)                                      # [K, 3, 3]
    step = max(1, chunk // len(keep))
    for s in range(0, len(good), step):
        idx = good[s:s + step]
        p = pts[idx].astype(dtype)[:, None, :]
        D, cl, _ = closest_on_triangle(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        assert D.dtype == dtype
        j = np.argmin(D, axis=1)                                        # the first minimum: the smaller face index
        r = np.arange(len(idx))
        dist[idx] = np.sqrt(D[r, j])
        face[idx] = keep[j]
        close[idx] = cl[r, j]
    return dist, face, close


def distance_to_face(points, verts, faces, face_of_point):
    """float64 distance of point i to face face_of_point[i]."""
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    tri = np.asarray(verts, np.float32).reshape(-1, 3)[np.asarray(faces, np.int64).reshape(-1, 3)[face_of_point]].astype(np.float64)
    return np.sqrt(closest_on_triangle(pts, tri[:, 0], tri[:, 1], tri[:, 2])[0])


# ---- the summary ------------------------------------------------------------------------------------------------------------------------
def summary(d_vertices, d_samples):
    dv, ds = np.asarray(d_vertices, np.float64).reshape(-1), np.asarray(d_samples, np.float64).reshape(-1)
    return {"mean": ds.mean(), "rms": np.sqrt((ds * ds).mean()), "max": np.concatenate([dv, ds]).max(), "p95": np.quantile(ds, 0.95),
            "n": len(ds)}


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------------
TRIANGLE = np.float32([[0.25, 0.5, 1.0], [2.25, 0.5, 1.0], [0.25, 1.5, 1.0]])          # a right triangle in the plane z = 1


def region_points():
    """One query point per region of TRIANGLE -> (points [7, 3] f32 in REGIONS order, distances in closed form, float64)."""
    a, b, c = TRIANGLE.astype(np.float64)
    h = np.hypot(2.0, 1.0)
    pts = np.float32([a + [-1, -1, 0.5], b + [2, -0.5, 0], a + [1, -2, 1], c + [-0.25, 3, 0], a + [-1.5, 0.5, -2],
                      (b + c) / 2 + np.array([1.0, 2.0, 0.0]) * 0.75, a + [0.5, 0.25, -3]])
    want = np.array([np.sqrt(1 + 1 + 0.25), np.hypot(2, 0.5), np.hypot(2, 1), np.hypot(0.25, 3), np.hypot(1.5, 2), 0.75 * h, 3.0])
    return pts, want


def zero_points():
    """In the plane (interior), on an edge, on a corner of TRIANGLE: distance 0 to rounding."""
    a, b, c = TRIANGLE
    return np.float32([a * 0.5 + b * 0.25 + c * 0.25, a * 0.5 + b * 0.5, c])


@functools.lru_cache(maxsize=None)
def soup():
    """300 random triangles in the unit cube (corners within 0.1 of a random centre), one spanning the whole cube, one 1e-4
    across; 2000 points: half inside the cube, a quarter within 1e-3 of a face, a quarter outside, up to 5 cube edges away.
    -> (verts f32, faces i32, points f32)."""
    rng = np.random.default_rng(20240607)
    centre = rng.uniform(0, 1, (300, 1, 3))
    tri = np.clip(centre + rng.uniform(-0.1, 0.1, (300, 3, 3)), 0, 1)
    tri[17] = [[0, 0, 0], [1, 1, 0], [1, 0, 1]]
    tri[211] = tri[211, :1] * 0.5 + 0.25 + rng.uniform(0, 1e-4, (3, 3))
    verts = tri.reshape(-1, 3).astype(np.float32)
    faces = np.arange(900, dtype=np.int32).reshape(-1, 3)
    inside = rng.uniform(0, 1, (1000, 3))
    on = rng.integers(0, 300, 500)
    bary = rng.dirichlet([1, 1, 1], 500)
    t64 = verts.astype(np.float64).reshape(-1, 3, 3)[on]
    nrm = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    near = (bary[:, :, None] * t64).sum(1) + nrm * rng.uniform(-1e-3, 1e-3, (500, 1))
    outside = rng.uniform(-5, 6, (500, 3))
    pts = np.concatenate([inside, near, outside]).astype(np.float32)
    return verts, faces, pts


SPHERE_CENTRE = np.array([48.3, 47.8, 48.1])
SPHERE_RADIUS = 40.3
SPHERE_SAMPLES, SPHERE_CHECKED = 20000, 500


@functools.lru_cache(maxsize=None)
def sphere_pair():
    """S.case("sphere")'s mesh and the same mesh scaled by 1.01 about the sphere's centre -> (verts, faces, scaled verts)."""
    from tests import simplify_reference as S
    v, f = S.case("sphere")[:2]
    v = np.asarray(v, np.float32)
    scaled = (SPHERE_CENTRE + (v.astype(np.float64) - SPHERE_CENTRE) * 1.01).astype(np.float32)
    return v, np.asarray(f, np.int32), scaled


@functools.lru_cache(maxsize=None)
def sphere_samples(dtype=np.float64):
    v, f, _ = sphere_pair()
    return sample(v, f, SPHERE_SAMPLES, 0, dtype)


def sphere_checked():
    """The indices of the SPHERE_CHECKED samples that are compared with the float64 restatement."""
    return np.arange(SPHERE_CHECKED) * (SPHERE_SAMPLES // SPHERE_CHECKED)


@functools.lru_cache(maxsize=None)
def sphere_distances(dtype=np.float64):
    """Brute-force distances of the checked samples (as the float32 points a device would hold) to the scaled sphere."""
    _, f, scaled = sphere_pair()
    pts = sphere_samples(np.float32)[0][sphere_checked()]
    return point_mesh(pts, scaled, f, dtype)
