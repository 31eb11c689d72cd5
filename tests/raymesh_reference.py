"""Numpy restatement of the ray-mesh contract of include/tensoir_hip.h (tir_ray_mesh) and of ops.mesh_inside.

    per face     A = a - o, B = b - o, C = c - o in float64 from the float32 inputs;
                 e(P, Q) = (dx (Py Qz - Pz Qy) + dy (Pz Qx - Px Qz)) + dz (Px Qy - Py Qx);  u = e(B, C), v = e(C, A), w = e(A, B);
                 the line meets the face iff u, v, w are all >= 0 or all <= 0 and not all zero;
                 n = (b - a) x (c - a), den = (dx nx + dy ny) + dz nz (0: a miss), t = ((Ax nx + Ay ny) + Az nz) / den;
                 accepted iff t0 <= t <= t1;  bary = (v, w) / ((u + v) + w);  grazed = an accepted hit with u, v or w == 0
    per ray      the nearest accepted hit (smaller float64 t, then the smaller face index), the number of accepted hits
    faces        the faces a grid lists: distance_reference.listed_faces (no area in float64, or a non-finite corner: skipped)
    invalid      a non-finite origin or direction, d == 0, a NaN in trange or t0 > t1: t = NaN, face = -1, count = 0, flags = 2

ray_mesh() is brute force over every listed face; traverse() restates the grid walk of k_ray_mesh for ONE ray (slow: the tests
give it a few dozen rays per grid) over a grid built by build_grid(), so that the walk can be checked against brute force
without a GPU.  Also the cases the CPU and the GPU tests share.
"""
import functools

import numpy as np

from tests import distance_reference as D

GRAZED, INVALID = 1, 2
SLACK = 1.0 / 8192.0
# ops.MESH_INSIDE_DIRECTIONS / TIR_RAY_INSIDE_DIRECTIONS of the header
DIRECTIONS = np.float32([[0.5345225, 0.2672612, 0.8017837], [-0.6882472, 0.6246950, -0.3692745], [0.1825742, -0.9128709, -0.3651484]])


def edge(d, P, Q):
    """e(P, Q) of the header: broadcasting [..., 3] float64 arrays."""
    return (d[..., 0] * (P[..., 1] * Q[..., 2] - P[..., 2] * Q[..., 1]) + d[..., 1] * (P[..., 2] * Q[..., 0] - P[..., 0] * Q[..., 2])) + \
        d[..., 2] * (P[..., 0] * Q[..., 1] - P[..., 1] * Q[..., 0])


def ray_triangle(o, d, a, b, c):
    """Broadcasting float64 [..., 3] -> (meets: the line meets the face and den != 0, t, u, v, w)."""
    with np.errstate(all="ignore"):
        A, B, C = a - o, b - o, c - o
        u, v, w = edge(d, B, C), edge(d, C, A), edge(d, A, B)
        meets = (((u >= 0) & (v >= 0) & (w >= 0)) | ((u <= 0) & (v <= 0) & (w <= 0))) & ~((u == 0) & (v == 0) & (w == 0))
        p, q = b - a, c - a
        nx = p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1]
        ny = p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2]
        nz = p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]
        den = (d[..., 0] * nx + d[..., 1] * ny) + d[..., 2] * nz
        t = ((A[..., 0] * nx + A[..., 1] * ny) + A[..., 2] * nz) / den
    return meets & (den != 0), t, u, v, w


def _ranges(n, trange):
    tr = np.empty((n, 2), np.float32)
    tr[:, 0], tr[:, 1] = 0.0, np.inf
    if trange is not None:
        tr[:] = np.asarray(trange, np.float32).reshape(n, 2)
    return tr


def invalid_rays(origins, dirs, trange=None):
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    tr = _ranges(len(o), trange)
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(o).all(1) | ~np.isfinite(d).all(1) | (d == 0).all(1) | ~(tr[:, 0] <= tr[:, 1])


def ray_mesh(origins, dirs, verts, faces, trange=None, chunk=2000000):
    """Brute force -> {"t" [n] f64, "face" [n] i32, "bary" [n, 2] f64, "count" [n] i32, "flags" [n] i32}.  A miss: +inf, -1, NaN."""
    o32 = np.asarray(origins, np.float32).reshape(-1, 3)
    d32 = np.asarray(dirs, np.float32).reshape(-1, 3)
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = len(o32)
    tr = _ranges(n, trange).astype(np.float64)
    keep, _ = D.listed_faces(v, f)
    bad = invalid_rays(o32, d32, trange)
    out = {"t": np.full(n, np.inf), "face": np.full(n, -1, np.int32), "bary": np.full((n, 2), np.nan), "count": np.zeros(n, np.int32),
           "flags": np.where(bad, INVALID, 0).astype(np.int32)}
    out["t"][bad] = np.nan
    good = np.nonzero(~bad)[0]
    if len(keep) == 0 or len(good) == 0:
        return out
    tri = v[f[keep]].astype(np.float64)                                  # [K, 3, 3]
    step = max(1, chunk // len(keep))
    for s in range(0, len(good), step):
        idx = good[s:s + step]
        o, d = o32[idx].astype(np.float64)[:, None, :], d32[idx].astype(np.float64)[:, None, :]
        meets, t, u, vv, w = ray_triangle(o, d, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        with np.errstate(invalid="ignore"):
            hit = meets & (t >= tr[idx, 0, None]) & (t <= tr[idx, 1, None])
        out["count"][idx] = hit.sum(1)
        out["flags"][idx] |= np.where((hit & ((u == 0) | (vv == 0) | (w == 0))).any(1), GRAZED, 0).astype(np.int32)
        tt = np.where(hit, t, np.inf)
        j = np.argmin(tt, axis=1)                                       # the first minimum: the smaller face index
        r = np.arange(len(idx))
        any_hit = hit.any(1)
        h = idx[any_hit]
        rj, jj = r[any_hit], j[any_hit]
        out["t"][h] = t[rj, jj]
        out["face"][h] = keep[jj]
        with np.errstate(all="ignore"):
            s3 = (u[rj, jj] + vv[rj, jj]) + w[rj, jj]
            out["bary"][h, 0], out["bary"][h, 1] = vv[rj, jj] / s3, w[rj, jj] / s3
    return out


def inside(points, verts, faces):
    """-> (inside bool, votes 0..3, grazed bool): a vote is an odd number of hits on [0, +inf) along one of DIRECTIONS."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    votes, grazed = np.zeros(len(p), np.int64), np.zeros(len(p), bool)
    for d in DIRECTIONS:
        r = ray_mesh(p, np.broadcast_to(d, p.shape), verts, faces)
        votes += r["count"] & 1
        grazed |= (r["flags"] & GRAZED) != 0
    return votes >= 2, votes.astype(np.uint8), grazed


# ---- the grid and the walk, scalar -----------------------------------------------------------------------------------------------------
def cell_of(x, origin, cell, dim):
    """clamp(floor((x - origin) / cell), 0, dim - 1), float32, every operation rounded on its own; NaN -> 0."""
    with np.errstate(all="ignore"):
        q = np.floor((np.float32(x) - np.float32(origin)) / np.float32(cell))
    if not q > 0:
        return 0
    return dim - 1 if q >= np.float32(dim - 1) else int(q)


def mesh_bounds(verts):
    """ops.face_grid's "bounds": the box of the finite vertices, padded by 2^-16 max(max |coordinate|, largest extent), float32."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    fin = np.isfinite(v)
    big = np.finfo(np.float32).max
    lo, hi = np.where(fin, v, big).min(0), np.where(fin, v, -big).max(0)
    pad = np.float32(2.0 ** -16) * max(np.maximum(np.abs(lo), np.abs(hi)).max(), (hi - lo).max())
    return np.concatenate([lo - pad, hi + pad]).astype(np.float32)


def build_grid(verts, faces, cell, origin, dims):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cells = {}
    ranges = {}
    for k in D.listed_faces(v, f)[0]:
        tri = v[f[k]]
        lo = [cell_of(tri[:, a].min(), origin[a], cell[a], dims[a]) for a in range(3)]
        hi = [cell_of(tri[:, a].max(), origin[a], cell[a], dims[a]) for a in range(3)]
        ranges[int(k)] = (lo, hi)
        for x in range(lo[0], hi[0] + 1):
            for y in range(lo[1], hi[1] + 1):
                for z in range(lo[2], hi[2] + 1):
                    cells.setdefault((x, y, z), []).append(int(k))
    return {"cell": [float(np.float32(c)) for c in cell], "origin": [float(np.float32(o)) for o in origin], "dims": list(dims),
            "cells": cells, "ranges": ranges, "bounds": mesh_bounds(v)}


def traverse(o, d, trange, verts, faces, grid, mode="count"):
    """The walk of k_ray_mesh for one valid ray -> (t f64, face, count, flags, cells visited, tests made)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    o, d = np.asarray(o, np.float32).astype(np.float64), np.asarray(d, np.float32).astype(np.float64)
    t0, t1 = (0.0, np.inf) if trange is None else (float(np.float32(trange[0])), float(np.float32(trange[1])))
    b = grid["bounds"].astype(np.float64)
    org, cl, dims = grid["origin"], grid["cell"], grid["dims"]
    miss = (np.inf, -1, 0, 0, 0, 0)
    T0, T1 = t0, t1
    for a in range(3):
        if d[a] == 0:
            if o[a] < b[a] or o[a] > b[3 + a]:
                return miss
        else:
            ta, tb = (b[a] - o[a]) / d[a], (b[3 + a] - o[a]) / d[a]
            T0, T1 = max(T0, min(ta, tb)), min(T1, max(ta, tb))
    if not T0 <= T1:
        return miss
    e = [SLACK * cl[a] + 2.0 ** -20 * max(abs(b[a]), abs(b[3 + a])) for a in range(3)]
    ad = np.abs(d)
    m = 1 if ad[1] > ad[0] else 0
    if ad[2] > max(ad[0], ad[1]):
        m = 2
    p, q = (m + 1) % 3, (m + 2) % 3
    tw = max(e) / ad[m]
    T0w, T1w = T0 - tw, T1 + tw
    x0, x1 = o[m] + T0 * d[m], o[m] + T1 * d[m]
    sa = cell_of(np.float32(min(x0, x1) - e[m]), org[m], cl[m], dims[m])
    sb = cell_of(np.float32(max(x0, x1) + e[m]), org[m], cl[m], dims[m])
    fwd = d[m] > 0
    best_t, best_f, count, flags, visited, tests = np.inf, 2 ** 31 - 1, 0, 0, 0, 0
    for k in range(sb - sa + 1):
        s = sa + k if fwd else sb - k
        L, H = org[m] + s * cl[m], org[m] + (s + 1) * cl[m]
        with np.errstate(all="ignore"):
            tl, th = ((L - e[m]) - o[m]) / d[m], ((H + e[m]) - o[m]) / d[m]
        if s == 0:
            tl = -np.inf if fwd else np.inf
        if s == dims[m] - 1:
            th = np.inf if fwd else -np.inf
        ta, tb = (tl, th) if fwd else (th, tl)
        if mode == "closest" and best_t < ta:
            break
        ta, tb = max(ta, T0w), min(tb, T1w)
        if not ta <= tb:
            continue
        rng = []
        for a in (p, q):
            ya, yb = o[a] + ta * d[a], o[a] + tb * d[a]
            rng.append((cell_of(np.float32(min(ya, yb) - e[a]), org[a], cl[a], dims[a]),
                        cell_of(np.float32(max(ya, yb) + e[a]), org[a], cl[a], dims[a])))
        for jp in range(rng[0][0], rng[0][1] + 1):
            for jq in range(rng[1][0], rng[1][1] + 1):
                c = [0, 0, 0]
                c[m], c[p], c[q] = s, jp, jq
                visited += 1
                for k2 in grid["cells"].get(tuple(c), ()):
                    tests += 1
                    tri = v[f[k2]]
                    meets, t, u, vv, w = ray_triangle(o, d, tri[0], tri[1], tri[2])
                    if not (meets and t0 <= t <= t1):
                        continue
                    if mode == "count":
                        lo, hi = grid["ranges"][k2]
                        with np.errstate(all="ignore"):
                            h = [min(max(cell_of(np.float32(o[a] + t * d[a]), org[a], cl[a], dims[a]), lo[a]), hi[a]) for a in range(3)]
                        if h != c:
                            continue
                        count += 1
                        flags |= GRAZED if (u == 0 or vv == 0 or w == 0) else 0
                    if t < best_t or (t == best_t and k2 < best_f):
                        best_t, best_f = float(t), k2
                        closest_grazed = GRAZED if (u == 0 or vv == 0 or w == 0) else 0
    if mode == "closest" and best_f != 2 ** 31 - 1:
        count, flags = 1, closest_grazed
    return (best_t, best_f if best_f != 2 ** 31 - 1 else -1, count, flags, visited, tests)


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------------
TRIANGLE_FACE = np.int32([[0, 1, 2]])


def triangle_rays():
    """Dyadic rays against D.TRIANGLE (a = (.25, .5, 1), b = (2.25, .5, 1), c = (.25, 1.5, 1), in the plane z = 1) with their
    outputs in closed form -> (origins, dirs, trange, t, face, bary (b, c weights), count, flags); every value is exact."""
    inf, nan = np.inf, np.nan
    rows = [
        # origin, direction, trange, t, face, bary, count, flags
        ([0.75, 0.75, 0.0], [0, 0, 1], [0, inf], 1.0, 0, [0.25, 0.25], 1, 0),             # interior, from below
        ([0.75, 0.75, 3.0], [0, 0, -1], [0, inf], 2.0, 0, [0.25, 0.25], 1, 0),            # interior, from above
        ([0.75, 0.75, 0.0], [0, 0, 4], [0, inf], 0.25, 0, [0.25, 0.25], 1, 0),            # a direction that is not unit
        ([0.25, 0.25, 0.0], [0.5, 0.5, 1], [0, inf], 1.0, 0, [0.25, 0.25], 1, 0),         # oblique, dyadic
        ([1.25, 0.5, 0.0], [0, 0, 1], [0, inf], 1.0, 0, [0.5, 0.0], 1, GRAZED),           # through edge ab
        ([0.25, 1.0, 2.0], [0, 0, -1], [0, inf], 1.0, 0, [0.0, 0.5], 1, GRAZED),          # through edge ca
        ([1.25, 1.0, 0.0], [0, 0, 1], [0, inf], 1.0, 0, [0.5, 0.5], 1, GRAZED),           # through edge bc
        ([0.25, 0.5, 0.0], [0, 0, 1], [0, inf], 1.0, 0, [0.0, 0.0], 1, GRAZED),           # through corner a
        ([2.25, 0.5, 0.0], [0, 0, 1], [0, inf], 1.0, 0, [1.0, 0.0], 1, GRAZED),           # through corner b
        ([0.25, 1.5, 0.0], [0, 0, 1], [0, inf], 1.0, 0, [0.0, 1.0], 1, GRAZED),           # through corner c
        ([-1.0, 0.75, 1.0], [1, 0, 0], [0, inf], inf, -1, [nan, nan], 0, 0),              # in the plane: den == 0
        ([0.75, 0.75, 2.0], [0, 0, 1], [0, inf], inf, -1, [nan, nan], 0, 0),              # the face lies behind the origin
        ([0.75, 0.75, 0.0], [0, 0, 1], [1.5, 8], inf, -1, [nan, nan], 0, 0),              # excluded by t0
        ([0.75, 0.75, 0.0], [0, 0, 1], [0, 0.75], inf, -1, [nan, nan], 0, 0),             # excluded by t1
        ([0.75, 0.75, 0.0], [0, 0, 1], [1.0, 8], 1.0, 0, [0.25, 0.25], 1, 0),             # t == t0: accepted
        ([0.75, 0.75, 0.0], [0, 0, 1], [0, 1.0], 1.0, 0, [0.25, 0.25], 1, 0),             # t == t1: accepted
        ([0.75, 0.75, 2.0], [0, 0, 1], [-4, 8], -1.0, 0, [0.25, 0.25], 1, 0),             # a negative range reaches behind
        ([3.0, 3.0, 0.0], [0, 0, 1], [0, inf], inf, -1, [nan, nan], 0, 0),                # beside the face
    ]
    cols = list(zip(*rows))
    return (np.float32(cols[0]), np.float32(cols[1]), np.float32(cols[2]), np.float64(cols[3]), np.int32(cols[4]), np.float64(cols[5]),
            np.int32(cols[6]), np.int32(cols[7]))


CUBE_VERTS = np.float32([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])          # index = 4 x + 2 y + z
# two faces per side, outward normals, each side split along the diagonal through its lowest and its highest corner
CUBE_FACES = np.int32([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                       [1, 5, 7], [1, 7, 3]])


def open_cube():
    """The cube minus the two faces of its side x = 1."""
    return CUBE_VERTS, np.delete(CUBE_FACES, [2, 3], axis=0)


def unwelded(verts, faces):
    """Three vertices of its own per face (what a .glb holds)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.asarray(verts, np.float32)[f.reshape(-1)], np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)


SOUP_GRIDS = {"1": dict(dims=[1, 1, 1]), "4": dict(dims=[4, 4, 4]), "16": dict(dims=[16, 16, 16]), "64": dict(dims=[64, 64, 64]),
              "anisotropic": dict(dims=[3, 50, 11]), "inside": dict(cell=[0.05, 0.07, 0.11], origin=[0.3, 0.2, 0.4], dims=[5, 6, 2])}


def numpy_grid(verts, faces, dims, cell=None, origin=None):
    """build_grid with ops.face_grid's defaults: origin = the lowest vertex, cell = extent / dims (1 + 1e-6)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    org = lo if origin is None else np.float64(origin)
    ext = np.maximum(hi - org, 0.0)
    cl = [e / g * (1.0 + 1e-6) if e > 0 else 1.0 for e, g in zip(ext, dims)] if cell is None else cell
    return build_grid(v, faces, cl, org, dims)


@functools.lru_cache(maxsize=None)
def soup_rays():
    """2000 rays against D.soup(): 667 from outside the unit cube aimed at a point inside it, 667 starting inside, 666 with one or
    two zero direction components or aimed away from the cube; a third of all carry a finite trange -> (origins, dirs, trange)."""
    rng = np.random.default_rng(20241021)
    n1, n2, n3 = 667, 667, 666
    o1 = rng.uniform(-3, 4, (n1, 3))
    o1[np.all((o1 > -0.2) & (o1 < 1.2), axis=1)] += 3.0
    d1 = rng.uniform(0, 1, (n1, 3)) - o1
    o2, d2 = rng.uniform(0, 1, (n2, 3)), rng.normal(size=(n2, 3))
    o3 = np.concatenate([rng.uniform(0, 1, (n3 // 2, 3)), rng.uniform(-2, 3, (n3 - n3 // 2, 3))])
    d3 = rng.normal(size=(n3, 3))
    kind = rng.integers(0, 3, n3)
    for i in range(n3):
        if kind[i] == 0:
            d3[i, rng.integers(0, 3)] = 0.0
        elif kind[i] == 1:
            keep = rng.integers(0, 3)
            d3[i, [a for a in range(3) if a != keep]] = 0.0
        else:
            d3[i] = (o3[i] - 0.5) + rng.normal(size=3) * 0.1            # away from the cube's centre
    o = np.concatenate([o1, o2, o3]).astype(np.float32)
    d = np.concatenate([d1, d2, d3]).astype(np.float32)
    d[(d == 0).all(1)] = [0, 0, 1]
    tr = np.empty((len(o), 2), np.float32)
    tr[:, 0], tr[:, 1] = 0.0, np.inf
    ranged = rng.uniform(size=len(o)) < 1 / 3
    tr[ranged, 0] = rng.uniform(-0.5, 0.5, ranged.sum())
    tr[ranged, 1] = tr[ranged, 0] + rng.uniform(0, 2.0, ranged.sum())
    order = rng.permutation(len(o))
    return o[order], d[order], tr[order]


@functools.lru_cache(maxsize=None)
def soup_reference():
    v, f, _ = D.soup()
    o, d, tr = soup_rays()
    return ray_mesh(o, d, v, f, tr)


SPHERE_POINTS = 120


@functools.lru_cache(maxsize=None)
def sphere_points(n=3000):
    """n points in the box of the sphere and a little beyond -> (points f32, analytic distance to the centre minus the radius)."""
    rng = np.random.default_rng(7)
    p = (D.SPHERE_CENTRE + rng.uniform(-50, 50, (n, 3))).astype(np.float32)
    return p, np.linalg.norm(p.astype(np.float64) - D.SPHERE_CENTRE, axis=1) - D.SPHERE_RADIUS


@functools.lru_cache(maxsize=None)
def sphere_rays(n=4096):
    """Rays from (near) the sphere's centre outward, unit directions -> (origins, dirs)."""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = D.SPHERE_CENTRE + rng.uniform(-1, 1, (n, 3))
    return o.astype(np.float32), d.astype(np.float32)


# ---- the figures of mesh.distance ----------------------------------------------------------------------------------------------------------
def face_normals(verts, faces, idx):
    """Unit float64 normals of faces idx."""
    tri = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)[idx]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def normal_figures(n_own, n_near):
    dot = (n_own * n_near).sum(1)
    return {"normal_consistency": float(np.abs(dot).mean()), "flipped_share": float((dot < 0).mean())}


def fscore(d_a, d_b, thresholds):
    out = []
    for tau in thresholds:
        p, r = float((np.asarray(d_a) <= tau).mean()), float((np.asarray(d_b) <= tau).mean())
        out.append({"threshold": float(tau), "precision": p, "recall": r, "fscore": 2 * p * r / (p + r) if p + r > 0 else 0.0})
    return out
