"""Numpy restatement of the mesh-simplification contract of include/tensoir_hip.h (tir_simplify_*): quadric vertex clustering.
Step 1 (the cell of a vertex) is float32 with every operation rounded on its own, because it is discrete: marching-cubes
vertices lie ON lattice planes, which are cluster boundaries.  Everything after it takes the float32 q and runs in float64 (or in
`dtype`, which is how the float32 deviation the GPU tolerances rest on was measured).

    q = (v - origin) / cell (fp32);  i = clamp(floor(q), 0, dims - 1), a NaN -> 0;  key = (ix * dims_y + iy) * dims_z + iz
    output vertices = occupied cells in ascending key order; cell_of_vertex maps input to output vertices
    per cell c, u = q - (i_c + 0.5):  m, s = sum u over its vertices;  per face corner in c, n = (q1 - q0) x (q2 - q0), l = |n| > 0:
        A += n n^T / l,  b += n (n . (q0 - (i_c + 0.5))) / l,  N += n
    mu = s / m, t = trace A;  x = mu if t == 0 else solve (A + reg t I) x = b + reg t mu;  x clamped to [-0.5, 0.5]^3
    position = origin + (i_c + 0.5 + x) * cell;  normal = normalize(N / cell), (0, 0, 1) when N == 0
    faces remapped, dropped when two corners are equal, otherwise in input order with their winding; duplicates stay

Also the test volumes the CPU and GPU tests share (each meshed once per process).
"""
import functools
import os

import numpy as np

from tests import mesh_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mesh_skimage.npz")
ORIGIN = (-0.25, 0.5, 1.0)                 # the origin the golden volumes are meshed with here: not a multiple of any spacing
CASES = ("alpha", "blob", "onlevel", "open")


def cell_indices(verts, cell, origin, dims=None):
    """-> (q [V, 3] float32, i [V, 3] int64, dims [3] int64); dims None: floor(max q) + 1 per axis (at least 1)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    cell = np.broadcast_to(np.asarray(cell, np.float32), (3,))
    q = (v - np.asarray(origin, np.float32)) / cell
    assert q.dtype == np.float32
    f = np.floor(q)
    f = np.where(f > 0, f, np.float32(0)).astype(np.float64)            # a NaN compares false: index 0
    if dims is None:
        dims = (f.max(0) if len(f) else np.zeros(3)) + 1
    dims = np.asarray(dims, np.int64).reshape(3)
    i = np.minimum(f, (dims - 1).astype(np.float64)).astype(np.int64)
    return q, i, dims


def simplify(verts, faces, cell, origin=(0.0, 0.0, 0.0), dims=None, reg=1e-2, centroid=False, dtype=np.float64):
    """-> (positions [V', 3] dtype, faces' [F', 3] int32, unit normals [V', 3] dtype, cell_of_vertex [V] int32).
    centroid=True places every vertex at the mean mu of its cell's vertices instead of the quadric's minimum."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cell32 = np.broadcast_to(np.asarray(cell, np.float32), (3,))
    q, ci, dims = cell_indices(verts, cell, origin, dims)
    key = (ci[:, 0] * dims[1] + ci[:, 1]) * dims[2] + ci[:, 2]
    uk, vid = np.unique(key, return_inverse=True)
    vid = vid.reshape(-1)
    K = len(uk)
    cidx = np.stack([uk // (dims[1] * dims[2]), (uk // dims[2]) % dims[1], uk % dims[2]], 1)
    centre = cidx.astype(dtype) + dtype(0.5)
    v = q.astype(dtype)
    A, b, N = np.zeros((K, 3, 3), dtype), np.zeros((K, 3), dtype), np.zeros((K, 3), dtype)
    s, m = np.zeros((K, 3), dtype), np.zeros(K, dtype)
    np.add.at(s, vid, v - centre[vid])
    np.add.at(m, vid, 1)
    p = v[faces]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(dtype).reshape(-1, 3)
    ln = np.sqrt((n * n).sum(1)).astype(dtype)
    ok = ln > 0
    nn, ll, p0 = n[ok], ln[ok], p[ok, 0]
    for c in range(3):                                                  # once per corner
        k = vid[faces[ok, c]]
        d = np.einsum("ij,ij->i", nn, p0 - centre[k])
        np.add.at(A, k, nn[:, :, None] * nn[:, None, :] / ll[:, None, None])
        np.add.at(b, k, nn * (d / ll)[:, None])
        np.add.at(N, k, nn)
    mu = s / m[:, None]
    x = mu.copy()
    if not centroid:
        t = np.trace(A, axis1=1, axis2=2)
        nz = t > 0
        r = (dtype(reg) * t[nz]).astype(dtype)
        M = A[nz] + r[:, None, None] * np.eye(3, dtype=dtype)
        rhs = b[nz] + r[:, None] * mu[nz]
        if nz.any():
            x[nz] = np.linalg.solve(M, rhs[:, :, None])[:, :, 0]
    x = np.clip(x, -0.5, 0.5)
    pos = np.asarray(origin, np.float32).astype(dtype) + (centre + x) * cell32.astype(dtype)
    nw = N / cell32.astype(dtype)
    flat = (N == 0).all(1)
    nl = np.sqrt((nw * nw).sum(1))
    normals = np.where(flat[:, None], np.array([0, 0, 1], dtype), nw / np.where(flat, 1, nl)[:, None])
    f = vid[faces]
    keep = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return pos, f[keep].astype(np.int32).reshape(-1, 3), normals, vid.astype(np.int32)


def edge_balance(faces):
    """count(a -> b) == count(b -> a) for every directed edge: what a closed oriented mesh keeps when only degenerate faces are
    dropped (collapsed faces remove an edge and its reverse together, duplicates count on both sides)."""
    d = MR.directed_edges(faces)
    key, rkey = d[:, 0] * (1 << 32) + d[:, 1], d[:, 1] * (1 << 32) + d[:, 0]
    u, c = np.unique(key, return_counts=True)
    ur, cr = np.unique(rkey, return_counts=True)
    return bool(np.array_equal(u, ur) and np.array_equal(c, cr))


def in_cell_units(pos, cell, origin):
    """Positions in cell units (float64): (pos - origin) / cell."""
    cell = np.broadcast_to(np.asarray(cell, np.float32), (3,)).astype(np.float64)
    return (np.asarray(pos, np.float64) - np.asarray(origin, np.float32).astype(np.float64)) / cell


# ---- the shared test meshes ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_mesh(name):
    """-> (verts, faces, spacing [3] f32) of a volume of tests/golden/mesh_skimage.npz, meshed at ORIGIN."""
    G = np.load(GOLDEN)
    assert sorted(str(c) for c in G["cases"]) == sorted(CASES)
    vol, level, sp = G[name + "/vol"], float(G[name + "/level"]), G[name + "/spacing"].astype(np.float32)
    v, f, _ = MR.marching_cubes(vol, level, sp, ORIGIN)
    return v, f, sp


BOX_LO, BOX_HI = np.array([5.3, 6.6, 4.45]), np.array([22.7, 20.4, 23.55])


def box_distance(p):
    """Signed distance of points to the box's surface (negative inside)."""
    c, h = (BOX_LO + BOX_HI) / 2, (BOX_HI - BOX_LO) / 2
    d = np.abs(np.asarray(p, np.float64) - c) - h
    return np.linalg.norm(np.maximum(d, 0), axis=1) + np.minimum(d.max(1), 0)


@functools.lru_cache(maxsize=None)
def box_mesh():
    """A 29^3 volume of -max(|p - c| - h): a box whose faces lie between lattice planes, level 0, unit spacing, origin 0."""
    ax = np.arange(29, dtype=np.float64)
    P = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1)
    c, h = (BOX_LO + BOX_HI) / 2, (BOX_HI - BOX_LO) / 2
    vol = (-(np.abs(P - c) - h).max(-1)).astype(np.float32)
    v, f, _ = MR.marching_cubes(vol, 0.0, (1, 1, 1), (0, 0, 0))
    return v, f


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    """A 97^3 volume of 40.3 - |p - (48.3, 47.8, 48.1)|, level 0: 61 236 faces, several scan blocks of faces and of cells."""
    ax = np.arange(97, dtype=np.float64)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (40.3 - np.sqrt((X - 48.3) ** 2 + (Y - 47.8) ** 2 + (Z - 48.1) ** 2)).astype(np.float32)
    v, f, _ = MR.marching_cubes(vol, 0.0, (1, 1, 1), (0, 0, 0))
    return v, f


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (verts, faces, cell [3] f32, origin) of a named comparison case: "<volume>-k<k>", "box", "sphere"."""
    if name == "box":
        v, f = box_mesh()
        return v, f, np.float32([3, 3, 3]), (0.0, 0.0, 0.0)
    if name == "sphere":
        v, f = sphere_mesh()
        return v, f, np.float32([2, 2, 2]), (0.0, 0.0, 0.0)
    vol, k = name.split("-k")
    v, f, sp = golden_mesh(vol)
    return v, f, sp * np.float32(int(k)), ORIGIN


@functools.lru_cache(maxsize=None)
def reference(name):
    """simplify() of case(name) -> (pos, faces, normals, cell_of_vertex, dims)."""
    v, f, cell, origin = case(name)
    dims = cell_indices(v, cell, origin)[2]
    return simplify(v, f, cell, origin, dims) + (dims,)


GOLDEN_CASES = tuple(f"{c}-k{k}" for c in CASES for k in (2, 3))
