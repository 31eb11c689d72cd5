"""Vectorised numpy restatement of the marching-cubes contract of include/tensoir_hip.h (tir_mc_*), built on the committed case
table (tensoir_amd/csrc/tir_mc_table.hpp).  The GPU tests compare the kernels against it; the CPU tests compare it against
scikit-image (tests/golden/mesh_skimage.npz).

    vol [gx][gy][gz] fp32 (z fastest); a lattice point is inside iff value > level.
    vertices: one per lattice edge that crosses the level, in (point linear index, axis x < y < z) order, at
              origin + (idx(p) + t e_axis) * spacing, t = (level - v0) / (v1 - v0), every fp32 operation rounded on its own;
    normals:  -(central-difference gradient) interpolated along the edge, normalised (index space, no spacing);
    faces:    int32, in (cell linear index, table order) order; right-hand normals point from inside to outside.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tensoir_amd", "csrc", "tir_mc_table.hpp")


def load_table(path=TABLE):
    """-> (ntri uint8 [256], tri int8 [256][3*max_tri])"""
    src = open(path).read()
    mt = int(re.search(r"#define TIR_MC_MAX_TRI (\d+)", src).group(1))
    ntri = re.search(r"tir_mc_ntri\[256\] = \{(.*?)\};", src, flags=re.S).group(1)
    tri = re.search(r"tir_mc_tri\[256\]\[\d+\] = \{(.*?)\n\};", src, flags=re.S).group(1)
    tri = re.sub(r"//[^\n]*", "", tri)
    ntri = np.array([int(x) for x in ntri.replace("\n", " ").split(",") if x.strip()], np.uint8)
    rows = re.findall(r"\{([^}]*)\}", tri)
    tri = np.array([[int(x) for x in r.split(",")] for r in rows], np.int8)
    assert ntri.shape == (256,) and tri.shape == (256, 3 * mt)
    return ntri, tri


def edge_corner_axis():
    """edge id -> (corner offset [3], axis)"""
    off, axis = np.zeros((12, 3), np.int64), np.zeros(12, np.int64)
    for e in range(12):
        a, k = divmod(e, 4)
        o = [b for b in range(3) if b != a]
        off[e, o[0]], off[e, o[1]] = k & 1, (k >> 1) & 1
        axis[e] = a
    return off, axis


def gradient(vol):
    """Central differences (x 0.5) inside, one-sided differences on the lattice boundary; [3][gx][gy][gz] fp32."""
    v = vol.astype(np.float32)
    g = np.zeros((3,) + v.shape, np.float32)
    for a in range(3):
        s = [slice(None)] * 3
        n = v.shape[a]

        def sl(i0, i1):
            t = list(s)
            t[a] = slice(i0, i1)
            return tuple(t)
        ga = g[a]
        ga[sl(1, n - 1)] = (v[sl(2, n)] - v[sl(0, n - 2)]) * np.float32(0.5)
        ga[sl(0, 1)] = v[sl(1, 2)] - v[sl(0, 1)]
        ga[sl(n - 1, n)] = v[sl(n - 1, n)] - v[sl(n - 2, n - 1)]
    return g


def marching_cubes(vol, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), table=None):
    """-> (verts [V,3] f32, faces [F,3] i32, normals [V,3] f32)"""
    vol = np.ascontiguousarray(vol, np.float32)
    gx, gy, gz = vol.shape
    level = np.float32(level)
    sp = np.asarray(spacing, np.float32).reshape(3)
    org = np.asarray(origin, np.float32).reshape(3)
    ntri, tri = load_table() if table is None else table
    inside = vol > level
    N = vol.size
    # crossing bits of the +x / +y / +z edge of every lattice point
    cross = np.zeros((gx, gy, gz, 3), bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(N, 3)
    cnt = flat.sum(1)
    vbase = np.zeros(N, np.int64)
    vbase[1:] = np.cumsum(cnt)[:-1]
    pid, ax = np.nonzero(flat)                       # row-major: (point, axis) order
    idx = np.stack(np.unravel_index(pid, vol.shape), 1)
    vf = vol.reshape(-1)
    strides = np.array([gy * gz, gz, 1], np.int64)
    v0 = vf[pid]
    v1 = vf[pid + strides[ax]]
    t = (level - v0) / (v1 - v0)                     # fp32: each operation rounded
    pos = idx.astype(np.float32)
    rows = np.arange(len(pid))
    pos[rows, ax] = pos[rows, ax] + t
    verts = (org + pos * sp).astype(np.float32)
    g = gradient(vol).reshape(3, N)
    g0 = g[:, pid].T
    g1 = g[:, pid + strides[ax]].T
    n = -(g0 + t[:, None] * (g1 - g0))
    ln = np.sqrt((n * n).sum(1))
    normals = np.where(ln[:, None] > 0, n / np.where(ln > 0, ln, 1)[:, None], 0).astype(np.float32)
    # faces
    if gx < 2 or gy < 2 or gz < 2:
        return verts, np.zeros((0, 3), np.int32), normals
    case = np.zeros((gx - 1, gy - 1, gz - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= inside[dx:gx - 1 + dx, dy:gy - 1 + dy, dz:gz - 1 + dz].astype(np.int64) << c
    case = case.reshape(-1)                           # cells in linear order of their lowest corner
    cells = np.stack(np.unravel_index(np.arange(case.size), (gx - 1, gy - 1, gz - 1)), 1)
    nt = ntri[case].astype(np.int64)
    cell_of = np.repeat(np.arange(case.size), nt)
    slot = np.arange(nt.sum()) - np.repeat(np.cumsum(nt) - nt, nt)
    off, eax = edge_corner_axis()
    faces = np.zeros((len(cell_of), 3), np.int64)
    for k in range(3):
        e = tri[case[cell_of], 3 * slot + k].astype(np.int64)
        assert (e >= 0).all()
        corner = cells[cell_of] + off[e]
        p = corner @ strides
        a = eax[e]
        low = (flat[p] & (np.arange(3)[None, :] < a[:, None])).sum(1)
        faces[:, k] = vbase[p] + low
    return verts, faces.astype(np.int32), normals


def n_crossing_edges(vol, level):
    v = np.asarray(vol, np.float32) > np.float32(level)
    return int((v[1:] != v[:-1]).sum() + (v[:, 1:] != v[:, :-1]).sum() + (v[:, :, 1:] != v[:, :, :-1]).sum())


def signed_volume(verts, faces):
    v = verts.astype(np.float64)[faces]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def area(verts, faces):
    v = verts.astype(np.float64)[faces]
    return float(np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1).sum() / 2.0)


def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_and_oriented(faces):
    """Every directed edge appears once and its reverse once (a closed, consistently oriented 2-manifold edge structure)."""
    d = directed_edges(faces)
    d = d[d[:, 0] != d[:, 1]]
    key = d[:, 0] * (1 << 32) + d[:, 1]
    rkey = d[:, 1] * (1 << 32) + d[:, 0]
    u, c = np.unique(key, return_counts=True)
    return bool((c == 1).all() and np.isin(rkey, key).all())


def edge_keys(verts, spacing, shape, origin=(0.0, 0.0, 0.0)):
    """The lattice edge (point linear index * 3 + axis) each vertex lies on, recovered from its position: the axis whose
    index coordinate is farthest from an integer.  Meaningful for vertices strictly inside their edge (0 < t < 1)."""
    c = (np.asarray(verts, np.float64) - np.asarray(origin, np.float64)) / np.asarray(spacing, np.float64)
    ax = np.abs(c - np.round(c)).argmax(1)
    pt = np.round(c).astype(np.int64)
    rows = np.arange(len(c))
    pt[rows, ax] = np.floor(c[rows, ax]).astype(np.int64)
    return ((pt[:, 0] * shape[1] + pt[:, 1]) * shape[2] + pt[:, 2]) * 3 + ax


def crossing_keys(vol, level):
    """Edge keys of the crossing lattice edges in the kernel's vertex order."""
    v = np.asarray(vol, np.float32) > np.float32(level)
    cross = np.zeros(v.shape + (3,), bool)
    cross[:-1, :, :, 0] = v[:-1] != v[1:]
    cross[:, :-1, :, 1] = v[:, :-1] != v[:, 1:]
    cross[:, :, :-1, 2] = v[:, :, :-1] != v[:, :, 1:]
    return np.nonzero(cross.reshape(-1))[0]


def cell_polygons(face_keys, shape):
    """Per cell: the undirected boundary segments of the cell's triangles (pairs of edge keys used by exactly one of them) --
    the surface polygon independent of how it was triangulated.  A triangle belongs to the lowest cell that holds all three
    of its edges."""
    shape = np.asarray(shape)
    fk = np.asarray(face_keys, np.int64)
    pts = np.stack(np.unravel_index(fk // 3, tuple(shape)), -1)
    axes = fk % 3
    polys = {}
    for f in range(len(fk)):
        common = None
        for k in range(3):
            o = [b for b in range(3) if b != axes[f, k]]
            cells = set()
            for d0 in (0, 1):
                for d1 in (0, 1):
                    c = pts[f, k].copy()
                    c[o[0]] -= d0
                    c[o[1]] -= d1
                    if (c >= 0).all() and (c < shape - 1).all():
                        cells.add(tuple(int(x) for x in c))
            common = cells if common is None else common & cells
        polys.setdefault(min(common), []).append(fk[f])
    out = {}
    for cell, tris in polys.items():
        cnt = {}
        for t in tris:
            for i in range(3):
                e = (min(t[i], t[(i + 1) % 3]), max(t[i], t[(i + 1) % 3]))
                cnt[e] = cnt.get(e, 0) + 1
        out[cell] = frozenset(e for e, n in cnt.items() if n == 1)
    return out


def ambiguous_cells(vol, level):
    """Cells (lowest corner index) with at least one face whose inside corners are diagonal."""
    v = np.asarray(vol, np.float32) > np.float32(level)
    gx, gy, gz = v.shape
    cor = {c: v[c & 1:gx - 1 + (c & 1), (c >> 1) & 1:gy - 1 + ((c >> 1) & 1), (c >> 2) & 1:gz - 1 + ((c >> 2) & 1)]
           for c in range(8)}
    amb = np.zeros((gx - 1, gy - 1, gz - 1), bool)
    for axis in range(3):
        u, w = [a for a in range(3) if a != axis]
        for side in (0, 1):
            b = side << axis
            c0, c1, c2, c3 = b, b | 1 << u, b | 1 << u | 1 << w, b | 1 << w
            amb |= (cor[c0] == cor[c2]) & (cor[c1] == cor[c3]) & (cor[c0] != cor[c1])
    return {tuple(int(x) for x in c) for c in np.argwhere(amb)}


def sorted_rows(a):
    a = np.asarray(a)
    return a[np.lexsort(a.T[::-1])]
