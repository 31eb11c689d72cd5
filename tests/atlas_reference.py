"""Numpy restatement of the texture-atlas contract of include/tensoir_hip.h (tir_atlas_*): the per-triangle layout, the per-texel
surface samples, the unwelded corners and the arithmetic of the three packed images.  Discrete steps (ownership, the nearest
point of the UV triangle) are integer arithmetic; uv is one float32 division, as the contract demands; everything continuous is
float64 unless dtype=np.float32 asks for the whole chain in float32 (the yardstick of the GPU test's bound)."""
import functools
import math

import numpy as np

MIN_T = 6
# The bounds of the GPU comparison (tests/test_gpu_atlas.py) on the continuous outputs: ten times the distance of this restatement
# run wholly in float32 from its float64 self over layout_cases(), which tests/test_atlas_cpu.py measures: 1.16e-7 of the largest
# |coordinate| for `point`, 1.20e-7 per component for `outward`, 3.52e-7 per component for the tangent.  Device float32 may fuse
# and associate the three-term sums differently; the factor of ten covers that.
POINT_TOL, OUTWARD_TOL, TAN_TOL = 1.2e-6, 1.2e-6, 3.6e-6


def layout(F, size):
    """-> (cols, T) of F faces in a size x size image; ValueError when a cell would have fewer than MIN_T texels per side."""
    n_cells = (int(F) + 1) // 2
    cols = math.isqrt(n_cells - 1) + 1 if n_cells > 0 else 1          # ceil(sqrt(n_cells))
    T = int(size) // cols
    if T < MIN_T:
        raise ValueError(f"size {size} leaves {T} texels per cell; {F} faces need at least {MIN_T * cols}")
    return cols, T


def corner_uv_local(T):
    """Cell-local UV corners in texel units -> (lower [3, 2], upper [3, 2]), corner order 0, 1, 2."""
    lower = np.array([[1, 1], [T - 3, 1], [1, T - 3]], dtype=np.int64)
    return lower, T - lower


def upper_owned(T):
    """[T, T] bool indexed [j, i]: the texels of a cell with two faces that the upper face owns."""
    j, i = np.mgrid[0:T, 0:T]
    return i + j >= T


def nearest(X, Y, L):
    """Nearest point of the triangle (0, 0), (L, 0), (0, L) to the integer points (X, Y) (quarter texels) -> (qx, qy), exact."""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    inside = (X >= 0) & (Y >= 0) & (X + Y <= L)
    ax, by = np.clip(X, 0, L), np.clip(Y, 0, L)
    s = L - X + Y
    assert (s % 2 == 0).all()
    u = np.clip(s // 2, 0, L)
    cand = [(ax, np.zeros_like(ax)), (np.zeros_like(by), by), (L - u, u)]
    qx, qy = cand[0]
    d = (X - qx) ** 2 + (Y - qy) ** 2
    for cx, cy in cand[1:]:
        dc = (X - cx) ** 2 + (Y - cy) ** 2
        take = dc < d
        qx, qy, d = np.where(take, cx, qx), np.where(take, cy, qy), np.where(take, dc, d)
    return np.where(inside, X, qx), np.where(inside, Y, qy)


@functools.lru_cache(maxsize=None)
def cell_barycentrics(T, dtype=np.float64):
    """-> (lower [T, T, 3], upper [T, T, 3]) indexed [j, i]: the clamped barycentrics of every texel centre of a cell with respect
    to the lower / the upper face's UV triangle (all texels, whoever owns them: an odd last face owns its whole cell)."""
    j, i = np.mgrid[0:T, 0:T]
    L = 4 * (T - 4)
    out = []
    for X, Y in ((4 * i - 2, 4 * j - 2), (4 * (T - i) - 6, 4 * (T - j) - 6)):
        qx, qy = nearest(X, Y, L)
        num = np.stack([L - qx - qy, qx, qy], -1)
        assert (num >= 0).all()
        out.append(num.astype(dtype) / dtype(L))
    return out[0], out[1]


def texel_index(F, cols, T):
    """Cell-major texels of the used cells -> (c, j, i, owner face, upper flag), each [N]."""
    n_cells = (F + 1) // 2
    idx = np.arange(n_cells * T * T, dtype=np.int64)
    c, r = idx // (T * T), idx % (T * T)
    j, i = r // T, r % T
    upper = (i + j >= T) & (2 * c + 1 < F)
    return c, j, i, 2 * c + upper, upper


def _len(x):
    return np.sqrt(x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1] + x[..., 2] * x[..., 2])


def unit_normals(b, v, n):
    """b [N, 3], v / n [N, 3, 3] (corner, axis) -> normalize(sum b_k n_k) with the contract's two fallbacks."""
    s = b[:, 0:1] * n[:, 0] + b[:, 1:2] * n[:, 1] + b[:, 2:3] * n[:, 2]
    l = _len(s)
    bad = ~(l >= 1e-20)
    if bad.any():
        fn = np.cross(v[bad, 1] - v[bad, 0], v[bad, 2] - v[bad, 0]).astype(s.dtype)
        fl = _len(fn)
        flat = ~(fl >= 1e-20)
        fn[flat] = (0, 0, 1)
        fl[flat] = 1
        s[bad], l[bad] = fn, fl
    return s / l[:, None]


def tangents(v, upper, n):
    """v [N, 3, 3], upper [N] bool, unit n [N, 3] -> t [N, 3] of the contract's step 5."""
    e = np.where(upper[:, None], v[:, 0] - v[:, 1], v[:, 1] - v[:, 0])
    d = n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1] + n[:, 2] * e[:, 2]
    t = e - n * d[:, None]
    l = _len(t)
    bad = ~(l >= 1e-20)
    if bad.any():
        nb = n[bad]
        ax = np.argmin(np.abs(nb), axis=1)                            # the first of equals
        ea = np.zeros_like(nb)
        ea[np.arange(len(nb)), ax] = 1
        tb = ea - nb * nb[np.arange(len(nb)), ax][:, None]
        t[bad], l[bad] = tb, _len(tb)
    return t / l[:, None]


def _mesh(verts, normals, faces, dtype):
    return np.asarray(verts, np.float32).astype(dtype), np.asarray(normals, np.float32).astype(dtype), np.asarray(faces, np.int64)


def texels(verts, normals, faces, cols, T, dtype=np.float64):
    """-> (point [N, 3], outward [N, 3], face [N] int32, b [N, 3]) for the cell-major texels of the used cells."""
    verts, normals, faces = _mesh(verts, normals, faces, dtype)
    F = len(faces)
    c, j, i, face, upper = texel_index(F, cols, T)
    bl, bu = cell_barycentrics(T, dtype)
    b = np.where(upper[:, None], bu[j, i], bl[j, i])
    v, n = verts[faces[face]], normals[faces[face]]
    point = b[:, 0:1] * v[:, 0] + b[:, 1:2] * v[:, 1] + b[:, 2:3] * v[:, 2]
    return point, unit_normals(b, v, n), face.astype(np.int32), b


def corners(verts, normals, faces, size, cols, T, dtype=np.float64):
    """-> (pos [3F, 3] f32, nrm [3F, 3] f32, tan [3F, 4], uv [3F, 2] f32) of the unwelded mesh."""
    v32, n32 = np.asarray(verts, np.float32), np.asarray(normals, np.float32)
    verts, normals, faces = _mesh(verts, normals, faces, dtype)
    F = len(faces)
    f = np.repeat(np.arange(F, dtype=np.int64), 3)
    k = np.tile(np.arange(3), F)
    c, upper = f // 2, (f % 2).astype(bool)
    lo, up = corner_uv_local(T)
    local = np.where(upper[:, None], up[k], lo[k])
    texel = np.stack([(c % cols) * T, (c // cols) * T], 1) + local
    uv = texel.astype(np.float32) / np.float32(size)
    v, n = verts[faces[f]], normals[faces[f]]
    b = np.eye(3, dtype=dtype)[k]
    t = tangents(v, upper, unit_normals(b, v, n))
    tan = np.concatenate([t, np.ones((3 * F, 1), dtype)], 1)
    return v32[faces.reshape(-1)], n32[faces.reshape(-1)], tan, uv


def linear2srgb(x):
    x = np.clip(x, 0, 1)
    return np.where(x <= 0.0031308, x * 12.92, 1.055 * np.power(x + 1e-6, 1 / 2.4) - 0.055)


UNOWNED = {"base": (0, 0, 0, 255), "orm": (0, 0, 0, 255), "normal": (128, 128, 255, 255)}


def pack(verts, normals, faces, size, cols, T, albedo, roughness, normal, coverage, irradiance=None, ao=None):
    """The three images BEFORE rounding -> ({"base" | "orm" | "normal": [size, size, 4] float64 = 255 x the channel value},
    owned [size, size] bool).  The per-texel inputs are cell-major float32 arrays; all arithmetic is float64."""
    verts, normals, faces = _mesh(verts, normals, faces, np.float64)
    F = len(faces)
    c, j, i, face, upper = texel_index(F, cols, T)
    _, outward, _, _ = texels(verts, normals, faces, cols, T)
    t = tangents(verts[faces[face]], upper, outward)
    bt = np.cross(outward, t)
    f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    col = f64(albedo)
    if irradiance is not None:
        col = np.clip(col / np.pi * f64(irradiance), 0, 1)
    N = f64(normal)
    enc = 0.5 + 0.5 * np.stack([(N * t).sum(1), (N * bt).sum(1), (N * outward).sum(1)], 1)
    enc[~(f64(coverage) > 0.5)] = (128 / 255, 128 / 255, 1.0)
    one = np.ones(len(c))
    vals = {"base": np.concatenate([linear2srgb(col), one[:, None]], 1),
            "orm": np.stack([np.clip(f64(ao), 0, 1) if ao is not None else one, np.clip(f64(roughness), 0, 1), 0 * one, one], 1),
            "normal": np.concatenate([np.clip(enc, 0, 1), one[:, None]], 1)}
    x, y = (c % cols) * T + i, (c // cols) * T + j
    owned = np.zeros((size, size), bool)
    owned[y, x] = True
    out = {}
    for name, v in vals.items():
        img = np.empty((size, size, 4), np.float64)
        img[:] = UNOWNED[name]
        img[y, x] = 255.0 * v
        out[name] = img
    return out, owned


def rounding_margin(img):
    """Distance of every channel value (in units of 1 / 255) from the nearest rounding boundary k + 0.5."""
    return np.abs(img - np.floor(img) - 0.5)


def bilinear_taps(x, y):
    """Continuous texel coordinates -> the four integer taps [..., 4, 2] (i, j) a LINEAR sampler reads (before edge clamping)."""
    i0, j0 = np.floor(x - 0.5).astype(np.int64), np.floor(y - 0.5).astype(np.int64)
    return np.stack([np.stack([i0 + a, j0 + b], -1) for b in (0, 1) for a in (0, 1)], -2)


# ---- test meshes --------------------------------------------------------------------------------------------------------------
def random_mesh(F, seed):
    """F triangles over F + 2 random vertices in [-1, 1]^3 with unit normals around +z (no sum of them comes near zero)."""
    rng = np.random.default_rng(seed)
    V = F + 2
    verts = rng.uniform(-1, 1, (V, 3)).astype(np.float32)
    n = rng.normal(size=(V, 3)) + (0, 0, 2.5)
    normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    faces = np.stack([np.arange(F), np.arange(F) + 1, np.arange(F) + 2], 1).astype(np.int32)
    return verts, normals, faces


def degenerate_mesh():
    """Four faces: v0 = v1 (no +u direction: the axis fallback of the tangent), a point (zero area) with zero normals (the
    (0, 0, 1) fallback), a proper face with zero normals (the face-normal fallback), and an ordinary one."""
    verts = np.float32([[0.25, -0.5, 0.125], [0.75, 0.5, -0.25], [-0.5, 0.25, 0.5], [0.5, 0.5, 0.5], [-0.25, -0.75, 0.0]])
    normals = np.float32([[0, 0.6, 0.8], [0.6, 0, 0.8], [0, 0, 1], [0, 0, 0], [0, 0, 0]])
    normals = np.concatenate([normals, np.float32([[0, 0, 0]])])
    verts = np.concatenate([verts, np.float32([[0.5, -0.25, 0.75]])])
    faces = np.int32([[0, 0, 1], [3, 3, 3], [3, 4, 5], [0, 1, 2]])
    return verts, normals, faces


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    """Marching cubes (tests/mesh_reference.py) of a 27^3 volume of 10.3 - |p - centre|: a few thousand faces, several blocks."""
    from tests import mesh_reference as MR
    ax = np.arange(27, dtype=np.float64)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (10.3 - np.sqrt((X - 13.3) ** 2 + (Y - 12.8) ** 2 + (Z - 13.1) ** 2)).astype(np.float32)
    v, f, n = MR.marching_cubes(vol, 0.0, (1, 1, 1), (0, 0, 0))
    return np.asarray(v, np.float32), np.asarray(n, np.float32), np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def layout_cases():
    """name -> (verts, normals, faces, sizes): the meshes and image sizes of the layout comparison."""
    small = (12, 27, 31)                              # T = 6 (the minimum) with two columns, T odd, not divisible by cols
    cases = {"F1": random_mesh(1, 1) + (small,), "F2": random_mesh(2, 2) + (small,), "F7": random_mesh(7, 7) + (small,),
             "degenerate": degenerate_mesh() + (small,)}
    v, n, f = sphere_mesh()
    cols = layout(len(f), 8192)[0]
    cases["sphere"] = (v, n, f, (6 * cols, 7 * cols + 5))
    return cases


# ---- the pack kernel's inputs --------------------------------------------------------------------------------------------------
PACK_MARGIN = 1e-2                    # in units of 1 / 255: how far every channel's float64 value stays from k + 0.5
PACK_SIZE = 27
PACK_VARIANTS = {"albedo": dict(diffuse=False, ao=True), "diffuse": dict(diffuse=True, ao=True),
                 "no-lighting": dict(diffuse=False, ao=False)}


def pack_variant(case, name):
    """-> pack() of the case for one variant of PACK_VARIANTS."""
    v = PACK_VARIANTS[name]
    return pack(case["verts"], case["normals"], case["faces"], PACK_SIZE, case["cols"], case["T"], case["albedo"], case["roughness"],
                case["normal"], case["coverage"], irradiance=case["irradiance"] if v["diffuse"] else None,
                ao=case["ao"] if v["ao"] else None)


@functools.lru_cache(maxsize=None)
def pack_case():
    """Five faces at size 27 (T = 13; cell 2 belongs to the odd last face, cell 3 and the 27th row and column to nobody) with
    seeded per-texel bake results.  A texel any of whose channels, in any variant, comes within PACK_MARGIN of a rounding boundary
    gets new random inputs until none does, so that the bytes are decided by the definition and not by float32 rounding."""
    verts, normals, faces = random_mesh(5, 5)
    cols, T = layout(len(faces), PACK_SIZE)
    N = ((len(faces) + 1) // 2) * T * T
    rng = np.random.default_rng(27)

    def draw(n):
        nv = rng.normal(size=(n, 3))
        cov = np.where(rng.random(n) < 0.25, 0.45 * rng.random(n), 0.55 + 0.45 * rng.random(n))
        return {"albedo": rng.random((n, 3)), "irradiance": 4.0 * rng.random((n, 3)) ** 2, "roughness": rng.random(n),
                "ao": rng.random(n), "normal": nv / np.linalg.norm(nv, axis=1, keepdims=True), "coverage": cov}

    case = {"verts": verts, "normals": normals, "faces": faces, "cols": cols, "T": T}
    case.update({k: v.astype(np.float32) for k, v in draw(N).items()})
    c, j, i, _, _ = texel_index(len(faces), cols, T)
    x, y = (c % cols) * T + i, (c // cols) * T + j
    for _ in range(64):
        close = np.zeros(N, bool)
        for name in PACK_VARIANTS:
            imgs, _ = pack_variant(case, name)
            for img in imgs.values():
                close |= (rounding_margin(img[y, x]) < PACK_MARGIN).any(1)
        if not close.any():
            return case
        for k, v in draw(int(close.sum())).items():
            case[k][close] = v.astype(np.float32)
    raise AssertionError("pack_case: the inputs did not qualify")
