"""Numpy restatement of the rasteriser contract of include/tensoir_hip.h (tir_raster_*): projection and snapping, the integer
coverage with its top-left rule, the depth key, perspective-correct barycentrics and the glTF-style shading.  Coverage is int64
arithmetic, exact.  Everything continuous is float64, unless dtype=np.float32 asks for the device's chain of operations in
float32 (the yardstick of the GPU tests' bounds: tests/test_raster_cpu.py measures the distance between the two modes)."""
import functools

import numpy as np

GUARD = 16384 * 256
DROP_NEAR, DROP_GUARD, DROP_NONFINITE, DROP_INDEX = 1, 2, 4, 8
DROPS = ("index", "near", "guard", "nonfinite")

# The bounds of the GPU comparison of resolve and shade with the float64 restatement (tests/test_gpu_raster.py): ten times the
# distance of this restatement's float32 mode from its float64 self over the two sphere views with shade_inputs() at SHADE_SIZES, which
# tests/test_raster_cpu.py measures and prints (test_float32_mode_distances_set_the_gpu_bounds keeps these constants at ten
# times what it measures).  invz and zc are relative, the others absolute (barycentrics, colours in [0, 1], unit normals).
# Measured: invz 1.673e-7, barycentrics 9.642e-8, zc 1.813e-7, albedo 2.430e-6, roughness / ao 2.171e-6, normal 1.021e-5.
INVZ_TOL, BARY_TOL, ZC_TOL = 1.7e-6, 1.0e-6, 1.9e-6
ALBEDO_TOL, ORM_TOL, NORMAL_TOL = 2.5e-5, 2.2e-5, 1.1e-4


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """c2w [3, 4] float64: z = normalize(target - eye), x = normalize(z x up), y = z x x; the eye in the last column."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z, eye], 1)


def project(pos, c2w, focal, W, H, near, faces=None, dtype=np.float64):
    """pos [3F, 3] (or verts [V, 3] with faces [F, 3]) -> dict: sx, sy int64 [3F]; x256, y256 [3F] (256 x the pixel coordinate
    before rounding, dtype); invz [3F] dtype; flags [3F] (the face's OR on each of its corners); counts {DROPS: faces}.  The camera
    and the positions are the float32 numbers the device gets; dtype is the arithmetic."""
    T = dtype
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    c = np.asarray(c2w, np.float32).reshape(3, 4).astype(T)
    f = T(np.float32(focal))
    V = len(pos)
    if faces is None:
        idx = np.arange(V, dtype=np.int64)
        bad_face = np.zeros(V // 3, bool)
    else:
        fc = np.asarray(faces, np.int64).reshape(-1, 3)
        bad_face = ((fc < 0) | (fc >= V)).any(1)
        idx = np.where(np.repeat(bad_face, 3), 0, fc.reshape(-1))
    n = len(idx)
    with np.errstate(all="ignore"):
        d = pos[idx].astype(T) - c[:, 3]
        cam = [(c[0, a] * d[:, 0] + c[1, a] * d[:, 1]) + c[2, a] * d[:, 2] for a in range(3)]
        X, Y, Z = cam
        flags = np.zeros(n, np.int64)
        nonfinite = ~(np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z))
        flags[nonfinite] = DROP_NONFINITE
        flags[~nonfinite & (Z <= T(np.float32(near)))] = DROP_NEAR
        x256 = ((f * X) / Z + T(0.5) * T(W)) * T(256)
        y256 = ((f * Y) / Z + T(0.5) * T(H)) * T(256)
        rx, ry = np.rint(x256), np.rint(y256)
        guard = (flags == 0) & (~(np.abs(rx) <= GUARD) | ~(np.abs(ry) <= GUARD))
        flags[guard] = DROP_GUARD
        invz = T(1) / Z
    flags[np.repeat(bad_face, 3)] = DROP_INDEX
    face_flags = np.bitwise_or.reduce(flags.reshape(-1, 3), axis=1)
    counts = {"index": int((face_flags & DROP_INDEX > 0).sum()),
              "nonfinite": int(((face_flags & DROP_INDEX == 0) & (face_flags & DROP_NONFINITE > 0)).sum()),
              "near": int(((face_flags & (DROP_INDEX | DROP_NONFINITE) == 0) & (face_flags & DROP_NEAR > 0)).sum()),
              "guard": int((face_flags == DROP_GUARD).sum())}
    flags = np.repeat(face_flags, 3)
    keep = flags == 0
    z = lambda a, t: np.where(keep, a, 0).astype(t)
    return {"sx": z(rx, np.int64), "sy": z(ry, np.int64), "x256": x256, "y256": y256, "invz": z(invz, T), "flags": flags,
            "counts": counts}


def _owns(n, dx, dy):
    """Does the edge with direction n (dx, dy) own its zero set: a left edge (d.y < 0) or a top edge (d.y == 0 and d.x > 0)."""
    dx, dy = n * dx, n * dy
    return (dy < 0) | ((dy == 0) & (dx > 0))


def face_setup(sx, sy, f):
    """-> (x [3], y [3], A) python ints of face f."""
    x = [int(v) for v in sx[3 * f:3 * f + 3]]
    y = [int(v) for v in sy[3 * f:3 * f + 3]]
    return x, y, (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])


def edges(x, y, n, px, py):
    """The oriented edge functions at the points (px, py) (int64 arrays) -> (E0, E1, E2, inside)."""
    ax, ay, bx, by, cx, cy = x[0] - px, y[0] - py, x[1] - px, y[1] - py, x[2] - px, y[2] - py
    e0, e1, e2 = n * (bx * cy - cx * by), n * (cx * ay - ax * cy), n * (ax * by - bx * ay)
    b0 = 0 if _owns(n, x[2] - x[1], y[2] - y[1]) else 1
    b1 = 0 if _owns(n, x[0] - x[2], y[0] - y[2]) else 1
    b2 = 0 if _owns(n, x[1] - x[0], y[1] - y[0]) else 1
    return e0, e1, e2, (e0 >= b0) & (e1 >= b1) & (e2 >= b2)


def cover(sx, sy, invz, flags, W, H, cull, dtype=np.float64):
    """-> dict: face [H, W] int64 (-1 = empty); invz [H, W] (the winner's, 0 where empty); second [H, W] (the largest invz of
    the other fragments, 0 where there is none); layers [H, W] (fragments per pixel); drawn (faces with a drawable sign)."""
    T = dtype
    sx, sy = np.asarray(sx, np.int64), np.asarray(sy, np.int64)
    w = np.asarray(invz).astype(T)
    best = np.zeros((H, W), T)
    second = np.zeros((H, W), T)
    face = np.full((H, W), -1, np.int64)
    layers = np.zeros((H, W), np.int64)
    drawn = 0
    for f in range(len(sx) // 3):
        if np.asarray(flags[3 * f:3 * f + 3]).any():
            continue
        x, y, A = face_setup(sx, sy, f)
        if A == 0 or (cull and A > 0):
            continue
        drawn += 1
        n = -1 if A < 0 else 1
        i0, i1 = max((min(x) + 127) >> 8, 0), min((max(x) - 128) >> 8, W - 1)
        j0, j1 = max((min(y) + 127) >> 8, 0), min((max(y) - 128) >> 8, H - 1)
        if i0 > i1 or j0 > j1:
            continue
        px = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128)[None, :]
        py = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)[:, None]
        e0, e1, e2, inside = edges(x, y, n, px, py)
        if not inside.any():
            continue
        s = (e0.astype(T) * w[3 * f] + e1.astype(T) * w[3 * f + 1]) + e2.astype(T) * w[3 * f + 2]
        z = s / T(abs(A))
        win = (slice(j0, j1 + 1), slice(i0, i1 + 1))
        b, sc, fc = best[win], second[win], face[win]
        better = inside & (z > b)                                       # faces come in ascending order: a tie keeps the earlier one
        other = inside & ~better
        second[win] = np.where(better, b, np.where(other, np.maximum(sc, z), sc))
        best[win] = np.where(better, z, b)
        face[win] = np.where(better, f, fc)
        layers[win] += inside
    return {"face": face, "invz": best, "second": second, "layers": layers, "drawn": drawn}


def resolve(face, sx, sy, invz, dtype=np.float64):
    """-> (b1, b2, zc, invz) [H, W] dtype of the winning faces (0 where face < 0)."""
    T = dtype
    H, W = face.shape
    sx, sy = np.asarray(sx, np.int64), np.asarray(sy, np.int64)
    w = np.asarray(invz).astype(T)
    jj, ii = np.nonzero(face >= 0)
    f = face[jj, ii]
    x = [sx[3 * f + k] for k in range(3)]
    y = [sy[3 * f + k] for k in range(3)]
    A = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
    n = np.where(A < 0, -1, 1)
    px, py = 256 * ii + 128, 256 * jj + 128
    ax, ay, bx, by, cx, cy = x[0] - px, y[0] - py, x[1] - px, y[1] - py, x[2] - px, y[2] - py
    e = [n * (bx * cy - cx * by), n * (cx * ay - ax * cy), n * (ax * by - bx * ay)]
    t = [e[k].astype(T) * w[3 * f + k] for k in range(3)]
    s = (t[0] + t[1]) + t[2]
    iz = s / np.abs(A).astype(T)
    out = [np.zeros((H, W), T) for _ in range(4)]
    for o, v in zip(out, (t[1] / s, t[2] / s, T(1) / iz, iz)):
        o[jj, ii] = v
    return tuple(out)


def srgb_to_linear(s):
    """The inverse of atlas_reference.linear2srgb, its + 1e-6 included."""
    T = s.dtype.type
    return np.where(s <= T(0.04045), s / T(12.92), np.maximum(np.power((s + T(0.055)) / T(1.055), T(2.4)) - T(1e-6), T(0)))


def _unit(v):
    l = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    return v / np.maximum(l, v.dtype.type(1e-20))[..., None]


def bilinear(img, u, v, lut):
    """LINEAR / CLAMP_TO_EDGE lookups of the [S, S, 4] uint8 image at glTF (u, v) [N], bytes decoded through lut [256] per channel
    column of `lut` ([256, C]) before filtering -> [N, C]."""
    T = u.dtype.type
    S = img.shape[0]
    x = np.clip(u * T(S) - T(0.5), T(-1), T(S))
    y = np.clip(v * T(S) - T(0.5), T(-1), T(S))
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
    ia, ib, ja, jb = (np.clip(a, 0, S - 1) for a in (i0, i0 + 1, j0, j0 + 1))
    C = lut.shape[1]
    tap = lambda j, i: np.stack([lut[img[j, i, c], c] for c in range(C)], 1)
    one = T(1)
    return (((one - fx) * (one - fy)) * tap(ja, ia) + (fx * (one - fy)) * tap(ja, ib)) + ((one - fx) * fy) * tap(jb, ia) + (fx * fy) * tap(jb, ib)


def shade(face, b1, b2, nrm, tan=None, uv=None, images=None, raw=False, dtype=np.float64):
    """-> [H, W, 9] dtype rows {albedo 3, roughness, ao, normal 3, coverage}; images = (base, orm, normal) or None."""
    T = dtype
    H, W = face.shape
    out = np.zeros((H, W, 9), T)
    jj, ii = np.nonzero(face >= 0)
    f = face[jj, ii]
    bb1, bb2 = b1[jj, ii].astype(T), b2[jj, ii].astype(T)
    b = [(T(1) - bb1) - bb2, bb1, bb2]
    mix = lambda a: sum(b[k][:, None] * np.asarray(a, np.float32).astype(T)[3 * f + k] for k in range(3))
    n = _unit(mix(nrm))
    N = n
    if images is not None:
        base, orm, normal = images
        s = (np.arange(256, dtype=T) / T(255))
        lin = np.stack([s, s, s], 1)
        col = lin if raw else np.stack([srgb_to_linear(s)] * 3, 1)
        u = mix(uv)
        out[jj, ii, 0:3] = bilinear(base, u[:, 0], u[:, 1], col)
        o = bilinear(orm, u[:, 0], u[:, 1], lin)
        out[jj, ii, 3], out[jj, ii, 4] = o[:, 1], o[:, 0]
        t = _unit(mix(np.asarray(tan)[:, :3]))
        sg = np.asarray(tan, np.float32).astype(T)[3 * f, 3][:, None]
        bt = np.cross(n, t) * sg
        c = T(2) * bilinear(normal, u[:, 0], u[:, 1], lin) - T(1)
        N = _unit(c[:, 0:1] * t + c[:, 1:2] * bt + c[:, 2:3] * n)
    out[jj, ii, 5:8] = N
    out[jj, ii, 8] = 1
    return out


# ---- cameras and scenes of the tests --------------------------------------------------------------------------------------------
IDENTITY = np.float32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])
FOCAL = 8.0                              # a power of two: with Z a power of two the projections below are exact in float32


def pixel_faces(tris, W, H, focal=FOCAL):
    """tris: [(p0, p1, p2, Z)] with p_k = (x, y) in pixels (dyadic numbers) -> pos [3F, 3] float32 in the identity camera."""
    pos = []
    for p0, p1, p2, Z in tris:
        for x, y in (p0, p1, p2):
            pos.append([(x - W / 2) * Z / focal, (y - H / 2) * Z / focal, Z])
    return np.float32(pos)


def _fan(cx, cy, rim, Z):
    return [((cx, cy), rim[k], rim[(k + 1) % len(rim)], Z) for k in range(len(rim))]


@functools.lru_cache(maxsize=None)
def exact_cases():
    """name -> (pos [3F, 3], W, H): faces in the identity camera (focal FOCAL, near 0.125) whose projected corners, edges and
    diagonals pass through pixel centres (coordinates n + 0.5)."""
    W = H = 16
    c = {}
    c["triangle"] = (pixel_faces([((0.5, 0.5), (0.5, 12.5), (12.5, 0.5), 1.0)], W, H), W, H)
    # a quad split along its diagonal; borders and diagonal on centres
    c["quad"] = (pixel_faces([((2.5, 1.5), (2.5, 11.5), (12.5, 11.5), 1.0), ((2.5, 1.5), (12.5, 11.5), (12.5, 1.5), 1.0)], W, H), W, H)
    rim = [(14.5, 8.5), (12.5, 13.5), (6.5, 14.5), (1.5, 10.5), (2.5, 3.5), (8.5, 0.5), (13.5, 2.5)]
    c["fan"] = (pixel_faces(_fan(8.5, 8.5, rim[::-1], 2.0), W, H), W, H)
    c["degenerate"] = (pixel_faces([((1.5, 1.5), (5.5, 5.5), (9.5, 9.5), 1.0), ((4.5, 4.5), (4.5, 4.5), (4.5, 4.5), 1.0),
                                    ((3.5, 2.5), (3.5, 9.5), (10.5, 2.5), 2.0)], W, H), W, H)
    c["outside"] = (pixel_faces([((-6.5, 3.5), (-6.5, 20.5), (9.5, 3.5), 1.0), ((20.5, 1.5), (20.5, 9.5), (30.5, 1.5), 1.0),
                                 ((1.5, -9.5), (1.5, -2.5), (9.5, -9.5), 1.0)], W, H), W, H)
    # a front face over its own back-facing copy (nearer), elsewhere a lone back face
    c["cull"] = (pixel_faces([((1.5, 1.5), (1.5, 10.5), (10.5, 1.5), 2.0), ((1.5, 1.5), (10.5, 1.5), (1.5, 10.5), 1.0),
                              ((9.5, 9.5), (14.5, 9.5), (9.5, 14.5), 1.0)], W, H), W, H)
    quad = lambda x0, y0, x1, y1, Z: [((x0, y0), (x0, y1), (x1, y1), Z), ((x0, y0), (x1, y1), (x1, y0), Z)]
    c["near-first"] = (pixel_faces(quad(1.5, 1.5, 11.5, 11.5, 1.0) + quad(4.5, 3.5, 14.5, 13.5, 2.0), W, H), W, H)
    c["far-first"] = (pixel_faces(quad(4.5, 3.5, 14.5, 13.5, 2.0) + quad(1.5, 1.5, 11.5, 11.5, 1.0), W, H), W, H)
    tri = ((2.5, 1.5), (2.5, 12.5), (13.5, 1.5), 1.0)
    c["coincident"] = (pixel_faces([tri, tri], W, H), W, H)
    for W, H in ((64, 64), (97, 61)):                  # larger than the image: the workgroup pass, widths no multiple of the block
        c[f"whole-{W}x{H}"] = (pixel_faces([((-10.5, -10.5), (-10.5, 3.0 * H + 0.5), (3.0 * W + 0.5, -10.5), 1.0),
                                            ((W + 0.5, H + 0.5), (W + 0.5, -2.0 * H), (-2.0 * W, H + 0.5), 2.0)], W, H), W, H)
    return c


NEAR = 0.125


def dropped_case():
    """Six faces in the identity camera at 16 x 16: kept, a corner behind near, beyond the guard band, a NaN corner, kept, a
    corner exactly at near -> (pos, W, H, the counts project must report)."""
    W = H = 16
    pos = pixel_faces([((1.5, 1.5), (1.5, 9.5), (9.5, 1.5), 1.0), ((2.5, 2.5), (2.5, 9.5), (9.5, 2.5), 1.0),
                       ((3.5, 3.5), (3.5, 9.5), (9.5, 3.5), 1.0), ((4.5, 4.5), (4.5, 9.5), (9.5, 4.5), 1.0),
                       ((5.5, 5.5), (5.5, 13.5), (13.5, 5.5), 2.0), ((6.5, 6.5), (6.5, 9.5), (9.5, 6.5), 1.0)], W, H)
    pos[3 + 1, 2] = -0.5                             # behind the camera
    pos[6 + 2, 0] = 20000.0                          # x_px = 160008 > 16384
    pos[9 + 0, 1] = np.nan
    pos[15 + 1, 2] = NEAR                            # Z <= near
    return pos, W, H, {"index": 0, "near": 2, "guard": 1, "nonfinite": 1}


SPHERE_CENTRE = (13.3, 12.8, 13.1)
# (W, H, eye - centre, front faces with culling, covered pixels): the last two were computed on the CPU in float64
SPHERE_VIEWS = {"sphere-64": (64, 64, (30.0, 12.0, 9.0), 1387, 1624), "sphere-97x61": (97, 61, (-11.0, 27.0, -16.0), 1368, 3596)}


@functools.lru_cache(maxsize=None)
def sphere_case(name):
    """-> (pos [3F, 3], nrm [3F, 3] float32 (unwelded), c2w float32 [3, 4], focal, W, H) of tests/atlas_reference.sphere_mesh()."""
    from tests import atlas_reference as A
    W, H, off, _, _ = SPHERE_VIEWS[name]
    v, n, f = A.sphere_mesh()
    c = np.asarray(SPHERE_CENTRE, np.float64)
    c2w = look_at(c + np.asarray(off, np.float64), c).astype(np.float32)
    return v[f.reshape(-1)], n[f.reshape(-1)], c2w, np.float32(1.1 * W), W, H


@functools.lru_cache(maxsize=None)
def shade_inputs(size, seed=0):
    """Per-corner tangents and uv for the sphere and three random RGBA images of side `size`.  uv is uniform in [0, 1] with every
    seventh corner snapped to exactly 0 or 1 (the clamp).  The tangents of a face derive from one random direction, made
    orthogonal to each corner's normal, the handedness random per face.  The normal image's blue channel is drawn from
    128 .. 255, like a real normal map (tz >= 0): the decoded vector then never comes near zero length, where normalising it
    would amplify any rounding without bound."""
    from tests import atlas_reference as A
    v, n, f = A.sphere_mesh()
    rng = np.random.default_rng(1000 + size + seed)
    F = len(f)
    nrm = n[f.reshape(-1)].astype(np.float64)
    d = np.repeat(rng.normal(size=(F, 3)), 3, axis=0)
    t = d - nrm * (nrm * d).sum(1, keepdims=True) / (nrm * nrm).sum(1, keepdims=True)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    sign = np.repeat(rng.choice([-1.0, 1.0], F), 3)
    tan = np.concatenate([t, sign[:, None]], 1).astype(np.float32)
    uv = rng.random((3 * F, 2))
    uv[::7] = np.round(uv[::7])
    images = [rng.integers(0, 256, (size, size, 4), dtype=np.uint8) for _ in range(3)]
    images[2][..., 2] = rng.integers(128, 256, (size, size), dtype=np.uint8)
    return tan, uv.astype(np.float32), tuple(images)


SHADE_SIZES = (6, 13, 27)
