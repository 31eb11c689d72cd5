"""numpy restatement of the shadow-map contract of include/tensoir_hip.h (tir_shadow_maps, tir_shadow_lookup,
tir_light_gbuffer_shadowed): the light frames, the per-cell orthographic z-buffers (integer coverage of
tests/raster_reference.py, exact), the visibility rule and the shadowed lighting sum.  Everything continuous is float64 unless
dtype=np.float32 asks for the device's chain of operations in float32; the distance between the two modes is the yardstick of the
GPU tests' bounds (tests/test_shadow_cpu.py prints it).  Also the fixtures both test files use."""
import functools

import numpy as np

from tests import light_reference as L
from tests import raster_reference as R

SMALL = 64                  # a pair whose box holds more texel centres goes to the per-face path (as the kernel's workgroup pass)
DEPTH_MARGIN = 1e-5         # lookup: a pair this close to the depth threshold may differ between float32 and float64
TEXEL_MARGIN = 1e-4         # lookup: so may one whose texel coordinate is this close to an integer
CONSTS, SLOPES = (0.5, 1.0, 1.5, 2.0, 3.0), (0.5, 1.0, 2.0)      # the candidates of the default bias


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def mesh_bounds(pos):
    """-> (centre [3], radius) float64: the middle of the positions' box and half its diagonal times 1 + 1/64."""
    p = np.asarray(pos, np.float32).reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    return 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo)) * (1.0 + 1.0 / 64.0)


def frame_axes(dirs):
    """dirs [D, 3] -> (L, u, v) float64 [D, 3]: L normalised, a = the axis with the smallest |L_a| (lowest index on ties),
    u = normalize(e_a x L), v = L x u."""
    Lh = np.asarray(dirs, np.float64).reshape(-1, 3)
    Lh = Lh / np.linalg.norm(Lh, axis=1, keepdims=True)
    u = np.empty_like(Lh)
    for d, l in enumerate(Lh):
        a = min(range(3), key=lambda k: (abs(l[k]), k))
        e = np.zeros(3)
        e[a] = 1.0
        u[d] = np.cross(e, l)
        u[d] /= np.linalg.norm(u[d])
    return Lh, u, np.cross(Lh, u)


def frames(dirs, centre, radius, S):
    """-> [D, 12] float64 {g u, S/2 - g u.c, g v, S/2 - g v.c, L / (4 r), 0.5 - L.c / (4 r)}, g = S / (2 r)."""
    Lh, u, v = frame_axes(dirs)
    c, r = np.asarray(centre, np.float64), float(radius)
    g = S / (2.0 * r)
    return np.concatenate([g * u, (S / 2.0 - g * (u @ c))[:, None], g * v, (S / 2.0 - g * (v @ c))[:, None], Lh / (4.0 * r),
                           (0.5 - (Lh @ c) / (4.0 * r))[:, None]], 1)


def project(fr, p, dtype=np.float64):
    """fr [12] (one frame: the float32 numbers the device gets), p [N, 3] float32 -> (x_px, y_px, w) in dtype, every product and
    sum on its own, in the contract's order."""
    f = np.asarray(fr, np.float32).astype(dtype)
    p = np.asarray(p, np.float32).reshape(-1, 3).astype(dtype)
    with np.errstate(all="ignore"):
        return tuple(((f[4 * k] * p[:, 0] + f[4 * k + 1] * p[:, 1]) + f[4 * k + 2] * p[:, 2]) + f[4 * k + 3] for k in range(3))


# ---- tir_shadow_maps ---------------------------------------------------------------------------------------------------------------
def _edges(x, y, n, px, py):
    """R.edges for arrays of faces: x, y lists of three int64 arrays, n the orientation, (px, py) one point per face."""
    ax, ay, bx, by, cx, cy = x[0] - px, y[0] - py, x[1] - px, y[1] - py, x[2] - px, y[2] - py
    e = [n * (bx * cy - cx * by), n * (cx * ay - ax * cy), n * (ax * by - bx * ay)]
    own = [R._owns(n, x[2] - x[1], y[2] - y[1]), R._owns(n, x[0] - x[2], y[0] - y[2]), R._owns(n, x[1] - x[0], y[1] - y[0])]
    inside = np.ones(np.shape(e[0]), bool)
    for k in range(3):
        inside &= e[k] >= np.where(own[k], 0, 1)
    return e, inside


def maps(pos, fr, S, faces=None, dtype=np.float64):
    """pos [3F, 3] (or verts [V, 3] with faces [F, 3]), fr [D, 12] float32 -> (depth [D, S, S] in dtype: the largest w of the
    fragments of every texel, 0 where there is none; counts {R.DROPS: dropped pairs})."""
    T = dtype
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    fr = np.asarray(fr, np.float32).reshape(-1, 12)
    V = len(pos)
    if faces is None:
        idx, bad = np.arange(V, dtype=np.int64), np.zeros(V // 3, bool)
    else:
        fc = np.asarray(faces, np.int64).reshape(-1, 3)
        bad = ((fc < 0) | (fc >= V)).any(1)
        idx = np.where(np.repeat(bad, 3), 0, fc.reshape(-1))
    F = len(idx) // 3
    depth = np.zeros((len(fr), S, S), T)
    counts = dict.fromkeys(R.DROPS, 0)
    for d in range(len(fr) if F else 0):
        x, y, w = (a.reshape(F, 3) for a in project(fr[d], pos[idx], T))
        with np.errstate(all="ignore"):
            finite = (np.isfinite(x) & np.isfinite(y) & np.isfinite(w)).all(1)
            rx, ry = np.rint(x * T(256)), np.rint(y * T(256))
            guard = ((np.abs(rx) <= R.GUARD) & (np.abs(ry) <= R.GUARD)).all(1)
        counts["index"] += int(bad.sum())
        counts["nonfinite"] += int((~bad & ~finite).sum())
        counts["guard"] += int((~bad & finite & ~guard).sum())
        keep = np.nonzero(~bad & finite & guard)[0]
        sx, sy, w = rx[keep].astype(np.int64), ry[keep].astype(np.int64), w[keep]
        A = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sx[:, 2] - sx[:, 0]) * (sy[:, 1] - sy[:, 0])
        i0, i1 = np.maximum((sx.min(1) + 127) >> 8, 0), np.minimum((sx.max(1) - 128) >> 8, S - 1)
        j0, j1 = np.maximum((sy.min(1) + 127) >> 8, 0), np.minimum((sy.max(1) - 128) >> 8, S - 1)
        live = (A != 0) & (i0 <= i1) & (j0 <= j1)
        n = np.where(A < 0, -1, 1)
        area = np.abs(A).astype(T)
        wd = i1 - i0 + 1
        npx = np.where(live, wd * (j1 - j0 + 1), 0)

        def fragments(sel, px_i, px_j):
            xs, ys = [sx[sel, k] for k in range(3)], [sy[sel, k] for k in range(3)]
            e, inside = _edges(xs, ys, n[sel], 256 * px_i + 128, 256 * px_j + 128)
            z = ((e[0].astype(T) * w[sel, 0] + e[1].astype(T) * w[sel, 1]) + e[2].astype(T) * w[sel, 2]) / area[sel]
            ok = inside & (z > 0)
            return z, ok

        small = np.nonzero(live & (npx <= SMALL))[0]
        for p in range(int(npx[small].max()) if len(small) else 0):
            s = small[npx[small] > p]
            r = p // wd[s]
            i, j = i0[s] + p - r * wd[s], j0[s] + r
            z, ok = fragments(s, i, j)
            np.maximum.at(depth[d], (j[ok], i[ok]), z[ok])
        for f in np.nonzero(live & (npx > SMALL))[0]:
            i = np.arange(i0[f], i1[f] + 1, dtype=np.int64)[None, :]
            j = np.arange(j0[f], j1[f] + 1, dtype=np.int64)[:, None]
            z, ok = fragments(f, i, j)
            win = depth[d, j0[f]:j1[f] + 1, i0[f]:i1[f] + 1]
            win[...] = np.where(ok, np.maximum(win, z), win)
    return depth, counts


# ---- the visibility rule -------------------------------------------------------------------------------------------------------------
def lookup(pts, nrm, cells, fr, depth, bias, dtype=np.float64, near=None):
    """pts, nrm [M, 3], cells [D, 8], fr [D, 12] (float32 inputs), depth [D, S, S] (any float type; 0 = empty) -> codes [M, D]
    uint8 (0: n.L <= 1e-6, 1: shadowed, 2: lit).  near (a dict) receives "depth" and "texel" [M, D] bool: the pairs within
    DEPTH_MARGIN of the threshold, and those with a texel coordinate within TEXEL_MARGIN of an integer."""
    T = dtype
    pts, nrm = (np.asarray(a, np.float32).reshape(-1, 3) for a in (pts, nrm))
    cells = np.asarray(cells, np.float32).reshape(-1, 8)
    fr = np.asarray(fr, np.float32).reshape(-1, 12)
    M, D, S = len(pts), len(cells), depth.shape[1]
    c = L._dot(nrm.astype(T)[:, None, :], cells[None, :, 0:3].astype(T))
    codes = np.zeros((M, D), np.uint8)
    near_d, near_t = np.zeros((M, D), bool), np.zeros((M, D), bool)
    texel_w = T(np.float32(0.5) / np.float32(S)) if T == np.float32 else T(0.5) / T(S)
    for d in range(D):
        x, y, w = project(fr[d], pts, T)
        with np.errstate(all="ignore"):
            fx, fy = np.floor(x), np.floor(y)
            inside = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
            i, j = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
            t = depth[d, j, i].astype(T)
            full = inside & (t != 0)
            cd = np.where(c[:, d] > 0, c[:, d], T(1))
            tn = np.minimum(np.sqrt(np.maximum(T(1) - cd * cd, T(0))) * (T(1) / cd), T(8))
            b = (T(bias[0]) + T(bias[1]) * tn) * texel_w
            lit = ~full | (w + b >= t)
            near_d[:, d] = full & (np.abs((w + b) - t) < DEPTH_MARGIN)
            near_t[:, d] = (np.abs(x - np.rint(x)) < TEXEL_MARGIN) | (np.abs(y - np.rint(y)) < TEXEL_MARGIN)
        codes[:, d] = np.where(c[:, d] > T(L.THRESHOLD), np.where(lit, 2, 1), 0)
    if near is not None:
        near["depth"], near["texel"] = near_d, near_t
    return codes


# ---- tir_light_gbuffer_shadowed ------------------------------------------------------------------------------------------------------
def light_gbuffer_shadowed(gbuf, view, cells, fresnel, flags, codes, dtype=np.float64):
    """L.light_gbuffer with the pairs' visibility codes [M, D]: a pair is added iff it contributes (n.L > 1e-6 in dtype, covered
    row) and its code is 2."""
    gbuf, view, cells = (np.asarray(x, np.float32) for x in (gbuf, view, cells))
    g, cl = gbuf.astype(dtype), cells.astype(dtype)
    cov = g[:, 8]
    S = L.surface(gbuf[:, 5:8], view, gbuf[:, 3], dtype)
    pi = dtype(np.float32(np.pi)) if dtype == np.float32 else dtype(np.pi)
    alb_pi = g[:, 0:3] / pi
    c = L._dot(g[:, None, 5:8], cl[None, :, 0:3])
    on = (c > dtype(L.THRESHOLD)) & (cov > 0)[:, None] & (np.asarray(codes) == 2)
    spec = L.specular(S, cl[:, 0:3], fresnel, dtype)
    acc = np.zeros((len(g), 3), dtype)
    for d in range(cl.shape[0]):
        term = ((((alb_pi + spec[:, d:d + 1]) * cl[d, 4:7][None, :]) * c[:, d:d + 1]) * cl[d, 3]).astype(dtype)
        acc = np.where(on[:, d:d + 1], acc + term, acc).astype(dtype)
    if flags & L.OCCLUSION:
        acc = acc * g[:, 4:5]
    if flags & L.SRGB:
        acc = L.linear2srgb(acc, dtype)
    out = np.concatenate([acc, cov[:, None]], 1).astype(dtype)
    out[~(cov > 0)] = 0
    return out


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
QUAD_HALF = 0.4
CONTACT_HEIGHT = 0.0718     # 0.05 r of the scene it makes (tests/test_shadow_cpu.py checks the ratio)
LIGHTS = {"overhead": (0.0, 0.0, 1.0), "slanted": (1.0, 0.0, 1.0)}


def _quad(half, z):
    a, b, c, d = (-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)
    return [a, b, c, a, c, d]                            # two triangles, facing +z


def ground_quad(h=0.25):
    """pos [12, 3] float32: the ground [-1, 1]^2 x {0} and the occluder [-0.4, 0.4]^2 x {h}, two triangles each."""
    return np.float32(_quad(1.0, 0.0) + _quad(QUAD_HALF, h))


SCENE_BOUNDS = ((0.0, 0.0, 0.125), 2.0)      # a power-of-two radius: at S = 64 the frame of e_z has g = 16, x_px = 32 - 16 y, y_px = 32 + 16 x


def fan():
    """The seven-face fan of R.exact_cases() laid into the plane z = 0.5 with its pixel grid at 1 / 16: in the frame of L = e_z
    round SCENE_BOUNDS at S = 64 its corners, and with them edges, fall on texel centres, exactly in float32."""
    pos, W, H = R.exact_cases()["fan"]
    p = np.zeros_like(pos)
    p[:, 0], p[:, 1], p[:, 2] = 0.5 * pos[:, 0] / pos[:, 2], 0.5 * pos[:, 1] / pos[:, 2], 0.5
    return p.astype(np.float32)


def scene():
    """ground and quad (h = 0.25) plus the fan: 11 faces."""
    return np.concatenate([ground_quad(), fan()])


def whole_map_triangle():
    """One triangle far larger than any map of its bounding sphere's frames, one small one in front of it."""
    return np.float32([(-40, -30, 0), (50, -30, 0), (0, 60, 0), (-0.5, -0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.5, 0.5)])


def cell_dirs(D):
    """D directions: e_z, -e_z, an axis-aligned grazing one, then seeded ones over the sphere."""
    fixed = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)]
    rng = np.random.default_rng(50 + D)
    rest = rng.normal(size=(max(D - 3, 0), 3))
    return np.float32((fixed + [tuple(r / np.linalg.norm(r)) for r in rest])[:D] if D >= 3 else fixed[:D])


def cells_of(dirs, rgb=(1.0, 1.0, 1.0), omega=1.0):
    """Light cells [D, 8] float32 with the directions dirs (normalised in float64, rounded once)."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out = np.zeros((len(d), 8), np.float32)
    out[:, 0:3], out[:, 3], out[:, 4:7] = d, omega, rgb
    return out


def scene_frames(pos, dirs, S, bounds=None):
    """-> float32 [D, 12]: the frames of dirs round pos' bounding sphere, as ops.shadow_frames hands them to the kernels."""
    c, r = mesh_bounds(pos) if bounds is None else bounds
    return frames(cells_of(dirs)[:, 0:3], c, r, S).astype(np.float32)


GRID_N = 41
GRID_OFFSET = (0.0137, -0.0071)      # keeps the restatement's excluded share of the lookup grid under 1 % (checked on the CPU)


def ground_grid(n=GRID_N, offset=GRID_OFFSET, extent=0.9):
    """n x n ground points with up normals on [-extent, extent]^2 + offset -> (pts, nrm) float32 [n n, 3]."""
    a = np.linspace(-extent, extent, n)
    X, Y = np.meshgrid(a + offset[0], a + offset[1], indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), np.zeros(n * n)], 1).astype(np.float32)
    return pts, np.tile(np.float32([[0, 0, 1]]), (n * n, 1))


def shadow_inset(pts, light, h, texels, S, radius):
    """For ground points pts and the direction `light` (towards the light): by how many map texels (an S-map of a sphere of this
    radius) more than `texels` each point lies inside the analytic shadow of the occluder at height h, the quad's footprint
    moved by -h L_xy / L_z (negative: less than that, or outside)."""
    l = np.asarray(light, np.float64)
    l = l / np.linalg.norm(l)
    q = np.asarray(pts, np.float64)[:, 0:2] + h * l[0:2] / l[2]            # where the ray towards the light crosses z = h
    per_axis = (QUAD_HALF - np.abs(q)) * np.sqrt(1.0 - l[0:2] ** 2)        # a ground step along e_a is sqrt(1 - L_a^2) of it in the map
    return per_axis.min(1) / (2.0 * radius / S) - texels


def bias_criteria(const, slope):
    """The two criteria of DESIGN 4.10 for one bias pair -> (self-shadowed pairs with c >= 0.25 on the sphere, contact pairs that
    came out lit, the pairs tested of each).  float32 mode: what the device does."""
    return _sphere_self_shadow(const, slope) + _contact(const, slope)


@functools.lru_cache(maxsize=None)
def _sphere_setup():
    pos, nrm, _, _, _, _ = R.sphere_case("sphere-64")
    cells = L.env_cells(np.ones((4, 8, 3), np.float32), 4, 8).astype(np.float32)
    fr = frames(cells[:, 0:3], *mesh_bounds(pos), 128).astype(np.float32)
    depth, _ = maps(pos, fr, 128, dtype=np.float32)
    P, N = pos.reshape(-1, 3, 3).astype(np.float64), nrm.reshape(-1, 3, 3).astype(np.float64)
    wts = np.float64([(1, 0, 0), (0, 1, 0), (0, 0, 1), (.5, .5, 0), (0, .5, .5), (.5, 0, .5), (1 / 3, 1 / 3, 1 / 3)])
    pts = np.einsum("qk,fkc->fqc", wts, P).reshape(-1, 3)
    n = np.einsum("qk,fkc->fqc", wts, N).reshape(-1, 3)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return pts.astype(np.float32), n.astype(np.float32), cells, fr, depth


def _sphere_self_shadow(const, slope):
    pts, n, cells, fr, depth = _sphere_setup()
    codes = lookup(pts, n, cells, fr, depth, (const, slope), np.float32)
    c = L._dot(n.astype(np.float64)[:, None, :], cells[None, :, 0:3].astype(np.float64))
    facing = c >= 0.25
    return int(((codes == 1) & facing).sum()), int(facing.sum())


@functools.lru_cache(maxsize=None)
def _contact_setup():
    pos = ground_quad(CONTACT_HEIGHT)
    c, r = mesh_bounds(pos)
    dirs = [LIGHTS["overhead"], LIGHTS["slanted"]]
    fr = scene_frames(pos, dirs, 256)
    depth, _ = maps(pos, fr, 256, dtype=np.float32)
    pts, nrm = ground_grid(81, (0.0031, 0.0017), 0.6)
    return pos, r, dirs, fr, depth, pts, nrm


def _contact(const, slope):
    pos, r, dirs, fr, depth, pts, nrm = _contact_setup()
    codes = lookup(pts, nrm, cells_of(dirs), fr, depth, (const, slope), np.float32)
    lit = tested = 0
    for d, l in enumerate(dirs):
        deep = shadow_inset(pts, l, CONTACT_HEIGHT, 2.0, 256, r) > 0
        lit += int((codes[deep, d] != 1).sum())
        tested += int(deep.sum())
    return lit, tested
