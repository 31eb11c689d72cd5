"""numpy restatement of the asset-lighting kernels (tir_env_cells, tir_light_gbuffer; contract: include/tensoir_hip.h, DESIGN
4.9), twice: in float32 in the kernels' stated order, and in float64.  The float32 version's distance from the float64 one is the
yardstick of the GPU tests (tests/test_gpu_light.py: the device must come within ten times it); tests/test_light_cpu.py prints it
per fixture and pins the float64 version's BRDF and tone map to the oracle.  Also the fixtures both test files use."""
import math

import numpy as np

OCCLUSION, SRGB = 1, 2
ROW = 12
THRESHOLD = 1e-6            # a pair contributes iff n.L > THRESHOLD


# ---- tir_env_cells -----------------------------------------------------------------------------------------------------------------
def row_weights(H, W):
    """float64 [H]: the solid angle of one texel of row i."""
    i = np.arange(H, dtype=np.float64)
    return (2.0 * math.pi / W) * 2.0 * np.sin(math.pi * (i + 0.5) / H) * math.sin(math.pi / (2.0 * H))


def cell_dirs(h, w, dtype=np.float64):
    """[h, w, 3]: Environment_Light's cell-centre directions on an h x w grid; the angles formed in float64 and rounded once."""
    phi = (0.5 * math.pi - (np.arange(h, dtype=np.float64) + 0.5) * (math.pi / h)).astype(dtype)[:, None]
    theta = (math.pi - (np.arange(w, dtype=np.float64) + 0.5) * (2.0 * math.pi / w)).astype(dtype)[None, :]
    cp = np.cos(phi)
    return np.stack([np.cos(theta) * cp, np.sin(theta) * cp, np.sin(phi) + 0 * theta], -1).astype(dtype)


def env_cells(hdr, h, w, dtype=np.float64):
    """hdr [H, W, 3] float32 -> cells [h * w, 8] in dtype.  The row weights are the float32 ones the wrapper hands the kernel; the
    sums run in row-major order over a cell's texels (the kernel fuses each multiply-add of the numerator, numpy does not)."""
    hdr = np.asarray(hdr, np.float32)
    H, W = hdr.shape[:2]
    if H % h or W % w:
        raise ValueError("the map's sides must be multiples of the cell grid's")
    a, b = H // h, W // w
    rw = row_weights(H, W).astype(np.float32).astype(dtype)
    px = hdr.astype(dtype).reshape(h, a, w, b, 3)
    rgb = np.zeros((h, w, 3), dtype)
    wsum = np.zeros((h, w), dtype)
    rows = np.zeros((h,), dtype)
    for i in range(a):
        wi = rw.reshape(h, a)[:, i]
        rows = (rows + wi).astype(dtype)
        for j in range(b):
            rgb = (rgb + (wi[:, None, None] * px[:, i, :, j, :]).astype(dtype)).astype(dtype)
            wsum = (wsum + wi[:, None]).astype(dtype)
    out = np.zeros((h, w, 8), dtype)
    out[..., 0:3] = cell_dirs(h, w, dtype)
    out[..., 3] = (dtype(b) * rows)[:, None]
    out[..., 4:7] = rgb / wsum[..., None]
    return out.reshape(h * w, 8)


# ---- tir_light_gbuffer -------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(x, eps, dtype):
    n = np.maximum(np.sqrt(_dot(x, x)), dtype(eps))
    return (x / n[..., None]).astype(dtype)


def surface(normal, view, rough, dtype=np.float64):
    """make_surface for scalar roughness: -> dict(N flipped unit normal [M, 3], V [M, 3], NoV, alpha2, k [M])."""
    n, v, r = (np.asarray(x, np.float32).astype(dtype) for x in (normal, view, rough))
    V = _normalize(v, 1e-12, dtype)
    N = _normalize(n, 1e-12, dtype)
    N = N * np.sign(_dot(V, N))[..., None]
    NoV = np.clip(_dot(N, V), dtype(1e-6), dtype(1))
    a = r * r
    return {"N": N, "V": V, "NoV": NoV, "alpha2": a * a, "k": (a + dtype(2) * r + dtype(1)) / dtype(8)}


def specular(S, L, fresnel, dtype=np.float64, stats=None):
    """GGX_specular with L [D, 3] used as given -> [M, D].  stats (a dict) receives "nom_low_mask" [M, D]: the pairs that drive
    the denominator into its lower clamp."""
    one, lo = dtype(1), dtype(1e-6)
    L = np.asarray(L).astype(dtype)[None, :, :]
    N, V = S["N"][:, None, :], S["V"][:, None, :]
    Hv = (L + V) * dtype(0.5)
    Hv = Hv * (one / np.sqrt(np.maximum(_dot(Hv, Hv), dtype(1e-24))))[..., None]
    NoL, NoH, VoH = (np.clip(_dot(x, y), lo, one) for x, y in ((N, L), (N, Hv), (V, Hv)))
    F = dtype(fresnel)
    a2, k = S["alpha2"][:, None], S["k"][:, None]
    p2 = np.exp2((dtype(-5.55473) * VoH - dtype(6.98316)) * VoH)
    frac = (F + (one - F) * p2) * a2
    nom0 = NoH * NoH * (a2 - one) + one
    nom1 = S["NoV"][:, None] * (one - k) + k
    nom2 = NoL * (one - k) + k
    four_pi = dtype(np.float32(4.0) * np.float32(math.pi)) if dtype == np.float32 else dtype(4.0 * math.pi)
    raw = four_pi * nom0 * nom0 * nom1 * nom2
    if stats is not None:
        stats["nom_low_mask"] = raw < lo
    return (frac / np.clip(raw, lo, four_pi)).astype(dtype)


def linear2srgb(x, dtype=np.float64):
    x = np.clip(x, dtype(0), dtype(1))
    return np.where(x <= dtype(0.0031308), x * dtype(12.92), dtype(1.055) * np.power(x + dtype(1e-6), dtype(1 / 2.4)) - dtype(0.055)).astype(dtype)


def light_gbuffer(gbuf, view, cells, fresnel, flags, dtype=np.float64, specular_on=True, stats=None):
    """gbuf [M, 12], view [M, 3], cells [D, 8] (float32 inputs) -> out [M, 4] in dtype; the cells are added in ascending order.
    stats receives "pairs" (above the horizon, covered rows), "near_threshold" (pairs within 1e-6 of it, in dtype) and "nom_low"."""
    gbuf, view, cells = (np.asarray(x, np.float32) for x in (gbuf, view, cells))
    g, cl = gbuf.astype(dtype), cells.astype(dtype)
    M = g.shape[0]
    cov = g[:, 8]
    S = surface(gbuf[:, 5:8], view, gbuf[:, 3], dtype)
    pi = dtype(np.float32(math.pi)) if dtype == np.float32 else dtype(math.pi)
    alb_pi = g[:, 0:3] / pi
    c = _dot(g[:, None, 5:8], cl[None, :, 0:3])                       # the stored, unflipped normal
    on = (c > dtype(THRESHOLD)) & (cov > 0)[:, None]
    spec = specular(S, cl[:, 0:3], fresnel, dtype, stats) if specular_on else np.zeros_like(c)
    if stats is not None:
        stats["pairs"] = int(on.sum())
        stats["near_threshold"] = int((np.abs(c - dtype(THRESHOLD)) < dtype(1e-6))[cov > 0].sum())
        stats["nom_low"] = int((stats.pop("nom_low_mask") & on).sum()) if specular_on else 0
    acc = np.zeros((M, 3), dtype)
    for d in range(cl.shape[0]):
        term = ((((alb_pi + spec[:, d:d + 1]) * cl[d, 4:7][None, :]) * c[:, d:d + 1]) * cl[d, 3]).astype(dtype)
        acc = np.where(on[:, d:d + 1], acc + term, acc).astype(dtype)
    if flags & OCCLUSION:
        acc = acc * g[:, 4:5]
    if flags & SRGB:
        acc = linear2srgb(acc, dtype)
    out = np.concatenate([acc, cov[:, None]], 1).astype(dtype)
    out[~(cov > 0)] = 0
    return out


def distance(a, ref):
    """max |a - ref| / max |ref| (0 when ref is all zeros and a equals it)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    d = np.abs(a - ref).max()
    return 0.0 if d == 0 else d / top


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def hdr_map(H, W, seed, hot=None):
    """float32 [H, W, 3]: exp(N(0, 1.5^2)) per channel with one texel (default: a seeded one) multiplied by 100."""
    rng = np.random.default_rng(seed)
    m = np.exp(rng.normal(0.0, 1.5, (H, W, 3)))
    i, j = (int(rng.integers(H)), int(rng.integers(W))) if hot is None else hot
    m[i, j] *= 100.0
    return m.astype(np.float32)


def light_cells(D, seed):
    """float32 [D, 8]: D cells, in a seeded order, of the 8 x 16 reduction of a seeded 16 x 32 map -- directions over the whole
    sphere, solid angles as tir_env_cells makes them, its radiances times 128 / D / 16 (so that the lit values spread over
    [0, 1] and beyond for every D: the tone map's clamp is reached, and not by everything)."""
    cells = env_cells(hdr_map(16, 32, seed), 8, 16).astype(np.float32)
    cells[:, 4:7] *= np.float32(8.0 / D)
    return np.ascontiguousarray(cells[np.random.default_rng(seed + 1).permutation(len(cells))[:D]])


def _rows(M, D, rough, seed):
    rng = np.random.default_rng(seed)
    cells = light_cells(D, seed)
    n = rng.normal(size=(M, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    v = rng.normal(size=(M, 3))
    v *= (rng.uniform(0.5, 4.0, (M, 1)) / np.linalg.norm(v, axis=1, keepdims=True))          # any length: the kernel normalises
    g = np.zeros((M, ROW))
    g[:, 0:3] = rng.uniform(0.0, 1.0, (M, 3))
    g[:, 3] = rough
    g[:, 4] = rng.uniform(0.2, 1.0, M)
    g[:, 8] = 1.0
    # designed rows, where the buffer is long enough for them
    if M > 2:
        g[1, 8] = 0.0                                                                       # an empty pixel between covered ones
    if M > 3:
        n[3], v[3] = (0.0, 0.0, 1.0), (2.0, 0.0, 0.0)                                       # N.V = 0: sign 0, NoV clamped
    if M > 4:
        n[4], v[4] = (0.0, 0.0, 1.0), (1.0, 0.0, 1e-7)                                      # N.V = 1e-7: below the NoV clamp
    if M > 5:
        n[5], v[5] = (0.0, 0.0, -1.0), (0.3, 0.2, 1.5)                                      # N.V < 0: the flip
    if M > 6:                                                                               # N = H for cell 0: nom's lower clamp at 0.02
        l0 = cells[0, 0:3].astype(np.float64)
        v[6] = l0 + (0.3, -0.2, 0.1)
        hv = l0 + v[6] / np.linalg.norm(v[6])
        n[6] = hv / np.linalg.norm(hv)
    g[:, 5:8] = n
    return g.astype(np.float32), v.astype(np.float32), cells


def surface_rows(M, D, rough=0.5, seed=0):
    """-> (gbuf [M, 12], view [M, 3], cells [D, 8]) float32, deterministic.  Unit normals and views in every relative orientation,
    random albedo and ao, the designed rows above.  A draw in which some pair has |n.L - 1e-6| < 1e-6 in float64, or a random row
    |N.V| < 1e-4 (float32 and float64 could then disagree on a pair or on the flip), is rejected and redrawn."""
    for attempt in range(100):
        g, v, cells = _rows(M, D, rough, 1000 * attempt + 7 * M + 13 * D + seed)
        c = _dot(g[:, None, 5:8].astype(np.float64), cells[None, :, 0:3].astype(np.float64))
        nv = np.abs(_dot(_normalize(g[:, 5:8].astype(np.float64), 1e-12, np.float64), _normalize(v.astype(np.float64), 1e-12, np.float64)))
        designed = np.zeros(M, bool)
        designed[3:5] = True
        if not (np.abs(c - THRESHOLD) < 1e-6).any() and not (nv[~designed] < 1e-4).any():
            return g, v, cells
    raise RuntimeError("no admissible fixture in 100 draws")


M_CASES = (1, 63, 64, 65, 257)
D_CASES = (1, 7, 31, 32, 33, 67)                 # the cell records arrive by scalar loads: no tile size to straddle
ROUGH_CASES = (0.02, 0.5, 1.0)
CELL_CASES = {"8x16->4x8": ((8, 16), (4, 8), None), "6x12->2x4": ((6, 12), (2, 4), None), "4x8->4x8": ((4, 8), (4, 8), None),
              "hot-corner": ((8, 16), (4, 8), (2, 4))}                 # the 100x texel on the corner of a 2 x 2 block


def cell_case(name):
    (H, W), (h, w), hot = CELL_CASES[name]
    return hdr_map(H, W, 11 + len(name), hot), h, w


def horizon_case():
    """N = V = (0, 0, 1) and four cells (1, 0, z), un-normalised, z in {0, 2^-20, 2^-19, -2^-19}: n.L = z exactly.  2^-20 < 1e-6 <
    2^-19, so only the third contributes.  Roughness 0 makes alpha2, hence the specular term, exactly 0: what is left is the
    product ((albedo / pi * rgb) * c) * Omega added to 0, which no fused multiply-add and no approximate instruction can change."""
    g = np.zeros((1, ROW), np.float32)
    g[0, 0:3], g[0, 4], g[0, 5:8], g[0, 8] = (0.7, 0.5, 0.3), 0.6, (0, 0, 1), 1.0
    v = np.float32([[0, 0, 1]])
    cells = np.zeros((4, 8), np.float32)
    for d, z in enumerate((0.0, 2.0 ** -20, 2.0 ** -19, -(2.0 ** -19))):
        cells[d] = (1, 0, z, 0.37 + d, 3.0 + d, 5.0 + d, 7.0 + d, 0)
    return g, v, cells
