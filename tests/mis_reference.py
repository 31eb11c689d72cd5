"""torch restatement of relighting with multiple importance sampling of the light map and the BRDF lobes (tir_shade.hip:
k_env_mis_setup, k_relight_mis), run in float32 or float64 on demand like tests/shade_reference.py: Philox-4x32-10
in integer numpy (the bits of tir::philox_uniform4), the light sampler (two-level inverse-CDF search, direction jittered inside
the cell), the BRDF mixture sampler (cosine lobe about the unit raw normal, GGX half-vector lobe about the flipped normal), both
densities per solid angle, the inverse cell mapping and the balance-heuristic estimator.  Also the fixtures of tests/test_mis_cpu.py
and tests/test_gpu_mis.py.

Exempt pairs: `cell`, `active` and the lobe choice are branches on rounded values; a pair is exempt from their exact comparison
when, in float64, its direction lies within BORDER_RAD of a cell border (angular distance, so the azimuth's is scaled by sin
theta; the poles count as borders: the azimuth is ill-conditioned there), |n.w - 1e-6| < COS_MARGIN or |v.h| < VOH_MARGIN.
tests/test_mis_cpu.py asserts that on every fixture at most 1 % of the pairs are exempt and that float32 and float64 agree on
every other pair."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tensoir_oracle as O

F32, F64 = torch.float32, torch.float64
COS_THRESHOLD = 1e-6
BORDER_RAD, COS_MARGIN, VOH_MARGIN = 1e-4, 1e-5, 1e-5
LIGHT, COSINE, LOBE = 0, 1, 2                    # which sampler drew a pair

MAPS = {"m8x16": (8, 16), "m5x12": (5, 12)}
POINTS = (1, 5, 67)
SPLITS = [(1, 0), (0, 1), (63, 0), (32, 32), (0, 64), (100, 30)]          # (n_l, n_b)
SEED, OFFSET, SELECT = 0x5EED0123456789, 3, 0.5


# ---- Philox ------------------------------------------------------------------------------------------------------------------------
def philox_uniform4(seed, offset, idx):
    """tir::philox_uniform4 for an array of counters -> [n, 4] float32, bit for bit: counter words (idx lo, idx hi, offset lo,
    offset hi), key (seed lo, seed hi), ten rounds, u = min((float(c) + 0.5f) * 2^-32, 0.99999994f) in float32 arithmetic."""
    idx = np.asarray(idx, dtype=np.uint64).reshape(-1)
    lo32 = np.uint64(0xFFFFFFFF)
    sh = np.uint64(32)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    c = [idx & lo32, idx >> sh, np.full_like(idx, offset & 0xFFFFFFFF), np.full_like(idx, offset >> 32)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]        # 32 x 32 bits: fits 64
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    u = np.stack([(w.astype(np.float32) + np.float32(0.5)) * np.float32(2.3283064365386963e-10) for w in c], axis=1)
    return np.minimum(u, np.float32(0.99999994)).astype(np.float32)


# ---- the map's tables --------------------------------------------------------------------------------------------------------------
def hdr_map(H, W):
    """A smooth positive pattern, distinct per channel, with one cell at 20 times the mean."""
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rgb = np.stack([0.7 + 0.4 * np.sin(0.9 * i + 0.3 + 0.2 * c) * np.cos(0.7 * j - 0.5 * c) + 0.15 * np.cos(0.37 * i * j + c)
                    for c in range(3)], axis=-1)
    rgb[H // 3, (2 * W) // 3] = 20.0 * rgb.mean()
    assert rgb.min() > 0.1
    return torch.from_numpy(rgb.astype(np.float32))


@functools.lru_cache(maxsize=None)
def light(name):
    """The tables Environment_Light builds for a fixture map, on the host."""
    from tensoir_amd import relight
    H, W = MAPS[name]
    hdr = hdr_map(H, W)
    env = relight.Environment_Light(hdr_maps={name: hdr}, device="cpu")
    return SimpleNamespace(name=name, H=H, W=W, hdr=hdr, rgb=env.hdr_rgbs[name].reshape(-1, 3), prob=env.hdr_pdf_sample[name].reshape(-1),
                           pdf_ret=env.hdr_pdf_return[name].reshape(-1), dirs=env.hdr_dir[name].reshape(-1, 3),
                           row_cdf=env.hdr_row_cdf[name], col_cdf=env.hdr_col_cdf[name], row_sin=env.hdr_row_sin[name])


def upper_bound(cdf, u):
    """first index with cdf[i] > u, clamped to the last (cdf [n] or per-pair rows [P, n], u [P]): the kernel's search"""
    cdf = cdf if cdf.ndim == 2 else cdf[None, :]
    return np.minimum((cdf <= u[:, None]).sum(axis=1), cdf.shape[1] - 1).astype(np.int64)


def cell_of(w, H, W):
    """The inverse of the direction table: (row, col) of the cell that contains the direction w [..., 3]."""
    th = torch.acos(w[..., 2].clamp(-1.0, 1.0))
    az = torch.atan2(w[..., 1], w[..., 0])
    row = torch.floor(th * H / math.pi).long().clamp(0, H - 1)
    col = torch.floor((math.pi - az) * W / (2 * math.pi)).long().clamp(0, W - 1)
    return row, col


# ---- surface points ----------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def points(M, seed=0):
    """M surface points: unit normals, view rays of length 1.3 with |n.v| >= 0.05 (about half of them with n.v < 0: the normal
    flips), roughness 0.1, 0.3 and 1 first, then uniform in [0.1, 1], albedo in [0.1, 0.9], fresnel in [0.02, 0.1]."""
    rng = np.random.default_rng(1000 * M + seed)
    n, d = _unit(rng, M), _unit(rng, M)
    for _ in range(100):
        bad = np.abs((n * d).sum(1)) < 0.05
        if not bad.any():
            break
        d[bad] = _unit(rng, int(bad.sum()))
    rough = rng.uniform(0.1, 1.0, M)
    rough[:3] = np.array([0.3, 0.1, 1.0])[:M]
    if M >= 5:                                   # a designed pair: the same point seen from either side
        n[4], d[4] = n[3], -d[3]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return SimpleNamespace(normal=t(n), rays_d=t(1.3 * d), rough=t(rough), albedo=t(rng.uniform(0.1, 0.9, (M, 3))),
                           fresnel=t(rng.uniform(0.02, 0.1, (M, 3))))


def take(pts, rows):
    return SimpleNamespace(**{k: v[rows].contiguous() for k, v in vars(pts).items()})


# ---- samplers and densities --------------------------------------------------------------------------------------------------------
def frame(a):
    """(t, b) perpendicular to the unit vectors a [..., 3] (Duff et al. 2017, as the kernel's mis_frame)"""
    x, y, z = a[..., 0], a[..., 1], a[..., 2]
    sg = torch.copysign(torch.ones_like(z), z)
    p = -1.0 / (sg + z)
    q = x * y * p
    return torch.stack([1.0 + sg * x * x * p, sg * q, -sg * x], -1), torch.stack([q, sg + y * y * p, -y], -1)


def surface(pts, dtype):
    """-> (raw normal, unit raw normal, flipped unit normal Nf, unit view V, alpha2), rows [M, .]"""
    normal, rays_d, rough = pts.normal.to(dtype), pts.rays_d.to(dtype), pts.rough.to(dtype)
    V = F.normalize(O.safe_l2_normalize(-rays_d), dim=-1)
    nh = F.normalize(normal, dim=-1)
    Nf = nh * torch.sum(V * nh, dim=-1, keepdim=True).sign()
    a = rough * rough
    return normal, nh, Nf, V, (a * a).reshape(-1, 1)


def pdf_light(lt, w, cell, dtype):
    """p_l(w) = P_cell H W / (2 pi^2 sin theta(w)) for directions w [..., 3] inside the cells `cell`"""
    sin_w = torch.sqrt(w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]).clamp(min=1e-8)
    return lt.prob.to(dtype)[cell] * (lt.H * lt.W) / (2 * math.pi * math.pi * sin_w)


def pdf_lobe(Nf, V, alpha2, w):
    """D(Nf.h) max(Nf.h, 0) / (4 v.h), h = normalize(v + w): the density per solid angle of w under the GGX lobe sampler"""
    h = F.normalize(w + V, dim=-1)
    noh = torch.sum(Nf * h, -1).clamp(min=0.0)
    voh = torch.sum(V * h, -1)
    cross = torch.linalg.cross(Nf.expand_as(h), h, dim=-1)
    t = torch.sum(cross * cross, -1) + alpha2 * noh * noh                      # 1 - noh^2 as |Nf x h|^2, as the kernel forms it
    return torch.where(voh > 0, (alpha2 / (math.pi * t * t)) * noh / (4.0 * voh.clamp(min=1e-300 if w.dtype == F64 else 1e-30)),
                       torch.zeros_like(voh))


def pdf_brdf(nh, Nf, V, alpha2, select, w, lobe=None):
    """p_b(w) = s max(n.w, 0) / pi + (1 - s) D(Nf.h) max(Nf.h, 0) / (4 v.h), h = normalize(v + w); nh, Nf, V [..., 3] and alpha2
    [...] broadcast against w [..., 3].  lobe: the second density where the caller knows it by other means."""
    cn = torch.sum(nh * w, -1).clamp(min=0.0)
    return select * cn / math.pi + (1.0 - select) * (pdf_lobe(Nf, V, alpha2, w) if lobe is None else lobe)


def setup(lt, pts, n_l, n_b, select, seed, offset, dtype):
    """k_env_mis_setup -> dirs [M, N, 3], cell [M, N], pdf_mix [M, N] (1 on inactive pairs), active [M, N], lobe [M, N] (LIGHT,
    COSINE or LOBE) and, meaningful in float64, exempt [M, N] (module docstring)."""
    M, N, H, W = pts.normal.shape[0], n_l + n_b, lt.H, lt.W
    select = float(np.float32(select))
    u32 = philox_uniform4(seed, offset, np.arange(M * N, dtype=np.uint64))
    u = torch.from_numpy(u32).to(dtype)
    pair = torch.arange(M * N)
    m, is_light = pair // N, (pair % N) < n_l
    normal, nh, Nf, V, alpha2 = (x[m] for x in surface(pts, dtype))
    alpha2 = alpha2[:, 0]
    # the light strategy
    row = upper_bound(lt.row_cdf.numpy(), u32[:, 0])
    col = upper_bound(lt.col_cdf.numpy()[row], u32[:, 1])
    row_l, col_l = torch.from_numpy(row), torch.from_numpy(col)
    theta = (row_l.to(dtype) + u[:, 2]) * math.pi / H
    az = math.pi - (col_l.to(dtype) + u[:, 3]) * 2 * math.pi / W
    w_l = torch.stack([torch.cos(az) * torch.sin(theta), torch.sin(az) * torch.sin(theta), torch.cos(theta)], -1)
    # the BRDF strategy: a one-sample mixture
    diffuse = torch.from_numpy(u32[:, 0] < np.float32(select))
    phi = 2 * math.pi * u[:, 2]
    ax = torch.where(diffuse[:, None], nh, Nf)
    # cos^2 = (1 - u1) / (1 + (a2 - 1) u1) and sin^2 = a2 u1 / the same, a2 = 1 for the cosine lobe; denominator as (1 - u1) + a2 u1
    a2 = torch.where(diffuse, torch.ones_like(alpha2), alpha2)
    den = (1.0 - u[:, 1]) + a2 * u[:, 1]
    cz, sz = torch.sqrt((1.0 - u[:, 1]) / den), torch.sqrt(a2 * u[:, 1] / den)
    t, b = frame(ax)
    d = (sz * torch.cos(phi))[:, None] * t + (sz * torch.sin(phi))[:, None] * b + cz[:, None] * ax
    vod = torch.sum(V * d, -1)
    w_b = torch.where(diffuse[:, None], d, 2.0 * vod[:, None] * d - V)
    row_b, col_b = cell_of(w_b, H, W)
    w = torch.where(is_light[:, None], w_l, w_b)
    cell = torch.where(is_light, row_l * W + col_l, row_b * W + col_b)
    lobe = torch.where(is_light, LIGHT, torch.where(diffuse, COSINE, LOBE))
    cosine = torch.sum(w * normal, -1)
    active = ((lobe != LOBE) | (vod > 0)) & (cosine > COS_THRESHOLD)
    # a lobe sample knows the density of its own half vector: sin^2 + alpha2 cos^2 = alpha2 / den, D = den^2 / (pi alpha2) -- the
    # same number as pdf_lobe(w) (tests/test_mis_cpu.py), without the trip through the rounded direction
    own = torch.where(vod > 0, den * den / (math.pi * a2) * cz / (4.0 * vod.clamp(min=1e-30)), torch.zeros_like(vod))
    lobe_pdf = torch.where(lobe == LOBE, own, pdf_lobe(Nf, V, alpha2, w))
    mix = (n_l * pdf_light(lt, w, cell, dtype) + n_b * pdf_brdf(nh, Nf, V, alpha2, select, w, lobe_pdf)) / N
    pdf_mix = torch.where(active, mix, torch.ones_like(mix))
    # exemptions
    th = torch.acos(w[:, 2].clamp(-1.0, 1.0))
    azc = math.pi - torch.atan2(w[:, 1], w[:, 0])
    d_th = (th - torch.round(th / (math.pi / H)) * (math.pi / H)).abs()
    d_az = (azc - torch.round(azc / (2 * math.pi / W)) * (2 * math.pi / W)).abs() * torch.sin(th)
    voh = torch.where(lobe == LOBE, vod, torch.sum(V * F.normalize(w + V, dim=-1), -1))
    exempt = (d_th < BORDER_RAD) | (d_az < BORDER_RAD) | ((cosine - COS_THRESHOLD).abs() < COS_MARGIN) | (voh.abs() < VOH_MARGIN)
    shape = lambda x: x.reshape(M, N, *x.shape[1:])
    return SimpleNamespace(dirs=shape(w), cell=shape(cell), pdf_mix=shape(pdf_mix), active=shape(active), lobe=shape(lobe),
                           exempt=shape(exempt), n_l=n_l, n_b=n_b, pdf_lobe_own=shape(own), pdf_lobe_w=shape(pdf_lobe(Nf, V, alpha2, w)))


# ---- the estimator -----------------------------------------------------------------------------------------------------------------
def samples(lt, pts, dirs, cell, pdf_mix, vis, dtype):
    """per-pair values (albedo / pi + spec) (vis L_cell) (n.w) / pdf_mix [M, N, 3]: k_relight_mis's summands"""
    normal, albedo, rough, fresnel, rays_d = (x.to(dtype) for x in (pts.normal, pts.albedo, pts.rough, pts.fresnel, pts.rays_d))
    dirs, pdf_mix, vis = dirs.to(dtype), pdf_mix.to(dtype), vis.to(dtype)
    M = normal.shape[0]
    cosine = torch.einsum("ijk,ik->ij", dirs, normal)
    spec = O.ggx_specular(normal, O.safe_l2_normalize(-rays_d), dirs, rough.reshape(M, 1), fresnel)
    brdf = albedo.unsqueeze(1) / math.pi + spec
    return brdf * (vis[:, :, None] * lt.rgb.to(dtype)[cell.long()]) * cosine[:, :, None] / pdf_mix[:, :, None]


def relight(lt, pts, dirs, cell, pdf_mix, vis, linear, dtype):
    """k_relight_mis -> [M, 3]: the mean over a point's pairs, raw (linear) or clamped to [0, 1] and sRGB-encoded"""
    total = samples(lt, pts, dirs, cell, pdf_mix, vis, dtype).mean(dim=1)
    return total if linear else O.linear2srgb(total.clamp(0.0, 1.0))


def integrand(lt, pts, w):
    """f(w) [M, K, 3] in float64 with V = 1 for directions w [K, 3]: (a / pi + spec) L_cell (n.w) on n.w > 1e-6"""
    M = pts.normal.shape[0]
    w = w.to(F64)
    row, col = cell_of(w, lt.H, lt.W)
    dirs = w.unsqueeze(0).expand(M, -1, -1)
    lit = (torch.einsum("ijk,ik->ij", dirs, pts.normal.to(F64)) > COS_THRESHOLD).to(F64)
    return samples(lt, pts, dirs, (row * lt.W + col).unsqueeze(0).expand(M, -1), torch.ones(M, w.shape[0], dtype=F64), lit, F64)


def sphere_grid(n_theta, n_phi, axis=None):
    """Midpoint grid over the sphere in polar coordinates about `axis` (default +z, with the map's own azimuth convention, so that
    n_theta, n_phi multiples of H, W put no grid cell across a map cell's border) -> (w [n_theta * n_phi, 3], solid angles)."""
    th = (torch.arange(n_theta, dtype=F64) + 0.5) * math.pi / n_theta
    ph = math.pi - (torch.arange(n_phi, dtype=F64) + 0.5) * 2 * math.pi / n_phi
    T, P = torch.meshgrid(th, ph, indexing="ij")
    loc = torch.stack([torch.cos(P) * torch.sin(T), torch.sin(P) * torch.sin(T), torch.cos(T)], -1).reshape(-1, 3)
    dw = (torch.sin(T) * (math.pi / n_theta) * (2 * math.pi / n_phi)).reshape(-1)
    if axis is None:
        return loc, dw
    a = torch.as_tensor(axis, dtype=F64)
    a = a / a.norm()
    t, b = frame(a)
    return loc[:, :1] * t + loc[:, 1:2] * b + loc[:, 2:3] * a, dw


# ---- the fixtures of the GPU tests -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(map_name, M, n_l, n_b, dtype=F64):
    """The restatement of one setup call of tests/test_gpu_mis.py (fixed seed, offset and lobe_select), computed once"""
    return setup(light(map_name), points(M), n_l, n_b, SELECT, SEED, OFFSET, dtype)


def random_vis(M, N, seed=0):
    rng = np.random.default_rng(77 + seed)
    return torch.from_numpy(rng.uniform(0.0, 1.0, (M, N)).astype(np.float32))
