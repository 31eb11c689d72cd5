"""Float64 numpy restatement of the guided a-trous denoiser (include/tensoir_hip.h, tir_denoise_guide / tir_atrous_level;
tensoir_amd/denoise.py): the yardstick of tests/test_denoise_cpu.py and tests/test_gpu_denoise.py.  It follows the formulas of
the header, not the kernels' code: whole-image shifts instead of a loop over pixels, float64 throughout."""
import numpy as np

TAPS = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
GUIDE = 12


def guide_rows(maps, rays, acc_thres=0.5):
    """maps [B, 20], rays [B, 6] -> guide [B, 12] float64: {o + depth d, acc > acc_thres, normal / max(|normal|, fp32(1e-6)),
    roughness, albedo, 0}."""
    maps, rays = np.asarray(maps, np.float64), np.asarray(rays, np.float64)
    g = np.zeros((maps.shape[0], GUIDE))
    g[:, 0:3] = rays[:, 0:3] + maps[:, 3:4] * rays[:, 3:6]
    g[:, 3] = maps[:, 14] > acc_thres
    nrm = maps[:, 4:7]
    g[:, 4:7] = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), float(np.float32(1e-6)))
    g[:, 7] = maps[:, 10]
    g[:, 8:11] = maps[:, 7:10]
    return g


def inverses(sigma_n=0.05, sigma_p=None, sigma_a=0.1, sigma_r=0.1, sigma_c=0.5):
    """AtrousConfig.inverses in float64; sigma_p must be a number here."""
    return (1.0 / sigma_n, 1.0 / sigma_p, 1.0 / sigma_a ** 2, 1.0 / sigma_r ** 2, 1.0 / sigma_c ** 2 if sigma_c > 0 else 0.0)


def _shift(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx] where that lies inside (anything elsewhere), and the mask of where it does"""
    H, W = a.shape[:2]
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    return a[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)], inside


def atrous_level(color, guide, step, inv_sn, inv_sp, inv_sa2, inv_sr2, inv_sc2=0.0):
    """color [H, W, K] (K = 3 n_maps), guide [H, W, 12] -> one level [H, W, K], float64."""
    color, guide = np.asarray(color, np.float64), np.asarray(guide, np.float64)
    H, W, K = color.shape
    assert K % 3 == 0 and guide.shape == (H, W, GUIDE) and step >= 1
    c = color.reshape(H, W, K // 3, 3)
    pos, valid, nrm, rough, alb = guide[..., 0:3], guide[..., 3] > 0.5, guide[..., 4:7], guide[..., 7], guide[..., 8:11]
    num, den = np.zeros_like(c), np.zeros((H, W, K // 3))
    for j in range(-2, 3):
        for i in range(-2, 3):
            gq, inside = _shift(guide, j * step, i * step)
            cq, _ = _shift(c, j * step, i * step)
            ok = inside & (gq[..., 3] > 0.5)
            a = (np.maximum(0.0, 1.0 - np.sum(nrm * gq[..., 4:7], -1)) * inv_sn
                 + np.abs(np.sum((gq[..., 0:3] - pos) * nrm, -1)) * inv_sp
                 + np.sum((alb - gq[..., 8:11]) ** 2, -1) * inv_sa2
                 + (rough - gq[..., 7]) ** 2 * inv_sr2)
            d2 = np.sum((c - cq) ** 2, -1)
            with np.errstate(under="ignore", over="ignore", invalid="ignore"):
                w = TAPS[abs(i)] * TAPS[abs(j)] * np.exp(-(a[..., None] + d2 * inv_sc2))
            w = np.where(ok[..., None], w, 0.0)
            num += w[..., None] * np.where(ok[..., None, None], cq, 0.0)
            den += w
    out = num / np.where(den > 0, den, 1.0)[..., None]
    return np.where(valid[..., None, None], out, c).reshape(H, W, K)


def atrous(color, guide, levels=3, inv=None, **sigmas):
    """denoise.atrous: level l with step 2^l, in float64 from start to end.  color [H, W, K] or [n_maps, H, W, 3].  inv: the five
    inverses where the caller has them (the fp32 values a kernel was handed) instead of the sigmas."""
    color = np.asarray(color, np.float64)
    stacked = color.ndim == 4
    x = color.transpose(1, 2, 0, 3).reshape(color.shape[1], color.shape[2], -1) if stacked else color
    inv = inverses(**sigmas) if inv is None else inv
    for level in range(levels):
        x = atrous_level(x, guide, 1 << level, *inv)
    return x.reshape(x.shape[0], x.shape[1], -1, 3).transpose(2, 0, 1, 3) if stacked else x


# ---- the synthetic scene of the benefit test ----------------------------------------------------------------------------------
def sphere_scene(side=96):
    """A sphere over a checkered plane under one directional light with a cast shadow, seen from above at an angle; a strip of
    invalid pixels on the left.  -> (clean colour [side, side, 3] in [0, 1], guide [side, side, 12]), float64."""
    H = W = side
    eye = np.array([0.0, -3.0, 2.2])
    fwd = np.array([0.0, 3.0, -1.7])
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    v, u = np.meshgrid((np.arange(H) + 0.5) / H * 2 - 1, (np.arange(W) + 0.5) / W * 2 - 1, indexing="ij")
    d = fwd + 0.55 * u[..., None] * right - 0.55 * v[..., None] * up
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    centre, radius = np.array([0.0, 0.0, 0.6]), 0.6
    light = np.array([0.5, -0.3, 0.8])
    light /= np.linalg.norm(light)

    def hit_sphere(o, dirs):
        oc = o - centre
        b = np.sum(oc * dirs, -1)
        disc = b * b - (np.sum(oc * oc, -1) - radius ** 2)
        t = -b - np.sqrt(np.maximum(disc, 0.0))
        return np.where((disc > 0) & (t > 1e-6), t, np.inf)

    t_s = hit_sphere(eye, d)
    t_p = np.where(d[..., 2] < -1e-9, -eye[2] / np.minimum(d[..., 2], -1e-9), np.inf)
    on_sphere = t_s < t_p
    t = np.minimum(t_s, t_p)
    valid = np.isfinite(t)
    t = np.where(valid, t, 0.0)
    pos = eye + t[..., None] * d
    nrm = np.where(on_sphere[..., None], (pos - centre) / radius, np.array([0.0, 0.0, 1.0]))
    check = (np.floor(pos[..., 0] * 1.5) + np.floor(pos[..., 1] * 1.5)) % 2
    alb = np.where(on_sphere[..., None], np.array([0.8, 0.3, 0.2]), np.where(check[..., None] > 0, 0.8, 0.25) * np.ones(3))
    rough = np.where(on_sphere, 0.3, 0.7)
    shadow = np.isfinite(hit_sphere(pos + 1e-4 * nrm, light)) & ~on_sphere
    shade = 0.15 + 0.85 * np.maximum(np.sum(nrm * light, -1), 0.0) * np.where(shadow, 0.0, 1.0)
    clean = np.clip(alb * shade[..., None], 0.0, 1.0)
    valid[:, :7] = False                                        # the invalid strip
    clean = np.where(valid[..., None], clean, 0.5)
    g = np.zeros((H, W, GUIDE))
    g[..., 0:3], g[..., 3], g[..., 4:7], g[..., 7], g[..., 8:11] = pos, valid, nrm, rough, alb
    return clean, g
