"""Float64 numpy restatements of the image metrics (tensoir_amd/metrics.py; contract in include/tensoir_hip.h) and the seeded
inputs the CPU and GPU tests share.  Written from the definitions, not from the kernels: SSIM sums each n x n window directly
(no separable passes), with the one rule that matters for agreement with the reference: x*x, y*y and x*y are float32 products
of the float32 images, everything after is float64.  tests/golden/metrics_ssim.npz holds what the reference's own
utils.rgb_ssim returned for the three-channel cases (tools/make_golden_metrics.py)."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_ssim.npz")
MAP_CASES = ("ragged_tiles", "anti", "smooth")        # the cases whose whole map is recorded


def gaussian(filter_size, filter_sigma):
    """exp(-d^2 / (2 sigma^2)) at the tap centres, symmetric about the window's middle (half-pixel centres for even sizes),
    normalised to sum 1."""
    d = np.arange(filter_size, dtype=np.float64) - (filter_size - 1) / 2.0
    w = np.exp(-0.5 * (d / filter_sigma) ** 2)
    return w / w.sum()


def window_mean(z, w):
    """z [H, W, C] float64, w [n] -> [H - n + 1, W - n + 1, C]: out[i, j] = sum_kl w[k] w[l] z[i + k, j + l], summed tap by tap."""
    n = w.shape[0]
    oh, ow = z.shape[0] - n + 1, z.shape[1] - n + 1
    out = np.zeros((oh, ow, z.shape[2]), dtype=np.float64)
    for k in range(n):
        for l in range(n):
            out += (w[k] * w[l]) * z[k:k + oh, l:l + ow]
    return out


def ssim_map(img0, img1, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, exact_products=False, mean_fn=window_mean):
    """The SSIM map of two [H, W, C] images, float64.  The images are taken as float32; their three products are float32 products
    (exact_products=True forms them in float64 instead: NOT what the reference computes, kept to pin the rule)."""
    x, y = np.asarray(img0, dtype=np.float32), np.asarray(img1, dtype=np.float32)
    assert x.shape == y.shape and x.ndim == 3
    w = gaussian(filter_size, filter_sigma)
    if exact_products:
        xd, yd = x.astype(np.float64), y.astype(np.float64)
        xx, yy, xy = xd * xd, yd * yd, xd * yd
    else:
        xx, yy, xy = (x * x).astype(np.float64), (y * y).astype(np.float64), (x * y).astype(np.float64)
    m0, m1 = mean_fn(x.astype(np.float64), w), mean_fn(y.astype(np.float64), w)
    mu00, mu11, mu01 = m0 * m0, m1 * m1, m0 * m1
    s00 = np.maximum(0.0, mean_fn(xx, w) - mu00)
    s11 = np.maximum(0.0, mean_fn(yy, w) - mu11)
    s01 = mean_fn(xy, w) - mu01
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    return ((2.0 * mu01 + c1) * (2.0 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))


def ssim(img0, img1, **kw):
    return float(np.mean(ssim_map(img0, img1, **kw)))


def separable_mean(z, w):
    """window_mean as two 1-D passes through scipy.signal.convolve2d (columns, then rows): the host baseline of
    tools/metrics_bench.py.  Needs scipy."""
    import scipy.signal
    return np.stack([scipy.signal.convolve2d(scipy.signal.convolve2d(z[..., c], w[:, None], mode="valid"), w[None, :], mode="valid")
                     for c in range(z.shape[-1])], -1)


def ssim_separable(img0, img1, **kw):
    return float(np.mean(ssim_map(img0, img1, mean_fn=separable_mean, **kw)))


def psnr(a, b, mask=None):
    a, b = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    d = (a - b) ** 2
    if mask is not None:
        d = d[np.asarray(mask).reshape(d.shape[:-1]) != 0]
    mse = float(d.sum()) / d.size if d.size else float("nan")
    return -10.0 * math.log10(mse) if mse > 0 else (float("inf") if mse == 0 else float("nan"))


def normal_mae(a, b, mask=None):
    a, b = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    deg = np.arccos(np.clip(dot, -1.0, 1.0)) * 180.0 / np.pi
    if mask is not None:
        deg = deg[np.asarray(mask).reshape(deg.shape) != 0]
    return float(deg.sum()) / deg.size if deg.size else float("nan")


def lower_median(v):
    v = np.sort(np.asarray(v).reshape(-1))
    return v[(v.shape[0] - 1) // 2]


def albedo_scale(pred, gt, mask):
    """(lower median of the first channel of r, per-channel lower medians of r), r = gt / max(pred, 1e-6) in float32 over the mask"""
    m = np.asarray(mask).reshape(-1) != 0
    pred, gt = np.asarray(pred, dtype=np.float32).reshape(-1, 3)[m], np.asarray(gt, dtype=np.float32).reshape(-1, 3)[m]
    r = gt / np.maximum(pred, np.float32(1e-6))
    return lower_median(r[:, 0]), np.array([lower_median(r[:, c]) for c in range(3)], dtype=np.float32)


def _smooth(rng, H, W, C):
    """a band-limited image in [0.1, 0.9]"""
    yy, xx = np.meshgrid(np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W), indexing="ij")
    img = np.zeros((H, W, C))
    for c in range(C):
        f = rng.uniform(1.0, 4.0, size=4)
        p = rng.uniform(0.0, 2 * np.pi, size=2)
        img[..., c] = 0.5 + 0.2 * np.sin(f[0] * xx * 2 * np.pi + p[0]) * np.cos(f[1] * yy * 2 * np.pi) + 0.2 * np.sin((f[2] * xx + f[3] * yy) * np.pi + p[1])
    return img.astype(np.float32)


def _pair(rng, H, W, C, noise=0.05):
    a = _smooth(rng, H, W, C)
    b = np.clip(a + rng.normal(0.0, noise, size=a.shape), 0.0, 1.0).astype(np.float32)
    return a, b


def cases(tile=16):
    """[(name, img0, img1, keyword arguments of ssim)]: the shapes and contents at which the kernel can go wrong.  tile = the side
    of a workgroup's output tile (metrics.SSIM_TILE).  Seeded: every call returns the same arrays."""
    rng = np.random.default_rng(20240611)
    T = int(tile)
    out = []
    a, b = _pair(rng, 11, 11, 3)
    out.append(("one_pixel", a, b, {}))                                      # a single output pixel
    a, b = _pair(rng, 11, 40, 3)
    out.append(("one_row", a, b, {}))                                        # one output row, two tiles wide
    a, b = _pair(rng, 2 * T + 5 + 10, 2 * T + T // 2 + 1 + 10, 3, noise=0.1)
    out.append(("ragged_tiles", a, b, {}))                                   # 3 x 3 tiles, the last ones ragged
    a, b = _pair(rng, 33, 34, 1)
    out.append(("gray", a, b, {}))
    a, b = _pair(rng, 20, 37, 4)
    out.append(("rgba", a, b, {}))
    a = _smooth(rng, 40, 45, 3)
    out.append(("smooth", a, (np.float32(0.9) * a + np.float32(0.03)).astype(np.float32), {}))
    a = _pair(rng, 30, 35, 3)[1]
    out.append(("self", a, a.copy(), {}))                                    # exactly 1.0
    flat0 = np.broadcast_to(np.array([0.7, 0.1, 0.3], dtype=np.float32), (24, 29, 3)).copy()
    flat1 = np.broadcast_to(np.array([0.7, 0.6, 0.9], dtype=np.float32), (24, 29, 3)).copy()
    out.append(("flat", flat0, flat1, {}))                                   # E[x^2] - mu^2 is rounding noise: the variance clamp
    a = _smooth(rng, 30, 35, 3)
    out.append(("anti", a, (np.float32(1.0) - a).astype(np.float32), {}))    # negative covariance: the sign / min branch
    a, b = _pair(rng, 28, 31, 3)
    out.append(("hdr", (4.0 * a).astype(np.float32), (4.0 * b).astype(np.float32), {"max_val": 4.0}))
    yy, xx = np.meshgrid(np.arange(36) - 17.5, np.arange(38) - 18.5, indexing="ij")
    a, b = _pair(rng, 36, 38, 3)
    in0, in1 = (yy ** 2 + xx ** 2 < 12 ** 2)[..., None], (yy ** 2 + (xx - 1) ** 2 < 12.5 ** 2)[..., None]
    out.append(("white_bg", np.where(in0, a, np.float32(1.0)).astype(np.float32), np.where(in1, b, np.float32(1.0)).astype(np.float32), {}))
    a, b = _pair(rng, 21, 26, 3)
    out.append(("filter5", a, b, {"filter_size": 5, "filter_sigma": 0.8}))
    a, b = _pair(rng, 19, 23, 3)
    out.append(("filter4", a, b, {"filter_size": 4, "filter_sigma": 1.0}))   # an even filter
    return out
