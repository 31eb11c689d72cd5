"""Float64 restatement of the total-variation loss and of its gradient (include/tensoir_hip.h, tir_tv_fwd / tir_tv_bwd), written
from the formulas; shared by tests/test_regularisers_cpu.py and tests/test_gpu_regularisers.py.

For a plane x [1, C, H, W]:   Sh = sum (x[h+1] - x[h])^2,   Sw = sum (x[w+1] - x[w])^2,   nh = C (H - 1) W,   nw = C H (W - 1)
    loss = sum_p coef_p 2 (Sh_p / nh_p + Sw_p / nw_p)
    d loss / d x_p [h, w, c] = 4 g coef_p ((dmh - dph) / nh_p + (dmw - dpw) / nw_p)
with dph = x[h+1] - x[h] (0 on the last row), dmh = x[h] - x[h-1] (0 on the first row), and dpw, dmw the same along W."""
import numpy as np
import torch

# (C, H, W): every element on an edge (one-sided stencils only) / the scalar path / several workgroups in one plane / more than
# TIR_TV_FWD_GROUPS shares of TIR_TV_SHARE floats (1 080 000 > 128 * 8192): the forward's workgroups grow beyond TIR_TV_SHARE, and its
# tail adds more than 64 partials for one plane
SINGLE_SHAPES = [(16, 2, 2), (48, 3, 2), (16, 2, 5), (5, 7, 6), (48, 37, 41), (48, 150, 150)]
# unequal planes in one call, as matMode produces them for the grid [20, 22, 24]
GRID_SHAPES = [(16, 22, 20), (16, 24, 20), (16, 24, 22)]
SEED = 20240607


def plane(shape, seed=SEED, channel_last=True):
    """0.1 * randn [1, C, H, W] float32 (as the constructor draws a plane), stored channel-last unless told otherwise"""
    c, h, w = shape
    x = 0.1 * torch.randn((1, c, h, w), generator=torch.Generator().manual_seed(seed + 1000 * c + 10 * h + w), dtype=torch.float32)
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if channel_last else x.contiguous()


def counts(x):
    _, c, h, w = x.shape
    return c * (h - 1) * w, c * h * (w - 1)


def sums(x):
    """-> (Sh, Sw) in float64 from the values of x as they are"""
    a = x.detach().cpu().double().numpy()[0]
    return float(np.sum((a[:, 1:, :] - a[:, :-1, :]) ** 2)), float(np.sum((a[:, :, 1:] - a[:, :, :-1]) ** 2))


def loss(planes, coefs):
    total = 0.0
    for x, k in zip(planes, coefs):
        (sh, sw), (nh, nw) = sums(x), counts(x)
        total += float(k) * 2.0 * (sh / nh + sw / nw)
    return total


def gradient(x, coef, g=1.0):
    """-> d (g coef TV(x)) / dx, float64 numpy [1, C, H, W]"""
    a = x.detach().cpu().double().numpy()[0]
    nh, nw = counts(x)
    dh, dw = a[:, 1:, :] - a[:, :-1, :], a[:, :, 1:] - a[:, :, :-1]
    out = np.zeros_like(a)
    out[:, 1:, :] += dh / nh          # dmh
    out[:, :-1, :] -= dh / nh         # dph
    out[:, :, 1:] += dw / nw          # dmw
    out[:, :, :-1] -= dw / nw         # dpw
    return (4.0 * float(g) * float(coef) * out)[None]


def gradient_tolerance(x, coef, g=1.0):
    """The bound of the backward tests: 32 * 2^-24 * 4 |g coef| (1 / nh + 1 / nw) * 4 max|x| -- the magnitude bound of the bracket (every
    difference is at most 2 max|x|, two of them per axis) times a few fp32 roundings, with slack."""
    nh, nw = counts(x)
    return 32 * 2.0 ** -24 * 4 * abs(float(g) * float(coef)) * (1.0 / nh + 1.0 / nw) * 4 * float(x.detach().abs().max())
