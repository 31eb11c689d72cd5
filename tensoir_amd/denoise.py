"""Guided a-trous denoiser of relit views: the edge-avoiding wavelet filter of Dammertz et al. 2010 on the GPU.

    from tensoir_amd import denoise, relight
    view = relight.relight_view(model, env, names, rays, H, W, num_samples=32, denoise=denoise.AtrousConfig())
    view["rgb"]                                # [n_maps, H, W, 3], filtered;  view["raw"]: the Monte-Carlo estimate as drawn

The relit colours are a Monte-Carlo estimate; depth, normal, albedo and roughness of the primary pass are exact.  The filter
averages a pixel with neighbours on the same surface -- close in normal, in distance to the pixel's tangent plane, in albedo and
in roughness, optionally in colour -- over `levels` passes of a 5 x 5 B3-spline kernel whose taps lie 2^level pixels apart.  The
guide rows come from tir_denoise_guide, a level is one tir_atrous_level launch for all maps of the view (include/tensoir_hip.h;
DESIGN 4.13; restated in float64 by tests/denoise_reference.py).  There is no CPU path: without a GPU the calls raise.

Not done here: demodulating by albedo (it needs linear, diffuse / specular outputs of the integration kernels), temporal
accumulation, any use in training.
"""
from __future__ import annotations

import dataclasses
import math

import torch

from . import ops

GUIDE = ops.DENOISE_GUIDE
MAX_LEVELS = 6


@dataclasses.dataclass(frozen=True)
class AtrousConfig:
    """levels: passes, 1..6 (pass l has its taps 2^l pixels apart).  sigma_n: scale of 1 - n_p.n_q.  sigma_p: scale of the
    distance of q to p's tangent plane, in world units; None: 0.005 x the diagonal of the model's aabb (it must be given where
    there is no model).  sigma_a, sigma_r: scales of the albedo and roughness differences.  sigma_c: scale of the colour
    difference of the map being filtered; 0 switches the term off."""
    levels: int = 3
    sigma_n: float = 0.05
    sigma_p: float | None = None
    sigma_a: float = 0.1
    sigma_r: float = 0.1
    sigma_c: float = 0.5

    def __post_init__(self):
        if isinstance(self.levels, bool) or not isinstance(self.levels, int) or not 1 <= self.levels <= MAX_LEVELS:
            raise ValueError(f"AtrousConfig: levels is an integer in 1..{MAX_LEVELS}, got {self.levels!r}")
        for name in ("sigma_n", "sigma_p", "sigma_a", "sigma_r"):
            v = getattr(self, name)
            if name == "sigma_p" and v is None:
                continue
            if not _finite(v) or not v > 0:
                raise ValueError(f"AtrousConfig: {name} is a positive finite number, got {v!r}")
        if not _finite(self.sigma_c) or self.sigma_c < 0:
            raise ValueError(f"AtrousConfig: sigma_c is a finite number >= 0 (0: no colour term), got {self.sigma_c!r}")

    def inverses(self, aabb=None):
        """-> (1 / sigma_n, 1 / sigma_p, 1 / sigma_a^2, 1 / sigma_r^2, 1 / sigma_c^2 or 0): tir_atrous_level's arguments.  aabb:
        the model's [2, 3] box, read for sigma_p = None only."""
        sp = self.sigma_p
        if sp is None:
            if aabb is None:
                raise ValueError("AtrousConfig: sigma_p=None stands for 0.005 x the diagonal of a model's aabb; there is no model here")
            box = torch.as_tensor(aabb, dtype=torch.float64).reshape(2, 3).cpu()
            sp = 0.005 * float(torch.linalg.norm(box[1] - box[0]))
            if not _finite(sp) or not sp > 0:
                raise ValueError(f"AtrousConfig: the aabb {box.tolist()} has no diagonal")
        return (1.0 / self.sigma_n, 1.0 / sp, 1.0 / self.sigma_a ** 2, 1.0 / self.sigma_r ** 2,
                1.0 / self.sigma_c ** 2 if self.sigma_c > 0 else 0.0)


def _finite(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def filter_rows(color, guide, H, W, levels, inv):
    """color [H * W, K] and guide [H * W, 12] on the device -> the filtered [H * W, K]: `levels` launches, level l with step
    2^l and the five inverses `inv` (AtrousConfig.inverses), ping-ponging between two buffers of this call; `color` is only read."""
    src, bufs = color, (torch.empty_like(color), torch.empty_like(color) if levels > 1 else None)
    for level in range(levels):
        dst = bufs[level & 1]
        ops.atrous_level(src, dst, guide, H, W, 1 << level, *inv)
        src = dst
    return src


@torch.no_grad()
def atrous(color, guide, cfg=AtrousConfig(), aabb=None):
    """color [H, W, K] (K = 3 n_maps, the maps side by side) or [n_maps, H, W, 3], guide [H, W, 12] (ops.denoise_guide), both
    float32 on the GPU -> the filtered image in color's shape.  The caller's tensor is never written.  aabb: the model's box,
    for cfg.sigma_p = None."""
    if not isinstance(cfg, AtrousConfig):
        raise TypeError(f"atrous: cfg is an AtrousConfig, got {type(cfg).__name__}")
    if not torch.is_tensor(color) or not torch.is_tensor(guide) or not (color.is_cuda and guide.is_cuda):
        raise ops._lib.TensoirHipError("tensoir_amd.denoise needs its images on a GPU: tensoir_amd has no CPU path")
    if guide.dim() != 3 or guide.shape[-1] != GUIDE:
        raise ValueError(f"atrous: guide is [H, W, {GUIDE}], got {tuple(guide.shape)}")
    H, W = guide.shape[:2]
    stacked = color.dim() == 4
    if not ((color.dim() == 3 and color.shape[:2] == (H, W) and color.shape[2] % 3 == 0 and 3 <= color.shape[2] <= ops.ATROUS_MAX_K)
            or (stacked and color.shape[1:] == (H, W, 3) and 1 <= color.shape[0] <= ops.ATROUS_MAX_K // 3)):
        raise ValueError(f"atrous: color is [H, W, 3 n_maps] or [n_maps, H, W, 3] with 1..{ops.ATROUS_MAX_K // 3} maps on the "
                         f"guide's {H} x {W} pixels, got {tuple(color.shape)}")
    rows = color.permute(1, 2, 0, 3).reshape(H * W, -1) if stacked else color.reshape(H * W, -1)
    out = filter_rows(ops.f32(rows, "color"), ops.f32(guide, "guide").view(H * W, GUIDE), H, W, cfg.levels, cfg.inverses(aabb))
    return out.view(H, W, -1, 3).permute(2, 0, 1, 3).contiguous() if stacked else out.view(color.shape)
