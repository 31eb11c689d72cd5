"""Image metrics on the GPU: the reference's SSIM, PSNR and mean angular error of normals, and an evaluation driver.

    from tensoir_amd import metrics
    metrics.ssim(img, gt)                      # the number utils.rgb_ssim(img, gt, 1) gives, from one HIP launch
    metrics.evaluate(model, dataset)           # the reference's test report for a checkpoint, every map kept on the device
    metrics.chamfer("mesh.ply", "gt.ply")      # Chamfer / Hausdorff distance of two meshes (mesh.distance; tir_distance.hip)
    python -m tensoir_amd.metrics CKPT --config configs/... [--views N]

ssim / psnr / normal_mae take numpy arrays or torch tensors on any device; host inputs are uploaded and host results come back
(there is no CPU path: without a GPU they raise).  The kernels are tir_ssim and tir_image_error (include/tensoir_hip.h; DESIGN
4.11): fp32 products and double sums, as the reference computes when it is handed fp32 images, and fixed-order means.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops

SSIM_TILE = ops.SSIM_TILE            # side of the output tile one workgroup of tir_ssim computes
MAX_FILTER = ops.SSIM_MAX_TAPS

# the report names of the reference (renderer.py:489-498)
REPORT_KEYS = ("PSNR_nvs", "PSNR_nvs_brdf", "PSNR_albedo_single_aligned", "PSNR_albedo_three_aligned", "SSIM_rgb", "SSIM_rgb_brdf",
               "SSIM_albedo_single", "SSIM_albedo_three", "MAE")


def gaussian_taps(filter_size=11, filter_sigma=1.5):
    """The reference's 1-D filter (utils.py:105-109) in numpy float64, even sizes included through its half-pixel shift."""
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    filt /= np.sum(filt)
    return filt


def _device_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise ops._lib.TensoirHipError("tensoir_amd.metrics needs a GPU: tensoir_amd has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _f32(x, dev):
    """numpy array / tensor on any device, any dtype -> contiguous float32 tensor on dev"""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.detach().to(dev, torch.float32).contiguous()


def _shape(x):
    return tuple(x.shape)


def ssim(img0, img1, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """The reference's rgb_ssim (utils.py:93-139), its parameters and its return convention, for [H, W, C] images (-> a numpy
    float64 scalar, or with return_map the float64 map [H - f + 1, W - f + 1, C]) or a batch [N, H, W, C] (-> [N] / [N, ...]).
    1 <= C <= 4.  numpy arrays or torch tensors on any device; anything that is not float32 is converted to float32 first (the
    reference is handed float32 images, and its squares are float32 squares).  Host inputs are uploaded, the result is returned
    on the host.  ValueError: shapes differ, C > 4, filter_size outside 1..31 or larger than the image."""
    s0, s1 = _shape(img0), _shape(img1)
    if s0 != s1 or len(s0) not in (3, 4):
        raise ValueError(f"ssim: two images of one shape [H, W, C] or [N, H, W, C], got {s0} and {s1}")
    filter_size = int(filter_size)
    if not 1 <= filter_size <= MAX_FILTER:
        raise ValueError(f"ssim: filter_size must lie in 1..{MAX_FILTER}, got {filter_size}")
    H, W, Cn = s0[-3:]
    if not 1 <= Cn <= 4:
        raise ValueError(f"ssim: 1 to 4 channels, got {Cn}")
    if filter_size > min(H, W):
        raise ValueError(f"ssim: a {filter_size}-tap filter does not fit a {H} x {W} image")
    dev = _device_of(img0, img1)
    a, b = _f32(img0, dev).view(-1, H, W, Cn), _f32(img1, dev).view(-1, H, W, Cn)
    taps = gaussian_taps(filter_size, filter_sigma)[::-1]           # convolve2d flips the (symmetric) filter
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    out = ops.ssim(a, b, taps, c1, c2, return_map=return_map)
    res = (out[1] if return_map else out).cpu().numpy()
    return res if len(s0) == 4 else res[0]


def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """ssim with the reference's signature and its assertions: one three-channel image pair."""
    assert len(img0.shape) == 3
    assert img0.shape[-1] == 3
    assert img0.shape == img1.shape
    return ssim(img0, img1, max_val, filter_size, filter_sigma, k1, k2, return_map)


def _errors(a, b, mask, angular):
    """a, b [..., C], mask None or [...] -> (count, sum of squares, sum of degrees, C) as floats, one image"""
    s0, s1 = _shape(a), _shape(b)
    if s0 != s1 or len(s0) < 1:
        raise ValueError(f"two images of one shape [..., C], got {s0} and {s1}")
    if mask is not None and _shape(mask) not in (s0[:-1], s0[:-1] + (1,)):
        raise ValueError(f"mask: one entry per pixel, got {_shape(mask)} for images {s0}")
    if not 1 <= s0[-1] <= 4:
        raise ValueError(f"1 to 4 channels, got {s0[-1]}")
    dev = _device_of(a, b, mask)
    a, b = _f32(a, dev).view(1, -1, s0[-1]), _f32(b, dev).view(1, -1, s0[-1])
    if mask is not None:
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask))
        mask = (m.to(dev) != 0).view(1, -1)
    cnt, sq, ang = ops.image_error(a, b, mask, angular)[0].tolist()
    return cnt, sq, ang, s0[-1]


def _psnr_of(mse):
    return -10.0 * math.log10(mse) if mse > 0 else float("inf")


def psnr(a, b, mask=None):
    """-10 log10 of the mean squared difference of two images [..., C] (1 <= C <= 4) over all channels of the pixels where mask
    [...] is set (default: all), as the evaluation loop forms it (renderer.py:300-303); the squares are summed in double on the
    device.  inf for equal images, nan when no pixel counts."""
    cnt, sq, _, Cn = _errors(a, b, mask, False)
    return _psnr_of(sq / (cnt * Cn)) if cnt else float("nan")


def normal_mae(a, b, mask=None):
    """Mean over the pixels (where mask is set; default: all, as renderer.py:470) of acos(clamp(a . b, -1, 1)) in degrees for two
    [..., 3] normal maps.  Nothing is normalised here."""
    if _shape(a)[-1] != 3:
        raise ValueError("normal_mae: [..., 3] maps")
    cnt, _, ang, _ = _errors(a, b, mask, True)
    return ang / cnt if cnt else float("nan")


def _mesh_on_device(m, dev):
    """(verts, faces) tensors, or the path of a .ply / .glb file as mesh.write_ply / export_mesh / export_textured write them."""
    from . import mesh
    if isinstance(m, (str, bytes)) or hasattr(m, "__fspath__"):
        import os
        path = os.fspath(m)
        path = path.decode() if isinstance(path, bytes) else path
        if path.lower().endswith(".glb"):
            v = mesh.read_glb(path)["pos"]                            # unwelded: three vertices per face, no index buffer
            f = np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)
        elif path.lower().endswith(".ply"):
            v, f, _ = mesh.read_ply_attributes(path)
        else:
            raise ValueError(f"chamfer: {path!r} is neither a .ply nor a .glb file")
        m = (v, f)
    v, f = m
    v = torch.as_tensor(np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v).to(dev, torch.float32).reshape(-1, 3)
    f = torch.as_tensor(np.ascontiguousarray(f) if isinstance(f, np.ndarray) else f).to(dev, torch.int32).reshape(-1, 3)
    return v.contiguous(), f.contiguous()


def chamfer(a, b, **kw):
    """mesh.distance under the name of the geometry figure of inverse-rendering papers: the Chamfer distance of a recovered
    mesh to a ground-truth one is result["chamfer"] (the sum of the two mean surface distances, in the meshes' coordinates).
    a, b: (verts, faces) tensors or arrays, or paths to .ply / .glb files; kw: mesh.distance's samples and seed, and its
    options signed, thresholds, normals and allow_open (the signed distance, F-score and normal consistency).  Host inputs
    are uploaded; there is no CPU path."""
    from . import mesh
    dev = _device_of(*[x for m in (a, b) if isinstance(m, (tuple, list)) for x in m])
    return mesh.distance(_mesh_on_device(a, dev), _mesh_on_device(b, dev), **kw)


def albedo_scale(pred, gt, mask):
    """The reference's rescale ratios (renderer.py:49-50): with r = gt / pred.clamp(min=1e-6) over the pixels where mask is set,
    (the lower median of r's first channel, the per-channel lower medians [3]) as device tensors.  torch on the device: a
    median is plumbing, not a hot path."""
    dev = _device_of(pred, gt, mask)
    pred, gt = _f32(pred, dev).view(-1, 3), _f32(gt, dev).view(-1, 3)
    m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask))
    m = (m.to(dev) != 0).view(-1)
    r = gt[m] / pred[m].clamp(min=1e-6)
    return r[:, 0].median(), r.median(dim=0)[0]


def _view_indices(views, n_all):
    if views is None:
        return list(range(n_all))
    if isinstance(views, int):                                         # N views at the reference's spacing (renderer.py:203, :214)
        n = max(1, min(views, n_all))
        return [i * (n_all // n) for i in range(n)]
    return [int(v) for v in views]


@torch.no_grad()
def evaluate(model, dataset, views=None, light_idx=0, chunk=16384, args=None, ssim=True, maps=None):
    """The reference's test report (evaluation_iter_TensoIR, renderer.py:211-338, :455-498) for `model` on a dataset that follows
    its item protocol (rays, rgbs, rgbs_mask, normals, albedo, img_wh; tensoir_amd.synth_dataset is one).  Every view is rendered
    with Renderer_TensoIR_train(is_train=False, is_relight=True) in chunks of `chunk` rays under light `light_idx`; no map leaves
    the device.  views: None (all), an int N (N views at the reference's spacing) or a list of indices.  args carries the
    re-render's second_nSample / second_near / second_far (default 96, 0.05, 1.5).
    -> {"views": [per view {...}], "mean": {...}} of plain floats under the reference's report names:
      PSNR_nvs, PSNR_nvs_brdf       rgb_map / rgb_with_brdf_map, clamped to [0, 1], against the view's image
      PSNR_albedo_single_aligned,   albedo_map times the rescale ratio (first-channel / per-channel lower median of gt / albedo over
      PSNR_albedo_three_aligned     the masked pixels, albedo_scale), clamped, 1 outside the mask, against the view's albedo; both
                                    raised to 1 / 2.2 first, as the reference stores them (:392-394, :465-468)
      SSIM_rgb, SSIM_rgb_brdf,      metrics.ssim of the same four pairs (the albedo pairs without the gamma, :315-319), in one
      SSIM_albedo_single / _three   batched launch per view; absent with ssim=False
      MAE                           normal_mae of the normalised normal_map against the normalised view normals, all pixels
    The ratio is the global one (over up to 20 sampled views, compute_rescale_ratio, :21-53) when the views cover the whole
    dataset and the view's own otherwise, as test_all selects.  "mean" averages the views; the two albedo PSNRs are formed from
    the mean of the views' squared errors (the reference pools them, :465-468).
    maps (a list) receives per view the device tensors that were measured: rgb, rgb_brdf, albedo_single, albedo_three, normal,
    gt_rgb, gt_albedo, gt_normal, the three albedo maps raised to 1 / 2.2 as <name>_gamma [H, W, 3], and mask [H, W]."""
    import types
    from .renderer import Renderer_TensoIR_train
    if args is None:
        args = types.SimpleNamespace(second_nSample=96, second_near=0.05, second_far=1.5)
    dev = model.aabb.device
    W, H = (int(x) for x in dataset.img_wh)
    n_all = len(dataset)
    idx_list = _view_indices(views, n_all)
    if not idx_list or min(idx_list) < 0 or max(idx_list) >= n_all:
        raise ValueError(f"evaluate: views must name some of the dataset's {n_all} views")
    white_bg = bool(getattr(dataset, "white_bg", True))
    cache = {}

    def render(idx):
        if idx in cache:
            return cache[idx]
        item = dataset[idx]
        rays = item["rays"].reshape(-1, 6).to(dev, torch.float32)
        lidx = torch.full((rays.shape[0], 1), int(light_idx), dtype=torch.int32, device=dev)
        parts = [Renderer_TensoIR_train(rays[a:a + chunk], None, lidx[a:a + chunk], model, N_samples=-1, white_bg=white_bg, is_train=False,
                                        is_relight=True, sample_method="fixed_envirmap", device=dev, args=args, _no_graph=True)
                 for a in range(0, rays.shape[0], int(chunk))]
        ret = {k: torch.cat([p[k].reshape(-1, 3) for p in parts]).reshape(H, W, 3)
               for k in ("rgb_map", "rgb_with_brdf_map", "albedo_map", "normal_map")}
        rgbs = item["rgbs"]
        gt = {"rgb": rgbs[min(int(light_idx), rgbs.shape[0] - 1)] if rgbs.dim() == 3 else rgbs, "albedo": item["albedo"], "normal": item["normals"]}
        gt = {k: v.reshape(H, W, 3).to(dev, torch.float32) for k, v in gt.items()}
        gt["mask"] = item["rgbs_mask"].reshape(H, W).to(dev) != 0
        return ret, gt

    whole = set(idx_list) == set(range(n_all))
    ratio = None
    if whole:                                       # compute_rescale_ratio: 20 views at interval len // 20 (all of them view 0 below 20 views)
        sampled = sorted({i * (n_all // 20) for i in range(20)})
        pred, gta = [], []
        for idx in sampled:
            cache[idx] = render(idx)
            ret, gt = cache[idx]
            pred.append(ret["albedo_map"][gt["mask"]])
            gta.append(gt["albedo"][gt["mask"]])
        pred = torch.cat(pred)
        ratio = albedo_scale(pred, torch.cat(gta), torch.ones(pred.shape[0], dtype=torch.bool, device=dev))

    out, mses = [], []
    for idx in idx_list:
        ret, gt = render(idx)
        cache.pop(idx, None)
        mask = gt["mask"]
        single, three = ratio if ratio is not None else albedo_scale(ret["albedo_map"], gt["albedo"], mask)
        m = {"rgb": ret["rgb_map"].clamp(0.0, 1.0), "rgb_brdf": ret["rgb_with_brdf_map"].clamp(0.0, 1.0),
             "normal": torch.nn.functional.normalize(ret["normal_map"], dim=-1),
             "gt_rgb": gt["rgb"], "gt_albedo": gt["albedo"], "gt_normal": torch.nn.functional.normalize(gt["normal"], dim=-1), "mask": mask}
        for name, r in (("albedo_single", single), ("albedo_three", three)):
            al = torch.ones_like(ret["albedo_map"])
            al[mask] = (r * ret["albedo_map"][mask]).clamp(min=0.0, max=1.0)
            m[name] = al
        for name in ("albedo_single", "albedo_three", "gt_albedo"):
            m[name + "_gamma"] = m[name] ** (1 / 2.2)
        if maps is not None:
            maps.append(m)
        a = torch.stack([m["rgb"], m["rgb_brdf"], m["albedo_single_gamma"], m["albedo_three_gamma"], m["normal"]]).view(5, H * W, 3)
        b = torch.stack([m["gt_rgb"], m["gt_rgb"], m["gt_albedo_gamma"], m["gt_albedo_gamma"], m["gt_normal"]]).view(5, H * W, 3)
        res = [ops.image_error(a, b, None, angular=True)]
        if ssim:
            a4 = torch.stack([m["rgb"], m["rgb_brdf"], m["albedo_single"], m["albedo_three"]])
            b4 = torch.stack([m["gt_rgb"], m["gt_rgb"], m["gt_albedo"], m["gt_albedo"]])
            f = min(11, H, W)
            res.append(ops.ssim(a4, b4, gaussian_taps(f, 1.5)[::-1], 0.01 ** 2, 0.03 ** 2))
        err = res[0].tolist()                                   # the view's one wait
        mse = [e[1] / (e[0] * 3) for e in err[:4]]
        v = dict(zip(REPORT_KEYS[:4], (_psnr_of(x) for x in mse)))
        if ssim:
            v.update(zip(REPORT_KEYS[4:8], res[1].tolist()))
        v["MAE"] = err[4][2] / err[4][0]
        mses.append(mse)
        out.append(v)
    mean = {k: float(np.mean([v[k] for v in out])) for k in out[0]}
    for j in (2, 3):
        mean[REPORT_KEYS[j]] = _psnr_of(float(np.mean([x[j] for x in mses])))
    return {"views": out, "mean": mean}


def main(argv=None):
    import argparse
    import json
    import types
    from . import bake, synth_dataset
    ap = argparse.ArgumentParser(prog="python -m tensoir_amd.metrics", description="Evaluate a checkpoint on its test split: the "
                                 "reference's PSNR / SSIM / MAE report as JSON, computed on the GPU.")
    ap.add_argument("ckpt")
    ap.add_argument("--config", required=True, help="a TensoIR config file; its datadir names the dataset (synthetic:views=..,res=..)")
    ap.add_argument("--views", type=int, default=None, metavar="N", help="evaluate N views at the reference's spacing (default: all, "
                    "with the global albedo rescale ratio)")
    ap.add_argument("--light", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--no-ssim", action="store_true")
    a = ap.parse_args(argv)
    cfg = {}
    with open(a.config) as fh:
        for line in fh:
            line = line.split("#", 1)[0].strip()
            if "=" in line:
                k, v = line.split("=", 1)
                cfg[k.strip()] = v.strip()
    datadir = cfg.get("datadir", "")
    if not synth_dataset.is_synthetic(datadir):
        raise SystemExit(f"datadir = {datadir!r}: only the synthetic dataset spec (synthetic:views=N,res=R) can be built here; for another "
                         "dataset call tensoir_amd.metrics.evaluate(model, dataset) with the reference's loader")
    rotation = cfg.get("light_rotation", "000").replace("[", "").replace("]", "").replace(",", " ").split()
    ds = synth_dataset.SyntheticDataset(datadir, split="test", downsample=float(cfg.get("downsample_test", 1.0)), light_rotation=rotation)
    model = bake.load_model(a.ckpt, "cuda")
    num = lambda key, default, typ: typ(cfg.get(key, default))
    args = types.SimpleNamespace(second_nSample=num("second_nSample", 96, int), second_near=num("second_near", 0.05, float),
                                 second_far=num("second_far", 1.5, float))
    print(json.dumps(evaluate(model, ds, views=a.views, light_idx=a.light, chunk=a.chunk, args=args, ssim=not a.no_ssim)))


if __name__ == "__main__":
    main()
