"""Look at an exported asset: a deterministic z-buffer rasteriser of the mesh the exporters write (contract:
include/tensoir_hip.h, tir_raster_*), and the comparison of a textured GLB with the field it was baked from.

    out = render_mesh(pos, nrm, tan, uv, images, c2w, focal, H, W)        # device tensors, one row per pixel
    out = render_glb("scene.glb", c2w, focal, H, W, aabb=model.aabb, grid=model.gridSize)
    report = compare_asset(model, "scene.glb", n_views=8)                  # silhouette, albedo, roughness, normals, depth

Camera: the datasets' convention.  Pixel (i, j) has its centre at (i + 0.5, j + 0.5) and the camera-space direction
((i + 0.5 - W/2) / f, (j + 0.5 - H/2) / f, 1); c2w [3, 4] has the columns x right, y down, z forward and the eye.  All per-corner
and per-pixel work runs in libtensoir_hip.so (ops.raster_*); there is no CPU path."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops

IMAGE_NAMES = ("base", "orm", "normal")
FIELD_MAPS = ("acc_map", "albedo_map", "roughness_map", "normal_map", "depth_map")      # what compare_asset reads of the field's render


def _camera_dirs(focal, H, W, device):
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=device), torch.arange(W, dtype=torch.float32, device=device),
                          indexing="ij")
    return torch.stack([(i + 0.5 - W / 2) / float(focal), (j + 0.5 - H / 2) / float(focal), torch.ones_like(i)], -1)


def camera_rays(c2w, focal, H, W, device=None):
    """The [H * W, 6] rays (origin, unit direction) of exactly the pixels render_mesh rasterises, row-major from the top left:
    the camera-space directions above rotated by c2w[:, :3] and normalised, as the datasets store them."""
    c2w = torch.as_tensor(c2w, dtype=torch.float32).reshape(3, 4)
    device = c2w.device if device is None else device
    c2w = c2w.to(device)
    d = _camera_dirs(focal, H, W, device).reshape(-1, 3) @ c2w[:, :3].T
    d = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    return torch.cat([c2w[:, 3].expand_as(d), d], 1).contiguous()


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """c2w [3, 4] float64 numpy of a camera at eye looking at target: z = normalize(target - eye), x = normalize(z x up),
    y = z x x."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.cross(z, up)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z, eye], 1)


def orbit_cameras(aabb, n, elevation_deg=20, distance=None):
    """n look-at poses [n, 3, 4] (float32, host) on a ring round the centre of the box aabb [2, 3], at elevation_deg above its
    x-y plane and `distance` from the centre (default: twice the box diagonal), world up +z."""
    box = torch.as_tensor(aabb).detach().to("cpu", torch.float64).reshape(2, 3).numpy()
    centre = 0.5 * (box[0] + box[1])
    dist = 2.0 * float(np.linalg.norm(box[1] - box[0])) if distance is None else float(distance)
    el = math.radians(float(elevation_deg))
    if int(n) < 1 or not dist > 0 or not abs(el) < math.pi / 2:
        raise ValueError("orbit_cameras: n >= 1, distance > 0 and |elevation| < 90 degrees")
    poses = []
    for k in range(int(n)):
        az = 2 * math.pi * k / int(n)
        eye = centre + dist * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        poses.append(look_at(eye, centre))
    return torch.from_numpy(np.stack(poses)).to(torch.float32)


def _device_images(images, device):
    if images is None:
        return None
    if sorted(images) != sorted(IMAGE_NAMES):
        raise ValueError(f"images takes {IMAGE_NAMES}")
    return [torch.as_tensor(np.ascontiguousarray(images[k]) if isinstance(images[k], np.ndarray) else images[k]).to(device).contiguous()
            for k in IMAGE_NAMES]


@torch.no_grad()
def render_mesh(pos, nrm, tan, uv, images, c2w, focal, H, W, cull=True, raw=False, near=1e-3):
    """Rasterise the unwelded mesh pos / nrm [3F, 3], tan [3F, 4], uv [3F, 2] (device float32; corner 3 f + k, as write_glb
    writes it) with the textures images = {"base", "orm", "normal": [S, S, 4] uint8}, or geometry only with images (and tan,
    uv) None.  -> dict of device tensors: face [H, W] int32 (-1 = empty), bary [H, W, 2] (b1, b2), depth [H, W] (the distance
    along the pixel's unit ray, comparable with depth_map; 0 where empty), albedo [H, W, 3] (linear; the bytes / 255 with
    raw=True), roughness, ao, coverage [H, W], normal [H, W, 3], and "drops", the faces project left out.
    cull: draw front faces only (outward-oriented meshes).  No clipping: a face with a corner at Z <= near is dropped."""
    pos = ops.f32(pos, "pos", 3).view(-1, 3)
    dev = pos.device
    rows, drops = ops.raster_project(pos, c2w, focal, H, W, near=near)
    keys = ops.raster_cover(rows, H, W, cull)
    face, bary, zc, pix = ops.raster_resolve(rows, keys)
    out = ops.raster_shade(pix, nrm, tan, uv, _device_images(images, dev), raw)
    depth = zc * torch.linalg.norm(_camera_dirs(focal, H, W, dev), dim=-1) * (face >= 0)
    return {"face": face, "bary": bary, "depth": depth, "albedo": out[..., 0:3], "roughness": out[..., 3], "ao": out[..., 4],
            "normal": out[..., 5:8], "coverage": out[..., 8], "drops": drops}


def render_glb(path, c2w, focal, H, W, aabb=None, grid=None, device="cuda", **kw):
    """render_mesh of a file written by mesh.export_textured.  With aabb and grid (the field's box and the export's lattice) the
    positions are first mapped by mesh.field_positions: the file keeps the reference's voxel-size quirk, the field
    does not."""
    return render_mesh(*load_glb(path, aabb, grid, device), c2w, focal, H, W, **kw)


def load_glb(path, aabb=None, grid=None, device="cuda"):
    """mesh.read_glb on the device -> (pos, nrm, tan, uv, images), render_mesh's first arguments; pos mapped to field coordinates
    when aabb and grid are given."""
    from . import mesh
    if (aabb is None) != (grid is None):
        raise ValueError("aabb and grid go together")
    g = mesh.read_glb(path)
    pos = torch.from_numpy(g["pos"]).to(device)
    if aabb is not None:
        pos = mesh.field_positions(aabb, [int(x) for x in grid], pos).contiguous()
    nrm, tan, uv = (torch.from_numpy(g[k]).to(device) for k in ("nrm", "tan", "uv"))
    return pos, nrm, tan, uv, dict(zip(IMAGE_NAMES, _device_images(g["images"], device)))


def _mean(values):
    return float(np.mean(values)) if len(values) else float("nan")


@torch.no_grad()
def compare_asset(model, path, cameras=None, H=200, W=200, focal=None, n_views=8, grid=None, args=None, chunk=16384):
    """Render the field (Renderer_TensoIR_train under its own first light -- no novel illumination --, no white background,
    `chunk` rays per call) and the asset at `path` (render_glb, mapped to field coordinates with the lattice `grid`, default the
    model's gridSize) from the same cameras.  The renderer decodes albedo, roughness and normals only with is_relight=True, which
    also runs its physically based re-render: `args` carries that pass's second_nSample / second_near / second_far (default 96,
    0.05, 1.5); its image is not used.  -> report
    {"views": [per view {...}], "mean": {...}, "H", "W", "focal", "n_views"} of plain floats:
      iou             silhouette: acc_map > 0.5 against the asset's coverage
      albedo_psnr     dB, over the pixels in both silhouettes (as are the following)
      roughness_rmse
      normal_deg      mean angle between normal_map and the asset's shading normal
      depth_rmse      in units of the model's stepSize
      pixels          how many pixels lie in both
    cameras: [n, 3, 4]; default orbit_cameras(model.aabb, n_views) at the middle of the model's near / far range, with a focal
    length that fits the box into 90 % of the image."""
    import types
    from .renderer import Renderer_TensoIR_train
    if args is None:
        args = types.SimpleNamespace(second_nSample=96, second_near=0.05, second_far=1.5)
    dev = model.aabb.device
    box = model.aabb.detach().to("cpu", torch.float64)
    radius = 0.5 * float(torch.linalg.norm(box[1] - box[0]))
    if cameras is None:
        dist = 0.5 * (float(model.near_far[0]) + float(model.near_far[1]))
        cameras = orbit_cameras(box, n_views, distance=dist)
    cameras = torch.as_tensor(cameras, dtype=torch.float32).reshape(-1, 3, 4).cpu()
    if focal is None:
        d = float(torch.linalg.norm(cameras[0, :, 3].to(torch.float64) - 0.5 * (box[0] + box[1])))
        focal = 0.45 * min(H, W) * d / radius
    grid = [int(g) for g in (model.gridSize if grid is None else grid)]
    step = float(model.stepSize)
    asset = load_glb(path, model.aabb, grid, dev)                      # read and decoded once for all views
    views = []
    for c2w in cameras:
        rays = camera_rays(c2w, focal, H, W, dev)
        lidx = torch.zeros((rays.shape[0], 1), dtype=torch.int32, device=dev)
        parts = [Renderer_TensoIR_train(rays[a:a + chunk], None, lidx[a:a + chunk], model, N_samples=-1, white_bg=False, is_train=False,
                                        is_relight=True, sample_method="fixed_envirmap", device=dev, args=args, _no_graph=True)
                 for a in range(0, rays.shape[0], int(chunk))]
        ret = {k: torch.cat([p[k].reshape(p["acc_map"].shape[0], -1) for p in parts]) for k in FIELD_MAPS}
        a = render_mesh(*asset, c2w, focal, H, W)
        fld = ret["acc_map"].reshape(H, W) > 0.5
        ast = a["coverage"] > 0.5
        both = fld & ast
        n = int(both.sum())
        union = int((fld | ast).sum())
        v = {"iou": n / union if union else float("nan"), "pixels": float(n)}
        if n:
            al = (ret["albedo_map"].reshape(H, W, 3)[both] - a["albedo"][both]).double()
            mse = float((al ** 2).mean())
            v["albedo_psnr"] = -10.0 * math.log10(mse) if mse > 0 else float("inf")
            v["roughness_rmse"] = float(((ret["roughness_map"].reshape(H, W)[both] - a["roughness"][both]).double() ** 2).mean().sqrt())
            nf = torch.nn.functional.normalize(ret["normal_map"].reshape(H, W, 3)[both].double(), dim=-1)
            cos = (nf * a["normal"][both].double()).sum(-1).clamp(-1, 1)
            v["normal_deg"] = float(torch.rad2deg(torch.acos(cos)).mean())
            v["depth_rmse"] = float((((ret["depth_map"].reshape(H, W)[both] - a["depth"][both]).double() / step) ** 2).mean().sqrt())
        else:
            v.update({k: float("nan") for k in ("albedo_psnr", "roughness_rmse", "normal_deg", "depth_rmse")})
        views.append(v)
    keys = ("iou", "pixels", "albedo_psnr", "roughness_rmse", "normal_deg", "depth_rmse")
    mean = {k: _mean([v[k] for v in views if math.isfinite(v[k])]) for k in keys}
    return {"views": views, "mean": mean, "H": int(H), "W": int(W), "focal": float(focal), "n_views": len(views)}
