"""Look at an exported asset: a deterministic z-buffer rasteriser of the mesh the exporters write (contract:
include/tensoir_hip.h, tir_raster_*), and the comparison of a textured GLB with the field it was baked from.

    out = render_mesh(pos, nrm, tan, uv, images, c2w, focal, H, W)        # device tensors, one row per pixel
    out = render_glb("scene.glb", c2w, focal, H, W, aabb=model.aabb, grid=model.gridSize)
    report = compare_asset(model, "scene.glb", n_views=8)                  # silhouette, albedo, roughness, normals, depth
    out = relight_glb("scene.glb", "city.hdr", c2w, focal, H, W)          # + "rgb": the asset under an environment
    report = compare_asset(model, "scene.glb", light="city.hdr")          # + relit_psnr: the same light on field and asset
    out = relight_glb("scene.glb", "city.hdr", c2w, focal, H, W, shadows=True)   # the mesh shadows itself: a shadow map per cell (4.10)
    report = compare_asset(model, "scene.glb", light="city.hdr", shadows=True)   # + shadow_agreement: the maps against the field's visibility
    out = relight_glb("scene.glb", "city.hdr", c2w, focal, H, W, shadows="traced")       # exact shadows: one any-hit ray per pair (4.17)
    report = compare_asset(model, "scene.glb", light="city.hdr", shadows="both")         # maps vs. field, traced vs. field, maps vs. traced

Camera: the datasets' convention.  Pixel (i, j) has its centre at (i + 0.5, j + 0.5) and the camera-space direction
((i + 0.5 - W/2) / f, (j + 0.5 - H/2) / f, 1); c2w [3, 4] has the columns x right, y down, z forward and the eye.  All per-corner
and per-pixel work runs in libtensoir_hip.so (ops.raster_*); there is no CPU path."""
from __future__ import annotations

import math
import os

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
    return _render(pos, nrm, tan, uv, images, c2w, focal, H, W, cull, raw, near)[0]


def _render(pos, nrm, tan, uv, images, c2w, focal, H, W, cull=True, raw=False, near=1e-3):
    """render_mesh -> (its dict, the [H, W, 12] G-buffer rows of tir_raster_shade the dict's entries are views of)."""
    pos = ops.f32(pos, "pos", 3).view(-1, 3)
    dev = pos.device
    rows, drops = ops.raster_project(pos, c2w, focal, H, W, near=near)
    keys = ops.raster_cover(rows, H, W, cull)
    face, bary, zc, pix = ops.raster_resolve(rows, keys)
    out = ops.raster_shade(pix, nrm, tan, uv, _device_images(images, dev), raw)
    depth = zc * torch.linalg.norm(_camera_dirs(focal, H, W, dev), dim=-1) * (face >= 0)
    return {"face": face, "bary": bary, "depth": depth, "albedo": out[..., 0:3], "roughness": out[..., 3], "ao": out[..., 4],
            "normal": out[..., 5:8], "coverage": out[..., 8], "drops": drops}, out


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


def _environment(hdr, device):
    """An environment map given as an array, a tensor or the path of a Radiance .hdr (or .npy) file -> float32 [H, W, 3] on device."""
    if isinstance(hdr, (str, bytes)) or hasattr(hdr, "__fspath__"):
        path = str(hdr)
        if path.endswith(".npy"):
            hdr = np.load(path)
        else:
            from .hdr import read_hdr
            hdr = read_hdr(path)
    t = torch.as_tensor(np.ascontiguousarray(hdr) if isinstance(hdr, np.ndarray) else hdr)
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"an environment map is [H, W, 3], got {tuple(t.shape)}")
    return ops.to_device(t.detach(), device, torch.float32).contiguous()


def environment_cells(hdr, rows=32, device="cuda"):
    """The light cells tir_light_gbuffer integrates: the equirectangular map hdr (array, tensor or .hdr path; row 0 at the top, as
    relight.Environment_Light reads it) reduced by solid-angle weighted means to rows x 2 rows cells (ops.env_cells) -> [2 rows^2,
    8] on the device.  ValueError when the map's sides are not multiples of the grid's."""
    rows = int(rows)
    if torch.is_tensor(hdr) and hdr.is_cuda:
        device = hdr.device
    env = _environment(hdr, device)
    if rows < 1 or env.shape[0] % rows or env.shape[1] % (2 * rows):
        raise ValueError(f"environment_cells: a {env.shape[0]} x {env.shape[1]} map does not divide into {rows} x {2 * rows} cells")
    return ops.env_cells(env, rows, 2 * rows)


def _tone_map(x):
    """linear2srgb of models/relight_utils.py:489-515 (what TIR_LIGHT_SRGB applies), for the background pixels."""
    x = x.clamp(0.0, 1.0)
    return torch.where(x <= 0.0031308, x * 12.92, 1.055 * torch.pow(x + 1e-6, 1.0 / 2.4) - 0.055)


SHADOW_BIAS = (0.5, 1.0)         # (constant, slope) in texels: the smallest candidate that passes both criteria of DESIGN 4.10
SHADOW_MAX_BYTES = 4 << 30


def mesh_bounds(pos):
    """The sphere the shadow frames are laid round: -> (centre (x, y, z), radius) as host floats; the centre is the middle of the
    positions' box, the radius half its diagonal times 1 + 1/64 (no silhouette touches a map's edge).  One aminmax on the device."""
    pos = ops.f32(pos, "pos", 3).view(-1, 3)
    if pos.shape[0] < 1:
        raise ValueError("mesh_bounds: no positions")
    lo, hi = torch.aminmax(pos, dim=0)
    box = torch.stack([lo, hi]).to("cpu", torch.float64).numpy()
    return tuple(float(x) for x in 0.5 * (box[0] + box[1])), 0.5 * float(np.linalg.norm(box[1] - box[0])) * (1.0 + 1.0 / 64.0)


def shadow_maps_for(pos, cells, S=256):
    """The shadow maps of the mesh pos [3F, 3] under the light cells [D, 8] (environment_cells): one S x S orthographic z-buffer per
    cell round mesh_bounds(pos) -> (frames [D, 12], maps [D, S, S]), what relight_mesh(shadows=True, shadow_maps=...) and
    ops.shadow_lookup take.  They depend on the mesh and the cells only: build them once for all views.  ValueError when the maps
    would exceed 4 GiB."""
    D, S = int(cells.shape[0]), int(S)
    if D * S * S * 4 > SHADOW_MAX_BYTES:
        raise ValueError(f"shadow maps of {D} cells at shadow_size {S} take {D * S * S * 4 / 2 ** 30:.1f} GiB (limit 4): lower "
                         f"shadow_size, or rows (the light cells are rows x 2 rows)")
    centre, radius = mesh_bounds(pos)
    if not radius > 0:
        raise ValueError("shadow_maps_for: the mesh has no extent")
    frames = ops.shadow_frames(cells, centre, radius, S)
    return frames, ops.shadow_maps(pos, frames, S)[0]


SHADOW_EPS = 1e-2                # traced shadows start at t0 = SHADOW_EPS x the radius of mesh_bounds: the rule of DESIGN 4.17
SHADOW_METHODS = {None: None, False: None, True: "maps", "maps": "maps", "traced": "traced"}


def _shadow_method(shadows, extra=()):
    """shadows -> None (no shadows), "maps" (True), "traced", or one of `extra` as it is."""
    if isinstance(shadows, str) and shadows in extra:
        return shadows
    try:
        return SHADOW_METHODS[shadows]
    except (KeyError, TypeError):
        raise ValueError(f"shadows is one of False, True, {', '.join(repr(k) for k in ('maps', 'traced') + tuple(extra))}") from None


def shadow_grid_for(pos, faces=None):
    """The mesh and its face grid as traced shadows take them: pos [3F, 3] (unwelded: faces = arange) or verts [V, 3] with faces
    [F, 3] int32 -> (verts, faces, grid = ops.face_grid(verts, faces)), what relight_mesh(shadows="traced", shadow_grid=...) takes.
    It depends on the mesh only: build it once for all views and lights."""
    pos = ops.f32(pos, "pos", 3).view(-1, 3)
    if faces is None:
        if pos.shape[0] % 3:
            raise ValueError("an unwelded mesh takes three rows of pos per face")
        faces = torch.arange(pos.shape[0], dtype=torch.int32, device=pos.device).view(-1, 3)
    faces = ops.i32(faces, "faces").view(-1, 3)
    return pos, faces, ops.face_grid(pos, faces)


def traced_occlusion(pts, nrm, cells, shadow_grid, radius, shadow_eps=SHADOW_EPS):
    """ops.shadow_trace of the rows pts, nrm [M, 3] against shadow_grid = (verts, faces, grid), rays starting at t0 = shadow_eps x
    radius (of mesh_bounds) -> occl [D, ceil(M / 64)].  The rows are not compacted: an empty pixel's normal is zero, its pairs do
    not contribute, and a wave of such rows skips the walk."""
    shadow_eps = float(shadow_eps)
    if not (shadow_eps >= 0.0 and math.isfinite(shadow_eps)):
        raise ValueError("shadow_eps is finite and >= 0")
    verts, faces, grid = shadow_grid
    return ops.shadow_trace(pts, nrm, cells, verts, faces, grid, shadow_eps * float(radius))


@torch.no_grad()
def relight_mesh(pos, nrm, tan, uv, images, cells, c2w, focal, H, W, hdr=None, occlusion=True, srgb=True, fresnel=0.04, shadows=False,
                 shadow_size=256, shadow_bias=SHADOW_BIAS, shadow_maps=None, shadow_eps=SHADOW_EPS, shadow_grid=None, **render_kw):
    """render_mesh, then what a glTF viewer does after the texture lookups: every covered pixel's albedo, roughness and normal
    lit by the light cells (environment_cells) through albedo / pi + GGX_specular, the pixel's ray reversed as the view vector
    (ops.light_gbuffer: one pass over the G-buffer, no indirect light) -> render_mesh's dict plus "rgb" [H, W, 3].
    occlusion: times the baked ambient occlusion; srgb: tone-mapped; fresnel: the scalar F0.  hdr (the [H, W, 3] map the cells
    were made from, on the device): empty pixels show the environment behind them (ops.env_lookup, tone-mapped the same way);
    without it they are zeros.
    shadows (default False: no shadows, every number as before): a cell lights a pixel only where the mesh does not stand between
    them, by one shadow_size x shadow_size shadow map per cell (hard shadows, nearest texel, shadow_bias = (constant,
    slope) in texels).  The pixel's surface point is the ray's origin + depth x its unit direction.  shadow_maps: the (frames,
    maps) of shadow_maps_for(pos, cells, shadow_size), for a caller who renders many views; by default they are built here.
    shadows="maps" is shadows=True.  shadows="traced" (DESIGN 4.17): no maps; one exact any-hit ray per (pixel, cell) pair from the
    pixel's surface point towards the cell over the mesh's face grid (ops.shadow_trace), starting at t0 = shadow_eps x the radius
    of mesh_bounds(pos); no bias in texels, no memory that grows with the cells.  shadow_grid: shadow_grid_for(pos), for a caller
    who renders many views; by default it is built here."""
    method = _shadow_method(shadows)
    out, gbuf = _render(pos, nrm, tan, uv, images, c2w, focal, H, W, **render_kw)
    rays = camera_rays(c2w, focal, H, W, gbuf.device)
    if method == "maps":
        frames, maps = shadow_maps_for(pos, cells, shadow_size) if shadow_maps is None else shadow_maps
        pts = rays[:, 0:3] + out["depth"].reshape(-1, 1) * rays[:, 3:6]
        lit = ops.light_gbuffer_shadowed(gbuf.view(-1, ops.RASTER_ROW), -rays[:, 3:6], cells, pts, frames, maps, shadow_bias, fresnel,
                                         occlusion, srgb)
    elif method == "traced":
        sgrid = shadow_grid_for(pos) if shadow_grid is None else shadow_grid
        pts = rays[:, 0:3] + out["depth"].reshape(-1, 1) * rays[:, 3:6]
        occl = traced_occlusion(pts, out["normal"].reshape(-1, 3), cells, sgrid, mesh_bounds(pos)[1], shadow_eps)
        lit = ops.light_gbuffer_occluded(gbuf.view(-1, ops.RASTER_ROW), -rays[:, 3:6], cells, occl, fresnel, occlusion, srgb)
    else:
        lit = ops.light_gbuffer(gbuf.view(-1, ops.RASTER_ROW), -rays[:, 3:6], cells, fresnel, occlusion, srgb)
    rgb = lit[:, 0:3]
    if hdr is not None:
        back = ops.env_lookup(_environment(hdr, gbuf.device), rays[:, 3:6].contiguous())
        rgb = torch.where(lit[:, 3:4] > 0, rgb, _tone_map(back) if srgb else back)
    out["rgb"] = rgb.reshape(H, W, 3)
    return out


def relight_glb(path, hdr, c2w, focal, H, W, rows=32, aabb=None, grid=None, device="cuda", background=True, **kw):
    """relight_mesh of a file written by mesh.export_textured under the environment hdr (array, tensor or .hdr path) reduced to
    rows x 2 rows cells; background=False leaves the empty pixels black.  aabb, grid: as render_glb.  shadows (False, True /
    "maps", "traced"), shadow_size, shadow_bias, shadow_eps, shadow_grid (and everything else of relight_mesh) pass through."""
    env = _environment(hdr, device)
    return relight_mesh(*load_glb(path, aabb, grid, device), environment_cells(env, rows), c2w, focal, H, W,
                        hdr=env if background else None, **kw)


def field_gbuffer(ret, n):
    """The field's maps of one view as G-buffer rows [n, 12]: albedo, roughness, ao = 1, the normalised normal_map, coverage =
    acc_map > 0.5."""
    g = torch.zeros((n, ops.RASTER_ROW), dtype=torch.float32, device=ret["acc_map"].device)
    g[:, 0:3] = ret["albedo_map"].reshape(n, 3)
    g[:, 3] = ret["roughness_map"].reshape(n)
    g[:, 4] = 1.0
    g[:, 5:8] = torch.nn.functional.normalize(ret["normal_map"].reshape(n, 3), dim=-1)
    g[:, 8] = (ret["acc_map"].reshape(n) > 0.5).to(torch.float32)
    return g


def relit_psnr(gbuf_a, gbuf_b, view, cells, fresnel=0.04, images=None):
    """Two G-buffers [n, 12] of the same pixels lit by the same cells from the same view vectors (no occlusion, tone-mapped) ->
    the PSNR in dB over the pixels covered in both (inf when the images agree there, nan when there are none).  images (a list)
    receives the two [n, 3] images."""
    lit = [ops.light_gbuffer(g, view, cells, float(fresnel), False, True) for g in (gbuf_a, gbuf_b)]
    if images is not None:
        images.extend(x[:, 0:3] for x in lit)
    both = (lit[0][:, 3] > 0) & (lit[1][:, 3] > 0)
    if not bool(both.any()):
        return float("nan")
    mse = float(((lit[0][both, 0:3] - lit[1][both, 0:3]).double() ** 2).mean())
    return -10.0 * math.log10(mse) if mse > 0 else float("inf")


def _contributing_codes(pts, nrm, cells):
    """ops.shadow_lookup against empty 1 x 1 maps -> codes [M, D] uint8: 2 where the pair contributes (n.L > 1e-6 exactly as the
    lighting kernels form it), 0 elsewhere."""
    D = cells.shape[0]
    frames = torch.zeros((D, 12), dtype=torch.float32, device=cells.device)
    return ops.shadow_lookup(pts, nrm, cells, frames, torch.zeros((D, 1, 1), dtype=torch.int32, device=cells.device))


def _shadow_agreement(model, relight, args, rays, field_depth, asset, both, cells, smaps, max_pixels, traced=None):
    """compare_asset's shadow agreements of one view: rays [n, 6], field_depth [n], the asset's render dict, both [n] bool; smaps
    = (frames, maps) or None; traced = (shadow_grid, radius, shadow_eps) or None -> {"maps": maps vs. field, "traced": traced vs.
    field, "maps_traced": maps vs. traced} for what was asked, each over the pairs that contribute on the asset side."""
    names = (("maps",) if smaps is not None else ()) + (("traced",) if traced is not None else ()) + \
            (("maps_traced",) if smaps is not None and traced is not None else ())
    idx = torch.nonzero(both).reshape(-1)
    if idx.numel() == 0:
        return {k: float("nan") for k in names}
    idx = idx[::max(1, -(-idx.numel() // max(max_pixels, 1)))]                  # a fixed stride: no random numbers
    o, d = rays[idx, 0:3], rays[idx, 3:6]
    D = cells.shape[0]
    apts, anrm = o + asset["depth"].reshape(-1, 1)[idx] * d, asset["normal"].reshape(-1, 3)[idx]
    codes = ops.shadow_lookup(apts, anrm, cells, *smaps, SHADOW_BIAS) if smaps is not None else _contributing_codes(apts, anrm, cells)
    pts = (o + field_depth.reshape(-1, 1)[idx] * d).repeat_interleave(D, dim=0)
    L = torch.nn.functional.normalize(cells[:, 0:3], dim=-1).repeat(idx.numel(), 1)
    vis = relight.compute_transmittance(model, pts, L, nSample=args.second_nSample, vis_near=args.second_near, vis_far=args.second_far)[0]
    field_lit = vis.reshape(idx.numel(), D) > 0.5
    on = codes != 0
    n = int(on.sum())
    share = lambda a, b: float((a == b)[on].sum()) / n if n else float("nan")
    out = {}
    if smaps is not None:
        out["maps"] = share(codes == 2, field_lit)
    if traced is not None:
        sgrid, radius, eps = traced
        traced_lit = ~ops.occlusion_bits(traced_occlusion(apts, anrm, cells, sgrid, radius, eps), idx.numel())
        out["traced"] = share(traced_lit, field_lit)
        if smaps is not None:
            out["maps_traced"] = share(codes == 2, traced_lit)
    return out


def _write_view(path, rgb):
    from . import mesh
    a = torch.cat([rgb.clamp(0, 1), torch.ones_like(rgb[..., :1])], -1)
    with open(path, "wb") as fh:
        fh.write(mesh.write_png((a * 255.0 + 0.5).to(torch.uint8)))


def _mean(values):
    return float(np.mean(values)) if len(values) else float("nan")


@torch.no_grad()
def compare_asset(model, path, cameras=None, H=200, W=200, focal=None, n_views=8, grid=None, args=None, chunk=16384, light=None,
                  light_rows=16, write_views=None, shadows=False, shadow_size=256, shadow_pixels=4096, ssim=False, shadow_eps=SHADOW_EPS):
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
    light (an environment map: array, tensor, .hdr or .npy path; default None: the report is exactly the one above) adds
      relit_psnr      dB between the field's and the asset's image under that environment, over the pixels in both silhouettes:
                      the field's albedo_map, roughness_map, normalised normal_map and acc_map > 0.5 are packed into G-buffer
                      rows with ao = 1, and BOTH G-buffers go through ops.light_gbuffer with the same light_rows x 2 light_rows
                      cells, the pixel's reversed ray as view, fresnel = model.fixed_fresnel, no occlusion, tone-mapped.  The
                      same estimator on both sides: the number isolates what the baked albedo, roughness and normal errors do
                      to a lit image, free of sampling noise and of shadows (which the file does not carry).  The field's own
                      shadowed relight is relight.relight_chunk; this check does not replace it.
    shadows (with light; default False: the report is exactly the one above) adds
      shadow_agreement  the share of (pixel, light cell) pairs on which the asset's shadow maps (shadow_maps_for at shadow_size,
                      SHADOW_BIAS) and the field's own visibility agree.  Up to shadow_pixels pixels of those in both silhouettes,
                      taken by a fixed stride.  Asset side: ops.shadow_lookup at the asset's surface points and shading normals.
                      Field side: relight.compute_transmittance(model, ray origin + depth_map x direction, L, args' second_nSample,
                      second_near, second_far) > 0.5 means lit.  Counted over the pairs that contribute on the asset side (n.L >
                      1e-6); nan when there are none.  Every other number is what it is without shadows: relit_psnr stays the
                      unshadowed comparison.
    shadows="maps" is shadows=True.  shadows="traced"  makes shadow_agreement the TRACED visibility of the asset
    (ops.shadow_trace over its face grid, rays from t0 = shadow_eps x the radius of mesh_bounds) against the same march of the
    field: the same pixels, the same field side, the same definition.  shadows="both" reports
      shadow_agreement         the maps against the field: the number of shadows=True, bit for bit
      shadow_agreement_traced  the traced visibility against the field
      shadow_map_agreement     the maps against the traced visibility, over the pairs that contribute on the asset side: what the
                      shadow map's bias and aliasing cost, free of the field
    ssim (default False: the report is exactly the one above) adds
      albedo_ssim     metrics.ssim (the reference's rgb_ssim, max_val 1) of the field's albedo_map against the asset's albedo over
                      the whole frame, both set to 0 outside the pixels in both silhouettes: the one structural number of the report
    write_views (a directory, with light): every view's two images as view_KK_field.png / view_KK_asset.png, and with shadows
    the asset under its own shadows as view_KK_asset_shadowed.png (maps) and view_KK_asset_traced.png (traced).
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
    cells = None if light is None else environment_cells(_environment(light, dev), light_rows)
    if write_views is not None:
        if light is None:
            raise ValueError("write_views writes the lit images: it needs light")
        os.makedirs(write_views, exist_ok=True)
    smaps = traced = None
    method = _shadow_method(shadows, ("both",))
    if method is not None:
        if cells is None:
            raise ValueError("shadows compares the shadows of a light: it needs light")
        from . import relight
        if method in ("maps", "both"):
            smaps = shadow_maps_for(asset[0], cells, shadow_size)
        if method in ("traced", "both"):
            traced = (shadow_grid_for(asset[0]), mesh_bounds(asset[0])[1], shadow_eps)
    skeys = {"maps": (("shadow_agreement", "maps"),), "traced": (("shadow_agreement", "traced"),),
             "both": (("shadow_agreement", "maps"), ("shadow_agreement_traced", "traced"), ("shadow_map_agreement", "maps_traced"))}.get(method, ())
    views = []
    for k, c2w in enumerate(cameras):
        rays = camera_rays(c2w, focal, H, W, dev)
        lidx = torch.zeros((rays.shape[0], 1), dtype=torch.int32, device=dev)
        parts = [Renderer_TensoIR_train(rays[a:a + chunk], None, lidx[a:a + chunk], model, N_samples=-1, white_bg=False, is_train=False,
                                        is_relight=True, sample_method="fixed_envirmap", device=dev, args=args, _no_graph=True)
                 for a in range(0, rays.shape[0], int(chunk))]
        ret = {k: torch.cat([p[k].reshape(p["acc_map"].shape[0], -1) for p in parts]) for k in FIELD_MAPS}
        a, gbuf = _render(*asset, c2w, focal, H, W)
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
        if ssim:
            from . import metrics
            keep = both[..., None].to(torch.float32)
            v["albedo_ssim"] = float(metrics.ssim(ret["albedo_map"].reshape(H, W, 3) * keep, a["albedo"] * keep))
        if cells is not None:
            lit = []
            v["relit_psnr"] = relit_psnr(field_gbuffer(ret, H * W), gbuf.view(-1, ops.RASTER_ROW), (-rays[:, 3:6]).contiguous(), cells,
                                         model.fixed_fresnel, lit)
            if write_views is not None:
                for name, img in zip(("field", "asset"), lit):
                    _write_view(os.path.join(write_views, f"view_{k:02d}_{name}.png"), img.reshape(H, W, 3))
        if method is not None:
            agree = _shadow_agreement(model, relight, args, rays, ret["depth_map"].reshape(-1), a, both.reshape(-1), cells, smaps,
                                      int(shadow_pixels), traced)
            v.update({name: agree[which] for name, which in skeys})
            if write_views is not None:
                pts = rays[:, 0:3] + a["depth"].reshape(-1, 1) * rays[:, 3:6]
                view = (-rays[:, 3:6]).contiguous()
                if smaps is not None:
                    img = ops.light_gbuffer_shadowed(gbuf.view(-1, ops.RASTER_ROW), view, cells, pts, *smaps, SHADOW_BIAS,
                                                     float(model.fixed_fresnel), False, True)
                    _write_view(os.path.join(write_views, f"view_{k:02d}_asset_shadowed.png"), img[:, 0:3].reshape(H, W, 3))
                if traced is not None:
                    occl = traced_occlusion(pts, a["normal"].reshape(-1, 3), cells, *traced)
                    img = ops.light_gbuffer_occluded(gbuf.view(-1, ops.RASTER_ROW), view, cells, occl, float(model.fixed_fresnel), False, True)
                    _write_view(os.path.join(write_views, f"view_{k:02d}_asset_traced.png"), img[:, 0:3].reshape(H, W, 3))
        views.append(v)
    keys = ("iou", "pixels", "albedo_psnr", "roughness_rmse", "normal_deg", "depth_rmse") + (() if cells is None else ("relit_psnr",)) + \
           tuple(name for name, _ in skeys) + (("albedo_ssim",) if ssim else ())
    mean = {k: _mean([v[k] for v in views if math.isfinite(v[k])]) for k in keys}
    return {"views": views, "mean": mean, "H": int(H), "W": int(W), "focal": float(focal), "n_views": len(views)}
