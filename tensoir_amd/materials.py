"""Material editing: change albedo, roughness and the Fresnel term of selected surface rows between the primary pass and the
shading stage (relight.relight_chunk / relight_view, edits=...) or between the bake and the texture atlas (mesh.bake_atlas /
export_textured, edits=...).  The definition is the C header's ("Material editing"); tests/materials_reference.py
restates it in float64.

    from tensoir_amd import materials as mt
    pal = mt.palette(model, 4)                                   # the object's four materials, the largest first
    edits = mt.EditList([mt.MaterialEdit(palette_id=2, albedo_mode="recolor", color=mt.srgb_to_linear((30, 60, 200)),
                                         roughness_scale=0.0, roughness_offset=0.15, metallic=1.0)], palette=pal)
    view = relight.relight_view(model, env, ["city"], rays, H, W, edits=edits)
    mesh.export_textured(model, "edited.glb", edits=edits)

A MaterialEdit selects rows by a sphere, a box, a colour, a roughness band and / or a palette entry (the product of those given;
none: every row) and blends targets in with the weight strength x selection.  Colours are linear RGB.  Everything is validated when
the objects are built, before anything touches the device."""
from __future__ import annotations

import json
import math
import numbers
from typing import NamedTuple

import numpy as np
import torch

from . import ops

MAX_EDITS, EDIT_FLOATS, MAX_PALETTE = ops.MATERIAL_MAX_EDITS, ops.MATERIAL_EDIT_FLOATS, ops.MATERIAL_MAX_PALETTE
ALBEDO_MODES = ("keep", "set", "multiply", "recolor")
_SPHERE, _BOX, _COLOUR, _BAND, _PALETTE = 1, 2, 4, 8, 16


def srgb_to_linear(rgb):
    """An sRGB colour -- three numbers in 0..1, or three integers in 0..255 -- as the linear RGB triple the edits take."""
    v = [float(c) for c in rgb]
    if len(v) != 3:
        raise ValueError(f"srgb_to_linear: three components, got {rgb!r}")
    if all(isinstance(c, numbers.Integral) and not isinstance(c, bool) for c in rgb):
        v = [c / 255.0 for c in v]
    if not all(0.0 <= c <= 1.0 for c in v):
        raise ValueError(f"srgb_to_linear: components in 0..1 (or integers in 0..255), got {rgb!r}")
    return tuple(c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4 for c in v)


def _number(name, v, lo=None, hi=None):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"{name}: expected a finite number, got {v!r}")
    v = float(v)
    if (lo is not None and v < lo) or (hi is not None and v > hi):
        raise ValueError(f"{name}: expected a number in {'' if lo is None else lo} .. {'' if hi is None else hi}, got {v!r}")
    return v


def _triple(name, v, lo=None, hi=None):
    try:
        v = tuple(v)
    except TypeError:
        raise ValueError(f"{name}: expected three numbers, got {v!r}") from None
    if len(v) != 3:
        raise ValueError(f"{name}: expected three numbers, got {v!r}")
    return tuple(_number(f"{name}[{i}]", c, lo, hi) for i, c in enumerate(v))


class MaterialEdit:
    """One edit.  Keyword arguments only; what is left out is not selected on / not changed.
    Selectors (their product; every one reads the row's original position, albedo and roughness):
      sphere_center [3], sphere_radius >= 0, sphere_feather >= 0     world-space ball, fading out over `feather` beyond the radius
      box_center [3], box_half [3] >= 0, box_feather >= 0            axis-aligned box
      select_color [3] linear RGB, color_tolerance >= 0, color_feather >= 0      Euclidean distance of the albedo to a colour
      roughness_band (lo, hi), band_feather >= 0                     lo <= roughness <= hi
      palette_id                                                     the row's nearest entry of the EditList's palette
    Targets, blended in with w = strength x selection:
      albedo_mode "keep" | "set" | "multiply" | "recolor" with color [3] (linear; "multiply" takes any factors >= 0, the others
          0..1): "recolor" gives the colour's hue at the texture's own luminance
      roughness_scale, roughness_offset                              clamp(roughness scale + offset, 0.09, 0.99)
      metallic in 0..1                                               glTF's metallic-roughness model (None: not changed)
    strength in 0..1."""
    _FIELDS = ("strength", "sphere_center", "sphere_radius", "sphere_feather", "box_center", "box_half", "box_feather", "select_color",
               "color_tolerance", "color_feather", "roughness_band", "band_feather", "palette_id", "albedo_mode", "color",
               "roughness_scale", "roughness_offset", "metallic")
    _DEFAULTS = {"strength": 1.0, "sphere_feather": 0.0, "box_feather": 0.0, "color_tolerance": 0.0, "color_feather": 0.0,
                 "band_feather": 0.0, "albedo_mode": "keep", "roughness_scale": 1.0, "roughness_offset": 0.0}

    def __init__(self, *, strength=1.0, sphere_center=None, sphere_radius=None, sphere_feather=0.0, box_center=None, box_half=None,
                 box_feather=0.0, select_color=None, color_tolerance=0.0, color_feather=0.0, roughness_band=None, band_feather=0.0,
                 palette_id=None, albedo_mode="keep", color=None, roughness_scale=1.0, roughness_offset=0.0, metallic=None):
        self.strength = _number("strength", strength, 0.0, 1.0)
        if (sphere_center is None) != (sphere_radius is None):
            raise ValueError("sphere_center and sphere_radius come together")
        self.sphere_center = None if sphere_center is None else _triple("sphere_center", sphere_center)
        self.sphere_radius = None if sphere_radius is None else _number("sphere_radius", sphere_radius, 0.0)
        self.sphere_feather = _number("sphere_feather", sphere_feather, 0.0)
        if (box_center is None) != (box_half is None):
            raise ValueError("box_center and box_half come together")
        self.box_center = None if box_center is None else _triple("box_center", box_center)
        self.box_half = None if box_half is None else _triple("box_half", box_half, 0.0)
        self.box_feather = _number("box_feather", box_feather, 0.0)
        self.select_color = None if select_color is None else _triple("select_color", select_color)
        self.color_tolerance = _number("color_tolerance", color_tolerance, 0.0)
        self.color_feather = _number("color_feather", color_feather, 0.0)
        if roughness_band is not None:
            band = tuple(roughness_band) if isinstance(roughness_band, (tuple, list)) else ()
            if len(band) != 2:
                raise ValueError(f"roughness_band: expected (lo, hi), got {roughness_band!r}")
            roughness_band = (_number("roughness_band[0]", band[0]), _number("roughness_band[1]", band[1]))
            if roughness_band[0] > roughness_band[1]:
                raise ValueError(f"roughness_band: lo <= hi, got {roughness_band!r}")
        self.roughness_band = roughness_band
        self.band_feather = _number("band_feather", band_feather, 0.0)
        if palette_id is not None and (isinstance(palette_id, bool) or not isinstance(palette_id, numbers.Integral)
                                       or not 0 <= palette_id < MAX_PALETTE):
            raise ValueError(f"palette_id: expected an integer in 0 .. {MAX_PALETTE - 1}, got {palette_id!r}")
        self.palette_id = None if palette_id is None else int(palette_id)
        if albedo_mode not in ALBEDO_MODES:
            raise ValueError(f"albedo_mode: one of {ALBEDO_MODES}, got {albedo_mode!r}")
        self.albedo_mode = albedo_mode
        if (albedo_mode == "keep") != (color is None):
            raise ValueError('color comes with albedo_mode "set", "multiply" or "recolor", and only with them')
        self.color = None if color is None else _triple("color", color, 0.0, None if albedo_mode == "multiply" else 1.0)
        self.roughness_scale = _number("roughness_scale", roughness_scale)
        self.roughness_offset = _number("roughness_offset", roughness_offset)
        self.metallic = None if metallic is None else _number("metallic", metallic, 0.0, 1.0)

    def record(self):
        """The edit as the header's record: [32] float32."""
        r = np.zeros(EDIT_FLOATS, np.float32)
        sel = 0
        r[1] = self.strength
        if self.sphere_center is not None:
            sel |= _SPHERE
            r[2:5], r[5], r[6] = self.sphere_center, self.sphere_radius, self.sphere_feather
        if self.box_center is not None:
            sel |= _BOX
            r[7:10], r[10:13], r[13] = self.box_center, self.box_half, self.box_feather
        if self.select_color is not None:
            sel |= _COLOUR
            r[14:17], r[17], r[18] = self.select_color, self.color_tolerance, self.color_feather
        if self.roughness_band is not None:
            sel |= _BAND
            r[19:21], r[21] = self.roughness_band, self.band_feather
        if self.palette_id is not None:
            sel |= _PALETTE
            r[22] = self.palette_id
        r[0] = sel
        r[23] = ALBEDO_MODES.index(self.albedo_mode)
        if self.color is not None:
            r[24:27] = self.color
        r[27], r[28] = self.roughness_scale, self.roughness_offset
        if self.metallic is not None:
            r[29], r[30] = 1.0, self.metallic
        return r

    def to_json(self):
        """A plain dict of what differs from the defaults (lists for triples)."""
        out = {}
        for name in self._FIELDS:
            v = getattr(self, name)
            if v is None or (name in self._DEFAULTS and v == self._DEFAULTS[name]):
                continue
            out[name] = list(v) if isinstance(v, tuple) else v
        return out

    @classmethod
    def from_json(cls, d):
        if not isinstance(d, dict):
            raise ValueError(f"an edit is a dict of MaterialEdit's keywords, got {type(d).__name__}")
        unknown = sorted(set(d) - set(cls._FIELDS))
        if unknown:
            raise ValueError(f"unknown edit field(s) {unknown}; known: {list(cls._FIELDS)}")
        return cls(**d)

    def __eq__(self, other):
        return isinstance(other, MaterialEdit) and self.to_json() == other.to_json()

    def __repr__(self):
        return "MaterialEdit(" + ", ".join(f"{k}={v!r}" for k, v in self.to_json().items()) + ")"


class Palette(NamedTuple):
    """k materials found by k-means over (albedo, rough_weight x roughness), the largest first.  centroids [k, 4] float32, counts
    [k] int64, labels [N] int32 (device tensors; labels index the rows palette_of was given), inertia (float: the sum of squared
    distances of the last assignment), passes (Lloyd passes run), rough_weight."""
    centroids: torch.Tensor
    counts: torch.Tensor
    labels: torch.Tensor
    inertia: float
    passes: int
    rough_weight: float = 1.0

    def to_json(self):
        return {"centroids": [[float(v) for v in row] for row in self.centroids.detach().cpu().tolist()],
                "counts": [int(c) for c in self.counts.detach().cpu().tolist()], "rough_weight": float(self.rough_weight)}


def _palette_arg(palette):
    """None, a Palette, a dict (to_json's) or (centroids, rough_weight) -> (centroids [k, 4] float32 numpy, rough_weight) or None"""
    if palette is None:
        return None
    if isinstance(palette, Palette):
        cent, wr = palette.centroids.detach().cpu().numpy(), palette.rough_weight
    elif isinstance(palette, dict):
        if "centroids" not in palette:
            raise ValueError('palette: a dict carries "centroids" (and "rough_weight")')
        cent, wr = palette["centroids"], palette.get("rough_weight", 1.0)
    else:
        try:
            cent, wr = palette
        except (TypeError, ValueError):
            raise ValueError("palette: a Palette, its dict, or (centroids [k, 4], rough_weight)") from None
    cent = np.asarray(cent.detach().cpu().numpy() if torch.is_tensor(cent) else cent, np.float64)
    if cent.ndim != 2 or cent.shape[1] != 4 or not 1 <= cent.shape[0] <= MAX_PALETTE or not np.isfinite(cent).all():
        raise ValueError(f"palette: 1 .. {MAX_PALETTE} finite centroids [k, 4], got an array of shape {cent.shape}")
    return np.ascontiguousarray(cent, np.float32), _number("rough_weight", wr, 0.0)


class EditList:
    """0 .. 16 MaterialEdits, applied in order, with the palette their palette_id selectors refer to."""

    def __init__(self, edits=(), palette=None):
        edits = list(edits)
        if len(edits) > MAX_EDITS:
            raise ValueError(f"an edit list holds at most {MAX_EDITS} edits, got {len(edits)}")
        for e in edits:
            if not isinstance(e, MaterialEdit):
                raise TypeError(f"an edit list holds MaterialEdit objects, got {type(e).__name__}")
        self.edits = tuple(edits)
        pal = _palette_arg(palette)
        self.centroids, self.rough_weight = (None, 1.0) if pal is None else pal
        k = 0 if self.centroids is None else self.centroids.shape[0]
        for i, e in enumerate(self.edits):
            if e.palette_id is not None and e.palette_id >= k:
                raise ValueError(f"edit {i}: palette_id {e.palette_id} needs a palette of more than {e.palette_id} entries, "
                                 f"the list carries {k}")
        self._device = {}

    def __len__(self):
        return len(self.edits)

    def records(self):
        """[n, 32] float32, the header's records"""
        return np.stack([e.record() for e in self.edits]) if self.edits else np.zeros((0, EDIT_FLOATS), np.float32)

    def on(self, device):
        """(records, centroids or None) as tensors on `device`, uploaded once per device"""
        key = str(torch.device(device))
        if key not in self._device:
            rec = torch.from_numpy(self.records()).to(device)
            cent = None if self.centroids is None else torch.from_numpy(self.centroids).to(device)
            self._device[key] = (rec, cent)
        return self._device[key]

    def to_json(self):
        out = {"edits": [e.to_json() for e in self.edits]}
        if self.centroids is not None:
            out["palette"] = {"centroids": [[float(v) for v in row] for row in self.centroids.tolist()],
                              "rough_weight": float(self.rough_weight)}
        return out

    @classmethod
    def from_json(cls, d):
        if isinstance(d, str):
            d = json.loads(d)
        if isinstance(d, list):
            d = {"edits": d}
        if not isinstance(d, dict) or not isinstance(d.get("edits"), list) or set(d) - {"edits", "palette"}:
            raise ValueError('an edit list is {"edits": [...], "palette": {...}} or the list of edits alone')
        return cls([MaterialEdit.from_json(e) for e in d["edits"]], d.get("palette"))

    def __eq__(self, other):
        return isinstance(other, EditList) and self.to_json() == other.to_json()


def as_edit_list(edits):
    """None -> None; an EditList as it is; a list of MaterialEdits -> EditList."""
    if edits is None or isinstance(edits, EditList):
        return edits
    if isinstance(edits, (list, tuple)):
        return EditList(edits)
    raise TypeError(f"edits: None, an EditList or a list of MaterialEdit, got {type(edits).__name__}")


@torch.no_grad()
def apply(points, albedo, roughness, fresnel, edits, m_dev=None):
    """The edit list on M rows (points [M, 3] world space, albedo [M, 3], roughness [M] or [M, 1], fresnel [M, 3]; fp32 on the
    GPU), out of place -> dict(albedo = base (1 - metal), roughness, fresnel = f0 (1 - metal) + base metal, base, metal).
    Rows no edit selects, and all rows of an empty list, keep their bits (base = albedo, metal = 0)."""
    edits = as_edit_list(edits)
    if edits is None:
        edits = EditList()
    rec, cent = edits.on(albedo.device)
    return ops.material_edit(rec, cent, edits.rough_weight, points, albedo, roughness, fresnel, m_dev=m_dev)


@torch.no_grad()
def apply_to_maps(maps, rays, edits, acc_thres=0.5):
    """The edit list IN PLACE on the albedo, roughness and Fresnel columns of a chunk's primary map rows [B, 20] (what
    model(rays, light_idx, _return_maps=True) hands back) for the rows with acc > acc_thres; the position of a row is the surface
    point ops.surface_compact gives it.  -> maps."""
    edits = as_edit_list(edits)
    if edits is None or len(edits) == 0:
        return maps
    rec, cent = edits.on(maps.device)
    return ops.material_edit_maps(rec, cent, edits.rough_weight, maps, rays, acc_thres)


@torch.no_grad()
def palette_of(albedo, roughness, k, rough_weight=1.0, max_iters=50):
    """k materials of N surface rows (albedo [N, 3], roughness [N]; fp32 on the GPU) by deterministic k-means on (albedo,
    rough_weight x roughness): farthest-point seeding from row 0, then Lloyd passes (tir_kmeans_assign + tir_kmeans_update, one
    4-byte read-back per pass) until a pass changes no label or max_iters passes have run.  No floating-point atomics: two calls
    give identical bits.  -> Palette, entries ordered by count descending (the lower original index first among equals), labels
    renumbered with them: entry 0 is the largest material."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= MAX_PALETTE:
        raise ValueError(f"k: expected an integer in 1 .. {MAX_PALETTE}, got {k!r}")
    if isinstance(max_iters, bool) or not isinstance(max_iters, numbers.Integral) or max_iters < 1:
        raise ValueError(f"max_iters: expected an integer >= 1, got {max_iters!r}")
    wr = _number("rough_weight", rough_weight, 0.0)
    if not torch.is_tensor(albedo) or not torch.is_tensor(roughness) or albedo.dim() != 2 or albedo.shape[1] != 3 \
            or roughness.numel() != albedo.shape[0]:
        raise ValueError("palette_of: albedo [N, 3] and roughness [N] tensors")
    N = albedo.shape[0]
    if N < k:
        raise ValueError(f"palette_of: {N} rows cannot seed {k} clusters")
    albedo, roughness = ops.f32(albedo, "albedo", 3), ops.f32(roughness, "roughness").reshape(-1)
    if not bool(torch.isfinite(albedo).all()) or not bool(torch.isfinite(roughness).all()):
        raise ValueError("palette_of: albedo and roughness must be finite")
    dev, k = albedo.device, int(k)
    centroids = ops.kmeans_seed(albedo, roughness, k, wr)
    work = ops.kmeans_workspace(N, k, dev)
    labels = torch.empty((N,), dtype=torch.int32, device=dev)
    counts = torch.empty((k,), dtype=torch.int64, device=dev)
    inertia = torch.empty((1,), dtype=torch.float64, device=dev)
    changed = torch.empty((1,), dtype=torch.int32, device=dev)
    passes = 0
    for p in range(int(max_iters)):
        ops.kmeans_assign(albedo, roughness, centroids, labels, work, p == 0, wr)
        ops.kmeans_update(work, centroids, counts, inertia, changed)
        passes = p + 1
        if int(changed.item()) == 0:
            break
    host = counts.cpu().tolist()
    order = sorted(range(k), key=lambda c: (-host[c], c))                  # new index -> old index
    perm = torch.tensor(order, dtype=torch.int64, device=dev)
    rank = torch.empty((k,), dtype=torch.int32, device=dev)
    rank[perm] = torch.arange(k, dtype=torch.int32, device=dev)            # old index -> new index
    return Palette(centroids[perm].contiguous(), counts[perm].contiguous(), rank[labels.long()].contiguous(), float(inertia.item()),
                   passes, wr)


@torch.no_grad()
def surface_samples(model, samples=65536, seed=0, **mesh_kw):
    """Albedo and roughness at `samples` area-weighted points of the extracted surface: mesh.extract_mesh(**mesh_kw) ->
    ops.sample_surface -> bake.bake_points(lighting=False), the points the bake covers (coverage > 0.5) only.
    -> dict(points [n, 3] world space, albedo [n, 3], roughness [n])."""
    from . import bake, mesh
    grid = mesh._model_grid(model, mesh_kw.get("gridSize"))
    verts, faces, normals = mesh.extract_mesh(model, **mesh_kw)
    pts, face = ops.sample_surface(verts, faces, int(samples), int(seed))
    fn = normals[faces.long()[face.long()]].sum(dim=1)                  # the face's outward side: its vertex normals (index space)
    p, d = mesh.field_positions(model.aabb, grid, pts, fn / torch.linalg.norm(fn, dim=-1, keepdim=True).clamp(min=1e-20))
    b = bake.bake_points(model, p.contiguous(), d.contiguous(), lighting=False)
    keep = b["coverage"] > 0.5
    return {"points": b["surface"][keep].contiguous(), "albedo": b["albedo"][keep].contiguous(),
            "roughness": b["roughness"][keep].contiguous()}


@torch.no_grad()
def palette(model, k, samples=65536, seed=0, rough_weight=1.0, max_iters=50, **mesh_kw):
    """palette_of on surface_samples(model, samples, seed, **mesh_kw): "the k materials of this object", entry 0 the largest."""
    s = surface_samples(model, samples, seed, **mesh_kw)
    return palette_of(s["albedo"], s["roughness"], k, rough_weight, max_iters)
