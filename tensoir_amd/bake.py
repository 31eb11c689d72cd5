"""Per-point bake of what the field has recovered: albedo, roughness, shading normal, coverage and (optionally) ambient
occlusion and direct irradiance under one of the model's lights, evaluated at surface points -- the vertices of the exported mesh
(mesh.export_mesh(..., attributes=True)) or any other point set.

    out = bake_points(model, points, outward)          # device tensors, one row per point
    python -m tensoir_amd.bake CKPT OUT.ply [--grid N] [--level L] [--color albedo|diffuse] [--light K]
    python -m tensoir_amd.bake CKPT OUT.glb --texture-size N [...]     # the same bake at every texel of an atlas (mesh.export_textured)
    python -m tensoir_amd.bake CKPT OUT.glb --texture-size N --check-views V [--check-size S]   # + raster.compare_asset, one JSON line
    ... --check-views V --check-light NAME|FILE.hdr|FILE.npy [--check-light-rows R] [--write-views DIR]   # + relit_psnr
    ... --check-light ... --check-shadows [--shadow-size S]   # + shadow_agreement: the mesh's shadow maps against the field's visibility (4.10)
    ... --check-shadows --shadow-method maps|traced|both [--shadow-eps X]   # the asset's exact traced shadows beside / instead of the maps (4.17)
    ... --environment OUT.hdr [--environment-size H W]                  # + the recovered light as a Radiance picture

Per point p with unit outward direction n and s = model.stepSize:
  1. inward march: origin o = p + n_outside * s * n, direction d = -n, n_sample samples at z_k = k * s -- the reference's short
     equispaced march (models/relight_utils.py:707-722 + cull + density + raw2alpha) with near = 0, far = (n_sample - 1) * s.  The
     spacing is the primary march's, so the weights are those of a camera ray arriving along -n, but the march starts a few voxels
     above the point and cannot be occluded by other geometry in a concavity.
  2. decode at the samples with w > rayMarch_weight_thres: intrinsic feature -> BRDF decoder (albedo, roughness = 0.9 raw + 0.09)
     and the shading normal the renderer composites for the model's normals_kind.
  3. composite over those samples (tir_bake_composite): coverage = min(sum w, 1); albedo, roughness = weighted means clamped to [0, 1]; normal = the
     normalised weighted sum, `n` where coverage <= 0.5; surface = o + d * (sum w z) / coverage.  No white background.
  4. lighting (tir_irradiance_integrate): from `surface` along model.fixed_viewdirs, for the pairs with cos > 1e-6 on covered
     points, visibility = T_end of the reference's visibility march; ao = sum vis cos w / sum cos w, irradiance = sum vis env cos w.
     Direct light only (the decoded indirect radiance belongs to the training illumination and a view direction).
All per-sample work runs in libtensoir_hip.so; there is no CPU path."""
from __future__ import annotations

import torch

from . import capacity, ops, relight

MAX_SAMPLES = 256      # the secondary march's limit


def _shading_normals(model, f, xyz, intr):
    """The per-sample normal forward() composites (field_model.py, models/tensorBase_rotated_lights.py:946-968)."""
    kind = model.normals_kind
    if kind in ("purely_predicted", "derived_plus_predicted"):
        return model.renderModule_normal.run(intr, xyz)
    if kind == "purely_derived":
        return ops.density_grad(f, xyz)[2]
    if kind == "residue_prediction":
        return model.renderModule_normal.rows(xyz, ops.density_grad(f, xyz)[2], intr)
    raise NotImplementedError(f"bake_points: normals_kind={kind!r} has no per-sample normal in the field")


def _march_records(model, f, origins, dirs, z):
    """The inward march with its w > thres samples recorded: the synchronous form of the record-capacity protocol (capacity.py) --
    the count is read back (one host synchronisation per chunk) and the march repeated with room when it did not fit."""
    n = origins.shape[0]
    rc = capacity.PassCapacity(model.__dict__.setdefault("_bake_cap_hints", {}), n, 1.5, decay=0, max_entries=32)
    cap = rc.hinted() or relight._rec_capacity(n)
    while True:
        _, _, rec = ops.march_secondary(f, origins, dirs, z, n, None, None, None, model.march_t_stop, True, cap, False, 0)
        total = int(rec["counter"][0].item())
        if total <= cap:
            break
        cap = rc.regrow(total)
    rc.settle(total)
    return rec, total


def _bake_chunk(model, f, pts, nrm, li, n_sample, n_outside, lighting, vis_z, light_tables):
    step = model.stepSize.to(pts.device, torch.float32)
    origins = (pts + nrm * (step * float(n_outside))).contiguous()
    dirs = (-nrm).contiguous()
    z = relight._z_table(n_sample, 0.0, float(step) * (n_sample - 1), pts.device)
    rec, total = _march_records(model, f, origins, dirs, z)
    rec_w, rec_xyz = rec["w"][:total], rec["xyz"][:total]
    if total > 0:
        intr = model.compute_intrinfeature(rec_xyz)
        brdf = model.renderModule_brdf.run(intr, rec_xyz)
        normal = _shading_normals(model, f, rec_xyz, intr)
    else:
        brdf = torch.empty((0, 4), dtype=torch.float32, device=pts.device)
        normal = torch.empty((0, 3), dtype=torch.float32, device=pts.device)
    rows = ops.bake_composite(rec["off"], rec["cnt"], rec_w, rec_xyz, brdf, normal, origins, dirs, nrm, model.aabb)
    if not lighting:
        return rows, None
    ldirs, area, env = light_tables
    M, D = rows.shape[0], ldirs.shape[0]
    n, cov = rows[:, 4:7], rows[:, 7]
    # the cosine test of the reference's shading stage (models/relight_utils.py:436-441), formed as the integration kernel
    # forms it (products and sums rounded one by one), so that both take the same pairs
    cos = (n[:, 0:1] * ldirs[None, :, 0] + n[:, 1:2] * ldirs[None, :, 1]) + n[:, 2:3] * ldirs[None, :, 2]
    active = (cos > 1e-6) & (cov > 0.5)[:, None]
    surf = rows[:, 8:11].contiguous()
    # only the pairs that pass get a ray: the march walks their compacted id list (as the shading stage's does) and addresses
    # vis by pair id; the others keep the zero they are created with.  One host synchronisation: the length of the list.
    ids = torch.nonzero(active.view(-1)).view(-1).to(torch.int32)
    vis = torch.zeros((M * D,), dtype=torch.float32, device=pts.device)
    if ids.numel():
        n_ids = torch.full((1,), ids.numel(), dtype=torch.int32, device=pts.device)
        ops.march_secondary(f, surf, ldirs, vis_z, ids.numel(), None, None, None, model.march_t_stop, False, 0, False, D,
                            ray_ids=ids, n_ids_dev=n_ids, vis=vis)
    return rows, ops.irradiance_integrate(rows, ldirs, vis.view(M, D), env, area, li)


@torch.no_grad()
def bake_points(model, points, outward, light_idx=0, n_sample=96, n_outside=16, lighting=True, vis_n_sample=96, vis_near=0.05,
                vis_far=1.5, chunk=16384):
    """points [N, 3] world positions, outward [N, 3] unit outward directions (device float32) -> dict of device tensors
    albedo [N, 3], roughness [N], normal [N, 3], coverage [N], surface [N, 3], and with lighting ao [N], irradiance [N, 3] under
    light `light_idx` (an int, or one int per point).  Points are processed `chunk` at a time, so no [chunk, D] buffer grows with
    the point set; the results do not depend on `chunk` (every point is reduced on its own, in a fixed order)."""
    pts = ops.f32(points, "points", 3).view(-1, 3)
    nrm = ops.f32(outward, "outward", 3).view(-1, 3)
    if nrm.shape[0] != pts.shape[0] or nrm.device != pts.device:
        raise ValueError("points and outward take one row per point, on one device")
    if not 1 <= int(n_sample) <= MAX_SAMPLES or not 1 <= int(vis_n_sample) <= MAX_SAMPLES:
        raise ValueError(f"n_sample and vis_n_sample must lie in 1 .. {MAX_SAMPLES} (the secondary march's limit)")
    if int(chunk) < 1:
        raise ValueError("chunk must be positive")
    dev, N = pts.device, pts.shape[0]
    f = model.packed_field_dense()          # inference: the marches read the dense density volume where there is one
    li = light_idx if torch.is_tensor(light_idx) else torch.full((N,), int(light_idx), dtype=torch.int32)
    li = ops.to_device(li.reshape(-1), dev, torch.int32).contiguous()
    if li.numel() != N:
        raise ValueError("light_idx: an int or one entry per point")
    tables = vis_z = None
    if lighting:
        ldirs = relight._on_device(model, "fixed_viewdirs", model.fixed_viewdirs, dev)
        area = relight._on_device(model, "light_area_weight", model.light_area_weight, dev)
        env = model.get_light_rgbs(ldirs, device=dev).detach().contiguous()
        if N and not (0 <= int(li.min()) and int(li.max()) < env.shape[0]):
            raise ValueError(f"light_idx outside 0 .. {env.shape[0] - 1}")
        if min(int(chunk), N) * ldirs.shape[0] >= 1 << 31:
            raise ValueError("chunk x light directions must stay below 2^31 pairs")
        tables = (ldirs, area, env)
        vis_z = relight._z_table(int(vis_n_sample), vis_near, vis_far, dev)
    rows = torch.empty((N, ops.BAKE_ROW), dtype=torch.float32, device=dev)
    light = torch.empty((N, 4), dtype=torch.float32, device=dev) if lighting else None
    for a in range(0, N, int(chunk)):
        b = min(N, a + int(chunk))
        r, l = _bake_chunk(model, f, pts[a:b], nrm[a:b], li[a:b], int(n_sample), n_outside, lighting, vis_z, tables)
        rows[a:b] = r
        if lighting:
            light[a:b] = l
    out = {"albedo": rows[:, 0:3].contiguous(), "roughness": rows[:, 3].contiguous(), "normal": rows[:, 4:7].contiguous(),
           "coverage": rows[:, 7].contiguous(), "surface": rows[:, 8:11].contiguous()}
    if lighting:
        out["ao"] = light[:, 0].contiguous()
        out["irradiance"] = light[:, 1:4].contiguous()
    return out


def load_model(path, device="cuda", **extra):
    """A checkpoint file in the reference's layout (TensorVMSplit.save) -> model, as model_from_checkpoint builds it; a
    checkpoint of the general multi-light variant (it carries light_name_list) gets that class."""
    import tensoir_amd
    from .run import _allow_numpy_in_checkpoints
    _allow_numpy_in_checkpoints()
    ckpt = torch.load(path, map_location=device)
    if "light_name_list" in ckpt["kwargs"]:
        from .general_multi_lights import TensorVMSplit
        kwargs = {**ckpt["kwargs"], "device": device, **extra}
        kwargs.pop("light_num", None)
        model = TensorVMSplit(**kwargs)
        model.load(ckpt)
        return model
    return tensoir_amd.model_from_checkpoint(ckpt, device, **extra)


def main(argv=None):
    import argparse
    from . import mesh, synth
    ap = argparse.ArgumentParser(prog="python -m tensoir_amd.bake", description="Export a checkpoint's surface as a binary PLY with "
                                 "per-vertex normals, colour, roughness, ambient occlusion, coverage, albedo and direct irradiance.")
    ap.add_argument("ckpt")
    ap.add_argument("out")
    ap.add_argument("--grid", type=int, default=None, help="lattice points per axis (default: the model's gridSize)")
    ap.add_argument("--level", type=float, default=0.005)
    ap.add_argument("--color", choices=("albedo", "diffuse"), default="albedo")
    ap.add_argument("--light", type=int, default=0)
    ap.add_argument("--envmap", type=int, nargs=2, metavar=("H", "W"), default=None, help="light direction grid (default 16 32)")
    ap.add_argument("--keep-largest", type=int, default=None, metavar="N", help="export only the N largest connected components "
                    "of the lattice (drops detached floaters)")
    ap.add_argument("--min-component-voxels", type=int, default=None, metavar="N", help="drop components of fewer than N lattice "
                    "points")
    ap.add_argument("--connectivity", type=int, choices=(6, 26), default=6, help="what joins two lattice points into one component")
    ap.add_argument("--simplify", type=int, default=None, metavar="K", help="reduce the mesh by quadric vertex clustering: one "
                    "vertex per block of K x K x K lattice cells (K >= 2); the attributes are baked at the reduced vertices")
    ap.add_argument("--simplify-tolerance", type=float, default=None, metavar="T", help="instead of --simplify: take the largest K "
                    "in 2 .. --simplify-max whose mesh stays within T lattice cells (Hausdorff distance) of the full-resolution one; "
                    "the search stops at the first K that does not")
    ap.add_argument("--simplify-max", type=int, default=mesh.SIMPLIFY_MAX, metavar="K", help="the largest K --simplify-tolerance tries")
    ap.add_argument("--check-distance", type=int, nargs="?", const=262144, default=None, metavar="N", help="after writing OUT (.ply or "
                    ".glb), read it back and print its surface distance (mesh.distance, N samples per direction, default 262144) "
                    "to the full-resolution extraction as one JSON line")
    ap.add_argument("--check-fscore", type=float, nargs="+", default=None, metavar="T", help="with --check-distance: add the F-score "
                    "(precision of OUT, recall of the full-resolution extraction) at every distance threshold T")
    ap.add_argument("--check-signed", action="store_true", help="with --check-distance: add the signed mean distance, the share of "
                    "samples inside the other mesh and the undecided / grazed counts per direction (both meshes must be closed)")
    ap.add_argument("--check-normals", action="store_true", help="with --check-distance: add normal_consistency and flipped_share per "
                    "direction")
    ap.add_argument("--texture-size", type=int, default=None, metavar="N", help="write OUT as a binary glTF (.glb) with an N x N "
                    "texture atlas baked at every texel (base colour, occlusion / roughness / metallic, normal) instead of a PLY "
                    "with per-vertex attributes")
    ap.add_argument("--check-views", type=int, default=None, metavar="V", help="after writing the .glb, rasterise it from V orbit "
                    "views, render the field from the same cameras and print the comparison (raster.compare_asset) as one JSON line")
    ap.add_argument("--check-size", type=int, default=200, metavar="S", help="side of the S x S comparison images (default 200)")
    ap.add_argument("--check-light", default=None, metavar="NAME|FILE", help="with --check-views: also light the field's and the "
                    "asset's G-buffer with this environment and report relit_psnr; one of the synthetic maps "
                    f"({', '.join(synth.HDR_NAMES)}; 64 x 128), a Radiance .hdr file or a .npy array [H, W, 3]")
    ap.add_argument("--check-light-rows", type=int, default=16, metavar="R", help="light cells: R x 2R (default 16)")
    ap.add_argument("--write-views", default=None, metavar="DIR", help="with --check-light: write every view's field-lit and "
                    "asset-lit image as PNG into DIR")
    ap.add_argument("--check-shadows", action="store_true", help="with --check-light: also build the asset's per-cell shadow maps and "
                    "report shadow_agreement, the share of (pixel, light cell) pairs on which they and the field's transmittance agree")
    ap.add_argument("--shadow-size", type=int, default=256, metavar="S", help="side of the S x S shadow maps (default 256)")
    ap.add_argument("--shadow-method", choices=("maps", "traced", "both"), default="maps", help="with --check-shadows: the asset's "
                    "visibility by its shadow maps (default), by exact any-hit rays over its face grid, or both -- then with "
                    "shadow_agreement_traced and shadow_map_agreement (maps against traced) beside shadow_agreement")
    ap.add_argument("--shadow-eps", type=float, default=None, metavar="X", help="traced shadows: rays start at X times the radius of "
                    "the mesh's bounding sphere (default raster.SHADOW_EPS)")
    ap.add_argument("--environment", default=None, metavar="OUT.hdr", help="also write the model's light --light as a Radiance "
                    "picture (mesh.export_environment)")
    ap.add_argument("--environment-size", type=int, nargs=2, metavar=("H", "W"), default=(256, 512))
    ap.add_argument("--edits", default=None, metavar="FILE.json", help="material edits applied between the bake and the texture atlas "
                    "(with --texture-size): a JSON file {\"edits\": [...], \"palette\": {...}} as materials.EditList.to_json writes it")
    ap.add_argument("--palette", type=int, default=None, metavar="K", help="print the K materials of the surface (materials.palette: "
                    "k-means over albedo and roughness, the largest first) as one JSON line; an edits file may carry it as "
                    "\"palette\".  With - for OUT nothing is exported")
    ap.add_argument("--palette-samples", type=int, default=65536, metavar="N", help="surface samples the palette is found on")
    a = ap.parse_args(argv)
    if a.edits is not None and a.texture_size is None:
        ap.error("--edits changes the texture atlas: it needs --texture-size")
    if a.palette is not None and (not 1 <= a.palette <= ops.MATERIAL_MAX_PALETTE or a.palette_samples < a.palette):
        ap.error(f"--palette K: 1 <= K <= {ops.MATERIAL_MAX_PALETTE} and --palette-samples >= K")
    edits = None
    if a.edits is not None:
        import json
        from . import materials
        with open(a.edits) as h:
            edits = materials.EditList.from_json(json.load(h))              # refused before the checkpoint is read
    if a.check_views is not None and (a.texture_size is None or a.check_views < 1 or a.check_size < 1):
        ap.error("--check-views V (V >= 1, --check-size >= 1) compares a textured export: it needs --texture-size")
    if a.check_light is not None and a.check_views is None:
        ap.error("--check-light lights the views of --check-views")
    if a.write_views is not None and a.check_light is None:
        ap.error("--write-views writes the images of --check-light")
    if a.check_shadows and a.check_light is None:
        ap.error("--check-shadows shadows the light of --check-light")
    if a.simplify_tolerance is not None and a.simplify is not None:
        ap.error("--simplify K and --simplify-tolerance T are mutually exclusive")
    if a.check_distance is not None and a.check_distance < 0:
        ap.error("--check-distance N: N >= 0")
    if a.check_distance is None and (a.check_fscore is not None or a.check_signed or a.check_normals):
        ap.error("--check-fscore, --check-signed and --check-normals add to --check-distance")
    if a.check_fscore is not None and any(not t >= 0.0 for t in a.check_fscore):
        ap.error("--check-fscore T: T >= 0")
    simp = {"simplify": a.simplify, "simplify_tolerance": a.simplify_tolerance, "simplify_max": a.simplify_max}
    extra = {} if a.envmap is None else {"envmap_h": a.envmap[0], "envmap_w": a.envmap[1]}
    model = load_model(a.ckpt, "cuda", **extra)
    grid = None if a.grid is None else [a.grid] * 3
    report = {}
    if a.palette is not None:
        import json
        from . import materials
        pal = materials.palette(model, a.palette, samples=a.palette_samples, level=a.level, gridSize=grid, keep_largest=a.keep_largest,
                                min_component_voxels=a.min_component_voxels, connectivity=a.connectivity)
        print(json.dumps({"palette": pal.to_json(), "passes": pal.passes, "inertia": pal.inertia}))
        if a.out == "-":
            return
    if a.texture_size is not None:
        more = {} if edits is None else {"edits": edits}
        nv, nf = mesh.export_textured(model, a.out, a.level, grid, a.texture_size, a.color, light_idx=a.light,
                                      keep_largest=a.keep_largest, min_component_voxels=a.min_component_voxels,
                                      connectivity=a.connectivity, report=report, **simp, **more)
    else:
        nv, nf = mesh.export_mesh(model, a.out, a.level, grid, attributes=True, color=a.color, light_idx=a.light,
                                  keep_largest=a.keep_largest, min_component_voxels=a.min_component_voxels,
                                  connectivity=a.connectivity, report=report, **simp)
    if "table" in report:
        sizes, kept = report["table"]["sizes"].cpu(), report["kept"].cpu()
        print(f"components: dropped {int((~kept).sum())} of {kept.numel()} ({int(sizes[~kept].sum())} of {int(sizes.sum())} voxels)")
    if "full" in report:
        print(f"simplify {report.get('simplify', a.simplify)}: {report['full'][0]} vertices, {report['full'][1]} faces before")
    if "simplify_error" in report:
        import json
        print(json.dumps({"simplify": report["simplify"], "simplify_error": {str(k): v for k, v in report["simplify_error"].items()}}))
    print(f"{a.out}: {nv} vertices, {nf} faces")
    if a.environment is not None:
        mesh.export_environment(model, a.environment, a.environment_size[0], a.environment_size[1], light=a.light)
        print(f"{a.environment}: light {a.light}, {a.environment_size[0]} x {a.environment_size[1]}")
    if a.check_distance is not None:
        import json
        import torch
        from . import metrics
        full_v, full_f, _ = mesh.extract_mesh(model, a.level, grid, keep_largest=a.keep_largest,
                                              min_component_voxels=a.min_component_voxels, connectivity=a.connectivity)
        if a.texture_size is not None:                     # the writer unwelds: three vertices per face, no index buffer
            full_v = full_v[full_f.reshape(-1).long()].contiguous()
            full_f = torch.arange(full_v.shape[0], dtype=torch.int32, device=full_v.device).view(-1, 3)
        more = {} if a.check_fscore is None else {"thresholds": tuple(a.check_fscore)}
        more.update({"signed": True} if a.check_signed else {})
        more.update({"normals": True} if a.check_normals else {})
        print(json.dumps({"check_distance": metrics.chamfer(a.out, (full_v, full_f), samples=a.check_distance, **more)}))
    if a.check_views is not None:
        import json
        from . import raster
        light = a.check_light
        if light in synth.HDR_NAMES:
            light = synth.make_hdr_maps(synth.HDR_NAMES, 64, 128)[light]            # as Environment_Light("synthetic:h=64,w=128")
        shadow = {}
        if a.check_shadows:
            shadow = {"shadows": True if a.shadow_method == "maps" else a.shadow_method, "shadow_size": a.shadow_size}
            if a.shadow_eps is not None:
                shadow["shadow_eps"] = a.shadow_eps
        print(json.dumps(raster.compare_asset(model, a.out, H=a.check_size, W=a.check_size, n_views=a.check_views, grid=grid, light=light,
                                              light_rows=a.check_light_rows, write_views=a.write_views, **shadow)))


if __name__ == "__main__":
    main()
