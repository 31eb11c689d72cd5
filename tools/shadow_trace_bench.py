"""Time the traced shadows of the exported asset (not part of bench.py) beside the shadow-map path on
the meshes of the small golden field's 300^3 lattice: the simplify=3 mesh and the full one, under rows x 2 rows cells of the
synthetic city map, at the --image x --image G-buffer of the simplified mesh (geometry render, albedo and roughness set to 0.5).
  grid      ops.face_grid per mesh (its read-backs included)
  trace     tir_shadow_trace per mesh and cell grid at t0 = SHADOW_EPS x the radius: contributing pairs per second, the share of
            them that is occluded
  lighting  tir_light_gbuffer_occluded beside tir_light_gbuffer with the traced bits of the simplified mesh
  maps      the map path on the same inputs: tir_shadow_maps per mesh at --sizes, tir_light_gbuffer_shadowed on the simplified mesh
Device events, medians of --reps warm runs after one warm-up.  One JSON line per measurement; --out writes them all.  Needs a GPU.
    python tools/shadow_trace_bench.py [--grid 300] [--image 800] [--rows 16 32] [--sizes 256 512] [--reps 5] [--out profiles/shadow_trace.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def median_ms(fn, reps):
    out, _ = timed(fn)                                                  # the first call warms up
    times = []
    for _ in range(reps):
        out, ms = timed(fn)
        times.append(ms)
    return out, float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--image", type=int, default=800)
    ap.add_argument("--rows", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shadow_trace_bench: no GPU")
    import tensoir_amd
    from tensoir_amd import mesh, ops, raster, synth
    from tests.helpers import golden_checkpoint
    g = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    model = tensoir_amd.model_from_checkpoint(golden_checkpoint(g), "cuda:0")
    grid = [a.grid] * 3
    cells = {}
    for rows in a.rows:
        hdr = synth.make_hdr_maps(("city",), 4 * rows, 8 * rows)["city"].cuda() * 0.05
        cells[rows] = ops.env_cells(hdr, rows, 2 * rows)
    results = []

    def emit(row):
        print(json.dumps(row), flush=True)
        results.append(row)

    meshes = {}
    for simplify in (3, None):
        verts, faces, normals = mesh.extract_mesh(model, 0.005, grid, simplify=simplify)
        pos, outward = mesh.field_positions(model.aabb, grid, verts, normals)
        meshes[simplify] = (pos.contiguous(), faces.to(torch.int32).contiguous(), outward)
    pos, faces, normals = meshes[3]
    corner = faces.reshape(-1).long()
    upos, unrm = pos[corner].contiguous(), normals[corner].contiguous()
    box = model.aabb.detach().to("cpu", torch.float64)
    dist = 0.5 * (float(model.near_far[0]) + float(model.near_far[1]))
    c2w = raster.orbit_cameras(box, 1, distance=dist)[0]
    focal = 0.45 * a.image * dist / (0.5 * float(torch.linalg.norm(box[1] - box[0])))
    out, gbuf = raster._render(upos, unrm, None, None, None, c2w, focal, a.image, a.image)
    covered = gbuf[..., 8] > 0
    gbuf[..., 0:4] = torch.where(covered[..., None], torch.full_like(gbuf[..., 0:4], 0.5), gbuf[..., 0:4])
    gbuf[..., 4] = covered.to(torch.float32)
    gbuf = gbuf.view(-1, ops.RASTER_ROW).contiguous()
    rays = raster.camera_rays(c2w, focal, a.image, a.image, gbuf.device)
    view = (-rays[:, 3:6]).contiguous()
    pts = (rays[:, 0:3] + out["depth"].reshape(-1, 1) * rays[:, 3:6]).contiguous()
    nrm = gbuf[:, 5:8].contiguous()
    n_cov, M = int(covered.sum()), int(gbuf.shape[0])
    sample = torch.nonzero(covered.reshape(-1)).reshape(-1)[::97]      # the pixels the shares are counted on
    bits = {}
    for simplify, (pos, faces, _) in meshes.items():
        F = int(faces.shape[0])
        fgrid, ms = median_ms(lambda: ops.face_grid(pos, faces), a.reps)
        emit({"what": "grid", "grid": a.grid, "simplify": simplify, "faces": F, "dims": fgrid["dims"], "pairs": fgrid["n_pairs"], "ms": ms,
              "reps": a.reps})
        t0 = raster.SHADOW_EPS * raster.mesh_bounds(pos)[1]
        for rows in a.rows:
            D = int(cells[rows].shape[0])
            occl, ms = median_ms(lambda: ops.shadow_trace(pts, nrm, cells[rows], pos, faces, fgrid, t0), a.reps)
            on = raster._contributing_codes(pts[sample], nrm[sample], cells[rows]) != 0
            occ = ops.occlusion_bits(ops.shadow_trace(pts[sample], nrm[sample], cells[rows], pos, faces, fgrid, t0), sample.numel())
            share_on = float(on.float().mean())
            emit({"what": "trace", "image": a.image, "simplify": simplify, "faces": F, "rows": M, "covered_pixels": n_cov, "cells": D,
                  "t0": t0, "ms": ms, "reps": a.reps, "contributing_share_of_covered_pairs": share_on,
                  "contributing_pairs_per_s": n_cov * D * share_on / (ms * 1e-3),
                  "occluded_share_of_contributing_pairs": float((occ & on).sum()) / max(int(on.sum()), 1), "occl_bytes": occl.numel() * 8})
            if simplify == 3:
                bits[rows] = occl
        for rows in a.rows:
            for S in a.sizes:
                frames = ops.shadow_frames(cells[rows], *raster.mesh_bounds(pos), S)
                (maps, drops), ms = median_ms(lambda: ops.shadow_maps(pos, frames, S, faces=faces), a.reps)
                emit({"what": "maps", "simplify": simplify, "faces": F, "cells": int(frames.shape[0]), "S": S, "ms": ms, "reps": a.reps,
                      "map_bytes": 4 * int(frames.shape[0]) * S * S})
                del maps
    for rows in a.rows:
        cl = cells[rows]
        D = int(cl.shape[0])
        _, plain = median_ms(lambda: ops.light_gbuffer(gbuf, view, cl, 0.04, True, True), a.reps)
        _, occluded = median_ms(lambda: ops.light_gbuffer_occluded(gbuf, view, cl, bits[rows], 0.04, True, True), a.reps)
        row = {"what": "lighting", "image": a.image, "covered_pixels": n_cov, "cells": D, "plain_ms": plain, "occluded_ms": occluded,
               "reps": a.reps}
        for S in a.sizes:
            frames, maps = raster.shadow_maps_for(upos, cl, S)
            _, row[f"shadowed_ms_S{S}"] = median_ms(
                lambda: ops.light_gbuffer_shadowed(gbuf, view, cl, pts, frames, maps, raster.SHADOW_BIAS, 0.04, True, True), a.reps)
            codes = ops.shadow_lookup(pts[sample], nrm[sample], cl, frames, maps, raster.SHADOW_BIAS)
            row[f"map_shadowed_share_S{S}"] = float((codes == 1).sum()) / max(int((codes != 0).sum()), 1)
            del maps
        emit(row)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/shadow_trace_bench.py", "device": torch.cuda.get_device_name(0), "shadow_eps": raster.SHADOW_EPS,
                       "results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
