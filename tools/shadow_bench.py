"""Time the shadow maps of the exported asset (not part of bench.py) on the meshes of the small golden field's 300^3
lattice: the simplify=3 mesh and the full one, under rows x 2 rows cells of the synthetic city map.
  maps      tir_shadow_maps (clearing included) per mesh, cell grid and map side: device events, best of --reps after a warm-up;
            (cell, face) pairs per second, and the bytes of the maps
  lighting  tir_light_gbuffer_shadowed beside tir_light_gbuffer on the same --image x --image G-buffer of the simplified mesh
            (geometry render, albedo and roughness set to 0.5), alternating, device events over --reps calls each: the ratio
            shadowed / unshadowed, and the share of contributing pairs the maps shadow
One JSON line per measurement; --out writes them all.  Needs a GPU.
    python tools/shadow_bench.py [--grid 300] [--image 800] [--rows 16 32] [--sizes 256 512] [--reps 3] [--out profiles/shadow_800.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--image", type=int, default=800)
    ap.add_argument("--rows", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--light-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shadow_bench: no GPU")
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

    small = None
    for simplify in (3, None):
        verts, faces, normals = mesh.extract_mesh(model, 0.005, grid, simplify=simplify)
        pos, outward = mesh.field_positions(model.aabb, grid, verts, normals)
        pos, faces = pos.contiguous(), faces.to(torch.int32).contiguous()
        if simplify is not None:
            small = (pos, faces, outward)
        centre, radius = raster.mesh_bounds(pos)
        for rows in a.rows:
            for S in a.sizes:
                frames = ops.shadow_frames(cells[rows], centre, radius, S)
                best, drops = float("inf"), None
                for rep in range(a.reps + 1):                          # the first call warms up
                    (maps, drops), ms = timed(lambda: ops.shadow_maps(pos, frames, S, faces=faces))
                    best = ms if rep == 0 else min(best, ms)
                D, F = int(frames.shape[0]), int(faces.shape[0])
                emit({"what": "maps", "grid": a.grid, "simplify": simplify, "faces": F, "cells": D, "S": S, "ms": best, "reps": a.reps,
                      "pairs_per_s": D * F / (best * 1e-3), "map_bytes": 4 * D * S * S, "occupied": float((maps != 0).float().mean()),
                      "drops": drops})
                del maps
    pos, faces, normals = small
    corner = faces.reshape(-1).long()
    upos = pos[corner].contiguous()
    unrm = normals[corner].contiguous()
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
    for rows in a.rows:
        for S in a.sizes:
            frames, maps = raster.shadow_maps_for(upos, cells[rows], S)
            plain = lambda: ops.light_gbuffer(gbuf, view, cells[rows], 0.04, True, True)
            shadowed = lambda: ops.light_gbuffer_shadowed(gbuf, view, cells[rows], pts, frames, maps, raster.SHADOW_BIAS, 0.04, True, True)
            for _ in range(3):
                plain(), shadowed()
            t = {"plain": 0.0, "shadowed": 0.0}
            for _ in range(a.light_reps):                              # alternating: both see the same machine
                t["plain"] += timed(plain)[1]
                t["shadowed"] += timed(shadowed)[1]
            idx = torch.nonzero(covered.reshape(-1)).reshape(-1)[::97]
            codes = ops.shadow_lookup(pts[idx], gbuf[idx, 5:8].contiguous(), cells[rows], frames, maps, raster.SHADOW_BIAS)
            n_cov, D = int(covered.sum()), int(cells[rows].shape[0])
            emit({"what": "lighting", "image": a.image, "faces": int(faces.shape[0]), "covered_pixels": n_cov, "cells": D, "S": S,
                  "plain_ms": t["plain"] / a.light_reps, "shadowed_ms": t["shadowed"] / a.light_reps, "ratio": t["shadowed"] / t["plain"],
                  "reps": a.light_reps, "pairs_per_s_shadowed": n_cov * D / (t["shadowed"] / a.light_reps * 1e-3),
                  "shadowed_share_of_contributing_pairs": float((codes == 1).sum()) / max(int((codes != 0).sum()), 1)})
            del maps
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/shadow_bench.py", "device": torch.cuda.get_device_name(0), "results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
