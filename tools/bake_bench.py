"""Timing of the per-vertex bake (not part of bench.py): export_mesh(attributes=True) on the 300^3 lattice of the field
tools/mesh_bench.py uses (the small golden checkpoint), with the default 16 x 32 light grid (D = 512 directions).

    python tools/bake_bench.py [--grid 300] [--reps 3]          # one JSON line
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bake -- python tools/bake_bench.py --reps 1
    python tools/bake_bench.py --stats DIR                      # per-kernel GPU time from that trace
    python tools/bake_bench.py --texture-size 2048 4096 [--simplify 3]     # the textured export instead: one JSON line per size
    python tools/bake_bench.py --raster [--views 8] [--image 800]           # the rasteriser on the exported assets: one JSON line per mesh

The JSON line: geometry_ms (extract_mesh), material_ms (bake_points(lighting=False): inward march, decoders, tir_bake_composite),
lighting_ms (the rest of bake_points: pair mask, visibility march, tir_irradiance_integrate) -- device events around the calls,
best of --reps; export_plain_s / export_baked_s (wall clock incl. the PLY write, after a warm-up, measured in this same run: the
yardstick for "is the bake cheap enough"); and for the two new kernels the bytes they must move, their time (events around the
launch, summed over the chunks) and the rate as a fraction of the 6.3 TB/s HBM ceiling.

The --texture-size leg (mesh.export_textured): layout_ms (tir_atlas_corners + tir_atlas_texels), bake_ms (field_positions
+ bake_points at every texel), pack_ms (tir_atlas_pack) -- device events, best of --reps; png_write_s (PNG compression of the
three images + the GLB write, wall clock); export_s (the whole export_textured call, wall clock, after a warm-up); and for
k_atlas_texels and k_atlas_pack the bytes they must move, their time and the rate against the same ceiling.

The --raster leg (tensoir_amd/raster.py): the simplify=3 mesh and the full mesh of the same lattice, exported with
export_textured, rasterised at --image x --image from --views orbit cameras.  Per mesh: project_ms / cover_ms / resolve_ms / shade_ms
(device events around each entry, memsets included, per view: the mean over the views of the best of --reps), faces and covered pixels
per second of cover (the covered pixels are a lower bound of the fragments), the bytes resolve and shade must move against the HBM
ceiling, and compare_wall_s (raster.compare_asset over the same views, wall clock, after a
warm-up; it includes the field's own renders and reading the file)."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 6.3


def stats(d):
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    out = {}
    for r in rows:
        name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        out[name] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6, "avg_us": float(r["AverageNs"]) / 1e3}
    top = dict(sorted(out.items(), key=lambda kv: -kv[1]["total_ms"])[:14])
    top.update({k: v for k, v in out.items() if k.startswith(("k_atlas_", "k_raster_"))})    # the streaming kernels of the textured / raster legs
    print(json.dumps({"kernels": top, "total_ms": sum(v["total_ms"] for v in out.values())}, indent=1))


def run(n, reps):
    import numpy as np
    import torch

    import tensoir_amd
    from tensoir_amd import bake, mesh, ops, relight
    from tests.helpers import golden_checkpoint
    g = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    model = tensoir_amd.model_from_checkpoint(golden_checkpoint(g), "cuda:0")
    grid = [n, n, n]
    D = model.fixed_viewdirs.shape[0]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    geo, mat, full, kern = [], [], [], []
    for rep in range(reps + 1):                                   # the first pass warms up (record-capacity hints, tables)
        (verts, faces, normals), t_geo = timed(lambda: mesh.extract_mesh(model, 0.005, grid))
        pos, outward = mesh.field_positions(model.aabb, grid, verts, normals)
        pos, outward = pos.contiguous(), outward.contiguous()
        _, t_mat = timed(lambda: bake.bake_points(model, pos, outward, lighting=False))
        ops.TIMING = []
        out, t_full = timed(lambda: bake.bake_points(model, pos, outward))
        calls, ops.TIMING = ops.TIMING, None
        if rep:
            geo.append(t_geo)
            mat.append(t_mat)
            full.append(t_full)
            kern.append({k: sum(e0.elapsed_time(e1) for name, e0, e1 in calls if name.startswith(k))
                         for k in ("tir_bake_composite", "tir_irradiance_integrate", "tir_march_secondary")})
    V = int(verts.shape[0])
    # records of the inward march: counted once more (the bake does not return them)
    step = float(model.stepSize)
    z = relight._z_table(96, 0.0, step * 95, pos.device)
    n_rec = 0
    for a in range(0, V, 16384):
        o = (pos[a:a + 16384] + outward[a:a + 16384] * (step * 16)).contiguous()
        rec, total = bake._march_records(model, model.packed_field(), o, (-outward[a:a + 16384]).contiguous(), z)
        n_rec += total
    comp_bytes = n_rec * (4 + 12 + 16 + 12) + V * (8 + 36 + 64)          # w, xyz, brdf, normal per record; off/cnt, o/d/n, row per point
    integ_bytes = V * D * 4 + V * (64 + 4 + 16)                            # vis; row, light index, output per point
    k = {name: min(r[name] for r in kern) for name in kern[0]}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.ply")
        walls = {}
        for key, kw in (("export_plain_s", {}), ("export_baked_s", {"attributes": True})):
            mesh.export_mesh(model, path, gridSize=grid, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh.export_mesh(model, path, gridSize=grid, **kw)
            walls[key] = time.perf_counter() - t0
            walls[key.replace("_s", "_bytes")] = os.path.getsize(path)
    rate = lambda b, ms: b / (ms * 1e-3) / 1e12
    print(json.dumps({
        "grid": n, "vertices": V, "faces": int(faces.shape[0]), "directions": D, "records": n_rec,
        "covered": float((out["coverage"] > 0.5).float().mean()),
        "geometry_ms": min(geo), "material_ms": min(mat), "lighting_ms": min(full) - min(mat), "bake_ms": min(full), **walls,
        "march_secondary_ms": k["tir_march_secondary"],
        "bake_composite": {"ms": k["tir_bake_composite"], "bytes": comp_bytes, "TB_s": rate(comp_bytes, k["tir_bake_composite"]),
                           "of_hbm": rate(comp_bytes, k["tir_bake_composite"]) / HBM_TBS},
        "irradiance_integrate": {"ms": k["tir_irradiance_integrate"], "bytes": integ_bytes,
                                 "TB_s": rate(integ_bytes, k["tir_irradiance_integrate"]),
                                 "of_hbm": rate(integ_bytes, k["tir_irradiance_integrate"]) / HBM_TBS}}), flush=True)


def run_textured(n, sizes, simplify, reps):
    import numpy as np
    import torch

    import tensoir_amd
    from tensoir_amd import bake, mesh, ops
    from tests.helpers import golden_checkpoint
    g = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    model = tensoir_amd.model_from_checkpoint(golden_checkpoint(g), "cuda:0")
    grid = [n, n, n]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    verts, faces, normals = mesh.extract_mesh(model, 0.005, grid, simplify=simplify)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    rate = lambda b, ms: b / (ms * 1e-3) / 1e12
    for size in sizes:
        cols, T = ops.atlas_layout(F, size)
        N = ((F + 1) // 2) * T * T
        lay, bk, pk, kern = [], [], [], []
        for rep in range(reps + 1):                               # the first pass warms up (record-capacity hints, tables)
            ops.TIMING = []
            (_, (point, outward, _)), t_lay = timed(lambda: (ops.atlas_corners(verts, normals, faces, size, cols, T),
                                                            ops.atlas_texels(verts, normals, faces, size, cols, T)))
            calls_lay, ops.TIMING = ops.TIMING, None

            def do_bake():
                p, d = mesh.field_positions(model.aabb, grid, point, outward)
                return bake.bake_points(model, p.contiguous(), d.contiguous())
            b, t_bake = timed(do_bake)
            ops.TIMING = []
            images, t_pack = timed(lambda: ops.atlas_pack(verts, normals, faces, size, cols, T, b["albedo"], b["roughness"], b["normal"],
                                                          b["coverage"], ao=b["ao"]))
            calls, ops.TIMING = calls_lay + ops.TIMING, None
            if rep:
                lay.append(t_lay)
                bk.append(t_bake)
                pk.append(t_pack)
                kern.append({k: sum(e0.elapsed_time(e1) for name, e0, e1 in calls if name == k)
                             for k in ("tir_atlas_corners", "tir_atlas_texels", "tir_atlas_pack")})
        covered = float((b["coverage"] > 0.5).float().mean())
        del b, point, outward
        a = mesh.bake_atlas(model, verts, faces, normals, grid, size)
        host = {k: a[k].cpu().numpy() for k in mesh.IMAGE_NAMES}
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.glb")
            t0 = time.perf_counter()
            pngs = {k: len(mesh.write_png(v)) for k, v in host.items()}
            t_png = time.perf_counter() - t0
            t0 = time.perf_counter()
            mesh.write_glb(path, a["pos"], a["nrm"], a["tan"], a["uv"], host, {})
            t_write = time.perf_counter() - t0
            del a
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh.export_textured(model, path, 0.005, grid, size, simplify=simplify)
            t_export = time.perf_counter() - t0
            glb_bytes = os.path.getsize(path)
        k = {name: min(r[name] for r in kern) for name in kern[0]}
        mesh_bytes = F * 12 + V * 24                              # faces, vertices and normals: read once from HBM, then from cache
        tex_bytes = N * (12 + 12 + 4) + mesh_bytes                # point, outward, face per texel
        pack_bytes = N * (12 + 4 + 12 + 4 + 4) + 3 * 4 * size * size + mesh_bytes     # albedo, roughness, normal, coverage, ao; 3 images
        print(json.dumps({
            "grid": n, "simplify": simplify, "vertices": V, "faces": F, "size": size, "cols": cols, "T": T, "texels": N,
            "covered": covered, "layout_ms": min(lay), "bake_ms": min(bk), "pack_ms": min(pk), "png_s": t_png,
            "png_write_s": t_write, "png_bytes": pngs, "glb_bytes": glb_bytes, "export_s": t_export,
            "bake_share_of_export": min(bk) * 1e-3 / t_export,
            "atlas_corners_ms": k["tir_atlas_corners"],
            "atlas_texels": {"ms": k["tir_atlas_texels"], "bytes": tex_bytes, "TB_s": rate(tex_bytes, k["tir_atlas_texels"]),
                             "of_hbm": rate(tex_bytes, k["tir_atlas_texels"]) / HBM_TBS},
            "atlas_pack": {"ms": k["tir_atlas_pack"], "bytes": pack_bytes, "TB_s": rate(pack_bytes, k["tir_atlas_pack"]),
                           "of_hbm": rate(pack_bytes, k["tir_atlas_pack"]) / HBM_TBS}}), flush=True)


def run_raster(n, views, image, reps):
    import numpy as np
    import torch

    import tensoir_amd
    from tensoir_amd import mesh, ops, raster
    from tests.helpers import golden_checkpoint
    g = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    model = tensoir_amd.model_from_checkpoint(golden_checkpoint(g), "cuda:0")
    grid = [n, n, n]
    H = W = image
    rate = lambda b, ms: b / (ms * 1e-3) / 1e12
    entries = ("tir_raster_project", "tir_raster_cover", "tir_raster_resolve", "tir_raster_shade")
    with tempfile.TemporaryDirectory() as d:
        for simplify, size in ((3, 2048), (None, 4096)):
            path = os.path.join(d, f"m{simplify}.glb")
            _, F = mesh.export_textured(model, path, 0.005, grid, size, simplify=simplify)
            report = raster.compare_asset(model, path, H=H, W=W, n_views=views, grid=grid)          # warm-up, and the cameras' focal
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            report = raster.compare_asset(model, path, H=H, W=W, n_views=views, grid=grid)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            file = mesh.read_glb(path)
            dev = lambda a: torch.from_numpy(a).cuda()
            pos = mesh.field_positions(model.aabb, grid, dev(file["pos"])).contiguous()
            nrm, tan, uv = dev(file["nrm"]), dev(file["tan"]), dev(file["uv"])
            images = {k: dev(np.ascontiguousarray(v)) for k, v in file["images"].items()}
            dist = 0.5 * (float(model.near_far[0]) + float(model.near_far[1]))
            cams = raster.orbit_cameras(model.aabb, views, distance=dist)
            best = {k: [float("inf")] * views for k in entries}
            covered = []
            for rep in range(reps + 1):
                for vi, c2w in enumerate(cams):
                    ops.TIMING = []
                    out = raster.render_mesh(pos, nrm, tan, uv, images, c2w, report["focal"], H, W)
                    torch.cuda.synchronize()
                    calls, ops.TIMING = ops.TIMING, None
                    if rep:
                        for k in entries:
                            best[k][vi] = min(best[k][vi], sum(e0.elapsed_time(e1) for name, e0, e1 in calls if name == k))
                    else:
                        covered.append(int((out["coverage"] > 0.5).sum()))
            ms = {k: sum(v) / views for k, v in best.items()}
            res_bytes = H * W * (8 + 16) + 3 * F * 16                       # key in, row out; the corner rows once
            shade_bytes = H * W * (16 + 48) + 3 * F * (12 + 16 + 8) + 3 * 4 * size * size     # row in, 12 floats out; corners, images once
            print(json.dumps({
                "grid": n, "simplify": simplify, "faces": F, "size": size, "image": image, "views": views,
                "covered_pixels": sum(covered) / views,
                "project_ms": ms["tir_raster_project"], "cover_ms": ms["tir_raster_cover"], "resolve_ms": ms["tir_raster_resolve"],
                "shade_ms": ms["tir_raster_shade"], "raster_ms": sum(ms.values()),
                "faces_per_s": F / (ms["tir_raster_cover"] * 1e-3),
                "covered_pixels_per_s": sum(covered) / views / (ms["tir_raster_cover"] * 1e-3),
                "resolve": {"bytes": res_bytes, "TB_s": rate(res_bytes, ms["tir_raster_resolve"]),
                            "of_hbm": rate(res_bytes, ms["tir_raster_resolve"]) / HBM_TBS},
                "shade": {"bytes": shade_bytes, "TB_s": rate(shade_bytes, ms["tir_raster_shade"]),
                          "of_hbm": rate(shade_bytes, ms["tir_raster_shade"]) / HBM_TBS},
                "compare_wall_s": wall, "compare_mean": report["mean"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats", default=None, help="summarise the rocprofv3 kernel stats under this directory and exit")
    ap.add_argument("--texture-size", type=int, nargs="+", default=None, metavar="N", help="time the textured export "
                    "(mesh.export_textured) at these atlas sizes instead of the per-vertex bake")
    ap.add_argument("--simplify", type=int, default=3, help="the face budget of the --texture-size leg")
    ap.add_argument("--raster", action="store_true", help="time the rasteriser (tensoir_amd/raster.py) on the exported assets instead")
    ap.add_argument("--views", type=int, default=8, help="orbit views of the --raster leg")
    ap.add_argument("--image", type=int, default=800, help="image side of the --raster leg")
    a = ap.parse_args()
    if a.stats:
        return stats(a.stats)
    if a.raster:
        return run_raster(a.grid, a.views, a.image, a.reps)
    if a.texture_size:
        return run_textured(a.grid, a.texture_size, a.simplify, a.reps)
    run(a.grid, a.reps)


if __name__ == "__main__":
    main()
