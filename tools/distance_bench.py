"""Timing of the surface-distance kernels (not part of bench.py): mesh.distance(full, simplified k) on the 300^3
lattice of the field tools/bake_bench.py uses (the small golden checkpoint), and the simplification error of k = 2 .. 8.

    python tools/distance_bench.py [--grid 300] [--samples 262144] [--reps 7] [--brute 4096]      # one JSON document

timing: per direction (a = the simplified mesh, b = the full one), medians over --reps warm runs of device events around
sampling (ops.sample_surface: weights, integer scan, draw, and its one read-back), grid build (ops.face_grid of the target mesh,
its read-back included) and query (ops.point_mesh_distance over the vertices and the samples), the whole mesh.distance call
(wall clock), and the mean number of point-triangle tests per query from a separate instrumented run (tested=True).
brute: the same query on the first --brute samples against a 1 x 1 x 1 grid (every face tested), and on the grid, which shows
what the grid buys.  simplify: face count and a_to_b (simplified -> full) mean / p95 / max and the Hausdorff distance in cells
(distances divided by the smallest component of the lattice spacing) for k = 2 .. 8."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--brute", type=int, default=4096)
    ap.add_argument("--simplify", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch

    import tensoir_amd
    from tensoir_amd import mesh, ops
    from tests.helpers import golden_checkpoint
    g = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    model = tensoir_amd.model_from_checkpoint(golden_checkpoint(g), "cuda:0")
    grid = [a.grid] * 3
    cell = min(mesh.reference_spacing(model.aabb.detach().cpu().float(), grid))
    full = mesh.extract_mesh(model, 0.005, grid)[:2]
    simp = mesh.extract_mesh(model, 0.005, grid, simplify=a.simplify)[:2]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    def direction(src, dst):
        used = torch.unique(src[1].reshape(-1).long())
        rows = {"sample_ms": [], "grid_ms": [], "query_ms": []}
        for rep in range(a.reps + 1):                                 # the first pass warms up
            (pts, _), t_s = timed(lambda: ops.sample_surface(src[0], src[1], a.samples, 0))
            fg, t_g = timed(lambda: ops.face_grid(dst[0], dst[1]))
            q = torch.cat([src[0][used], pts])
            _, t_q = timed(lambda: ops.point_mesh_distance(q, dst[0], dst[1], fg))
            if rep:
                rows["sample_ms"].append(t_s)
                rows["grid_ms"].append(t_g)
                rows["query_ms"].append(t_q)
        tested = ops.point_mesh_distance(q, dst[0], dst[1], fg, tested=True)[2]
        out = {k: statistics.median(v) for k, v in rows.items()}
        out.update(queries=int(q.shape[0]), source_faces=int(src[1].shape[0]), target_faces=int(dst[1].shape[0]), dims=fg["dims"],
                   pairs=fg["n_pairs"], tests_per_query=float(tested.double().mean()), tests_max=int(tested.max()))
        return out

    timing = {"a_to_b": direction(simp, full), "b_to_a": direction(full, simp)}
    walls = []
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = mesh.distance(simp, full, samples=a.samples)
        torch.cuda.synchronize()
        if rep:
            walls.append(time.perf_counter() - t0)
    timing["distance_wall_ms"] = statistics.median(walls) * 1e3
    # what the grid buys: the first --brute samples of the simplified mesh against the full mesh, every face tested
    pts = ops.sample_surface(simp[0], simp[1], a.samples, 0)[0][:a.brute].contiguous()
    one, fg = ops.face_grid(full[0], full[1], dims=[1, 1, 1]), ops.face_grid(full[0], full[1])
    brute = {}
    for name, gr in (("brute_ms", one), ("grid_ms", fg)):
        ts = []
        for rep in range(4):
            out, t = timed(lambda: ops.point_mesh_distance(pts, full[0], full[1], gr))
            if rep:
                ts.append(t)
        brute[name] = statistics.median(ts)
        brute[name.replace("_ms", "_dist")] = out[0]
    same = bool(torch.equal(brute.pop("brute_dist").view(torch.int32), brute.pop("grid_dist").view(torch.int32)))
    brute.update(points=int(pts.shape[0]), faces=int(full[1].shape[0]), bit_identical=same, speedup=brute["brute_ms"] / brute["grid_ms"])
    table = []
    for k in range(2, 9):
        v, f, _ = mesh.extract_mesh(model, 0.005, grid, simplify=k)
        d = mesh.distance((v, f), full, samples=a.samples)
        table.append({"k": k, "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "mean_cells": d["a_to_b"]["mean"] / cell,
                      "p95_cells": d["a_to_b"]["p95"] / cell, "max_cells": d["a_to_b"]["max"] / cell,
                      "hausdorff_cells": d["hausdorff"] / cell, "chamfer_cells": d["chamfer"] / cell})
    print(json.dumps({"what": f"mesh.distance(simplified k={a.simplify}, full) of the small golden field at {a.grid}^3, {a.samples} samples per "
                              f"direction, on one MI355X; medians of {a.reps} warm runs, device events", "grid": a.grid,
                      "samples": a.samples, "cell": cell, "full": {"vertices": int(full[0].shape[0]), "faces": int(full[1].shape[0])},
                      "timing": timing, "result": result, "brute_force": brute, "simplify": table}, indent=1))


if __name__ == "__main__":
    main()
