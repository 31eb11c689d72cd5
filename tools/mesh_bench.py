"""Mesh export timing (not part of bench.py): dense alpha lattice (tir_dense_alpha), marching cubes (tir_mc_*) and the
connected-component filter (tir_ccl_*: label + table, filter) at the final grid sizes of a scene, on the small golden
checkpoint's field or (--trained) on the field tests/train_sequence.reconstruct() trains.

    python tools/mesh_bench.py [--grids 300,512] [--reps 3]      # event-timed passes, counts, export_mesh wall time
    python tools/mesh_bench.py --trained --connectivity 26       # the trained lattice (a few seconds of training first)
    python tools/mesh_bench.py --trained --grids 300 --simplify 2,3,4     # + the simplification of the full mesh per cluster size
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mesh -- python tools/mesh_bench.py --grids 300
    python tools/mesh_bench.py --stats DIR                       # per-kernel GPU time from that trace

One JSON line per grid: dense_alpha_ms / mc_ms / ccl_label_ms / ccl_filter_ms (CUDA events around the calls; the marching-cubes
and labelling figures include their one read-back of the totals), components, vertices, faces, export_s (extract_mesh +
write_ply, wall clock, after a warm-up export) and export_keep1_s (the same with keep_largest=1).  With --simplify K[,K...]:
"simplify": {K: {"ms", "vertices", "faces"}}, mesh.simplify_extracted (ops.simplify_mesh and the rescaling of its normals) on the
marching-cubes mesh of the same pass (events around the call, its read-back of the totals included, best of --reps after one
warm-up call).
"""
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


def stats(d):
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    keep = ("k_dense_alpha", "k_mc_", "k_exclusive_scan", "k_ccl_", "k_simplify_")
    out = {}
    for r in rows:
        name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        if any(k in name for k in keep):
            out[name] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                         "avg_us": float(r["AverageNs"]) / 1e3}
    mc = sum(v["total_ms"] for k, v in out.items() if "k_mc_" in k or "k_exclusive_scan" in k)
    da = sum(v["total_ms"] for k, v in out.items() if "k_dense_alpha" in k)
    ccl = sum(v["total_ms"] for k, v in out.items() if "k_ccl_" in k)
    # (k_exclusive_scan is shared: marching cubes runs it twice per call, the labelling once)
    print(json.dumps({"kernels": out, "dense_alpha_total_ms": da, "marching_cubes_total_ms": mc, "components_total_ms": ccl}, indent=1))


def run(grids, reps, trained=False, connectivity=6, simplify=()):
    import numpy as np
    import torch

    import tensoir_amd
    from tensoir_amd import mesh, ops
    if trained:
        from tests.train_sequence import reconstruct
        model = reconstruct().model
    else:
        from tests.helpers import golden_checkpoint
        g = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
        eh, ew = [int(x) for x in g["scene/envmap_hw"]]
        model = tensoir_amd.model_from_checkpoint(golden_checkpoint(g), "cuda:0", envmap_h=eh, envmap_w=ew)
    aabb = model.aabb.detach().cpu().float()
    for n in grids:
        grid = [n, n, n]
        sp = mesh.reference_spacing(aabb, grid)
        da, mc, lab, flt = [], [], [], []
        for _ in range(reps):
            e0, e1, e2, e3, e4 = (torch.cuda.Event(enable_timing=True) for _ in range(5))
            e0.record()
            alpha, _ = ops.dense_alpha(model.packed_field(), grid, float(model.stepSize))
            e1.record()
            v, f, nrm = ops.marching_cubes(alpha, 0.005, sp, aabb[0].tolist())
            e2.record()
            labels, table = ops.label_components(alpha, 0.005, connectivity)      # (timed on its own below)
            kept = mesh.select_components(table, keep_largest=1)                  # (a host policy: outside the timed spans)
            torch.cuda.synchronize()
            e3.record()
            filtered = ops.keep_components(alpha, labels, table, kept, fill=0.0, level=0.005)
            e4.record()
            torch.cuda.synchronize()
            da.append(e0.elapsed_time(e1))
            mc.append(e1.elapsed_time(e2))
            flt.append(e3.elapsed_time(e4))
            n_comp, largest = int(table["roots"].shape[0]), int(table["sizes"].max()) if table["roots"].shape[0] else 0
            del alpha, labels, filtered
        # the labelling span (label + table, with the read-back of the component count) on its own
        alpha, _ = ops.dense_alpha(model.packed_field(), grid, float(model.stepSize))
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            labels, table = ops.label_components(alpha, 0.005, connectivity)
            e1.record()
            torch.cuda.synchronize()
            lab.append(e0.elapsed_time(e1))
        del alpha, labels
        simp = {}
        for k in simplify:
            ms = []
            for r in range(reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sv, sf, _, _ = mesh.simplify_extracted(v, f, aabb, grid, k)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    ms.append(e0.elapsed_time(e1))
            simp[k] = {"ms": min(ms), "vertices": int(sv.shape[0]), "faces": int(sf.shape[0])}
            del sv, sf
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.ply")
            mesh.export_mesh(model, path, gridSize=grid)      # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nv, nf = mesh.export_mesh(model, path, gridSize=grid)
            export_s = time.perf_counter() - t0
            ply_bytes = os.path.getsize(path)
            t0 = time.perf_counter()
            mesh.export_mesh(model, path, gridSize=grid, keep_largest=1, connectivity=connectivity)
            export_keep1_s = time.perf_counter() - t0
        print(json.dumps({"grid": n, "dense_alpha_ms": min(da), "mc_ms": min(mc), "ccl_label_ms": min(lab), "ccl_filter_ms": min(flt),
                          "connectivity": connectivity, "components": n_comp, "largest_component": largest,
                          "export_keep1_s": export_keep1_s, "vertices": int(v.shape[0]),
                          "faces": int(f.shape[0]), "export_s": export_s, "export_vertices": nv, "export_faces": nf,
                          "ply_bytes": ply_bytes, **({"simplify": simp} if simp else {})}), flush=True)
        del v, f, nrm
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="300,512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats", default=None, help="summarise the rocprofv3 kernel stats under this directory and exit")
    ap.add_argument("--trained", action="store_true", help="time the field tests/train_sequence.reconstruct() trains")
    ap.add_argument("--connectivity", type=int, choices=(6, 26), default=6)
    ap.add_argument("--simplify", default="", metavar="K[,K...]", help="also time the simplification of the full mesh with clusters "
                    "of K x K x K cells")
    a = ap.parse_args()
    if a.stats:
        return stats(a.stats)
    run([int(x) for x in a.grids.split(",")], a.reps, a.trained, a.connectivity, [int(x) for x in a.simplify.split(",") if x])


if __name__ == "__main__":
    main()
