"""Timing of the ray-mesh kernel (not part of bench.py) on the 300^3 lattice of the field tools/distance_bench.py
uses (the small golden checkpoint): the full-resolution mesh and its simplify=3 reduction.

    python tools/raymesh_bench.py [--grid 300] [--res 800] [--points 262144] [--samples 262144] [--reps 7] [--brute 4096]

camera: --res x --res pinhole rays from outside the box of the mesh towards its centre, mode "closest", against each mesh over its
default ops.face_grid: the median over --reps warm runs of device events around ops.ray_mesh, the share of rays that hit, and the
ray-triangle tests per ray (mean and max) from a separate instrumented run (tested=True; the kernel does not count the cells it
visits).  count: the same rays in mode "count".  inside: ops.mesh_inside (three "count" launches) of --points uniform points of
the padded box of the mesh.  signed: mesh.distance(simplified, full, signed=True) against the same call without it (wall clock).
brute: --brute camera rays from the middle rows of the frame through a 1 x 1 x 1 grid (every face tested) and through the default
grid; the outputs must be bit-identical."""
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
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--points", type=int, default=262144)
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
    meshes = {"full": mesh.extract_mesh(model, 0.005, grid)[:2], "simplified": mesh.extract_mesh(model, 0.005, grid, simplify=a.simplify)[:2]}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    def median_ms(fn):
        ts = []
        for rep in range(a.reps + 1):                                 # the first pass warms up
            out, t = timed(fn)
            if rep:
                ts.append(t)
        return out, statistics.median(ts)

    # a pinhole camera outside the box of the full mesh, looking at its centre, the box filling most of the frame
    v = meshes["full"][0]
    lo, hi = v.amin(0), v.amax(0)
    centre, radius = (lo + hi) / 2, float((hi - lo).norm()) / 2
    eye = centre + torch.tensor([0.6, -0.64, 0.48], device=v.device) * (3.0 * radius)
    fwd = (centre - eye) / (centre - eye).norm()
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], device=v.device))
    right = right / right.norm()
    up = torch.linalg.cross(right, fwd)
    px = (torch.arange(a.res, device=v.device, dtype=torch.float32) + 0.5) / a.res * 2 - 1
    yy, xx = torch.meshgrid(-px, px, indexing="ij")
    half = 1.1 * radius / (3.0 * radius)                              # tan of half the field of view
    dirs = (fwd + half * (xx[..., None] * right + yy[..., None] * up)).reshape(-1, 3).contiguous()
    origins = eye.expand_as(dirs).contiguous()

    doc = {}
    for name, (mv, mf) in meshes.items():
        fg = ops.face_grid(mv, mf)
        topo = mesh.topology(mv, mf)
        row = {"vertices": int(mv.shape[0]), "faces": int(mf.shape[0]), "dims": fg["dims"], "pairs": fg["n_pairs"], "topology": topo}
        for mode in ("closest", "count"):
            out, ms = median_ms(lambda: ops.ray_mesh(origins, dirs, mv, mf, fg, mode=mode, count=True))
            tested = ops.ray_mesh(origins, dirs, mv, mf, fg, mode=mode, tested=True)[2]
            row[mode] = {"rays": int(dirs.shape[0]), "ms": ms, "mrays_per_s": dirs.shape[0] / ms / 1e3, "hit_share": float((out[1] >= 0).float().mean()),
                         "tests_per_ray": float(tested.double().mean()), "tests_max": int(tested.max())}
        row["count"]["hits_max"] = int(out[2].max())
        pad = 0.05 * (hi - lo)
        pts = (lo - pad) + torch.rand((a.points, 3), device=v.device, generator=torch.Generator(v.device).manual_seed(1)) * (hi - lo + 2 * pad)
        (inside, votes, grazed), ms = median_ms(lambda: ops.mesh_inside(pts, mv, mf, fg))
        row["inside"] = {"points": a.points, "ms": ms, "inside_share": float(inside.float().mean()),
                         "undecided": int(((votes == 1) | (votes == 2)).sum()), "grazed": int(grazed.sum())}
        # what the grid buys: --brute camera rays, every face tested
        centre_rows = slice((a.res // 2) * a.res, (a.res // 2) * a.res + a.brute)              # rows through the middle of the frame: they hit
        o, d = origins[centre_rows].contiguous(), dirs[centre_rows].contiguous()
        one = ops.face_grid(mv, mf, dims=[1, 1, 1])
        brute = {}
        outs = {}
        for key, gr in (("brute_ms", one), ("grid_ms", fg)):
            ts = []
            for rep in range(4):
                outs[key], t = timed(lambda: ops.ray_mesh(o, d, mv, mf, gr, mode="count", bary=True, count=True, flags=True))
                if rep:
                    ts.append(t)
            brute[key] = statistics.median(ts)
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs["brute_ms"], outs["grid_ms"]))
        assert same, "the grid and the 1 x 1 x 1 grid disagree"
        brute.update(rays=int(o.shape[0]), hit_share=float((outs["grid_ms"][1] >= 0).float().mean()), bit_identical=same,
                     speedup=brute["brute_ms"] / brute["grid_ms"])
        row["brute_force"] = brute
        doc[name] = row

    closed = all(doc[n]["topology"]["closed"] for n in doc)
    walls = {"plain": [], "signed": []}
    for rep in range(a.reps + 1):
        for key, kw in (("plain", {}), ("signed", {"signed": True, "allow_open": not closed})):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = mesh.distance(meshes["simplified"], meshes["full"], samples=a.samples, **kw)
            torch.cuda.synchronize()
            if rep:
                walls[key].append(time.perf_counter() - t0)
    signed = {k: statistics.median(w) * 1e3 for k, w in walls.items()}
    print(json.dumps({"what": f"ops.ray_mesh / mesh_inside / mesh.distance(signed=True) on the small golden field at {a.grid}^3 and its "
                              f"simplify={a.simplify} reduction, on one MI355X; medians of {a.reps} warm runs, device events (distance: wall clock)",
                      "grid": a.grid, "res": a.res, "meshes": doc,
                      "distance_wall_ms": {"plain": signed["plain"], "signed": signed["signed"], "samples": a.samples, "both_closed": closed},
                      "signed_result": result}, indent=1))


if __name__ == "__main__":
    main()
