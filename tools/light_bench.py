"""Time tir_light_gbuffer on a synthetic G-buffer: an --image x --image view of a unit sphere that fills --fill of the
image's width (normals of the sphere, random albedo and roughness, the rest empty), lit by rows x 2 rows cells of a seeded map.
One JSON line per cell grid: device-event time per call over --reps calls after a warm-up, and pairs (covered pixels x cells) per
second.  Needs a GPU.
    python tools/light_bench.py [--image 800] [--rows 16 32 64] [--reps 50] [--out profiles/light_800.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def gbuffer(side, fill, seed=0):
    j, i = np.meshgrid(np.arange(side) + 0.5, np.arange(side) + 0.5, indexing="ij")
    r = 0.5 * fill * side
    x, y = (i - side / 2) / r, (j - side / 2) / r
    inside = x * x + y * y < 1
    z = np.sqrt(np.where(inside, 1 - x * x - y * y, 0.0))
    rng = np.random.default_rng(seed)
    g = np.zeros((side, side, 12), np.float32)
    g[..., 0:3] = rng.uniform(0, 1, (side, side, 3))
    g[..., 3] = rng.uniform(0.09, 0.99, (side, side))
    g[..., 4] = 1.0
    g[..., 5], g[..., 6], g[..., 7] = x, y, z
    g[..., 8] = inside
    g[~inside] = 0
    view = np.zeros((side, side, 3), np.float32)
    view[..., 2] = 1.0
    return g.reshape(-1, 12), view.reshape(-1, 3), int(inside.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", type=int, default=800)
    ap.add_argument("--fill", type=float, default=0.9)
    ap.add_argument("--rows", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("light_bench: no GPU")
    from tensoir_amd import ops, synth
    g, v, covered = gbuffer(a.image, a.fill)
    g, v = torch.from_numpy(g).cuda(), torch.from_numpy(v).cuda()
    results = []
    for rows in a.rows:
        hdr = synth.make_hdr_maps(("city",), 4 * rows, 8 * rows)["city"].cuda() * 0.05
        cells = ops.env_cells(hdr, rows, 2 * rows)
        for _ in range(3):
            out = ops.light_gbuffer(g, v, cells, 0.04, True, True)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            out = ops.light_gbuffer(g, v, cells, 0.04, True, True)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        pairs = covered * cells.shape[0]
        row = {"image": a.image, "covered_pixels": covered, "cells": int(cells.shape[0]), "ms_per_call": ms, "reps": a.reps,
               "pairs_per_s": pairs / (ms * 1e-3), "mean_rgb": float(out[:, :3].sum() / max(covered, 1) / 3)}
        print(json.dumps(row))
        results.append(row)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/light_bench.py", "device": torch.cuda.get_device_name(0), "results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
