"""Forward / backward time of the per-point autograd methods (tensoir_amd/pointwise.py) at 2^20 points.

Three point orders: `random` (uniform in the box), `ray` (4096 straight rays x 256 samples half a voxel apart, in ray order --
the order of the training step's records) and `sorted` (the random points sorted by their density-plane-0 cell with
torch.argsort first; the sort is included in the time).  Times are device events around the call after a warm-up, the median
of --reps repetitions.  For the scatter-bound backwards the line also gives the atomic bytes added per second against the
chip-wide fp32 atomic rate of ~1.3 TB/s (MI355X_MICROARCH.md, global float atomics):
density 3 x (4 + 2) taps x n_dcomp floats per point, appearance 3 x (4 + 2) taps x n_acomp floats per point.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/pointwise_bwd_bench.py`.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ATOMIC_RATE = 1.3e12


def make_model(grid, dcomp, acomp):
    from tensoir_amd import TensorVMSplit
    torch.manual_seed(0)
    m = TensorVMSplit(aabb=torch.tensor([[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]), gridSize=[grid] * 3, device="cuda",
                      density_n_comp=dcomp, appearance_n_comp=acomp, shadingMode="MLP_Fea", light_kind="sg")
    with torch.no_grad():
        for p in m.density_plane:
            p.mul_(30.0)
    return m


def point_sets(n, grid, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rnd = torch.rand(n, 3, device="cuda", generator=gen) * 1.98 - 0.99
    S = 256
    B = n // S
    o = torch.rand(B, 3, device="cuda", generator=gen) * 1.6 - 0.8
    d = torch.nn.functional.normalize(torch.randn(B, 3, device="cuda", generator=gen), dim=-1)
    k = torch.arange(S, device="cuda", dtype=torch.float32) - S / 2
    ray = (o[:, None, :] + d[:, None, :] * k[None, :, None] * (1.0 / (grid - 1))).reshape(-1, 3).clamp(-0.99, 0.99)
    return {"random": rnd, "ray": ray.contiguous()}


def cell_sort(x, grid):
    """Random points -> ordered by their density-plane-0 cell (x, y) and line cell z."""
    i = ((x + 1) * 0.5 * (grid - 1)).floor().long().clamp(0, grid - 1)
    key = (i[:, 1] * grid + i[:, 0]) * grid + i[:, 2]
    return x[torch.argsort(key)]


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def methods(m):
    li = None

    def app(x):
        nonlocal li
        if li is None or li.shape[0] != x.shape[0]:
            li = torch.zeros(x.shape[0], dtype=torch.int32, device="cuda")
        return m.compute_appfeature(x, li)

    return {
        "densityfeature": (m.compute_densityfeature, "density"),
        "alpha": (lambda x: m.compute_alpha(x * 1.5), "density"),
        "densityfeature_with_xyz_grad": (m.compute_densityfeature_with_xyz_grad, "density"),
        "derived_normals": (lambda x: m.compute_derived_normals(x.clone()), "density"),
        "appfeature": (app, "app"),
        "intrinfeature": (m.compute_intrinfeature, "app"),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    m = make_model(args.grid, 16, 48)
    sets = point_sets(args.n, args.grid)
    sets["sorted"] = sets["random"]
    for name, (fn, kind) in methods(m).items():
        if args.only and name not in args.only.split(","):
            continue
        floats = 3 * 6 * (m.density_n_comp[0] if kind == "density" else m.app_n_comp[0])
        for order, x in sets.items():
            prep = (lambda x=x: cell_sort(x, args.grid)) if order == "sorted" else (lambda x=x: x)
            with torch.no_grad():
                fn(x)
            fwd = timed(lambda: fn(prep()), args.reps)

            def step():
                out = fn(prep())
                outs = out if isinstance(out, tuple) else (out,)
                torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])

            step()
            tot = timed(step, args.reps)
            bwd = max(tot - fwd, 1e-6)
            abytes = args.n * floats * 4
            print(json.dumps({"method": name, "order": order, "n": args.n, "fwd_ms": round(fwd, 4),
                              "fwd_bwd_ms": round(tot, 4), "bwd_ms": round(bwd, 4),
                              "atomic_GBps": round(abytes / (bwd * 1e-3) / 1e9, 1),
                              "atomic_floor_ms": round(abytes / ATOMIC_RATE * 1e3, 3)}), flush=True)
            for p in m.parameters():
                p.grad = None


if __name__ == "__main__":
    main()
