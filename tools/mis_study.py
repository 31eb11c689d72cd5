"""relight.relight_view with the map-only estimator (mis=None) and with multiple importance sampling of the map and the BRDF lobes
(mis=MisConfig()): image quality per sample count, time per view, the two new kernels' times.  Not part of bench.py.
Needs a GPU: fails without one.

    python tools/mis_study.py [--parent-root DIR]       # -> profiles/mis_relight.json

The configuration and the protocol are tools/denoise_bench.py's: one 800 x 800 view of the 400^3 synthetic
checkpoint under five synthetic 2048 x 1024 HDR maps, chunks of 4096 rays; per-map PSNR on the hit pixels against the mean of
eight independent 512-sample views.

  (1) quality  PSNR at 16, 64 and 512 samples for both estimators, raw and after the guided a-trous filter (AtrousConfig()), against
               TWO references: the mean of eight 512-sample views of the map-only estimator (section 4.13's) and that of eight
               MisConfig() views.  The map-only estimator samples cell centres -- a quadrature over the map's cells -- while the
               other one integrates the piecewise-constant map; they converge to images that differ slightly
               ("between_references"), and each reference favours its own estimator.
  (2) time     wall time per view (host clock, the device waited for before and after), one warm-up view, then min / median / max
               of --views, for both estimators at every count, raw and filtered.
  (3) kernels  k_env_mis_setup and k_relight_mis next to k_env_sample_list, k_relight_importance_cells and the visibility march,
               from a child run of this tool under `rocprofv3 --kernel-trace --stats` (--kernel-only: one 512-sample view each way).
  (4) parent   with --parent-root (a checkout of the parent commit with its library built): time per view with mis=None from
               child processes that import the package of either checkout, alternating parent / this / parent / this.
"""
import argparse
import contextlib
import csv
import glob
import io
import json
import math
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_VIEWS, REF_SAMPLES = 8, 512
COUNTS = (16, 64, 512)
KERNELS = r"k_env_mis_setup|k_relight_mis|k_env_sample_list|k_relight_importance_cells<[^>]*>|k_march_secondary\w*(?:<[^>]*>)?"


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def make_scene(side, grid, n_maps):
    import torch
    import tensoir_amd
    from tensoir_amd import relight, synth
    model = tensoir_amd.model_from_checkpoint(synth.make_checkpoint(grid=(grid,) * 3, seed=20211202), "cuda")
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        model.updateAlphaMask((128, 128, 128))
    maps = synth.make_hdr_maps([f"env{i}" for i in range(n_maps)], 1024, 2048)
    env = relight.Environment_Light(hdr_maps=maps, device="cuda")
    return model, env, list(maps), synth.make_rays(side, side, narrow=1.0).cuda()


def timed_views(render, views):
    import torch
    render()                                                   # warm-up: record capacities, lazily built tables
    ms = []
    for _ in range(views):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = render()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms), out


def psnr_per_map(img, ref, hit):
    """img, ref [n_maps, H, W, 3], hit [H, W] -> PSNR per map over the hit pixels (peak 1)"""
    out = []
    for m in range(img.shape[0]):
        mse = float(((img[m][hit] - ref[m][hit]).double() ** 2).mean())
        out.append(round(-10.0 * math.log10(max(mse, 1e-300)), 3))
    return out


def child(args, root, *flags, timeout=600):
    """this tool in a fresh process that imports the package under `root` -> its last output line as JSON"""
    root = os.path.abspath(root)
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--views", str(args.views), "--side", str(args.side), "--grid", str(args.grid),
           "--maps", str(args.maps), *flags]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"child run failed ({' '.join(cmd)}): " + (r.stderr or r.stdout)[-400:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_times_us(args):
    """-> {kernel: {...}} from a child run under rocprofv3, or the reason there is none"""
    if shutil.which("rocprofv3") is None:
        return "not measured: rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "mis", "--", sys.executable,
               os.path.abspath(__file__), "--kernel-only", "--side", str(args.side), "--grid", str(args.grid), "--maps", str(args.maps)]
        try:
            r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True, timeout=420)
        except subprocess.TimeoutExpired:
            return "not measured: the rocprofv3 run did not end in 420 s"
        if r.returncode != 0:
            return "not measured: rocprofv3 run failed: " + (r.stderr or r.stdout)[-300:]
        out = {}
        for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    name = re.search(KERNELS, row["Name"])
                    if name:
                        out[name.group(0)] = {
                            "average_us": float(row["AverageNs"]) / 1e3, "launches": int(row["Calls"]),
                            **{k: float(row[c]) / 1e3 for k, c in (("min_us", "MinNs"), ("max_us", "MaxNs"), ("total_us", "TotalDurationNs"))
                               if row.get(c)}}
    return out or "not measured: the relighting kernels are not in the kernel stats"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "mis_relight.json"))
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--grid", type=int, default=400)
    ap.add_argument("--maps", type=int, default=5)
    ap.add_argument("--root", default=HERE, help="the checkout whose tensoir_amd package is imported")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, library built: adds (4)")
    ap.add_argument("--kernel-only", action="store_true", help="one 512-sample view each way (what (3) profiles)")
    ap.add_argument("--time-none", action="store_true", help="time per view with the map-only estimator alone; one JSON line")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/mis_study.py needs a GPU")
    from tensoir_amd import denoise, relight
    model, env, names, rays = make_scene(args.side, args.grid, args.maps)
    cfg = denoise.AtrousConfig()
    S = args.side

    def view(ns, mis=None, dn=None):
        kw = {} if mis is None else {"mis": mis}               # (the parent commit's relight_view has no such argument)
        return relight.relight_view(model, env, names, rays, S, S, num_samples=ns, chunk=4096, denoise=dn, **kw)

    if args.time_none:
        stamp = os.path.join(os.path.dirname(os.path.abspath(relight.__file__)), "libtensoir_hip.so.srchash")
        print(json.dumps({"library_source_hash": open(stamp).read().strip() if os.path.exists(stamp) else "unknown",
                          "ms_per_view": {str(ns): timed_views(lambda: view(ns), args.views)[0] for ns in COUNTS}}))
        return
    mis = relight.MisConfig()
    if args.kernel_only:
        for m in (None, mis):
            view(REF_SAMPLES, m)
            view(REF_SAMPLES, m)
        torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "unknown"),
           "config": {"view": f"{S}x{S}", "grid": args.grid, "maps": f"{args.maps} synthetic 2048x1024", "chunk": 4096, "mis": repr(mis),
                      "denoise": {**{k: getattr(cfg, k) for k in ("levels", "sigma_n", "sigma_a", "sigma_r", "sigma_c")},
                                  "sigma_p": 1.0 / cfg.inverses(model.aabb)[1]}, "timed_views": args.views},
           "references": {"none": f"mean of {REF_VIEWS} independent {REF_SAMPLES}-sample views, mis=None",
                          "mis": f"mean of {REF_VIEWS} independent {REF_SAMPLES}-sample views, {mis!r}"},
           "bias": "a reference is a mean of sRGB values after the clamp, not the sRGB of the mean radiance, and still holds 1/"
                   f"{REF_VIEWS} of a {REF_SAMPLES}-sample view's variance; the two estimators converge to slightly different images "
                   "(cell-centre quadrature against the integral of the piecewise-constant map), so each reference favours its own"}
    refs = {}
    for key, m in (("none", None), ("mis", mis)):
        view(REF_SAMPLES, m)
        acc = None
        for _ in range(REF_VIEWS):
            v = view(REF_SAMPLES, m)
            acc = v["rgb"].double() if acc is None else acc + v["rgb"].double()
        refs[key] = (acc / REF_VIEWS).float()
    hit = v["acc"] > 0.5
    out["hit_pixels"] = int(hit.sum())
    out["between_references_psnr_per_map"] = psnr_per_map(refs["mis"], refs["none"], hit)
    out["samples"] = {}
    for ns in COUNTS:
        row = {}
        for key, m in (("none", None), ("mis", mis)):
            t_raw, _ = timed_views(lambda: view(ns, m), args.views)
            t_flt, v = timed_views(lambda: view(ns, m, cfg), args.views)
            row[key] = {"ms_per_view": t_raw, "ms_per_view_filtered": t_flt,
                        **{f"psnr_per_map_{kind}_vs_{r}": psnr_per_map(v[img], refs[r], hit)
                           for kind, img in (("raw", "raw"), ("filtered", "rgb")) for r in refs}}
        out["samples"][str(ns)] = row
    del refs, acc, v
    torch.cuda.empty_cache()
    out["kernels"] = kernel_times_us(args)
    if args.parent_root:
        runs = [(which, child(args, root, "--time-none")) for which, root in
                (("parent", args.parent_root), ("this", HERE), ("parent", args.parent_root), ("this", HERE))]
        out["mis_none_vs_parent"] = {"order": [w for w, _ in runs], "runs": [r["ms_per_view"] for _, r in runs],
                                     "library_source_hash": {w: r["library_source_hash"] for w, r in runs}}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
