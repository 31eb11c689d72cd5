"""relight.relight_view with and without the guided a-trous denoiser (not part of bench.py).  Needs a GPU: fails without one.

    python tools/denoise_bench.py                      # -> profiles/relight_denoise.json

The configuration is the relight workload's own (bench.py --workload relight): one 800 x 800 view of the 400^3 synthetic
checkpoint under five synthetic 2048 x 1024 HDR maps, chunks of 4096 rays.

  (1) time     wall time per view (host clock, the device waited for before and after) of relight_view: 512 samples without the
               filter, and 128 / 64 / 32 / 16 samples with AtrousConfig(); one warm-up view, then min / median / max of --views.
  (2) quality  per-map PSNR on the hit pixels (acc > 0.5) against the mean of eight independent 512-sample views: of a ninth
               512-sample view as it is, and of a view at each lower sample count before and after the filter.  The mean is taken
               over sRGB values after the clamp, which is not the sRGB of the mean radiance: every figure carries that bias, and
               the reference itself still holds an eighth of a 512-sample view's variance.
  (3) kernels  k_atrous_level and k_denoise_guide alone, from a child run of this tool under `rocprofv3 --kernel-trace --stats`
               (--kernel-only: one filtered 16-sample view).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF_VIEWS, REF_SAMPLES = 8, 512
COUNTS = (128, 64, 32, 16)


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


def kernel_times_us():
    """-> {kernel: {...}} of k_atrous_level / k_denoise_guide from a child run under rocprofv3, or the reason there is none"""
    if shutil.which("rocprofv3") is None:
        return "not measured: rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "denoise", "--", sys.executable,
               os.path.abspath(__file__), "--kernel-only"]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=420)
        except subprocess.TimeoutExpired:
            return "not measured: the rocprofv3 run did not end in 420 s"
        if r.returncode != 0:
            return "not measured: rocprofv3 run failed: " + (r.stderr or r.stdout)[-300:]
        out = {}
        for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    name = re.search(r"k_atrous_level<[^>]*>|k_atrous_level|k_denoise_guide", row["Name"])
                    if name:
                        out[name.group(0)] = {
                            "average_us": float(row["AverageNs"]) / 1e3, "launches": int(row["Calls"]),
                            **{k: float(row[c]) / 1e3 for k, c in (("min_us", "MinNs"), ("max_us", "MaxNs"), ("total_us", "TotalDurationNs"))
                               if row.get(c)}}
    return out or "not measured: the denoiser's kernels are not in the kernel stats"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relight_denoise.json"))
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--grid", type=int, default=400)
    ap.add_argument("--maps", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="one filtered 16-sample view (what (3) profiles)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/denoise_bench.py needs a GPU")
    from tensoir_amd import denoise, relight
    model, env, names, rays = make_scene(args.side, args.grid, args.maps)
    cfg = denoise.AtrousConfig()
    S = args.side

    def view(ns, dn=None):
        return relight.relight_view(model, env, names, rays, S, S, num_samples=ns, chunk=4096, denoise=dn)

    if args.kernel_only:
        view(16, cfg)
        view(16, cfg)
        torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "unknown"),
           "config": {"view": f"{S}x{S}", "grid": args.grid, "maps": f"{args.maps} synthetic 2048x1024", "chunk": 4096,
                      "denoise": {**{k: getattr(cfg, k) for k in ("levels", "sigma_n", "sigma_a", "sigma_r", "sigma_c")},
                                  "sigma_p": 1.0 / cfg.inverses(model.aabb)[1]}, "timed_views": args.views},
           "reference": f"mean of {REF_VIEWS} independent {REF_SAMPLES}-sample views",
           "bias": "the reference is a mean of sRGB values after the clamp, not the sRGB of the mean radiance, and it still holds 1/"
                   f"{REF_VIEWS} of a {REF_SAMPLES}-sample view's variance: a PSNR here is an underestimate against the converged image, "
                   f"by up to 10 log10(1 + 1/{REF_VIEWS}) = {10 * math.log10(1 + 1 / REF_VIEWS):.2f} dB for the {REF_SAMPLES}-sample view"}
    # the eight reference views are the timed 512-sample views as well (at least --views of them)
    ref_sum, ms = None, []
    view(REF_SAMPLES)
    for _ in range(max(REF_VIEWS, args.views)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = view(REF_SAMPLES)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if len(ms) <= REF_VIEWS:
            ref_sum = v["rgb"].double() if ref_sum is None else ref_sum + v["rgb"].double()
    ref = (ref_sum / REF_VIEWS).float()
    hit = v["acc"] > 0.5
    out["hit_pixels"] = int(hit.sum())
    ninth = view(REF_SAMPLES)
    out["raw_512"] = {"ms_per_view": spread(ms), "psnr_per_map": psnr_per_map(ninth["rgb"], ref, hit)}
    out["filtered"] = {}
    for ns in COUNTS:
        t, v = timed_views(lambda: view(ns, cfg), args.views)
        t_raw, _ = timed_views(lambda: view(ns), args.views)
        out["filtered"][str(ns)] = {"ms_per_view": t, "ms_per_view_without_filter": t_raw, "psnr_per_map": psnr_per_map(v["rgb"], ref, hit),
                                    "psnr_per_map_before_filter": psnr_per_map(v["raw"], ref, hit)}
    del ref_sum, ref, ninth, v
    torch.cuda.empty_cache()
    out["kernels"] = kernel_times_us()
    reach = [ns for ns in COUNTS if all(a >= b for a, b in zip(out["filtered"][str(ns)]["psnr_per_map"], out["raw_512"]["psnr_per_map"]))]
    out["sample_counts_reaching_raw_512_psnr_on_every_map"] = reach
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
