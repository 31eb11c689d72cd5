"""SSIM timing at 800 x 800 x 3 (not part of bench.py).  Needs a GPU: fails without one.

    python tools/metrics_bench.py                  # -> profiles/metrics_ssim.json
    python tools/metrics_bench.py --kernel-only    # a few launches on resident images (what the tool profiles, see (c))

  (a) single_ms      wall time of metrics.ssim on host float32 inputs, upload and synchronise included: median of 20 after 3 warm-ups
  (b) batch4_ms      the same for one batched call of four pairs
  (c) kernel_us      k_ssim alone, from a separate run of this tool under `rocprofv3 --kernel-trace --stats` (a child process)
  (d) hbm_share      the bytes the kernel must read (both images once) over (c), as a share of the HBM peak: the bound below which
                     no SSIM kernel can go is memory; how far above it this one runs is what the share says
  (e) host_ms        the host baseline, the scipy separable form of tests/metrics_reference.py (what the reference's rgb_ssim
                     does), alternated with (a) in the same call; "not measured" where scipy is missing
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H = W = 800
HBM_PEAK = 8.0e12          # bytes / s, MI355X
CPU_FIGURE_MS = 1090.0     # the reference's rgb_ssim at this size on the build machine's CPU (scipy 1.15.3), quoted where (e) is missing


def images(n=1):
    import numpy as np
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    a = np.stack([0.5 + 0.4 * np.sin(7 * xx + c) * np.cos(5 * yy - c) for c in range(3)], -1)[None].repeat(n, 0).astype(np.float32)
    b = np.clip(a + rng.normal(0, 0.05, size=a.shape), 0, 1).astype(np.float32)
    return (a, b) if n > 1 else (a[0], b[0])


def kernel_only(launches=10):
    import torch
    from tensoir_amd import metrics, ops
    a, b = (torch.from_numpy(x[None]).cuda() for x in images())
    for _ in range(launches):
        ops.ssim(a, b, metrics.gaussian_taps(), 0.01 ** 2, 0.03 ** 2)
    torch.cuda.synchronize()


def kernel_time_us():
    """-> (median-free) average k_ssim time in us from a child run under rocprofv3, or None with the reason"""
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ssim", "--", sys.executable,
               os.path.abspath(__file__), "--kernel-only"]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            return None, "rocprofv3 run failed: " + (r.stderr or r.stdout)[-300:]
        for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    if "k_ssim" in row["Name"]:
                        return float(row["AverageNs"]) / 1e3, f"average of {row['Calls']} launches"
    return None, "k_ssim not in the kernel stats"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_ssim.json"))
    ap.add_argument("--host-reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/metrics_bench.py needs a GPU")
    if args.kernel_only:
        return kernel_only()
    from tensoir_amd import metrics
    from tests import metrics_reference as MR
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    a, b = images()
    a4, b4 = images(4)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    single, batch, host = [], [], []
    value = None
    for i in range(23):
        t = wall(lambda: metrics.ssim(a, b))
        t4 = wall(lambda: metrics.ssim(a4, b4))
        if i >= 3:
            single.append(t)
            batch.append(t4)
            if have_scipy and len(host) < args.host_reps and (i - 3) % 4 == 0:
                t0 = time.perf_counter()
                value = MR.ssim_separable(a, b)
                host.append((time.perf_counter() - t0) * 1e3)
    got = float(metrics.ssim(a, b))
    kernel_us, how = kernel_time_us()
    must_read = 2 * H * W * 3 * 4
    out = {"shape": [H, W, 3], "single_ms": statistics.median(single), "single_ms_min": min(single), "batch4_ms": statistics.median(batch),
           "kernel_us": kernel_us, "kernel_us_source": how, "bytes_must_read": must_read,
           "hbm_share": (must_read / (kernel_us * 1e-6) / HBM_PEAK) if kernel_us else None,
           "host_ms": statistics.median(host) if host else "not measured",
           "host_note": f"scipy {scipy.__version__} separable form, median of {len(host)}, alternated with (a)" if host else
                        f"(e) not measured: no scipy on this host; the build machine's CPU took {CPU_FIGURE_MS:.0f} ms (its figure, not this host's)",
           "speedup_over_host": (statistics.median(host) / statistics.median(single)) if host else None,
           "ssim": got, "ssim_minus_host": (got - value) if value is not None else None,
           "device": torch.cuda.get_device_name(0)}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    if host and out["speedup_over_host"] < 20:
        raise SystemExit(f"acceptance floor missed: (a) {out['single_ms']:.2f} ms is not 20x faster than the host baseline {out['host_ms']:.0f} ms")


if __name__ == "__main__":
    main()
