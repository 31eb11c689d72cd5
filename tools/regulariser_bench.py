"""Total-variation regulariser: the fused kernels against the eager PyTorch path (not part of bench.py).  Needs a GPU: fails without one.

    python tools/regulariser_bench.py                  # -> profiles/tv_regulariser.json

Both sides run in this process on this build.  The eager side is the path before the kernels existed: the same model methods
(TV_loss_density / TV_loss_app) given a plain callable; the fused side gives them regularisers.TVLoss().

  (1) alone     the armadillo plane shapes (3 x [1, 16, g, g] + 3 x [1, 48, g, g]) at g = 128 and g = 300: forward plus backward of
                TV_loss_density * 0.05 + TV_loss_app * 0.005.  gpu_us: device events around a window of calls, per call.  host_us:
                the host clock around the same window with nothing waited on inside it, per call (how long the host is busy
                enqueueing).  launches: the device activities of one call by name, from torch.profiler (kernels, memsets and copies
                counted apart; "not measured" where it cannot).
                The two sides alternate; min / median / max over the windows.
  (2) loop      tests/train_sequence.reconstruct in its radiance-only phase at grid0 = 128 (mask updates and up-sampling placed
                beyond the end), once with train_sequence.tv as it is and once with it replaced by regularisers.TVLoss(): ms per
                iteration (the loop waits for its loss every iteration, so the host clock per iteration is the iteration), the
                median over the iterations after the warm-up; the runs alternate, min / median / max over the runs.

  (3) kernels   k_tv_fwd and k_tv_bwd alone at both sizes, from child runs of this tool under `rocprofv3 --kernel-trace --stats`
                (--kernel-only G: ten forward and ten backward launches on resident planes), and the bytes each must move (forward:
                every plane read once; backward: read once and written once) over that time as a share of the HBM peak.

Acceptance (checked after the file is written): on both sizes the fused side's median is no higher than the eager side's in GPU
time and in host time, and in (2) the fused per-iteration time is no higher, each allowing the eager side's own spread (max - min).
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
TV_D, TV_A = 0.05, 0.005
HBM_PEAK = 8.0e12          # bytes / s, MI355X


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def plain_tv(x):
    """the reference's expression as a plain callable (tests/helpers.tv_loss)"""
    n, c, h, w = x.shape
    dh = (x[:, :, 1:, :] - x[:, :, :h - 1, :]).pow(2).sum()
    dw = (x[:, :, :, 1:] - x[:, :, :, :w - 1]).pow(2).sum()
    return 2 * (dh / (c * (h - 1) * w) + dw / (c * h * (w - 1))) / n


def make_model(g):
    import torch
    from tensoir_amd import TensorVMSplit
    torch.manual_seed(0)
    return TensorVMSplit(aabb=torch.tensor([[-1.5] * 3, [1.5] * 3]), gridSize=[g, g, g], device="cuda", density_n_comp=[16] * 3,
                         appearance_n_comp=[48] * 3, shadingMode="MLP_Fea", light_kind="sg", normals_kind="purely_predicted", pos_pe=2,
                         view_pe=2, fea_pe=2)


def one_call(m, reg):
    for p in list(m.density_plane) + list(m.app_plane):
        p.grad = None
    loss = m.TV_loss_density(reg) * TV_D + m.TV_loss_app(reg) * TV_A
    loss.backward()
    return loss


def count_launches(m, reg):
    """-> {"kernels": n, "memsets": n, "memcpys": n, "names": {device activity: count}} of one call, from torch.profiler: every
    device activity by name, so that what the count consists of can be read off"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        one_call(m, reg)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            one_call(m, reg)
            torch.cuda.synchronize()
        names = {}
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA"):
                names[e.name] = names.get(e.name, 0) + 1
        if not names:
            return "not measured: the profiler recorded no device activity"
        is_set = lambda k: "memset" in k.lower()
        is_cpy = lambda k: "memcpy" in k.lower()
        return {"kernels": sum(v for k, v in names.items() if not is_set(k) and not is_cpy(k)),
                "memsets": sum(v for k, v in names.items() if is_set(k)), "memcpys": sum(v for k, v in names.items() if is_cpy(k)),
                "names": dict(sorted(names.items()))}
    except Exception as e:                                    # a torch build without device tracing
        return f"not measured: {type(e).__name__}: {e}"[:200]


def alone(g, windows, calls, warmup):
    import torch
    from tensoir_amd import regularisers
    m = make_model(g)
    sides = {"eager": plain_tv, "fused": regularisers.TVLoss()}
    out = {"grid": g, "plane_shapes": [list(p.shape) for p in list(m.density_plane) + list(m.app_plane)],
           "floats": sum(p.numel() for p in list(m.density_plane) + list(m.app_plane)), "calls_per_window": calls, "windows": windows}
    values, grads = {}, {}
    for name, reg in sides.items():
        for _ in range(warmup):
            loss = one_call(m, reg)
        values[name] = float(loss.detach())
        grads[name] = [p.grad.detach().clone() for p in list(m.density_plane) + list(m.app_plane)]
    out["loss"] = values
    out["loss_rel_diff"] = abs(values["fused"] - values["eager"]) / abs(values["eager"])
    out["grad_max_rel_diff"] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads["fused"], grads["eager"]))
    del grads
    gpu, host = {k: [] for k in sides}, {k: [] for k in sides}
    for w in range(windows):
        order = list(sides) if w % 2 == 0 else list(sides)[::-1]
        for name in order:
            reg = sides[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(calls):
                one_call(m, reg)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            gpu[name].append(e0.elapsed_time(e1) * 1e3 / calls)
            host[name].append((t1 - t0) * 1e6 / calls)
    for name, reg in sides.items():
        out[name] = {"gpu_us": spread(gpu[name]), "host_us": spread(host[name]), "launches": count_launches(m, reg)}
    del m
    torch.cuda.empty_cache()
    return out


def kernel_only(g, launches=10):
    import torch
    from tensoir_amd import ops
    m = make_model(g)
    planes = [p.detach() for p in list(m.density_plane) + list(m.app_plane)]
    coefs = [TV_D * 1e-2] * 3 + [TV_A * 1e-2] * 3
    up = torch.ones((), dtype=torch.float32, device="cuda")
    for _ in range(launches):
        ops.tv_forward(planes, coefs)
        ops.tv_backward(planes, coefs, up)
    torch.cuda.synchronize()


def kernel_times_us(g):
    """-> {kernel: average us} of k_tv_fwd / k_tv_bwd at grid g from a child run under rocprofv3, or the reason there is none"""
    if shutil.which("rocprofv3") is None:
        return "not measured: rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "tv", "--", sys.executable,
               os.path.abspath(__file__), "--kernel-only", str(g)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            return "not measured: rocprofv3 run failed: " + (r.stderr or r.stdout)[-300:]
        out = {}
        for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    for k in ("k_tv_fwd", "k_tv_bwd"):
                        if k in row["Name"]:
                            out[k] = {"average_us": float(row["AverageNs"]) / 1e3, "launches": int(row["Calls"])}
    return out or "not measured: k_tv_* not in the kernel stats"


def loop(runs, iters, warmup, batch):
    import torch
    from tensoir_amd import regularisers
    from tests import train_sequence
    eager_tv = train_sequence.tv
    sides = {"eager": eager_tv, "fused": regularisers.TVLoss()}
    per_run = {k: [] for k in sides}
    last_loss = {}
    try:
        for r in range(runs):
            order = list(sides) if r % 2 == 0 else list(sides)[::-1]
            for name in order:
                train_sequence.tv = sides[name]                   # reconstruct() reads the module's `tv` when it runs
                stamps = []
                res = train_sequence.reconstruct(n_iters=iters, batch=batch, upsamp=(10 ** 9,), mask_updates=(10 ** 9, 10 ** 9 + 1),
                                                 dataset="synthetic:views=8,res=48", grid0=128, grid1=128,
                                                 on_iter=lambda it, m, ret: stamps.append(time.perf_counter()))
                torch.cuda.synchronize()
                d = [(b - a) * 1e3 for a, b in zip(stamps[warmup:-1], stamps[warmup + 1:])]
                per_run[name].append(statistics.median(d))
                last_loss[name] = res.losses[-1]
                del res
                torch.cuda.empty_cache()
    finally:
        train_sequence.tv = eager_tv
    return {"grid0": 128, "iters": iters, "warmup_iters": warmup, "batch": batch, "runs": runs, "final_image_loss": last_loss,
            "eager": {"ms_per_iter": spread(per_run["eager"])}, "fused": {"ms_per_iter": spread(per_run["fused"])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tv_regulariser.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--kernel-only", type=int, default=0, metavar="G", help="a few launches on resident planes of grid G (what (3) profiles)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/regulariser_bench.py needs a GPU")
    if args.kernel_only:
        return kernel_only(args.kernel_only)
    out = {"device": torch.cuda.get_device_name(0), "weights": {"TV_weight_density": TV_D, "TV_weight_app": TV_A},
           "alone": [alone(g, args.windows, args.calls, warmup=5) for g in (128, 300)]}
    if not args.skip_loop:
        out["loop"] = loop(args.runs, args.iters, warmup=50, batch=args.batch)
    for a in out["alone"]:
        k = a["kernels"] = kernel_times_us(a["grid"])
        if isinstance(k, dict):
            for name, passes in (("k_tv_fwd", 1), ("k_tv_bwd", 2)):
                if name in k:
                    k[name]["bytes_must_move"] = passes * 4 * a["floats"]
                    k[name]["hbm_share"] = k[name]["bytes_must_move"] / (k[name]["average_us"] * 1e-6) / HBM_PEAK
    missed = []
    for a in out["alone"]:
        for key in ("gpu_us", "host_us"):
            e, f = a["eager"][key], a["fused"][key]
            if f["median"] > e["median"] + (e["max"] - e["min"]):
                missed.append(f"alone grid {a['grid']} {key}: fused {f['median']:.1f} above eager {e['median']:.1f} (spread {e['max'] - e['min']:.1f})")
    if "loop" in out:
        e, f = out["loop"]["eager"]["ms_per_iter"], out["loop"]["fused"]["ms_per_iter"]
        if f["median"] > e["median"] + (e["max"] - e["min"]):
            missed.append(f"loop: fused {f['median']:.3f} ms above eager {e['median']:.3f} ms (spread {e['max'] - e['min']:.3f})")
    out["acceptance"] = "met" if not missed else missed
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    if missed:
        raise SystemExit("acceptance missed: " + "; ".join(missed))


if __name__ == "__main__":
    main()
