"""Time material editing (not part of bench.py):
  view      one --image x --image relight_view (one synthetic map, --samples samples, the synthetic 96^3 field the denoiser's tests
            use; the Environment_Light is built before the clock starts) without edits and with a 4-edit list (sphere, box, colour
            and roughness-band selectors; recolour, metal, roughness)
  edit      tir_material_edit_maps alone on one chunk of that view's map rows
  palette   materials.palette_of at --palette-rows rows, k = --k, on seeded Gaussian blobs of (albedo, roughness): the whole call,
            its passes, and one assign + update pair
Device events, medians of --reps warm runs after one warm-up.  One JSON line per measurement; --out writes them all.  Needs a GPU.
    python tools/material_edit_bench.py [--image 800] [--samples 64] [--palette-rows 262144] [--k 8] [--reps 5] [--out profiles/material_edit.json]"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def median_ms(fn, reps):
    out, _ = timed(fn)                                                  # the first call warms up
    times = []
    for _ in range(reps):
        out, ms = timed(fn)
        times.append(ms)
    return out, float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", type=int, default=800)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--palette-rows", type=int, default=262144)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("material_edit_bench: no GPU")
    import tensoir_amd
    from tensoir_amd import materials, ops, relight, synth
    from tensoir_amd.materials import EditList, MaterialEdit as E
    results = []

    def emit(row):
        print(json.dumps(row), flush=True)
        results.append(row)

    model = tensoir_amd.model_from_checkpoint(synth.make_checkpoint(grid=(96,) * 3), "cuda")
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        model.updateAlphaMask((48,) * 3)
    maps = synth.make_hdr_maps(["city"], 32, 64)
    rays = synth.make_rays(a.image, a.image).cuda()
    edits = EditList([E(sphere_center=(0.0, 0.0, 0.2), sphere_radius=0.3, sphere_feather=0.2, albedo_mode="recolor", color=(0.1, 0.2, 0.9)),
                      E(box_center=(0.0, 0.0, -0.3), box_half=(1.0, 1.0, 0.2), box_feather=0.1, metallic=1.0, roughness_scale=0.0,
                        roughness_offset=0.2),
                      E(select_color=(0.6, 0.3, 0.2), color_tolerance=0.2, color_feather=0.2, albedo_mode="multiply", color=(0.5, 1.0, 0.5)),
                      E(roughness_band=(0.09, 0.4), band_feather=0.1, strength=0.5, roughness_scale=1.5, roughness_offset=0.0)])

    def fresh_envs():                                                   # built outside the timed region; the same draws every run
        for _ in range(a.reps + 1):
            torch.manual_seed(0)
            yield relight.Environment_Light(hdr_maps=maps, device="cuda")

    def view(e, envs):
        return relight.relight_view(model, next(envs), ["city"], rays, a.image, a.image, num_samples=a.samples, edits=e)

    with torch.no_grad():
        envs = iter(list(fresh_envs()))
        plain, ms_plain = median_ms(lambda: view(None, envs), a.reps)
        envs = iter(list(fresh_envs()))
        edited, ms_edit = median_ms(lambda: view(edits, envs), a.reps)
        hit = plain["acc"] > 0.5
        changed = (edited["rgb"][0] != plain["rgb"][0]).any(dim=-1)
        emit({"what": "view", "image": a.image, "samples": a.samples, "edits": len(edits), "hit_pixels": int(hit.sum()),
              "changed_pixels": int(changed.sum()), "plain_ms": ms_plain, "edited_ms": ms_edit, "reps": a.reps})
        B = 4096
        lidx = torch.zeros((B, 1), dtype=torch.int32, device="cuda")
        mid = (a.image * a.image // 2 // B) * B
        _, rows = model(rays[mid:mid + B], lidx, _return_maps=True)
        rec, cent = edits.on("cuda")
        scratch = rows.clone()
        _, ms = median_ms(lambda: ops.material_edit_maps(rec, cent, 1.0, scratch.copy_(rows), rays[mid:mid + B], 0.5), a.reps)
        _, ms_copy = median_ms(lambda: scratch.copy_(rows), a.reps)
        emit({"what": "edit", "rows": B, "hit_rows": int((rows[:, 14] > 0.5).sum()), "edits": len(edits), "ms_with_copy": ms, "copy_ms": ms_copy,
              "reps": a.reps})
    rng = np.random.default_rng(0)
    N, k = a.palette_rows, a.k
    cent = rng.uniform(0.1, 0.9, (k, 4))
    X = (cent[rng.integers(0, k, N)] + rng.normal(0, 0.06, (N, 4))).clip(0, 1).astype(np.float32)
    albedo, rough = torch.from_numpy(X[:, :3].copy()).cuda(), torch.from_numpy(X[:, 3].copy()).cuda()
    pal, ms = median_ms(lambda: materials.palette_of(albedo, rough, k), a.reps)
    work = ops.kmeans_workspace(N, k, "cuda")
    labels = torch.zeros((N,), dtype=torch.int32, device="cuda")
    counts, inertia = torch.empty((k,), dtype=torch.int64, device="cuda"), torch.empty((1,), dtype=torch.float64, device="cuda")
    changed = torch.empty((1,), dtype=torch.int32, device="cuda")
    c0 = pal.centroids.clone()

    def one_pass():
        ops.kmeans_assign(albedo, rough, c0, labels, work, False)
        ops.kmeans_update(work, c0, counts, inertia, changed)
    _, ms_pass = median_ms(one_pass, a.reps)
    emit({"what": "palette", "rows": N, "k": k, "passes": pal.passes, "ms": ms, "assign_update_ms": ms_pass, "counts": pal.counts.tolist(),
          "reps": a.reps})
    if a.out:
        with open(a.out, "w") as fh:
            prop = torch.cuda.get_device_properties(0)                  # the marketing name may be generic: record the part too
            json.dump({"tool": "tools/material_edit_bench.py", "device": torch.cuda.get_device_name(0),
                       "arch": getattr(prop, "gcnArchName", None), "compute_units": prop.multi_processor_count,
                       "memory_gib": round(prop.total_memory / 2 ** 30, 1), "results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
