"""Record what the reference's host-side code computes, for the CPU tests that compare against it without a checkout.

TEST INFRASTRUCTURE ONLY (see oracle/ref_loader.py): run where the reference checkout exists.  Writes

    tests/golden/host_reference.json   digests / values of the reference model after load, upsample_volume_grid and shrink
                                       (the golden scene), its regularisers and optimizer groups, and its seeded construction
                                       (tests/test_host_model.py)
    tests/golden/port_reference.npz    the reference's maps on a strided sample of the C2+C3 bench batch, 96^3 field, with the
                                       reference-built 128^3 occupancy mask (tests/test_port_calibration.py)

Usage: python oracle/make_golden_host.py"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from oracle.ref_on_gpu import MAPS, reference_model, with_mask  # noqa: E402
from tests.helpers import (SEEDED_CASES, golden_checkpoint, regulariser_trace, seeded_construction_trace,  # noqa: E402
                           upsample_shrink_trace)

PORT_RAYS, PORT_GRID, PORT_SAMPLES, PORT_SECOND, PORT_ENV = 32, 96, 512, 96, (8, 16)


def reference_twin(ref, golden):
    ckpt = golden_checkpoint(golden)
    eh, ew = [int(x) for x in golden["scene/envmap_hw"]]
    kw = dict(ckpt["kwargs"])
    kw.pop("light_num", None)
    aabb, grid = kw.pop("aabb"), kw.pop("gridSize")
    kw["light_rotation"] = [f"{int(r):03d}" for r in kw["light_rotation"]]
    with contextlib.redirect_stdout(io.StringIO()):
        rm = ref.TensorVMSplit(aabb.clone(), list(grid), "cpu", envmap_h=eh, envmap_w=ew, **kw)
        rm.load(ckpt)
    return rm


def host_reference(ref):
    golden = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    tv = __import__("importlib").import_module("utils").TVLoss()
    return {
        "upsample_shrink": upsample_shrink_trace(reference_twin(ref, golden)),
        "regularisers": regulariser_trace(reference_twin(ref, golden), tv),
        "seeded_construction": {f"{lk}-{nk}": seeded_construction_trace(ref.TensorVMSplit, lk, nk) for lk, nk in SEEDED_CASES},
    }


def port_reference(ref):
    """The inputs oracle/calibrate_port.py uses (--rays 32 --grid 96), the reference's mask and maps."""
    from tensoir_amd import synth
    envh, envw = PORT_ENV
    ckpt = synth.make_checkpoint(grid=(PORT_GRID,) * 3, seed=20211202)
    rays_all = synth.make_rays(64, 64)
    stride = max(1, rays_all.shape[0] // PORT_RAYS)
    rays = rays_all[::stride][:PORT_RAYS].contiguous()
    lidx = torch.zeros(rays.shape[0], 1, dtype=torch.int32)
    args = types.SimpleNamespace(second_nSample=PORT_SECOND, second_near=0.05, second_far=1.5)
    rmodel = reference_model(ref, ckpt, "cpu", envh, envw)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        rmodel.updateAlphaMask((128, 128, 128))
        out = ref.renderer.Renderer_TensoIR_train(rays, None, lidx, rmodel, N_samples=PORT_SAMPLES, white_bg=True, is_train=False,
                                                  is_relight=True, sample_method="fixed_envirmap", chunk_size=160000, device="cpu",
                                                  args=args)
    ck = with_mask(ckpt, rmodel)
    rec = {"rays": rays.numpy(), "light_idx": lidx.numpy(), "stride": np.int64(stride),
           "mask/bits": np.asarray(ck["alphaMask.mask"]), "mask/shape": np.asarray(ck["alphaMask.shape"], np.int64),
           "mask/aabb": ck["alphaMask.aabb"].numpy()}
    for k in MAPS:
        rec["ref/" + k] = out[k].detach().numpy()
    return rec


def main():
    ref = ref_loader.load()
    d = host_reference(ref)
    with open(os.path.join(ROOT, "tests", "golden", "host_reference.json"), "w") as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write("\n")
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "port_reference.npz"), **port_reference(ref))


if __name__ == "__main__":
    main()
