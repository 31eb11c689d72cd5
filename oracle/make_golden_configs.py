"""Generate tests/golden/config_scenes.npz: the IMPORTED REFERENCE's results on two scenes of the configuration matrix
(tests/config_scenes.py) that the other goldens do not cover -- 8 density / 24 appearance components per plane (the
constructor default) with softplus, and the same widths with fea2denseAct='relu' (models/tensorBase_rotated_lights.py:
813-817).  Per scene: density / appearance / intrinsic features and sigma at seeded points, the occupancy mask the reference
builds, the maps of the evaluation render and one training step's loss, maps and parameter gradients.

Only inputs that are not reproducible from a seed and the reference's outputs are stored; the checkpoints are rebuilt from
tests/config_scenes.checkpoint (a digest of every state_dict entry is stored to notice a drifted generator).

Run in the build container (needs the read-only reference checkout):
    python oracle/make_golden_configs.py
TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from oracle import tensoir_oracle as O  # noqa: E402
from oracle.make_golden import build_reference_model, npy  # noqa: E402
from tests import config_scenes as CS  # noqa: E402
from tests.helpers import digest  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
ALPHA_GRID = (16, 18, 20)
MAPS = ("rgb_map", "depth_map", "normal_map", "albedo_map", "roughness_map", "fresnel_map", "acc_map", "rgb_with_brdf_map",
        "normals_diff_map", "normals_orientation_loss_map", "albedo_smoothness_loss", "roughness_smoothness_loss")


def record(ref, name):
    row = CS.ROW[name]
    ck = CS.checkpoint(row)
    envh, envw = CS.ENVMAP_HW
    model = build_reference_model(ref, ck, envh, envw, alpha_grid=ALPHA_GRID)
    assert model.fea2denseAct == row.act
    args = types.SimpleNamespace(**CS.SECOND)
    g = {"sd_digest": np.array([f"{k}={digest(v)}" for k, v in sorted(ck["state_dict"].items())])}
    vol = model.alphaMask.alpha_volume[0, 0]
    g["alpha_shape"] = np.array(vol.shape, np.int64)
    g["alpha_bits"] = np.packbits(vol.bool().numpy().reshape(-1))
    g["alpha_aabb"] = npy(model.alphaMask.aabb)
    xyz = CS.feature_points()
    lidx = CS.light_indices(xyz.shape[0], row.n_lights)
    with torch.no_grad():
        f = model.compute_densityfeature(xyz)
        g["feat/density"], g["feat/sigma"] = npy(f), npy(model.feature2density(f))
        g["feat/app"] = npy(model.compute_appfeature(xyz, lidx))
        g["feat/intrin"] = npy(model.compute_intrinfeature(xyz))
    xg = xyz.clamp(-0.95, 0.95)
    g["feat/derived_normals"] = npy(model.compute_derived_normals(xg.clone()))
    rays, light_idx, rgb_gt = CS.rays_for(row)
    B = rays.shape[0]
    model.eval()
    torch.manual_seed(CS.SEED + 3)
    with torch.no_grad():
        ret = ref.renderer.Renderer_TensoIR_train(
            rays, None, light_idx, model, N_samples=-1, white_bg=True, is_train=False, is_relight=True,
            sample_method="fixed_envirmap", chunk_size=777, device="cpu", args=args)
    for k in MAPS:
        if k in ret:
            g[f"eval/{k}"] = npy(ret[k])
    model.train()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(CS.SEED + 12)
    ret = ref.renderer.Renderer_TensoIR_train(
        rays, None, light_idx, model, N_samples=CS.N_SAMPLES, white_bg=True, is_train=True, is_relight=True,
        sample_method="fixed_envirmap", chunk_size=777, device="cpu", args=args)
    loss = O.training_loss(ret, rgb_gt, True)
    loss.backward()
    g["train/loss"] = npy(loss).reshape(1)
    for k in MAPS:
        g[f"train/out/{k}"] = npy(ret[k])
    for pname, p in model.named_parameters():
        g[f"train/grad/{pname}"] = npy(torch.zeros_like(p) if p.grad is None else p.grad)
    torch.manual_seed(CS.SEED + 12)
    g["train/ray_jitter"] = npy(torch.rand(B, 1))
    return {f"{name}/{k}": v for k, v in g.items()}


def build():
    ref = ref_loader.load()
    g = {}
    for name in CS.GOLDEN_ROWS:
        g.update(record(ref, name))
    return g


def main():
    g = build()
    path = os.path.join(OUT, "config_scenes.npz")
    if "--check" in sys.argv:                 # the stored arrays regenerate bit for bit
        old = np.load(path)
        assert sorted(old.files) == sorted(g), "array names differ"
        bad = [k for k in g if not np.array_equal(old[k], g[k])]
        assert not bad, bad
        print(f"{path}: {len(g)} arrays regenerate bit-identically")
        return
    np.savez_compressed(path, **g)
    print(f"wrote {path}: {len(g)} arrays, {os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    main()
