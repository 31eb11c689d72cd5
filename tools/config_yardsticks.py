"""The yardsticks of tests/test_gpu_config_matrix.py (YARDSTICK, GRAD_BOUND, DETERMINATE_RAYS): per row of the configuration
matrix, the oracle evaluated in fp32 against the same oracle in fp64 on the row's own batch -- CPU only.

    python tools/config_yardsticks.py

Per row: whether fp32 and fp64 agree on every ray's hit / miss decision, the worst rendered map of the jittered training forward,
the worst parameter gradient (max |d| / max |ref| per tensor, fp32 autograd against fp64 autograd) with relight on and off, and
the number of rays of the evaluation render whose normals_diff_map the oracle determines to a quarter of the map bound.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import tensoir_oracle as O  # noqa: E402
from tests import config_scenes as CS  # noqa: E402
from tests.helpers import scene_from_checkpoint  # noqa: E402
from tests.train_check import gerr  # noqa: E402

MASK_GRID = (16, 18, 20)


def main():
    print("row | hit/miss agree | worst map | worst gradient, relight on | relight off | determinate rays")
    for row in CS.ROWS:
        sc = scene_from_checkpoint(CS.checkpoint(row), *CS.ENVMAP_HW)
        if row.mask:
            O.update_alpha_mask(sc, MASK_GRID)
        sc64 = sc.to(torch.float64)
        rays, lidx, gt = CS.rays_for(row)
        jit, noise = CS.training_draws(rays.shape[0])
        out = {}
        for relight in (True, False):
            kw = dict(is_relight=relight, n_samples=CS.N_SAMPLES, second_n_sample=CS.SECOND["second_nSample"],
                      second_near=CS.SECOND["second_near"], second_far=CS.SECOND["second_far"])
            _, g32, r32 = O.train_step_grads(sc, rays, lidx, gt, ray_jitter=jit, brdf_jitter=noise, **kw)
            _, g64, r64 = O.train_step_grads(sc64, rays.double(), lidx, gt.double(), ray_jitter=jit.double(),
                                             brdf_jitter=noise.double(), **kw)
            gr = {k: gerr(g32[k], g64[k]) for k in g32 if float(g64[k].abs().max()) > 0}
            worst = max(gr, key=gr.get)
            out[relight] = (worst, gr[worst])
            if relight:
                maps = max(float((r32[k].double() - r64[k]).abs().max()) for k in r32
                           if torch.is_tensor(r32[k]) and r32[k].is_floating_point() and r32[k].dim() > 0)
                same = bool(((r32["acc_map"] > 0.5) == (r64["acc_map"] > 0.5)).all())
        with torch.no_grad():
            e32 = O.renderer_train(sc, rays, lidx, second_n_sample=CS.SECOND["second_nSample"])
            e64 = O.renderer_train(sc64, rays.double(), lidx, second_n_sample=CS.SECOND["second_nSample"])
        same = same and bool(((e32["acc_map"] > 0.5) == (e64["acc_map"] > 0.5)).all())
        det = int(((e32["normals_diff_map"].double() - e64["normals_diff_map"]).abs().view(-1) < 1e-4 / 4).sum())
        print(f"{row.name} | {same} | {maps:.1e} | {out[True][1]:.2e} ({out[True][0]}) | {out[False][1]:.2e} ({out[False][0]}) | "
              f"{det} of {rays.shape[0]}", flush=True)


if __name__ == "__main__":
    main()
