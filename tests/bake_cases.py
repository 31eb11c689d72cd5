"""The models and point sets of the bake tests, built on the host from seeds so that tests/test_bake_cpu.py (which qualifies
them: fp32 against fp64 restatement) and tests/test_gpu_bake.py (HIP against the fp64 restatement) see the same inputs.

  golden               tests/golden/small_scene.npz; the surface points and shading normals of its rays with acc > 0.5
                       (O.forward_primary: o + depth * d, normal_map) + seeded points off the surface, outside the box and in
                       empty space (beside the box, marching parallel to its face: every sample is culled, coverage exactly 0)
  a16, a96             tests/config_scenes.py rows d16_a16 / d16_a96 (the non-48 appearance gathers)
  purely_derived, residue_prediction      row d16_a48 with that normals_kind (the residue decoder's 153-column layer 1 is seeded)
  general              row d16_a48 as the general multi-light model (one spherical-Gaussian set per light), light_idx = 1
The configuration cases take seeded in-box points with the derived normal at the point as the outward direction (the oracle's
density_grad, i.e. what compute_derived_normals returns)."""
import os
import types

import numpy as np
import torch

from oracle import tensoir_oracle as O
from tests import config_scenes as CS
from tests.helpers import golden_checkpoint, scene_from_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["golden", "a16", "a96", "purely_derived", "residue_prediction", "general"]
N_EXTRA = 100           # golden: points per extra group
N_CONFIG = 300          # configuration cases: in-box points
# Seeds of the configuration cases' point sets (and of the seeded decoder / light tables): per case the FIRST seed from 301 upward
# that tests/test_bake_cpu.py qualifies, scanned on the host with the restatement alone.  A first choice by the fp32-against-fp64
# outputs only (a16: 305) held a sample whose fp64 weight is 9.99996e-05 -- 4.4e-06 (relative) below rayMarch_weight_thres, while
# the restatement's own fp32 weights near the threshold are off by up to 3.4e-04: its fp32 run happened to fall on the fp64
# side, the device's fp32 march on the other (coverage then differs by that sample's 1e-4, `surface` by 3.8e-4).  The
# qualification therefore also demands a margin to the two discontinuities (MARGIN in tests/test_bake_cpu.py), which about one
# seeded set of 300 points in fifteen keeps.
POINT_SEED = {"a16": 302, "a96": 326, "purely_derived": 305, "residue_prediction": 316, "general": 310}

def _unit(x):
    return x / torch.linalg.norm(x, dim=-1, keepdim=True)


def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    ck = golden_checkpoint(g)
    eh, ew = [int(x) for x in g["scene/envmap_hw"]]
    sc = scene_from_checkpoint(ck, eh, ew)
    rays = torch.from_numpy(np.array(g["rays/rays"])).float()
    lidx = torch.from_numpy(np.array(g["rays/light_idx"]))
    with torch.no_grad():
        out = O.forward_primary(sc, rays, lidx)
    hit = out[6] > 0.5
    surf = (rays[:, :3] + out[1][:, None] * rays[:, 3:6])[hit]
    nrm = _unit(out[2][hit])
    gen = torch.Generator().manual_seed(20240917)
    lo, hi = sc.aabb[0], sc.aabb[1]
    pick = torch.randint(0, surf.shape[0], (N_EXTRA,), generator=gen)
    off = surf[pick] + 0.1 * torch.randn(N_EXTRA, 3, generator=gen)
    outside = lo + (torch.rand(N_EXTRA, 3, generator=gen) * 1.6 - 0.3) * (hi - lo)
    rand_dirs = _unit(torch.randn(2 * N_EXTRA, 3, generator=gen))
    empty = lo + torch.rand(N_EXTRA, 3, generator=gen) * (hi - lo)
    empty[:, 0] = hi[0] + 0.5 + torch.rand(N_EXTRA, generator=gen)
    ang = torch.rand(N_EXTRA, generator=gen) * (2 * np.pi)
    empty_dirs = torch.stack([torch.zeros(N_EXTRA), torch.cos(ang), torch.sin(ang)], -1)
    points = torch.cat([surf, off, outside, empty]).float().contiguous()
    outward = torch.cat([nrm, rand_dirs, _unit(empty_dirs)]).float().contiguous()
    n_surf = surf.shape[0]
    return types.SimpleNamespace(ckpt=ck, envmap_hw=(eh, ew), scene=sc, sgs=None, points=points, outward=outward, light_idx=0,
                                 n_surface=n_surf, empty=slice(n_surf + 2 * N_EXTRA, n_surf + 3 * N_EXTRA))


def _config(name):
    row = CS.ROW[{"a16": "d16_a16", "a96": "d16_a96"}.get(name, "d16_a48")]
    ck = CS.checkpoint(row)
    gen = torch.Generator().manual_seed(CS.SEED + POINT_SEED[name])
    sgs = None
    if name == "purely_derived":
        ck["kwargs"]["normals_kind"] = name
        ck["state_dict"] = {k: v for k, v in ck["state_dict"].items() if not k.startswith("renderModule_normal")}
    elif name == "residue_prediction":
        ck["kwargs"]["normals_kind"] = name
        w0 = ck["state_dict"]["renderModule_normal.mlp.0.weight"]
        bound = 1.0 / np.sqrt(w0.shape[1] + 3)
        ck["state_dict"]["renderModule_normal.mlp.0.weight"] = (torch.rand(w0.shape[0], w0.shape[1] + 3, generator=gen) * 2 - 1) * bound
    sc = scene_from_checkpoint(ck, *CS.ENVMAP_HW)
    if name == "general":
        sgs = [(sc.lgtSGs + 0.3 * torch.randn(sc.lgtSGs.shape, generator=gen)).float() for _ in range(row.n_lights)]
        sc.lgtSGs_list = sgs
    lo, hi = sc.aabb[0], sc.aabb[1]
    points = (lo + (0.05 + 0.9 * torch.rand(N_CONFIG, 3, generator=gen)) * (hi - lo)).float().contiguous()
    with torch.no_grad():
        nrm = O.density_grad(sc, O.normalize_coord(sc, points))[2]
    length = torch.linalg.norm(nrm, dim=-1, keepdim=True)
    outward = torch.where(length > 0.5, nrm / length.clamp(min=0.5), torch.tensor([0.0, 0.0, 1.0])).float().contiguous()
    return types.SimpleNamespace(ckpt=ck, envmap_hw=CS.ENVMAP_HW, scene=sc, sgs=sgs, points=points, outward=outward,
                                 light_idx={"general": 1, "a16": 2}.get(name, 0), n_surface=0, empty=slice(0, 0))


_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = _golden() if name == "golden" else _config(name)
    return _CACHE[name]


def model(c, device="cuda"):
    """The product model of a case."""
    import tensoir_amd
    eh, ew = c.envmap_hw
    if c.sgs is None:
        return tensoir_amd.model_from_checkpoint(c.ckpt, device, envmap_h=eh, envmap_w=ew)
    from tensoir_amd.general_multi_lights import TensorVMSplit as General
    kw = {k: v for k, v in c.ckpt["kwargs"].items() if k not in ("light_num", "light_rotation")}
    m = General(device=device, light_name_list=[f"light{i}" for i in range(len(c.sgs))], envmap_h=eh, envmap_w=ew, **kw)
    m.load_state_dict({k: v for k, v in c.ckpt["state_dict"].items() if k != "lgtSGs"}, strict=False)
    m._field_key = None
    with torch.no_grad():
        for sg, src in zip(m.lgtSGs_list, c.sgs):
            sg.copy_(src.to(sg.device))
    return m
