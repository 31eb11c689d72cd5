"""The configuration matrix: one seeded synthetic scene per field configuration the kernels dispatch on (density / appearance
components per plane, density activation, light count).  Shared by tests/test_gpu_config_matrix.py (HIP against the oracle),
tests/test_abi.py (descriptor contents), tests/test_oracle_configs.py and oracle/make_golden_configs.py (the two scenes whose
reference results are recorded in tests/golden/config_scenes.npz).

Grid and box are non-cubic so that a swapped axis or stride shows.  The random density components are scaled by DENSITY_SCALE
(as the per-point autograd test's random model does): their sum has a spread of a few units, so softplus' / softplus'' are not
negligible off the blob and a relu scene has density features of both signs.
"""
from collections import namedtuple

import numpy as np
import torch

from tensoir_amd import synth

GRID = [20, 24, 28]
AABB = [[-1.5, -1.4, -1.3], [1.5, 1.4, 1.6]]
ENVMAP_HW = (4, 8)
DENSITY_SCALE = 30.0
SEED = 20240611
# relu has no shift: the (everywhere positive) blob is kept narrower there, so that the random components decide the sign of
# the density feature in most of the box and both arms of relu are taken
BLOB_SIGMA = {"softplus": 0.35, "relu": 0.25}
N_SAMPLES = 48                     # primary samples of a training step
SECOND = dict(second_nSample=24, second_near=0.05, second_far=1.5)

# name, density comps, appearance comps, activation, lights, occupancy mask built (updateAlphaMask) before the product calls
Row = namedtuple("Row", "name n_dcomp n_acomp act n_lights mask")
ROWS = [
    Row("d16_a48", 16, 48, "softplus", 3, True),          # the control: the configuration every other GPU test runs
    Row("d4_a48", 4, 48, "softplus", 3, False),
    Row("d8_a48", 8, 48, "softplus", 3, False),
    Row("d32_a48", 32, 48, "softplus", 3, False),
    Row("d16_a16", 16, 16, "softplus", 3, False),
    Row("d16_a24", 16, 24, "softplus", 3, False),
    Row("d16_a96", 16, 96, "softplus", 3, False),
    Row("d8_a24", 8, 24, "softplus", 3, True),            # TensorVMSplit's constructor default
    Row("relu_d16_a48", 16, 48, "relu", 3, False),
    Row("relu_d8_a24", 8, 24, "relu", 3, True),
    Row("d16_a48_l9", 16, 48, "softplus", 9, False),
    Row("d16_a48_l17", 16, 48, "softplus", 17, False),
]
ROW = {r.name: r for r in ROWS}
GOLDEN_ROWS = ("d8_a24", "relu_d8_a24")                   # recorded from the reference (tests/golden/config_scenes.npz)


def checkpoint(row, grid=GRID, aabb=AABB):
    """Reference-format checkpoint of a matrix row (seeded per row: no two rows share planes)."""
    seed = SEED + ROWS.index(row) if row in ROWS else SEED + 100
    rot = [f"{(i * 360) // row.n_lights:03d}" for i in range(row.n_lights)]
    ck = synth.make_checkpoint(grid=tuple(grid), seed=seed, light_rotation=rot, aabb=aabb,
                               density_n_comp=(row.n_dcomp,) * 3, app_n_comp=(row.n_acomp,) * 3,
                               fea2dense_act=row.act, blob_sigma=BLOB_SIGMA[row.act])
    for i in range(3):
        ck["state_dict"][f"density_plane.{i}"][:, 1:] *= DENSITY_SCALE          # component 0 is the blob
    return ck


def light_indices(n, n_lights):
    """[n, 1] int32 light indices that cover the first and the last light and -- where they exist -- 8, 9 and 16 (the borders
    of the indirect-light tiers), then cycle through all of them."""
    head = [i for i in (0, n_lights - 1, 8, 9, 16) if 0 <= i < n_lights]
    idx = (head + [i % n_lights for i in range(n)])[:n]
    return torch.tensor(idx, dtype=torch.int32).view(-1, 1)


def rays_for(row):
    """36 rays of a pin-hole camera aimed at the blob and four that pass beside the box; light indices; target colours."""
    rays = synth.make_rays(6, 6)
    d = torch.tensor([[0.9, 0.9, -1.0], [-0.9, 0.9, -1.0], [0.9, -0.9, -1.0], [-0.95, -0.9, -1.0]])
    miss = torch.cat([rays[:4, :3], d / d.norm(dim=-1, keepdim=True)], -1)
    rays = torch.cat([rays, miss]).contiguous()
    B = rays.shape[0]
    gen = torch.Generator().manual_seed(SEED + 7)
    return rays, light_indices(B, row.n_lights), torch.rand(B, 3, generator=gen)


def training_draws(B, S=N_SAMPLES):
    """The two random draws of a training forward, fixed: ray jitter [B, 1] and the dense BRDF-smoothness noise [B, S, 3]."""
    gen = torch.Generator().manual_seed(SEED + 21)
    return torch.rand(B, 1, generator=gen), torch.randn(B, S, 3, generator=gen)


def feature_points(n=96):
    """Seeded points for the recorded features: in the box, on its faces and a few just outside."""
    gen = torch.Generator().manual_seed(SEED + 3)
    x = torch.rand(n, 3, generator=gen) * 2.2 - 1.1
    x[:6] = torch.tensor([[-1, -1, -1], [1, 1, 1], [0, 0, 0], [1, -1, 0.5], [-1, 1, -0.25], [0.1, -1, 1]])
    return x


def with_golden_mask(ck, g, name):
    """The row's checkpoint with the occupancy mask the reference built (recorded bits), as save() would have written it."""
    ck = dict(ck)
    shape = tuple(int(v) for v in g[f"{name}/alpha_shape"])
    ck["alphaMask.shape"] = shape
    ck["alphaMask.mask"] = np.array(g[f"{name}/alpha_bits"])
    ck["alphaMask.aabb"] = torch.from_numpy(np.array(g[f"{name}/alpha_aabb"]))
    return ck
