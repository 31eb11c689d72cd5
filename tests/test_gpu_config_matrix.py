"""The field configurations the launchers dispatch on, each run on the GPU against the fp64 oracle: density components per
plane 4 / 8 / 16 / 32, appearance components 16 / 24 / 48 / 96, softplus and relu, 3 / 9 / 17 lights, density lines that fit
the 96 KB LDS staging of the backward and lines that do not.  Every other GPU test runs 16 / 48 / softplus / <= 3 lights.

The scenes are tests/config_scenes.py's (non-cubic grid and box, random density components scaled so that both signs of the
density feature occur); tests/test_oracle_configs.py pins the oracle on two of them (8 / 24 softplus, 8 / 24 relu) to the
reference's recorded results, and `test_golden_scenes` holds the HIP path to the same file.

Bounds are the project's existing ones, for every row (none needed its own):
    features 2e-5 and rendered maps 1e-4 (tests/test_gpu_parity.py), per-point gradients 1e-5 and derived normals 5e-4
    (tests/test_gpu_pointwise_grad.py), training gradients 2e-3 and loss 1e-5 (tests/train_check.py).
The yardstick next to each row is the oracle's own fp32 result against its fp64 result on the row's training batch, measured on
the CPU (worst rendered map of the jittered forward / worst parameter gradient, max |d| / max |ref|): what a bound of 4 x
yardstick would be if a row ever missed the existing one -- never above 10 x the control row's bound.  In every row the
oracle's fp32 and fp64 forward agree on each ray's hit / miss decision (acc_map is 0 or 1 to 1e-7: margin 0.5).

Measured on an MI355X (worst over the twelve rows; every row's own figures are printed by the tests, `pytest -s`):
    per-point forward: density 1.7e-5 (d32_a48; the oracle's own fp32 evaluation is 2.4e-5 from fp64 there), sigma 1.3e-5,
    alpha 3.7e-6, appearance features 9e-8, derived normals 4.2e-5; gathers: mfma / valu 5.4e-8, x3 7.3e-8, bf16x3 2.9e-7;
    evaluation render: worst map 2.5e-5 (normals_diff_map on the rays it is compared on; normal_map 1.4e-5); training step:
    DESIGN 4.5 lists every row's figures in both decoder modes.

Three places where the operation itself is discontinuous are left out of a comparison by a rule that involves the oracle only:
  * relu' jumps at 0, so the derived normal and every parameter gradient of sigma jump there: per-point sets of relu rows
    drop points whose fp64 density feature is within 1e-4 of zero (5 x the feature bound).
  * the first sample of an un-jittered ray lies exactly on the face of the box, where the border-clamped derived normal is
    discontinuous: in the evaluation render `normals_diff_map` is compared on the rays whose fp32 and fp64 oracle values agree
    to a quarter of the bound (at least half of the rays in every row; the oracle's own spread is up to 0.15 on the relu rows,
    whose fog gives that sample weight).  The jittered training forward compares the map on every ray.
  * a decoder's hidden unit whose pre-activation is within rounding of zero takes either side of its ReLU: test_training_step
    applies DESIGN 5's existing rule on a strict miss (all rays but one, found by bisection), in both decoder modes.
Not compared here: the recorded training gradients of tests/golden/config_scenes.npz against the HIP step (the reference drew
its BRDF noise on compacted points; the HIP step is held to the oracle on dense draws, the oracle to the record on the CPU).
"""
import os
import types

import numpy as np
import pytest
import torch

from oracle import tensoir_oracle as O
from tests import config_scenes as CS
from tests.helpers import T, max_err, rel_err, scene_from_checkpoint, scene_from_model
from tests.pointwise_ref import (APP, DENSITY, NORMAL_TOL, _clamped_feature, _ref_normals, check_params, close, scene64,
                                 zero_grads)
from tests.train_check import GTOL, check_training_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT_TOL, MAP_TOL = 2e-5, 1e-4
ALPHA_GRID = (16, 18, 20)
RELU_KINK = 1e-4

# row -> yardsticks: the oracle in fp32 against itself in fp64 on the row's training batch, as tools/config_yardsticks.py
# prints them (CPU): worst rendered map of the jittered forward, worst parameter gradient (max |d| / max |ref| per tensor) with
# relight on, the same with relight off (density gradients only: a difference of nearly equal terms, hence the larger figures).
# 4 x yardstick is below the existing bounds (1e-4 / 2e-3) except where GRAD_BOUND says so.
YARDSTICK = {
    "d16_a48": (3.9e-6, 5.2e-5, 3.1e-4), "d4_a48": (1.0e-6, 1.3e-5, 7.4e-4), "d8_a48": (1.5e-6, 2.7e-5, 7.3e-4),
    "d32_a48": (2.7e-6, 2.0e-5, 3.4e-4), "d16_a16": (1.4e-6, 1.9e-5, 4.6e-4), "d16_a24": (1.8e-6, 1.7e-5, 3.6e-4),
    "d16_a96": (1.9e-6, 1.1e-5, 5.1e-4), "d8_a24": (1.1e-6, 7.1e-6, 2.1e-4), "relu_d16_a48": (4.7e-6, 4.2e-5, 9.0e-4),
    "relu_d8_a24": (2.6e-6, 1.9e-5, 1.4e-4), "d16_a48_l9": (1.4e-6, 1.7e-5, 5.1e-4), "d16_a48_l17": (9.3e-7, 3.5e-5, 4.2e-4),
}
NAMES = [r.name for r in CS.ROWS]
assert sorted(YARDSTICK) == sorted(NAMES)
# rays (of 40) of the evaluation render on which the oracle itself determines normals_diff_map (module docstring): the count
# each row has today -- a changed scene that leaves fewer has to be looked at
DETERMINATE_RAYS = {"d16_a48": 40, "d4_a48": 36, "d8_a48": 38, "d32_a48": 24, "d16_a16": 34, "d16_a24": 37, "d16_a96": 39,
                    "d8_a24": 40, "relu_d16_a48": 20, "relu_d8_a24": 20, "d16_a48_l9": 34, "d16_a48_l17": 32}
# (row, relight) -> gradient bound of the one case that does not meet GTOL: 4 x its yardstick (tools/config_yardsticks.py: the
# oracle's fp32 autograd against its fp64 autograd is 7.39e-4 on density_plane.2 there -- with relight off the density
# gradient of this batch is a difference of nearly equal terms); measured on the GPU: 2.13e-3 (split-bf16), 1.22e-3 (fp32)
GRAD_BOUND = {("d4_a48", False): 4 * 7.39e-4}
assert all(GTOL <= v <= 10 * GTOL for v in GRAD_BOUND.values())

# the appearance gathers tir_field.hip's launchers accept per width (app_fwd / tir_vm_app_fwd_x3: the switch on n_acomp)
APP_IMPLS = {16: ("mfma", "valu", "bf16x3", "x3"), 24: ("mfma", "valu", "bf16x3", "x3"), 48: ("mfma", "valu", "bf16x3", "x3"),
             96: ("mfma", "valu")}
# C entries that exist for 48 appearance components only: the merged primary gather (with in-kernel jitter), the fp16 shadow
# gather and both fused indirect kernels
ONLY_48 = ("tir_vm_app_primary_fwd", "tir_vm_app_primary_x3_fwd", "tir_vm_app_fwd_h16", "tir_indirect_fused_fwd",
           "tir_indirect_fused_hp_fwd")
COUNTS = (1, 255, 256, 257, 8 * 1024 + 77)          # the backward's grid is capped at 1024 blocks and loops beyond


# ---- models -----------------------------------------------------------------------------------------------------------------
class World:
    def __init__(self):
        import tensoir_amd
        from tensoir_amd import _lib
        assert torch.cuda.is_available()
        assert _lib.lib().tir_device_check() == 0
        self.tensoir_amd = tensoir_amd
        self.cache = {}
        self.cg = np.load(os.path.join(ROOT, "tests", "golden", "config_scenes.npz"))
        self.args = types.SimpleNamespace(**CS.SECOND)

    def get(self, name):
        """(model, fp32 oracle scene) of a row; rows with `mask` get their occupancy mask from the device's updateAlphaMask, the
        two recorded rows the mask the reference built."""
        if name not in self.cache:
            row = CS.ROW[name]
            ck = CS.checkpoint(row)
            if name in CS.GOLDEN_ROWS:
                ck = CS.with_golden_mask(ck, self.cg, name)
            m = self.tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=CS.ENVMAP_HW[0], envmap_w=CS.ENVMAP_HW[1])
            m.march_t_stop = 0.0
            if row.mask and name not in CS.GOLDEN_ROWS:
                m.updateAlphaMask(ALPHA_GRID)
            assert (m.alphaMask is not None) == row.mask
            sc = scene_from_model(ck, m, *CS.ENVMAP_HW) if row.mask else scene_from_checkpoint(ck, *CS.ENVMAP_HW)
            self.cache[name] = (m, sc)
        return self.cache[name]


@pytest.fixture(scope="module")
def world():
    return World()


class entries:
    """The C entry points called inside the block (ops.TIMING brackets every call)."""

    def __enter__(self):
        from tensoir_amd import ops
        self.ops, self.old = ops, ops.TIMING
        ops.TIMING = []
        return self

    def __exit__(self, *exc):
        self.names = {t[0] for t in self.ops.TIMING}
        self.ops.TIMING = self.old
        return False


# ---- point sets (normalised coordinates) ------------------------------------------------------------------------------------
def mixed_points(n, seed, grid=CS.GRID):
    """Interior points, points exactly on lattice nodes, on faces and corners of the box, and points slightly outside it
    (where the zero-padded and the border-clamped samplers differ), interleaved so that any count has all kinds."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=gen) * 1.9 - 0.95
    node = torch.stack([torch.randint(0, g, (n,), generator=gen) for g in grid], -1).float()
    node = node / (torch.tensor(grid).float() - 1) * 2 - 1
    sign = torch.randint(0, 2, (n, 3), generator=gen).float() * 2 - 1
    axis = torch.nn.functional.one_hot(torch.randint(0, 3, (n,), generator=gen), 3).bool()
    out = sign * (1.0 + torch.rand(n, 3, generator=gen) * 0.05)
    kind = torch.arange(n) % 8
    x = torch.where((kind == 3)[:, None], node, x)                                   # all three coordinates on a node
    x = torch.where((kind == 4)[:, None] & axis, node, x)                            # one coordinate on a grid line
    x = torch.where((kind == 5)[:, None] & axis, sign, x)                            # on a face
    x = torch.where((kind == 6)[:, None], sign, x)                                   # a corner
    x = torch.where((kind == 7)[:, None] & axis, out, x)                             # just outside through one face
    return x.contiguous()


def dyadic_points(n, seed):
    """Points whose coordinates are multiples of 2^-9 in [-1.05, 1.05] (faces included): (x + 1) / 2 * (size - 1) is exact in
    fp32 for any axis shorter than 4096, so kernel and fp64 reference sample the same position.  On a 750-long axis a general
    fp32 coordinate fixes the position to 2e-5 cells only, which white-noise lines turn into 3e-4 of the feature on both sides
    of any fp32 implementation (the oracle's included)."""
    gen = torch.Generator().manual_seed(seed)
    j = torch.randint(-26, 1024 + 27, (n, 3), generator=gen)
    j[::7, 0], j[3::7, 1], j[5::7, 2] = 0, 1024, 0
    return (j.float() / 512.0 - 1.0).contiguous()


def settle(sc64, x, act):
    """relu rows: a point within RELU_KINK of relu's kink (module docstring) is replaced by its neighbour 0.9 x (again if
    need be), so the count -- 255 / 256 / 257 sit on the 256-thread block border -- stays exact; the set is held to both arms."""
    if act != "relu":
        return x
    x = x.clone()
    moved = 0
    for _ in range(20):
        with torch.no_grad():
            f = O.density_feature(sc64, x.double(), "explicit")
            fc = _clamped_feature(sc64, x, x.double())
        bad = (f.abs() <= RELU_KINK) | (fc.abs() <= RELU_KINK)
        if not bool(bad.any()):
            break
        moved += int(bad.sum())
        x[bad] = x[bad] * 0.9
    assert not bool(bad.any())
    if x.shape[0] >= 255:
        inside = (x.abs() <= 1).all(-1)
        assert float((f[inside] > 0).float().mean()) >= 0.25 and float((f[inside] < 0).float().mean()) >= 0.25
        assert moved <= 0.01 * x.shape[0]
    return x.contiguous()


def frozen64(model):
    sc, _ = scene64(model)
    return sc


# ---- 0. the descriptor ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_descriptor(world, name):
    row = CS.ROW[name]
    m, sc = world.get(name)
    f = m.packed_field()
    assert (int(f.n_dcomp), int(f.n_acomp), int(f.act), int(f.n_lights)) == (row.n_dcomp, row.n_acomp,
                                                                           {"softplus": 0, "relu": 1}[row.act], row.n_lights)
    assert [int(g) for g in f.grid] == CS.GRID and sc.fea2denseAct == row.act
    assert (m.packed_field_half() is not None) == (row.n_acomp == 48)


# ---- 1. per-point forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_pointwise_forward(world, name):
    row = CS.ROW[name]
    m, _ = world.get(name)
    sc = frozen64(m)
    worst = {}

    def note(what, err, tol, n):
        worst[what] = max(worst.get(what, 0.0), err)
        assert err < tol, (name, what, n, err)

    with torch.no_grad():
        for n in COUNTS:
            x = settle(sc, mixed_points(n, 100 + n), row.act)
            xd, x64 = x.cuda(), x.double()
            li = CS.light_indices(x.shape[0], row.n_lights).view(-1)
            f_ref = O.density_feature(sc, x64, "explicit")
            f = m.compute_densityfeature(xd)
            note("density", rel_err(f, f_ref), FEAT_TOL, n)
            fc_ref = _clamped_feature(sc, x, x64)
            note("density (clamped taps)", rel_err(m.compute_densityfeature_with_xyz_grad(xd), fc_ref), FEAT_TOL, n)
            sig_ref = O.feature2density(sc, f_ref)
            note("sigma", rel_err(m.feature2density(f), sig_ref), FEAT_TOL, n)
            if row.act == "relu":
                assert float(sig_ref.min()) == 0.0 or n == 1
            lo, hi = m.aabb[0].cpu(), m.aabb[1].cpu()
            xw = (lo + (x + 1) / 2 * (hi - lo)).cuda()
            xn = m.normalize_coord(xw).cpu()
            hit = m.alphaMask.sample_alpha(xw).cpu().double() if m.alphaMask is not None else torch.ones(x.shape[0], dtype=torch.float64)
            a_ref = 1 - torch.exp(-O.feature2density(sc, O.density_feature(sc, xn.double(), "explicit")) * hit * 0.7)
            note("alpha", max_err(m.compute_alpha(xw, length=0.7), a_ref), FEAT_TOL, n)
            note("app", rel_err(m.compute_appfeature(xd, li.cuda()), O.app_feature(sc, x64, li, "explicit")), FEAT_TOL, n)
            note("intrin", rel_err(m.compute_intrinfeature(xd), O.intrin_feature(sc, x64, "explicit")), FEAT_TOL, n)
            r, i = m.compute_bothfeature(xd, li.cuda())
            r_ref, i_ref = O.both_feature(sc, x64, li, "explicit")
            note("both (radiance)", rel_err(r, r_ref), FEAT_TOL, n)
            note("both (intrinsic)", rel_err(i, i_ref), FEAT_TOL, n)
    # derived normals: autograd on the reference side
    for n in COUNTS:
        x = settle(sc, mixed_points(n, 200 + n).clamp(-0.999, 0.999), row.act)
        xg = x.double().requires_grad_(True)
        n_ref = _ref_normals(sc, x, xg).detach()
        with torch.no_grad():
            got = m.compute_derived_normals(x.cuda())
        # -g / max(|g|, 1e-6): compared where the reference normal is normalised (or exactly zero: relu below zero, a flat
        # clamped tap); where |g| < 1e-6 the division by the clamp multiplies the gradient's fp32 rounding by 1e6
        ok = (n_ref.norm(dim=-1) > 0.5) | (n_ref.norm(dim=-1) == 0.0)
        assert float(ok.float().mean()) > 0.9 or n == 1, (name, n)
        if bool(ok.any()):
            note("derived normals", max_err(got.cpu()[ok], n_ref[ok]), NORMAL_TOL, n)
    print(f"\n[config-matrix] {name} forward worst: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---- 2. per-point backward --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", COUNTS)
def test_pointwise_backward(world, name, n):
    row = CS.ROW[name]
    m, _ = world.get(name)
    x0 = settle(frozen64(m), mixed_points(n, 300 + n), row.act)
    n = x0.shape[0]
    gen = torch.Generator().manual_seed(400 + n)
    w, V = torch.randn(n, generator=gen), torch.randn(n, 3, generator=gen)
    li = CS.light_indices(n, row.n_lights).view(-1)
    wa = torch.randn(2, n, m.app_dim, generator=gen)
    x64 = x0.double()
    # compute_densityfeature
    zero_grads(m)
    (m.compute_densityfeature(x0.cuda()) * w.cuda()).sum().backward()
    sc, params = scene64(m)
    (O.density_feature(sc, x64, "explicit") * w.double()).sum().backward()
    check_params(m, params, DENSITY)
    # compute_alpha (world coordinates, through the mask where the row has one)
    lo, hi = m.aabb[0].cpu(), m.aabb[1].cpu()
    xw = (lo + (x0 + 1) / 2 * (hi - lo)).cuda()
    zero_grads(m)
    (m.compute_alpha(xw, length=0.7) * w.cuda()).sum().backward()
    hit = m.alphaMask.sample_alpha(xw).cpu().double() if m.alphaMask is not None else torch.ones(n, dtype=torch.float64)
    xn = m.normalize_coord(xw).cpu().double()
    sc, params = scene64(m)
    sigma = O.feature2density(sc, O.density_feature(sc, xn, "explicit")) * hit
    ((1 - torch.exp(-sigma * 0.7)) * w.double()).sum().backward()
    check_params(m, params, DENSITY)
    # appearance features
    for method in ("app", "intrin", "both"):
        zero_grads(m)
        if method == "app":
            outs = (m.compute_appfeature(x0.cuda(), li.cuda()),)
        elif method == "intrin":
            outs = (m.compute_intrinfeature(x0.cuda()),)
        else:
            outs = m.compute_bothfeature(x0.cuda(), li.cuda())
        sum(((o * wa[i].cuda()).sum() for i, o in enumerate(outs)), torch.zeros((), device="cuda")).backward()
        sc, params = scene64(m)
        if method == "app":
            refs = (O.app_feature(sc, x64, li, "explicit"),)
        elif method == "intrin":
            refs = (O.intrin_feature(sc, x64, "explicit"),)
        else:
            refs = O.both_feature(sc, x64, li, "explicit")
        sum((r * wa[i].double()).sum() for i, r in enumerate(refs)).backward()
        check_params(m, params, APP)
    # compute_densityfeature_with_xyz_grad: first and second order
    zero_grads(m)
    x = x0.cuda().requires_grad_(True)
    (m.compute_densityfeature_with_xyz_grad(x) * w.cuda()).sum().backward()
    sc, params = scene64(m)
    xg = x0.double().requires_grad_(True)
    (_clamped_feature(sc, x0, xg) * w.double()).sum().backward()
    check_params(m, params, DENSITY)
    close(x.grad, xg.grad, "xyz")
    zero_grads(m)
    x = x0.cuda().requires_grad_(True)
    gx = torch.autograd.grad((m.compute_densityfeature_with_xyz_grad(x) * w.cuda()).sum(), x, create_graph=True)[0]
    (gx * V.cuda()).sum().backward()
    sc, params = scene64(m)
    xg = x0.double().requires_grad_(True)
    g64 = torch.autograd.grad((_clamped_feature(sc, x0, xg) * w.double()).sum(), xg, create_graph=True)[0]
    (g64 * V.double()).sum().backward()
    check_params(m, params, DENSITY)
    close(x.grad, xg.grad, "xyz (second order)")
    # compute_derived_normals
    xc = settle(frozen64(m), x0.clamp(-0.999, 0.999), row.act)
    zero_grads(m)
    xd = xc.cuda()
    nrm = m.compute_derived_normals(xd)
    (nrm * V[:xc.shape[0]].cuda()).sum().backward()
    sc, params = scene64(m)
    xg = xc.double().requires_grad_(True)
    (_ref_normals(sc, xc, xg) * V[:xc.shape[0]].double()).sum().backward()
    check_params(m, params, DENSITY, NORMAL_TOL)
    close(xd.grad, xg.grad, "xyz (normals)", NORMAL_TOL)
    zero_grads(m)


# ---- 3. every appearance gather the launcher accepts ------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("name", NAMES)
def test_app_gather_implementations(world, name):
    from tensoir_amd import ops
    from tensoir_amd._lib import TensoirHipError
    row = CS.ROW[name]
    m, _ = world.get(name)
    sc = frozen64(m)
    f = m.packed_field()
    worst = {}
    for impl in ("mfma", "valu", "bf16x3", "x3"):
        if impl not in APP_IMPLS[row.n_acomp]:
            x = mixed_points(64, 500).cuda()
            li = CS.light_indices(64, row.n_lights).view(-1).cuda()
            with pytest.raises(TensoirHipError, match="not supported"):
                ops.vm_app(f, x, li, None, True, True, impl)
            continue
        for n in (600, 599, 17, 1):
            x = mixed_points(n, 500 + n)
            li = CS.light_indices(n, row.n_lights).view(-1)
            r_ref, i_ref = O.both_feature(sc, x.double(), li, "explicit")
            r, i = ops.vm_app(f, x.cuda(), li.cuda(), None, True, True, impl)
            e = max(rel_err(r[:, :27], r_ref), rel_err(i[:, :27], i_ref))
            worst[impl] = max(worst.get(impl, 0.0), e)
            assert e < FEAT_TOL, (name, impl, n, e)
            assert float(r[:, 27:].abs().max()) == 0.0 and float(i[:, 27:].abs().max()) == 0.0
            r1 = ops.vm_app(f, x.cuda(), li.cuda(), None, True, False, impl)[0]
            i1 = ops.vm_app(f, x.cuda(), None, None, False, True, impl)[1]
            assert rel_err(r1[:, :27], r_ref) < FEAT_TOL and rel_err(i1[:, :27], i_ref) < FEAT_TOL, (name, impl, n)
        n = 600
        x = mixed_points(n, 500 + n)
        li = CS.light_indices(n, row.n_lights).view(-1)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
        r = ops.vm_app(f, x.cuda(), li[perm].contiguous().cuda(), torch.argsort(perm).int().cuda(), True, False, impl)[0]
        assert rel_err(r[:, :27], O.app_feature(sc, x.double(), li, "explicit")) < FEAT_TOL, (name, impl, "index map")
    if row.n_acomp != 48:                     # the 48-only entries refuse the field; none of them runs another width's kernel
        x = mixed_points(64, 77).cuda()
        li = CS.light_indices(64, row.n_lights).view(-1).cuda()
        with pytest.raises(TensoirHipError, match="not supported"):
            ops.vm_app_primary(f, x, li, torch.arange(64, dtype=torch.int32, device="cuda"), 0.01, None)
    print(f"\n[config-matrix] {name} gathers worst: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---- 4. the product calls ---------------------------------------------------------------------------------------------------
MAPS = ("rgb_map", "depth_map", "normal_map", "albedo_map", "roughness_map", "fresnel_map", "acc_map", "rgb_with_brdf_map",
        "normals_orientation_loss_map")


def render_eval(world, m, rays, lidx, relight):
    from tensoir_amd import Renderer_TensoIR_train
    with torch.no_grad(), entries() as e:
        ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=-1, white_bg=True, is_train=False, is_relight=relight,
                                     sample_method="fixed_envirmap", device="cuda", args=world.args)
    return ret, e.names


def oracle_eval(sc, rays, lidx, relight, dtype):
    s = sc.to(dtype)
    with torch.no_grad():
        return O.renderer_train(s, rays.to(dtype), lidx, n_samples=-1, is_relight=relight,
                                second_n_sample=CS.SECOND["second_nSample"], second_near=CS.SECOND["second_near"],
                                second_far=CS.SECOND["second_far"])


def check_eval_maps(name, ret, ref32, ref64, relight, report):
    for k in (MAPS if relight else ("rgb_map", "depth_map", "acc_map")):
        report[k] = max_err(ret[k], ref64[k])
    for k in (MAPS if relight else ("rgb_map", "depth_map", "acc_map")):
        assert report[k] < MAP_TOL, (name, relight, k, report[k])
    if relight:        # module docstring: rays on which the oracle itself determines normals_diff_map
        d = (ref32["normals_diff_map"].double() - ref64["normals_diff_map"]).abs().view(-1)
        ok = d < MAP_TOL / 4
        report["normals_diff_map rays compared"] = int(ok.sum())
        assert int(ok.sum()) >= DETERMINATE_RAYS[name], (name, int(ok.sum()))
        report["normals_diff_map"] = max_err(ret["normals_diff_map"].cpu().view(-1)[ok], ref64["normals_diff_map"].view(-1)[ok])
        assert report["normals_diff_map"] < MAP_TOL, (name, report["normals_diff_map"])
    assert float(ref64["acc_map"].max()) > 0.99 and float(ref64["acc_map"].min()) < 0.01      # rays that hit, rays that miss


@pytest.mark.parametrize("name", NAMES)
def test_render(world, name):
    row = CS.ROW[name]
    m, sc = world.get(name)
    rays, lidx, _ = CS.rays_for(row)
    for relight in (False, True):
        ret, names = render_eval(world, m, rays, lidx, relight)
        report = {}
        ref32, ref64 = (oracle_eval(sc, rays, lidx, relight, dt) for dt in (torch.float32, torch.float64))
        assert bool(((ref32["acc_map"] > 0.5) == (ref64["acc_map"] > 0.5)).all())
        try:
            check_eval_maps(name, ret, ref32, ref64, relight, report)
        finally:
            print(f"\n[config-matrix] {name} render relight={relight}: " + ", ".join(f"{k} {v:.2e}" for k, v in report.items()))
        if row.n_acomp != 48:                    # the fallback route: none of the 48-only kernels may have run
            assert not names & set(ONLY_48), (name, sorted(names & set(ONLY_48)))
        elif relight:
            assert names & {"tir_vm_app_primary_fwd", "tir_vm_app_primary_x3_fwd"}, sorted(names)


class decoder_mode:
    def __init__(self, impl):
        self.impl = impl

    def __enter__(self):
        from tensoir_amd import ops
        self.ops, self.old = ops, ops.MLP_IMPL
        ops.MLP_IMPL = self.impl

    def __exit__(self, *exc):
        self.ops.MLP_IMPL = self.old
        return False


@pytest.mark.parametrize("relight", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_training_step(world, name, relight):
    """tests/train_check.py on the row's batch in both decoder modes -- the split-bf16 default and the exact fp32 decoders,
    which take different launches through training.py (per-call / merged decoder forwards and backwards, tir_gemm_tn /
    tir_gemm_tn_small for the basis-matrix gradient, the latter instantiated per appearance width): loss 1e-5, maps 1e-4, every
    parameter gradient that is non-zero in the oracle at GTOL = 2e-3 (GRAD_BOUND for the one case with its own bound), on all
    rays; on a strict miss DESIGN 5's existing rule, unchanged: the rays are bisected down to one (a hidden unit whose
    pre-activation lies within rounding of zero takes the other side of its ReLU there), all the other rays together keep
    the strict bound on every tensor and the excluded ray's own deviation is bounded."""
    row = CS.ROW[name]
    m, sc = world.get(name)
    rays, lidx, gt = CS.rays_for(row)
    jitter, noise = CS.training_draws(rays.shape[0])
    batch = dict(rays=rays, lidx=lidx, gt=gt, S=CS.N_SAMPLES, jitter=jitter, noise=noise)
    env = types.SimpleNamespace(O=O, args=world.args)
    report = {}
    try:
        with decoder_mode("mfma"), entries() as e:
            check_training_step(env, m, sc, relight, 0.0, None, batch=batch, report=report, single_ray=True)        # GTOL
    finally:
        if report:
            print(f"\n[config-matrix] {name} train relight={relight} (fp32 decoders): loss {report.get('loss', float('nan')):.2e}, "
                  f"worst map {max(report.get('maps', {'-': float('nan')}).values()):.2e}, worst gradient "
                  f"{max(report.get('grads', {'-': float('nan')}).values()):.2e} over {len(report.get('grads', {}))} tensors")
            if "single_ray" in report:
                sr = report["single_ray"]
                print(f"[config-matrix] {name} relight={relight}: strict miss -> ray {sr['ray']} alone {sr['alone']}, all rays but it: "
                      f"worst gradient {max(sr['rest'].values()):.2e}")
    if row.n_acomp != 48:
        assert not e.names & set(ONLY_48), (name, sorted(e.names & set(ONLY_48)))
    # the split-bf16 default
    report = {}
    try:
        with decoder_mode("bf16x3"):
            check_training_step(env, m, sc, relight, 0.0, None, batch=batch, report=report, single_ray=True,
                                gtol=GRAD_BOUND.get((name, relight), GTOL))
    finally:
        if report:
            if "single_ray" in report:
                sr = report["single_ray"]
                print(f"\n[config-matrix] {name} relight={relight} (split-bf16): strict miss -> ray {sr['ray']} alone {sr['alone']}, all "
                      f"rays but it: worst gradient {max(sr['rest'].values()):.2e}")
            print(f"\n[config-matrix] {name} train relight={relight} (split-bf16 decoders): loss {report.get('loss', float('nan')):.2e}, "
                  f"worst map {max(report.get('maps', {'-': float('nan')}).values()):.2e}, worst gradient "
                  f"{max(report.get('grads', {'-': float('nan')}).values()):.2e} over {len(report.get('grads', {}))} tensors")


# ---- 5. light counts across the indirect-light tiers ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d16_a48_l9", "d16_a48_l17"])
def test_light_count_tiers(world, name):
    from tensoir_amd import ops
    row = CS.ROW[name]
    m, sc = world.get(name)
    rays, lidx, _ = CS.rays_for(row)
    want = {0, 8, row.n_lights - 1} | ({9, 16} if row.n_lights > 16 else set())
    assert want <= set(lidx.view(-1).tolist())
    ref64 = oracle_eval(sc, rays, lidx, True, torch.float64)
    hits = ref64["acc_map"] > 0.5
    assert want <= set(lidx.view(-1)[hits].tolist())               # ... on rays that are shaded
    old = ops.SECONDARY_MLP_IMPL, ops.SECONDARY_APP_IMPL, ops.INDIRECT_GUARD
    try:
        # "policy": the product default.  "full", "hp", "f16": the tier requested outright, guard off -- a tier whose fused kernel
        # does not exist for this light count must come out of the kernels that do (same numbers, no fused entry run)
        for tier in ("policy", "full", "hp", "f16"):
            if tier != "policy":
                ops.SECONDARY_MLP_IMPL, ops.SECONDARY_APP_IMPL = {"full": (None, None), "hp": ("hp", None), "f16": ("f16", "h16")}[tier]
                ops.INDIRECT_GUARD = False
            ret, names = render_eval(world, m, rays, lidx, True)
            err = max_err(ret["rgb_with_brdf_map"], ref64["rgb_with_brdf_map"])
            pol = m.indirect_precision()
            print(f"\n[config-matrix] {name} indirect tier {tier}: rgb_with_brdf_map {err:.2e}, policy {pol['policy']} mode {pol['mode']}, "
                  f"fused entries run: {sorted(n_ for n_ in names if 'indirect_fused' in n_)}")
            assert "tir_indirect_fused_hp_fwd" not in names, (name, tier)          # stages at most 8 light rows
            if row.n_lights > 16:
                assert "tir_indirect_fused_fwd" not in names, (name, tier)         # stages at most 16
            assert err < MAP_TOL, (name, tier, err)
            assert pol["policy"] == {"policy": "auto", "full": "full", "hp": "hp", "f16": "f16"}[tier], (tier, pol)
            if tier == "policy":
                assert pol["mode"] in ("f16", "full") or (pol["mode"] == "hp" and row.n_lights <= 8), pol
    finally:
        ops.SECONDARY_MLP_IMPL, ops.SECONDARY_APP_IMPL, ops.INDIRECT_GUARD = old
    # the per-light row is the one the index names: first, last and the tier borders, one light at a time
    with torch.no_grad():
        x = mixed_points(300, 900)
        s64 = frozen64(m)
        for l in sorted(want):
            li = torch.full((300,), l, dtype=torch.int32)
            for impl in APP_IMPLS[48]:
                r = ops.vm_app(m.packed_field(), x.cuda(), li.cuda(), None, True, False, impl)[0]
                assert rel_err(r[:, :27], O.app_feature(s64, x.double(), li, "explicit")) < FEAT_TOL, (name, l, impl)


# ---- 6. density lines inside / beyond the backward's 96 KB LDS staging -------------------------------------------------------
@pytest.mark.parametrize("long_axis", [0, 1, 2])
@pytest.mark.parametrize("total", [768, 776])
def test_density_line_staging_arms(world, total, long_axis):
    """point_density_bwd stages the three density lines in LDS while (gx + gy + gz) * n_dcomp * 4 <= 96 KB and uses global
    atomics beyond: with 32 components the border is a total line length of 768 -- exactly on it and above it, the long axis
    in each position.  Points: dyadic_points (exact positions on the long axis)."""
    row = CS.Row("lines", 32, 16, "softplus", 1, False)
    grid = [6, 8, 10]
    grid[long_axis] = total - (sum(grid) - grid[long_axis])
    assert sum(grid) == total and ((sum(grid) * 32 * 4 <= 96 * 1024) == (total == 768))
    ck = CS.checkpoint(row, grid=grid)
    m = world.tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=CS.ENVMAP_HW[0], envmap_w=CS.ENVMAP_HW[1])
    for n in (257, 8 * 1024 + 77):
        x0 = dyadic_points(n, 700 + n)
        w = torch.randn(n, generator=torch.Generator().manual_seed(5))
        zero_grads(m)
        out = m.compute_densityfeature(x0.cuda())
        (out * w.cuda()).sum().backward()
        sc, params = scene64(m)
        ref = O.density_feature(sc, x0.double(), "explicit")
        assert rel_err(out, ref) < FEAT_TOL
        (ref * w.double()).sum().backward()
        check_params(m, params, DENSITY)
        # the other two users of point_density_bwd
        zero_grads(m)
        x = x0.cuda().requires_grad_(True)
        (m.compute_densityfeature_with_xyz_grad(x) * w.cuda()).sum().backward()
        sc, params = scene64(m)
        xg = x0.double().requires_grad_(True)
        (_clamped_feature(sc, x0, xg) * w.double()).sum().backward()
        check_params(m, params, DENSITY)
        close(x.grad, xg.grad, "xyz")


# ---- 7. the two recorded scenes: the HIP path against the reference's own results -------------------------------------------
@pytest.mark.parametrize("name", CS.GOLDEN_ROWS)
def test_golden_scenes(world, name):
    row = CS.ROW[name]
    cg = world.cg
    m, _ = world.get(name)
    x = CS.feature_points()
    li = CS.light_indices(x.shape[0], row.n_lights)
    with torch.no_grad():
        f = m.compute_densityfeature(x.cuda())
        assert rel_err(f, cg[f"{name}/feat/density"]) < FEAT_TOL
        assert rel_err(m.feature2density(f), cg[f"{name}/feat/sigma"], 1e-3) < 1e-4
        assert rel_err(m.compute_appfeature(x.cuda(), li.cuda()), cg[f"{name}/feat/app"]) < FEAT_TOL
        assert rel_err(m.compute_intrinfeature(x.cuda()), cg[f"{name}/feat/intrin"]) < FEAT_TOL
        nrm = m.compute_derived_normals(x.clamp(-0.95, 0.95).cuda()).cpu()
    ref_n = T(cg, f"{name}/feat/derived_normals")
    n64 = O.density_grad(frozen64(m), x.clamp(-0.95, 0.95).double())[2]
    ok = (ref_n.double() - n64).abs().amax(-1) < 1e-3           # as tests/test_oracle_configs.py: where fp32 determines the normal
    assert float(ok.float().mean()) > 0.9 and max_err(nrm[ok], ref_n[ok]) < 2e-3
    rays, lidx, _ = CS.rays_for(row)
    ret, _ = render_eval(world, m, rays, lidx, True)
    for k in ("rgb_map", "depth_map", "normal_map", "albedo_map", "roughness_map", "acc_map", "rgb_with_brdf_map"):
        err = max_err(ret[k], cg[f"{name}/eval/{k}"])
        print(f"\n[config-matrix] {name} vs recorded reference {k}: {err:.2e}")
        assert err < MAP_TOL, (name, k, err)
