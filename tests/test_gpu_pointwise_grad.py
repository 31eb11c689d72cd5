"""Autograd of the model's public per-point methods (tensoir_amd/pointwise.py) against fp64 CPU autograd.

Field features and decoders are checked against oracle/tensoir_oracle.py.  compute_densityfeature_with_xyz_grad and
compute_derived_normals use the border-clamped taps of the reference's second-order grid_sample (models/relight_utils.py:
57-107), restated below in fp64 autograd; its floor decision is taken in the kernels' fp32 arithmetic, so that points on cell
edges select the same cells on both sides.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tensoir_oracle as O
from tests.helpers import golden_checkpoint
from tests.pointwise_ref import (ABS, ABS_REL, APP, DENSITY, NORMAL_TOL, REL, _axis, _clamped_feature, _ref_normals,  # noqa: F401
                                 check_params, close, scene64, zero_grads)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AABB = [[-1.5, -1.4, -1.3], [1.5, 1.4, 1.6]]
GRID = [20, 24, 28]


# ---- models -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    import tensoir_amd
    g = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    eh, ew = [int(x) for x in g["scene/envmap_hw"]]
    return tensoir_amd.model_from_checkpoint(golden_checkpoint(g), "cuda", envmap_h=eh, envmap_w=ew)


def random_model(app_comp, general=False, normals_kind="purely_predicted", seed=0):
    from tensoir_amd import TensorVMSplit
    from tensoir_amd.general_multi_lights import TensorVMSplit as General
    torch.manual_seed(seed)
    kw = dict(aabb=torch.tensor(AABB), gridSize=GRID, device="cuda", density_n_comp=16, appearance_n_comp=app_comp,
              shadingMode="MLP_Fea", light_kind="sg", normals_kind=normals_kind, pos_pe=2, view_pe=2, fea_pe=2)
    m = General(**kw) if general else TensorVMSplit(**kw)
    with torch.no_grad():                        # densities in a range where softplus' and softplus'' are not negligible
        for p in m.density_plane:
            p.mul_(30.0)
        for mod in (m.renderModule, m.renderModule_brdf, getattr(m, "renderModule_normal", None)):
            if mod is not None:
                mod.mlp[-1].bias.normal_(0.0, 0.3)
    return m


MODELS = ["golden", "rand48", "rand16", "general"]


@pytest.fixture(scope="module")
def models(golden):
    return {"golden": golden, "rand48": random_model(48), "rand16": random_model(16, seed=1),
            "general": random_model(48, general=True, seed=2)}


# ---- point sets (normalised coordinates) ------------------------------------------------------------------------------------
def points(kind, n=1000, seed=0):
    gen = torch.Generator().manual_seed(seed)
    if kind == "inbox":
        return torch.rand(n, 3, generator=gen) * 1.9 - 0.95
    if kind == "edges":           # on grid lines of every axis, and on +-1
        k = torch.stack([torch.randint(0, g, (n,), generator=gen) for g in GRID], -1).float()
        p = k / (torch.tensor(GRID).float() - 1) * 2 - 1
        p[: n // 4, 0] = 1.0
        p[n // 4: n // 2, 1] = -1.0
        off = torch.rand(n, 3, generator=gen) * 0.1 - 0.05
        sel = torch.rand(n, 3, generator=gen) < 0.3       # some coordinates off the line: mixes edge and interior axes
        return torch.where(sel, (p + off).clamp(-1, 1), p)
    if kind == "outside":
        return torch.rand(n, 3, generator=gen) * 2.6 - 1.3
    if kind == "dups":
        return (torch.rand(1, 3, generator=gen) * 1.8 - 0.9).expand(4096, 3).contiguous()
    if kind == "empty":
        return torch.zeros(0, 3)
    raise ValueError(kind)


POINTS = ["inbox", "edges", "outside", "dups", "empty"]


# ---- field methods ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("kind", POINTS)
def test_densityfeature(models, name, kind):
    model = models[name]
    x = points(kind).cuda()
    w = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(3)).cuda()
    zero_grads(model)
    out = model.compute_densityfeature(x)
    with torch.no_grad():
        assert torch.equal(out, model.compute_densityfeature(x))
    assert x.grad is None and out.requires_grad
    (out * w).sum().backward()
    sc, params = scene64(model)
    (O.density_feature(sc, x.cpu().double(), "explicit") * w.cpu().double()).sum().backward()
    check_params(model, params, DENSITY)


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("kind", ["inbox", "edges", "outside", "dups"])       # (the appearance gathers refuse n = 0)
@pytest.mark.parametrize("method", ["app", "intrin", "both"])
def test_app_features(models, name, kind, method):
    model = models[name]
    x = points(kind, seed=4).cuda()
    n = x.shape[0]
    gen = torch.Generator().manual_seed(5)
    li = torch.randint(0, model.light_num, (n,), generator=gen)
    w = torch.randn(2, n, model.app_dim, generator=gen).cuda()
    zero_grads(model)
    if method == "app":
        outs = (model.compute_appfeature(x, li.cuda()),)
        with torch.no_grad():
            ref_vals = (model.compute_appfeature(x, li.cuda()),)
    elif method == "intrin":
        outs = (model.compute_intrinfeature(x),)
        with torch.no_grad():
            ref_vals = (model.compute_intrinfeature(x),)
    else:
        outs = model.compute_bothfeature(x, li.cuda())
        with torch.no_grad():
            ref_vals = model.compute_bothfeature(x, li.cuda())
    for a, b in zip(outs, ref_vals):
        assert torch.equal(a, b)
    sum(((o * w[i]).sum() for i, o in enumerate(outs)), torch.zeros((), device="cuda")).backward()
    sc, params = scene64(model)
    x64 = x.cpu().double()
    if method == "app":
        refs = (O.app_feature(sc, x64, li, "explicit"),)
    elif method == "intrin":
        refs = (O.intrin_feature(sc, x64, "explicit"),)
    else:
        refs = O.both_feature(sc, x64, li, "explicit")
    sum((r * w[i].cpu().double()).sum() for i, r in enumerate(refs)).backward()
    check_params(model, params, APP)


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("kind", POINTS)
def test_densityfeature_with_xyz_grad(models, name, kind):
    model = models[name]
    x0 = points(kind, seed=6).cuda()
    n = x0.shape[0]
    gen = torch.Generator().manual_seed(7)
    w, V = torch.randn(n, generator=gen), torch.randn(n, 3, generator=gen)
    # first order: parameters and xyz
    zero_grads(model)
    x = x0.clone().requires_grad_(True)
    out = model.compute_densityfeature_with_xyz_grad(x)
    with torch.no_grad():
        assert torch.equal(out, model.compute_densityfeature_with_xyz_grad(x0))
        assert torch.equal(out[(x0.abs() <= 1).all(-1)], model.compute_densityfeature(x0)[(x0.abs() <= 1).all(-1)])
    (out * w.cuda()).sum().backward()
    sc, params = scene64(model)
    x64 = x0.cpu().double().requires_grad_(True)
    (_clamped_feature(sc, x0.cpu(), x64) * w.double()).sum().backward()
    check_params(model, params, DENSITY)
    close(x.grad, x64.grad, "xyz")
    # second order: a loss on d feature / d xyz (create_graph=True), as compute_derived_normals builds
    zero_grads(model)
    x = x0.clone().requires_grad_(True)
    feat = model.compute_densityfeature_with_xyz_grad(x)
    gx = torch.autograd.grad((feat * w.cuda()).sum(), x, create_graph=True)[0]
    (gx * V.cuda()).sum().backward()
    sc, params = scene64(model)
    x64 = x0.cpu().double().requires_grad_(True)
    f64 = _clamped_feature(sc, x0.cpu(), x64)
    g64 = torch.autograd.grad((f64 * w.double()).sum(), x64, create_graph=True)[0]
    (g64 * V.double()).sum().backward()
    check_params(model, params, DENSITY)
    close(x.grad, x64.grad, "xyz (second order)")


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("kind", POINTS)
def test_derived_normals(models, name, kind):
    model = models[name]
    x0 = points(kind, seed=8).cuda()
    if kind == "outside":
        x0 = x0.clamp(-0.999, 0.999)          # outside the box sigma is flat along clamped axes: normals of a zero gradient
    W = torch.randn(x0.shape[0], 3, generator=torch.Generator().manual_seed(9))
    zero_grads(model)
    x = x0.clone()
    nrm = model.compute_derived_normals(x)
    assert x.requires_grad                     # as the reference (models/tensorBase_rotated_lights.py:841)
    with torch.no_grad():
        assert torch.equal(nrm, model.compute_derived_normals(x0))
    (nrm * W.cuda()).sum().backward()
    sc, params = scene64(model)
    x64 = x0.cpu().double().requires_grad_(True)
    (_ref_normals(sc, x0.cpu(), x64) * W.double()).sum().backward()
    check_params(model, params, DENSITY, NORMAL_TOL)
    close(x.grad, x64.grad, "xyz", NORMAL_TOL)


@pytest.mark.parametrize("name", ["golden", "rand48"])
@pytest.mark.parametrize("kind", ["inbox", "outside", "dups", "empty"])
def test_compute_alpha(models, name, kind):
    model = models[name]
    lo, hi = model.aabb[0].cpu(), model.aabb[1].cpu()
    xw = (lo + (points(kind, seed=10) + 1) / 2 * (hi - lo)).cuda()
    w = torch.randn(xw.shape[0], generator=torch.Generator().manual_seed(11)).cuda()
    for masked in ((False, True) if model.alphaMask is not None else (False,)):
        mask_obj = model.alphaMask
        if not masked:
            model.alphaMask = None
        try:
            zero_grads(model)
            a = model.compute_alpha(xw, length=0.7)
            with torch.no_grad():
                assert torch.equal(a, model.compute_alpha(xw, length=0.7))
            (a * w).sum().backward()
            xn = model.normalize_coord(xw).cpu().double()
            hit = mask_obj.sample_alpha(xw).cpu().double() if masked else torch.ones(xw.shape[0], dtype=torch.float64)
        finally:
            model.alphaMask = mask_obj
        sc, params = scene64(model)
        sigma = F.softplus(O.density_feature(sc, xn, "explicit") + sc.density_shift) * hit
        ((1 - torch.exp(-sigma * 0.7)) * w.cpu().double()).sum().backward()
        check_params(model, params, DENSITY)


# ---- decoders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["golden", "rand48", "general"])
@pytest.mark.parametrize("which", ["rgb", "brdf", "normal"])
def test_decoders(models, name, which):
    model = models[name]
    n = 1000
    gen = torch.Generator().manual_seed(12)
    feat0 = torch.randn(n, model.app_dim, generator=gen) * 0.5
    aux = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    dec = {"rgb": model.renderModule, "brdf": model.renderModule_brdf, "normal": model.renderModule_normal}[which]
    W = torch.randn(n, dec.outc, generator=gen)
    zero_grads(model)
    feat = feat0.cuda().requires_grad_(True)
    out = dec(aux.cuda(), aux.cuda(), feat) if which == "rgb" else dec(aux.cuda(), feat)
    with torch.no_grad():
        ref_out = dec(aux.cuda(), aux.cuda(), feat0.cuda()) if which == "rgb" else dec(aux.cuda(), feat0.cuda())
    assert torch.equal(out, ref_out)
    (out * W.cuda()).sum().backward()
    sc, params = scene64(model)
    f64 = feat0.double().requires_grad_(True)
    fn = {"rgb": O.render_rgb, "brdf": O.render_brdf, "normal": O.render_normal}[which]
    (fn(sc, aux.double(), f64) * W.double()).sum().backward()
    prefix = {"rgb": "renderModule", "brdf": "renderModule_brdf", "normal": "renderModule_normal"}[which]
    check_params(model, params, [n_ for n_ in params if n_.startswith(prefix + ".")])
    close(feat.grad, f64.grad, "features")


def test_residue_normal_decoder():
    model = random_model(48, normals_kind="residue_prediction", seed=13)
    dec = model.renderModule_normal
    n = 777
    gen = torch.Generator().manual_seed(14)
    feat0 = torch.randn(n, model.app_dim, generator=gen) * 0.5
    pts = torch.rand(n, 3, generator=gen) * 2 - 1
    nrm0 = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    W = torch.randn(n, 3, generator=gen)
    feat, nrm = feat0.cuda().requires_grad_(True), nrm0.cuda().requires_grad_(True)
    out = dec(pts.cuda(), nrm, feat)
    with torch.no_grad():
        assert torch.equal(out, dec(pts.cuda(), nrm0.cuda(), feat0.cuda()))
    (out * W.cuda()).sum().backward()
    sc, params = scene64(model)
    f64, n64 = feat0.double().requires_grad_(True), nrm0.double().requires_grad_(True)
    (O.render_normal_residue(sc, pts.double(), n64, f64) * W.double()).sum().backward()
    check_params(model, params, [k for k in params if k.startswith("renderModule_normal.")])
    close(feat.grad, f64.grad, "features")
    close(nrm.grad, n64.grad, "normal input")


def test_decoder_positional_inputs_refused(models):
    model = models["rand48"]
    feat = torch.randn(10, model.app_dim, device="cuda", requires_grad=True)
    pts = torch.rand(10, 3, device="cuda").requires_grad_()
    with pytest.raises(NotImplementedError, match="positional-encoding"):
        model.renderModule_brdf(pts, feat)
    with pytest.raises(NotImplementedError, match="positional-encoding"):
        model.renderModule(pts, pts, feat)


# ---- semantics --------------------------------------------------------------------------------------------------------------
def test_backward_calls_accumulate(models):
    model = models["rand48"]
    x = points("inbox").cuda()
    zero_grads(model)
    model.compute_densityfeature(x).sum().backward()
    once = [p.grad.clone() for p in model.density_plane]
    model.compute_densityfeature(x).sum().backward()
    for p, g in zip(model.density_plane, once):
        torch.testing.assert_close(p.grad, 2 * g, rtol=1e-6, atol=1e-7)


def test_two_uses_in_one_graph_sum(models):
    model = models["golden"]
    x1, x2 = points("inbox", 500, seed=15).cuda(), points("outside", 300, seed=16).cuda()
    li1, li2 = torch.zeros(500, dtype=torch.long), torch.ones(300, dtype=torch.long)
    zero_grads(model)
    loss = model.compute_appfeature(x1, li1.cuda()).sum() + 2 * model.compute_appfeature(x2, li2.cuda()).sum()
    loss = loss + model.compute_densityfeature_with_xyz_grad(x1).sum() + model.compute_densityfeature_with_xyz_grad(x2).sum()
    loss.backward()
    sc, params = scene64(model)
    ref = (O.app_feature(sc, x1.cpu().double(), li1, "explicit").sum() + 2 * O.app_feature(sc, x2.cpu().double(), li2, "explicit").sum()
           + _clamped_feature(sc, x1.cpu(), x1.cpu().double()).sum() + _clamped_feature(sc, x2.cpu(), x2.cpu().double()).sum())
    ref.backward()
    check_params(model, params, APP + DENSITY)


def test_fused_forward_unchanged(golden):
    """The fused render is untouched by the per-point autograd: every output that two plain calls reproduce bit for bit is
    the same after the new methods have run forward and backward."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    rays = torch.from_numpy(np.array(g["rays/rays"]))[:256].cuda()
    lidx = torch.from_numpy(np.array(g["rays/light_idx"]))[:256].cuda()
    flat = lambda r: [t for t in (r.values() if isinstance(r, dict) else (r if isinstance(r, (tuple, list)) else [r])) if torch.is_tensor(t)]
    with torch.no_grad():
        first, before = flat(golden(rays, lidx)), flat(golden(rays, lidx))
    stable = [i for i, (a, b) in enumerate(zip(first, before)) if torch.equal(a, b)]
    assert stable
    x = points("inbox").cuda()
    loss = golden.compute_densityfeature(x).sum() + golden.compute_intrinfeature(x).sum() + golden.compute_derived_normals(x.clone()).sum()
    loss = loss + golden.compute_alpha(x).sum() + golden.renderModule_brdf(x, golden.compute_intrinfeature(x)).sum()
    loss.backward()
    zero_grads(golden)
    with torch.no_grad():
        after = flat(golden(rays, lidx))
    for i in stable:
        assert torch.equal(before[i], after[i])
