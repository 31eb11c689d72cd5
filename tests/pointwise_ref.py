"""fp64 CPU references and comparison helpers of the per-point autograd tests (tests/test_gpu_pointwise_grad.py,
tests/test_gpu_config_matrix.py).

compute_densityfeature_with_xyz_grad and compute_derived_normals use the border-clamped taps of the reference's second-order
grid_sample (models/relight_utils.py:57-107), restated here in fp64 autograd; its floor decision is taken in the kernels' fp32
arithmetic, so that points on cell edges select the same cells on both sides.
"""
from types import SimpleNamespace

import torch

from oracle import tensoir_oracle as O

REL, ABS_REL, ABS = 1e-5, 1e-5, 1e-7
# the derived normal is the field gradient divided by its length: fp32 rounding of the gradient (and the cancellation in
# dn - n (n . dn)) is amplified where the field is flat, so its gradients are compared at a looser bound
NORMAL_TOL = 5e-4


def scene64(model):
    """fp64 CPU leaf copies of the model's parameters in the oracle's Scene layout (+ name -> tensor)."""
    named = dict(model.named_parameters())
    leaf = lambda name: named[name].detach().double().cpu().contiguous().requires_grad_(True)
    sc = SimpleNamespace(density_shift=float(model.density_shift), fea_pe=model.fea_pe, view_pe=model.view_pe,
                         pos_pe=model.pos_pe, fea2denseAct=str(model.fea2denseAct))
    params = {}
    for kind in ("density_plane", "density_line", "app_plane", "app_line"):
        ts = [leaf(f"{kind}.{i}") for i in range(3)]
        setattr(sc, kind, ts)
        params.update({f"{kind}.{i}": t for i, t in enumerate(ts)})
    sc.basis_mat, sc.light_line = leaf("basis_mat.weight"), leaf("light_line.weight")
    params["basis_mat.weight"], params["light_line.weight"] = sc.basis_mat, sc.light_line
    for attr, prefix in (("mlp_rgb", "renderModule"), ("mlp_brdf", "renderModule_brdf"), ("mlp_normal", "renderModule_normal")):
        if f"{prefix}.mlp.0.weight" not in named:
            continue
        d = {}
        for j, k in ((0, "0"), (1, "2"), (2, "4")):
            for w, n in (("w", "weight"), ("b", "bias")):
                name = f"{prefix}.mlp.{k}.{n}"
                d[f"{w}{j}"] = params[name] = leaf(name)
        setattr(sc, attr, d)
    return sc, params


def zero_grads(model):
    for p in model.parameters():
        p.grad = None


def close(ours, ref, what, tol=REL):
    ours, ref = ours.detach().double().cpu(), ref.detach().double().cpu()
    assert ours.shape == ref.shape, what
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = (ours - ref).abs()
    rel = float(torch.linalg.vector_norm(ours - ref) / torch.linalg.vector_norm(ref).clamp(min=1e-30)) if ref.numel() else 0.0
    assert rel <= tol or scale == 0.0, f"{what}: relative L2 {rel:.3g}"
    assert float(err.max()) <= tol * scale + ABS if err.numel() else True, f"{what}: max err {float(err.max()):.3g} (scale {scale:.3g})"


def check_params(model, params, names, tol=REL):
    named = dict(model.named_parameters())
    for name in names:
        g = named[name].grad
        ref = params[name].grad
        assert g is not None, f"{name}: no gradient"
        close(g, torch.zeros_like(params[name]) if ref is None else ref, name, tol)


DENSITY = [f"density_{k}.{i}" for k in ("plane", "line") for i in range(3)]
APP = [f"app_{k}.{i}" for k in ("plane", "line") for i in range(3)] + ["basis_mat.weight", "light_line.weight"]



# ---- fp64 restatement of the border-clamped taps (models/relight_utils.py:57-107) -------------------------------------------
def _axis(x32, size):
    """floor index in the kernels' fp32 arithmetic (tir::unnorm, each operation rounded) and the fp64 position."""
    ix32 = ((x32 + 1.0) * 0.5) * float(size - 1)
    i0 = torch.floor(ix32)
    ix = ((x32.double() + 1) / 2) * (size - 1)
    return i0.long(), ix


def _clamped_feature(sc, x32, x64):
    """compute_densityfeature_with_xyz_grad with the reference's grid_sample: clamped tap indices, unclamped weights.  Evaluated
    in the type of x64 (float64 for every caller but the float32 yardstick of tests/fieldgrad_reference.py)."""
    out = torch.zeros(x64.shape[0], dtype=x64.dtype)
    for i in range(3):
        m0, m1 = O.MAT_MODE[i]
        vi = O.VEC_MODE[i]
        plane, line = sc.density_plane[i][0], sc.density_line[i][0, :, :, 0]
        C, H, W = plane.shape
        R = line.shape[1]
        x0, _ = _axis(x32[:, m0], W)
        y0, _ = _axis(x32[:, m1], H)
        l0, _ = _axis(x32[:, vi], R)
        ix = ((x64[:, m0] + 1) / 2) * (W - 1)
        iy = ((x64[:, m1] + 1) / 2) * (H - 1)
        il = ((x64[:, vi] + 1) / 2) * (R - 1)
        tx, ty, tl = ix - x0.to(x64.dtype), iy - y0.to(x64.dtype), il - l0.to(x64.dtype)
        flat = plane.reshape(C, H * W)
        tap = lambda xx, yy: flat[:, yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)]
        P = (tap(x0, y0) * ((1 - tx) * (1 - ty)) + tap(x0 + 1, y0) * (tx * (1 - ty)) + tap(x0, y0 + 1) * ((1 - tx) * ty)
             + tap(x0 + 1, y0 + 1) * (tx * ty))
        L = line[:, l0.clamp(0, R - 1)] * (1 - tl) + line[:, (l0 + 1).clamp(0, R - 1)] * tl
        out = out + (P * L).sum(0)
    return out


def _ref_normals(sc, x32, x64):
    """compute_derived_normals (models/tensorBase_rotated_lights.py:839-856) on the restatement, create_graph=True."""
    feat = _clamped_feature(sc, x32, x64)
    sigma = O.feature2density(sc, feat)
    g = torch.autograd.grad(sigma, x64, torch.ones_like(sigma), create_graph=True)[0]
    return -g / torch.clamp(torch.linalg.vector_norm(g, dim=-1, keepdim=True), min=1e-6)
