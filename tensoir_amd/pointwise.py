"""Autograd of the model's public per-point methods.

In the reference every one of them is plain differentiable PyTorch (F.grid_sample, the custom second-order grid_sample of
models/relight_utils.py:57-107, nn.Linear), so a fork can put a loss on sampled points.  Here each method is one
torch.autograd.Function whose forward launches exactly the kernels of the no-grad call (the values are bit-identical) and
whose backward is HIP launches too:

  DensityFeatureFn   compute_densityfeature                 tir_vm_density_fwd   -> tir_vm_density_bwd
  DensitySigmaFn     sigma of compute_alpha                 tir_vm_density_fwd   -> tir_vm_density_bwd
  DensityFeatXyzFn   compute_densityfeature_with_xyz_grad   tir_density_feat_grad_fwd -> DensityFeatXyzBwdFn
  DensityFeatXyzBwdFn  (its backward, differentiable once more: tir_density_feat_bwd -> tir_density_feat_grad_bwd)
  DerivedNormalFn    compute_derived_normals                tir_density_grad_fwd -> tir_density_grad_bwd + Hessian product
  AppFeatureFn       compute_{app,intrin,both}feature       tir_vm_app_fwd       -> tir_vm_app_bwd + tir_gemm_tn
  DecoderFn          the three decoders' forward            tir_mlp_fwd*         -> tir_mlp_bwd + tir_gemm_tn

Gradients accumulate into the packed channel-last buffers of training._grad_buffers and reach autograd in parameter shape.
The coordinates get no gradient where the reference detaches them (compute_densityfeature, the appearance features: the
coordinates are `.detach()`ed at models/tensoRF_rotated_lights.py:98-100, :141-143); the decoders' position / view-direction
inputs have no input-gradient kernel and are refused.  The backward passes use the exact fp32 decoder and GEMM kernels
whatever the forward's decoder precision is.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import ops, training


def density_params(model):
    return list(model.density_plane) + list(model.density_line)


def app_params(model):
    return list(model.app_plane) + list(model.app_line) + [model.basis_mat.weight, model.light_line.weight]


def _grads(bufs, names):
    return tuple(training._to_param_layout(bufs[f"{name}{i}"]) for name in names for i in range(3))


def _density_grads(bufs):
    return _grads(bufs, ("dp", "dl"))


class DensityFeatureFn(torch.autograd.Function):
    """compute_densityfeature (models/tensoRF_rotated_lights.py:95-110): F.grid_sample taps, zero padding."""

    @staticmethod
    def forward(ctx, model, xyz, *params):
        ctx.model = model
        ctx.save_for_backward(xyz)
        return ops.vm_density(model.packed_field(), xyz)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_feat):
        model, (xyz,) = ctx.model, ctx.saved_tensors
        f = model.packed_field()
        bufs = training._grad_buffers(model, f)
        ops.vm_density_bwd(f, bufs["desc"], xyz, g_feat)
        return (None, None) + _density_grads(bufs)


class DensitySigmaFn(torch.autograd.Function):
    """feature2density(compute_densityfeature(x)) of compute_alpha (models/tensorBase_rotated_lights.py:813-837)."""

    @staticmethod
    def forward(ctx, model, xyz, *params):
        feat, sigma = ops.vm_density(model.packed_field(), xyz, True, True)
        ctx.model = model
        ctx.save_for_backward(xyz, feat)
        return sigma

    @staticmethod
    @once_differentiable
    def backward(ctx, g_sigma):
        model, (xyz, feat) = ctx.model, ctx.saved_tensors
        if model.fea2denseAct == "softplus":          # torch's own softplus / relu derivatives (beta 1, threshold 20)
            g_feat = torch.ops.aten.softplus_backward(g_sigma, feat + model.density_shift, 1.0, 20.0)
        else:
            g_feat = torch.ops.aten.threshold_backward(g_sigma, feat, 0.0)
        f = model.packed_field()
        bufs = training._grad_buffers(model, f)
        ops.vm_density_bwd(f, bufs["desc"], xyz, g_feat)
        return (None, None) + _density_grads(bufs)


class DensityFeatXyzFn(torch.autograd.Function):
    """compute_densityfeature_with_xyz_grad (models/tensoRF_rotated_lights.py:113-129): border-clamped taps, gradients to
    the parameters and to xyz, twice differentiable (the backward is DensityFeatXyzBwdFn)."""

    @staticmethod
    def forward(ctx, model, xyz, *params):
        ctx.model = model
        ctx.save_for_backward(xyz, *params)
        return ops.density_feat_grad(model.packed_field(), xyz, True, False)[0]

    @staticmethod
    def backward(ctx, g_feat):
        xyz, *params = ctx.saved_tensors
        res = DensityFeatXyzBwdFn.apply(ctx.model, xyz, g_feat, *params)
        return (None, res[0] if ctx.needs_input_grad[1] else None) + tuple(res[1:])


class DensityFeatXyzBwdFn(torch.autograd.Function):
    """(g_xyz, parameter gradients) = VJP of DensityFeatXyzFn for g_feat.  g_xyz = g_feat grad f(x) is what
    compute_derived_normals' create_graph=True differentiates again (models/tensorBase_rotated_lights.py:839-856): its backward
    is tir_density_feat_grad_bwd (parameter VJP + Hessian-vector product) and g_feat's cotangent v . grad f(x)."""

    @staticmethod
    def forward(ctx, model, xyz, g_feat, *params):
        f = model.packed_field()
        bufs = training._grad_buffers(model, f)
        g_xyz = ops.density_feat_bwd(f, bufs["desc"], xyz, g_feat)
        ctx.model = model
        ctx.save_for_backward(xyz, g_feat)
        ctx.set_materialize_grads(False)
        return (g_xyz,) + _density_grads(bufs)

    @staticmethod
    @once_differentiable
    def backward(ctx, gg_xyz, *gg_params):
        if any(g is not None for g in gg_params):
            raise NotImplementedError("compute_densityfeature_with_xyz_grad: differentiating its parameter gradients again "
                                      "(a third-order term) has no backward kernel")
        n_out = 3 + len(gg_params)
        if gg_xyz is None:
            return (None,) * n_out
        model, (xyz, g_feat) = ctx.model, ctx.saved_tensors
        f = model.packed_field()
        bufs = training._grad_buffers(model, f)
        hv = ops.density_feat_grad_bwd(f, bufs["desc"], xyz, g_feat.reshape(-1, 1) * gg_xyz, want_xyz=ctx.needs_input_grad[1])
        d_gfeat = None
        if ctx.needs_input_grad[2]:
            d_gfeat = (ops.density_feat_grad(f, xyz, False, True)[1] * gg_xyz).sum(-1).view_as(g_feat)
        return (None, hv, d_gfeat) + _density_grads(bufs)


def _normal_cotangents(model, feat, grad, g_normal):
    """Cotangents (F of the feature, G of its xyz gradient) of the derived normal n = -normalize(act'(feat) grad, eps=1e-6)
    for g_normal -- the arithmetic of tir_density_grad_bwd (tensoir_amd/csrc/tir_train.hip, k_density_grad_bwd)."""
    if model.fea2denseAct == "softplus":
        x = feat + model.density_shift
        big = x > 20.0
        ds = torch.where(big, torch.ones_like(x), torch.sigmoid(x))
        dds = torch.where(big, torch.zeros_like(x), ds * (1.0 - ds))
    else:
        ds, dds = (feat > 0).to(feat.dtype), torch.zeros_like(feat)
    g = ds[:, None] * grad
    nrm = torch.linalg.vector_norm(g, dim=-1, keepdim=True)
    n = -g / nrm.clamp_min(1e-6)
    dot = (n * g_normal).sum(-1, keepdim=True)
    dg = torch.where(nrm > 1e-6, -(g_normal - n * dot) / nrm.clamp_min(1e-6), -g_normal / 1e-6)
    return dds * (dg * grad).sum(-1), ds[:, None] * dg


class DerivedNormalFn(torch.autograd.Function):
    """compute_derived_normals (models/tensorBase_rotated_lights.py:839-856): tir_density_grad_fwd's normal.  Backward: the
    parameters through tir_density_grad_bwd (the training step's own derived-normal backward), xyz through the feature's
    gradient and Hessian: g_xyz = F grad f + H G (tir_density_feat_grad_fwd, tir_density_feat_grad_bwd)."""

    @staticmethod
    def forward(ctx, model, xyz, *params):
        ctx.model = model
        ctx.save_for_backward(xyz)
        return ops.density_grad(model.packed_field(), xyz)[2]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_normal):
        model, (xyz,) = ctx.model, ctx.saved_tensors
        f = model.packed_field()
        g_normal = g_normal.contiguous()
        bufs = training._grad_buffers(model, f)
        ops.density_grad_bwd(f, bufs["desc"], xyz, g_normal)
        g_xyz = None
        if ctx.needs_input_grad[1]:
            feat, grad = ops.density_feat_grad(f, xyz)
            F, G = _normal_cotangents(model, feat, grad, g_normal)
            g_xyz = ops.density_feat_grad_bwd(f, None, xyz, G).addcmul_(F[:, None], grad)
        return (None, g_xyz) + _density_grads(bufs)


def _basis_grad(model, pairs):
    """d basis_mat.weight = sum over the gathers of g_feat^T y (tir_gemm_tn, exact fp32; at most 160 columns per launch)."""
    nb = 3 * model.app_n_comp[0]
    d_basis = torch.zeros((model.app_dim, nb), dtype=torch.float32, device=pairs[0][0].device)
    for g, y in pairs:
        if g.shape[0] == 0:
            continue
        for j in range(0, nb, 160):
            w = min(160, nb - j)
            if j == 0 and w == nb:
                ops.gemm_tn(g, model.app_dim, y, nb, d_basis, impl="fp32")
            else:
                part = torch.zeros((model.app_dim, w), dtype=torch.float32, device=g.device)
                d_basis[:, j:j + w] += ops.gemm_tn(g, model.app_dim, y[:, j:j + w].contiguous(), w, part, impl="fp32")
    return d_basis


class AppFeatureFn(torch.autograd.Function):
    """compute_appfeature / compute_intrinfeature / compute_bothfeature (models/tensoRF_rotated_lights.py:132-224):
    radiance features (light row light_idx) and / or intrinsic features (mean light row), [n, app_dim] each."""

    @staticmethod
    def forward(ctx, model, xyz, light_idx, want_rad, want_int, *params):
        rad, intr = ops.vm_app(model.packed_field(), xyz, light_idx, None, want_rad, want_int, ops.APP_IMPL)
        ad = model.app_dim
        outs = [t[:, :ad].contiguous() for t in (rad, intr) if t is not None]
        ctx.model, ctx.flags = model, (want_rad, want_int)
        ctx.save_for_backward(xyz, light_idx)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        model, (xyz, light_idx) = ctx.model, ctx.saved_tensors
        want_rad, want_int = ctx.flags
        gs = list(gs)
        g_rad = gs.pop(0) if want_rad else None
        g_int = gs.pop(0) if want_int else None
        n_out = 5 + 8
        if g_rad is None and g_int is None:
            return (None,) * n_out
        f = model.packed_field()
        n, ad = xyz.shape[0], model.app_dim

        def padded(g):                   # feature-gradient rows in the gathers' 128-byte row layout
            if g is None:
                return None
            p = torch.zeros((n, ops.FEAT_STRIDE), dtype=torch.float32, device=xyz.device)
            p[:, :ad] = g
            return p

        g_rad, g_int = padded(g_rad), padded(g_int)
        bufs = training._grad_buffers(model, f)
        y_rad, y_int = ops.vm_app_bwd(f, bufs["desc"], xyz, light_idx if g_rad is not None else None, None, g_rad, g_int)
        d_basis = _basis_grad(model, [(g, y) for g, y in ((g_rad, y_rad), (g_int, y_int)) if g is not None])
        d_light = torch.add(bufs["ll"], bufs["lm"][None, :], alpha=1.0 / float(model.light_num))     # mean row: 1/L per light
        return (None,) * 5 + _grads(bufs, ("ap", "al")) + (d_basis, d_light)


def decoder_params(dec):
    m = dec.mlp
    return [m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias]


class DecoderFn(torch.autograd.Function):
    """MLPRender_Fea / MLPBRDF_PEandFeature / MLPNormal_normal_and_PExyz forward (models/tensorBase_rotated_lights.py:122-262):
    gradients to the features, the six weights and biases and -- residue decoder -- its derived-normal input.  The hidden
    activations are recomputed in the backward (the forward launches the inference kernel of the no-grad call)."""

    @staticmethod
    def forward(ctx, dec, feat, aux, normal, *params):
        out = ops.mlp(dec.packed(), feat, aux) if normal is None else dec.rows(aux, normal, feat)
        ctx.dec = dec
        ctx.save_for_backward(feat, aux, normal, out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        dec, (feat, aux, normal, out) = ctx.dec, ctx.saved_tensors
        n, fd = feat.shape[0], dec.in_chanel
        feat_p = torch.zeros((n, ops.FEAT_STRIDE), dtype=torch.float32, device=feat.device)
        feat_p[:, :fd] = feat
        if normal is None:
            _, h1, h2 = ops.mlp_train(dec.packed(), feat_p, aux, impl="fp32")
        else:
            _, h1, h2 = dec.rows(aux, normal, feat_p, save_hidden=True)
        call = training._DecoderCall(feat=feat_p, aux=aux, aux_map=None, out=out, g_out=g_out.contiguous(), h1=h1, h2=h2)
        dz1 = [] if normal is not None else None
        (g_feat,), grads = training._decoder_backward(dec, [call], impl="fp32", keep_dz1=dz1)
        g_normal = None
        if normal is not None:
            # the three derived-normal columns of layer 1 ride outside the kernels (as in training.PrimaryRenderFn.backward)
            full = torch.empty_like(dec.mlp[0].weight)
            full.index_copy_(1, dec.std_cols_index(full.device), grads[0])
            full[:, 3:6] = dz1[0].t() @ normal
            grads[0] = full
            if ctx.needs_input_grad[3]:
                g_normal = dz1[0] @ dec.w0_normal()
        g_feat = g_feat[:, :fd] if ctx.needs_input_grad[1] else None
        return (None, g_feat, None, g_normal) + tuple(grads)
