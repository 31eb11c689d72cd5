"""The total-variation regulariser of the VM planes on the GPU: one launch forward and one launch backward for a whole list of
planes (kernels tir_tv_fwd / tir_tv_bwd, include/tensoir_hip.h).

    tvreg = regularisers.TVLoss()                    # the reference's utils.TVLoss: same constructor, same attribute
    loss = tvreg(plane)                              # [1, C, H, W] float32 on the GPU: the kernels; anything else: PyTorch
    loss = regularisers.tv_planes(planes, coefs)     # sum_p coefs[p] * TV(planes[p]), the whole list in one launch

The training scripts add TV_loss_density(tvreg) and TV_loss_app(tvreg) to the loss in every iteration up to the first alpha-mask
update (train_tensoIR.py:276-285); written plane by plane in PyTorch the two terms and their backward are 222
device kernels per iteration; here they are 10, of which four are these kernels and six the scalar weighting around them.
TensorVMSplit.TV_loss_density / TV_loss_app call tv_planes when they are handed a TVLoss of this module; tensoir_amd.run rebinds the
scripts' utils.TVLoss to it.  TENSOIR_TORCH_TV=1 switches all of it back to PyTorch.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import ops


def torch_tv_enabled():
    """TENSOIR_TORCH_TV=1: every TV term is evaluated by PyTorch (read at call time)."""
    return os.environ.get("TENSOIR_TORCH_TV", "0") == "1"


def on_kernel_path(x):
    """Whether x is a plane the kernels take: a float32 [1, C, H, W] tensor on the GPU with H, W >= 2 (and C >= 1)."""
    return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] == 1 and x.shape[1] >= 1
            and x.shape[2] >= 2 and x.shape[3] >= 2)


def tv_torch(x, weight=1):
    """The plain PyTorch expression: weight * 2 * (mean squared forward difference along H + that along W) / batch, the means over
    C (H - 1) W and C H (W - 1) elements.  A unit H or W divides by a zero count, as the reference does (utils.py:148-159)."""
    n, c, h, w = x.shape
    count_h, count_w = c * (h - 1) * w, c * h * (w - 1)
    sq_h = torch.pow(x[:, :, 1:, :] - x[:, :, :h - 1, :], 2).sum()
    sq_w = torch.pow(x[:, :, :, 1:] - x[:, :, :, :w - 1], 2).sum()
    return weight * 2 * (sq_h / count_h + sq_w / count_w) / n


def _packed(x):
    """x as the kernels read it: itself when it is stored channel-last, else a channel-last copy."""
    x = x.detach()
    return x if ops.is_channel_last(x) else x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


class _TvPlanesFn(torch.autograd.Function):
    """loss = sum_p coefs[p] * TV(planes[p]): tir_tv_fwd, and tir_tv_bwd for the planes whose gradient is needed."""

    @staticmethod
    def forward(ctx, coefs, *planes):
        packed = [_packed(p) for p in planes]
        loss, _ = ops.tv_forward(packed, coefs)
        ctx.coefs = coefs
        ctx.save_for_backward(*packed)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        grads = ops.tv_backward(ctx.saved_tensors, ctx.coefs, g, needs=ctx.needs_input_grad[1:])
        return (None, *grads)


def tv_planes(planes, coefs):
    """sum_p coefs[p] * TV(planes[p]) for a list of at most ops.TV_MAX_PLANES float32 [1, C, H, W] GPU tensors (H, W >= 2) and one
    host float per plane: a 0-dim float32 on the device, differentiable in the planes.  One launch forward, one backward; a
    channel-last plane (every VM parameter) is read in place and its gradient comes back channel-last."""
    planes = list(planes)
    for i, p in enumerate(planes):
        if not on_kernel_path(p):
            raise ValueError(f"tv_planes: plane {i} must be a float32 [1, C, H >= 2, W >= 2] tensor on the GPU")
    return _TvPlanesFn.apply(tuple(float(c) for c in coefs), *planes)


class TVLoss(nn.Module):
    """The reference's utils.TVLoss.  A float32 [1, C, H, W] GPU tensor with H, W >= 2 goes through the kernels; every other input
    (host tensors, other dtypes, a batch, a unit dimension) and every input under TENSOIR_TORCH_TV=1 through tv_torch -- there the
    behaviour is the reference's own."""

    def __init__(self, TVLoss_weight=1):
        super().__init__()
        self.TVLoss_weight = TVLoss_weight

    def forward(self, x):
        if on_kernel_path(x) and not torch_tv_enabled():
            return tv_planes([x], [self.TVLoss_weight])
        return tv_torch(x, self.TVLoss_weight)


def model_tv(planes, reg):
    """TensorVMSplit.TV_loss_density / TV_loss_app: sum over the planes of reg(plane) * 1e-2.  A TVLoss of this module on GPU planes
    is one launch (coef = TVLoss_weight * 1e-2); any other callable is called plane by plane, as the reference does."""
    planes = list(planes)
    if isinstance(reg, TVLoss) and not torch_tv_enabled() and 0 < len(planes) <= ops.TV_MAX_PLANES and all(on_kernel_path(p) for p in planes):
        return tv_planes(planes, [float(reg.TVLoss_weight) * 1e-2] * len(planes))
    return sum((reg(plane) * 1e-2 for plane in planes), 0)
