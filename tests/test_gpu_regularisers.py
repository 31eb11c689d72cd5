"""tir_tv_fwd / tir_tv_bwd on the GPU against the float64 restatement (tests/regulariser_reference.py): values, gradients, layouts,
determinism, and the model methods with an optimiser step.  Every bound is derived (stated where it is used), none is measured."""
import json
import os

import numpy as np
import pytest
import torch

from tests import regulariser_reference as RR
from tests.helpers import golden_checkpoint, regulariser_trace, tv_loss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_UP = 0.037                                                       # the upstream gradient of the backward tests (a device scalar)
CALLS = [[s] for s in RR.SINGLE_SHAPES] + [RR.GRID_SHAPES]
IDS = ["x".join(map(str, c[0])) if len(c) == 1 else "grid-20-22-24" for c in CALLS]


def coefs_of(n):
    return [0.01 * (1.0 + 0.7 * i) for i in range(n)]              # unequal per plane


@pytest.fixture(scope="module")
def cases():
    """call id -> (host planes, coefs, float64 sums, float64 loss, float64 gradients for G_UP), computed once and left unchanged"""
    out = {}
    for name, shapes in zip(IDS, CALLS):
        planes, coefs = [RR.plane(s) for s in shapes], coefs_of(len(shapes))
        out[name] = (planes, coefs, [RR.sums(x) for x in planes], RR.loss(planes, coefs),
                     [RR.gradient(x, k, G_UP) for x, k in zip(planes, coefs)])
    return out


def dev(planes):
    """device copies in the same storage order"""
    return [p.cuda() for p in planes]


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_forward_against_float64(cases, name):
    """Relative 1e-6: every term carries three fp32 roundings (the difference, the square -- its relative error doubles the
    difference's -- : <= 3 * 2^-24 = 1.8e-7 relative) and all terms are non-negative, so the sums carry the same; the double sums
    add nothing visible; the loss's final rounding adds 6e-8."""
    from tensoir_amd import ops
    planes, coefs, want_sums, want_loss, _ = cases[name]
    xs = dev(planes)
    assert all(ops.is_channel_last(x) for x in xs)
    loss, sums = ops.tv_forward(xs, coefs)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and sums.dtype == torch.float64 and tuple(sums.shape) == (len(xs), 2)
    got = sums.cpu().numpy()
    print(f"\n[tv fwd {name}] loss {float(loss):.9e} (float64 {want_loss:.9e}), sums rel err "
          f"{max(abs(got[p][k] - want_sums[p][k]) / want_sums[p][k] for p in range(len(xs)) for k in range(2)):.2e}")
    for p in range(len(xs)):
        for k in range(2):
            assert abs(got[p][k] - want_sums[p][k]) <= 1e-6 * want_sums[p][k], (p, k)
    assert abs(float(loss) - want_loss) <= 1e-6 * want_loss


# ---- backward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_backward_against_float64(cases, name):
    """Elementwise, to RR.gradient_tolerance (32 * 2^-24 * 4 |g coef| (1 / nh + 1 / nw) * 4 max|x|: the magnitude bound of the bracket
    times a few fp32 roundings, with slack).  g is a non-unit device scalar; the coefficients differ per plane."""
    from tensoir_amd import ops
    planes, coefs, _, _, want = cases[name]
    xs = dev(planes)
    g = torch.tensor(G_UP, dtype=torch.float32, device="cuda")
    grads = ops.tv_backward(xs, coefs, g)
    for p, (x, k) in enumerate(zip(planes, coefs)):
        assert ops.is_channel_last(grads[p]) and grads[p].shape == x.shape
        err, tol = float(np.abs(grads[p].cpu().double().numpy() - want[p]).max()), RR.gradient_tolerance(x, k, G_UP)
        print(f"\n[tv bwd {name} plane {p}] max err {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (p, err, tol)


def test_backward_leaves_an_unwanted_plane_unwritten(cases):
    from tensoir_amd import ops
    planes, coefs, _, _, want = cases["grid-20-22-24"]
    xs = dev(planes)
    g = torch.tensor(G_UP, dtype=torch.float32, device="cuda")
    sentinel = -7.25
    outs = [torch.full_like(x, sentinel) for x in xs]
    assert all(ops.is_channel_last(o) for o in outs)
    back = ops.tv_backward(xs, coefs, g, out=[outs[0], None, outs[2]])
    assert back[1] is None and bool((outs[1] == sentinel).all())
    for p in (0, 2):
        assert float(np.abs(outs[p].cpu().double().numpy() - want[p]).max()) <= RR.gradient_tolerance(planes[p], coefs[p], G_UP)
        assert not bool((outs[p] == sentinel).any())              # every element written
    # through autograd: a plane that needs no gradient gets none, the others the same values
    ys = [x.clone().requires_grad_(p != 1) for p, x in enumerate(xs)]
    from tensoir_amd import regularisers
    (regularisers.tv_planes(ys, coefs) * G_UP).backward()
    assert ys[1].grad is None and torch.equal(ys[0].grad, outs[0]) and torch.equal(ys[2].grad, outs[2])


@pytest.mark.parametrize("shape", [(48, 37, 41), (5, 7, 6)])
def test_layouts_through_the_module(shape):
    """A channel-last input gives a channel-last gradient; an NCHW-contiguous input gives the same values."""
    from tensoir_amd import ops, regularisers
    reg = regularisers.TVLoss(0.5)
    a = RR.plane(shape).cuda().requires_grad_(True)
    b = RR.plane(shape, channel_last=False).cuda().requires_grad_(True)
    assert ops.is_channel_last(a) and not ops.is_channel_last(b) and b.is_contiguous() and torch.equal(a.detach(), b.detach())
    la, lb = reg(a), reg(b)
    (la * G_UP).backward()
    (lb * G_UP).backward()
    assert torch.equal(la, lb) and ops.is_channel_last(a.grad) and b.grad.shape == b.shape and torch.equal(a.grad, b.grad)
    want, tol = RR.gradient(a, 0.5, G_UP), RR.gradient_tolerance(a, 0.5, G_UP)
    assert float(np.abs(a.grad.cpu().double().numpy() - want).max()) <= tol
    assert abs(float(la.detach()) - RR.loss([a], [0.5])) <= 1e-6 * RR.loss([a], [0.5])
    # the switch: the same module on the same tensor evaluates the PyTorch expression (fp32 sums: a looser, still derived, bound --
    # n terms added in fp32 in some order are within n * 2^-24 relative of the exact sum of non-negative terms)
    os.environ["TENSOIR_TORCH_TV"] = "1"
    try:
        lt = reg(a.detach())
    finally:
        del os.environ["TENSOIR_TORCH_TV"]
    assert abs(float(lt) - float(la.detach())) <= a.numel() * 2.0 ** -24 * float(la.detach())


def test_planes_are_read_in_place(cases):
    """A channel-last plane is its own packed form: neither entry point copies it.  Counted on the caching allocator's cumulative
    figures: tv_forward requests its three small outputs (workspace, sums, loss) and nothing the size of a plane, tv_backward into
    given outputs requests nothing at all, and through autograd the only plane-sized requests are the gradients themselves."""
    from tensoir_amd import ops, regularisers
    planes, coefs = cases["48x150x150"][0] + cases["grid-20-22-24"][0], [0.01, 0.02, 0.03, 0.04]
    xs = dev(planes)
    outs = [torch.empty_like(x) for x in xs]
    g = torch.tensor(G_UP, dtype=torch.float32, device="cuda")
    smallest = min(x.numel() for x in xs) * 4

    def requested(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()
        fn()
        torch.cuda.synchronize()
        after = torch.cuda.memory_stats()
        return tuple(after[k] - before[k] for k in ("allocation.all.allocated", "allocated_bytes.all.allocated"))

    ops.tv_forward(xs, coefs)                                      # (first use of the library in the process)
    n, nbytes = requested(lambda: ops.tv_forward(xs, coefs))
    assert n == 3 and nbytes < smallest, (n, nbytes)
    n, nbytes = requested(lambda: ops.tv_backward(xs, coefs, g, out=outs))
    assert (n, nbytes) == (0, 0), (n, nbytes)
    ys = [x.clone().requires_grad_(True) for x in xs]
    loss = regularisers.tv_planes(ys, coefs)
    n, nbytes = requested(lambda: loss.backward())
    grads = sum(x.numel() for x in xs) * 4
    assert nbytes < grads + smallest, (n, nbytes, grads)            # the four gradients, the seed of backward(), nothing plane-sized more


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits_together_and_alone(cases):
    """Eight planes in one call (the most a launch takes: every wave of the tail adds two planes), among them one whose forward
    shares exceed TIR_TV_SHARE: identical bits from call to call, and every plane's sums and gradient equal those of a call of its
    own.  The eight-plane loss is checked against float64 like the others (relative 1e-6, test_forward_against_float64)."""
    from tensoir_amd import ops
    names = ["grid-20-22-24", "48x37x41", "48x150x150", "16x2x2", "48x3x2", "5x7x6"]
    planes = [x for n in names for x in cases[n][0]]
    ks = [0.01 * (1.0 + 0.3 * i) for i in range(len(planes))]
    assert len(planes) == ops.TV_MAX_PLANES
    xs = dev(planes)
    g = torch.tensor(G_UP, dtype=torch.float32, device="cuda")
    l0, s0 = ops.tv_forward(xs, ks)
    l1, s1 = ops.tv_forward(xs, ks)
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    want = RR.loss(planes, ks)
    assert abs(float(l0) - want) <= 1e-6 * want
    g0, g1 = ops.tv_backward(xs, ks, g), ops.tv_backward(xs, ks, g)
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    for p, (x, k) in enumerate(zip(xs, ks)):
        la, sa = ops.tv_forward([x], [k])
        lb, sb = ops.tv_forward([x], [k])
        assert torch.equal(la, lb) and torch.equal(sa, sb)
        assert torch.equal(sa[0], s0[p])                           # a plane's sums do not depend on what else is in the call
        ga, gb = ops.tv_backward([x], [k], g), ops.tv_backward([x], [k], g)
        assert torch.equal(ga[0], gb[0]) and torch.equal(ga[0], g0[p])
    with pytest.raises(ValueError):
        ops.tv_forward(xs + xs[:1], ks + ks[:1])                   # nine planes


# ---- through the model ------------------------------------------------------------------------------------------------------------
def build_model(golden):
    import tensoir_amd
    eh, ew = [int(v) for v in golden["scene/envmap_hw"]]
    return tensoir_amd.model_from_checkpoint(golden_checkpoint(golden), "cuda", envmap_h=eh, envmap_w=ew)


@pytest.fixture(scope="module")
def model(golden):
    return build_model(golden)


def test_model_methods_stay_on_the_recorded_reference_values(model):
    from tensoir_amd import regularisers
    got = regulariser_trace(model, regularisers.TVLoss())
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "host_reference.json")))["regularisers"]
    for name in ("TV_loss_density", "TV_loss_app"):
        a = want["values"][name]
        print(f"\n[tv model {name}] {got['values'][name]:.9e} (recorded {a:.9e})")
        assert abs(a - got["values"][name]) <= 1e-6 * max(1.0, abs(a)), name


def _regularised_loss(m, reg):
    return m.TV_loss_density(reg) * 0.05 + m.TV_loss_app(reg) * 0.005 + m.density_L1() * 8e-5


def test_model_gradients_and_one_adam_step(model, golden):
    """The loss of a radiance-phase iteration without its image term.  Gradients: each plane within the backward tolerance (g = the
    TV weight, coef = 1e-2) of float64 autograd on the restated expression; the lines get only the L1 term.
    The Adam step (first step, lr, eps = 1e-8): p' = p - lr f(g), f(g) = g / (|g| + eps) after bias correction, and
    |f'(g)| = eps / (|g| + eps)^2 <= 1 / eps, so two steps from gradients that differ by d differ by at most lr d / eps.  Both sides'
    TV gradients lie within the backward tolerance T of the exact one (the eager side is an fp32 evaluation of the same stencil), and
    each side adds the identical L1 term to it in fp32 (one rounding of the total, 2^-24 |g|): d <= 2 T + 2 * 2^-24 |g|.  The
    step's own fp32 arithmetic is the same kernel on both sides; its input-independent roundings (the moments, the quotient, the
    final subtraction) move the result by a few ulps of max(|p|, lr): 8 * 2^-24 max(|p|, lr) covers them."""
    from tensoir_amd import optim, regularisers
    lr, eps = 0.02, 1e-8
    fused, eager = build_model(golden), build_model(golden)
    results = {}
    for name, m, reg in (("fused", fused, regularisers.TVLoss()), ("eager", eager, tv_loss)):
        m.zero_grad(set_to_none=True)
        _regularised_loss(m, reg).backward()
        results[name] = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    planes = [f"{kind}_plane.{i}" for kind in ("density", "app") for i in range(3)]
    lines = [f"density_line.{i}" for i in range(3)]
    assert sorted(results["fused"]) == sorted(planes + lines) == sorted(results["eager"])
    named = dict(model.named_parameters())
    tols = {}
    for k in planes:
        x = named[k].detach().cpu().double().requires_grad_(True)
        w = 0.05 if k.startswith("density") else 0.005
        ref = w * 1e-2 * RR_tv64(x)
        if k.startswith("density"):
            ref = ref + 8e-5 * x.abs().mean()
        ref.backward()
        tols[k] = RR.gradient_tolerance(named[k], 1e-2, w)
        err = float((results["fused"][k].cpu().double() - x.grad).abs().max())
        print(f"\n[tv model grad {k}] max err {err:.3e} (bound {tols[k]:.3e})")
        # the density planes' .grad also carries the L1 term, added in fp32: one more rounding of the total
        assert err <= tols[k] + (2.0 ** -24 * float(x.grad.abs().max()) if k.startswith("density") else 0.0), k
    for k in lines:
        assert torch.equal(results["fused"][k], results["eager"][k]), k            # only the L1 term: the same code on both sides
    for m in (fused, eager):
        optim.Adam(m.get_optparam_groups(lr, 1e-3), betas=(0.9, 0.99), eps=eps).step()
    after_f, after_e = dict(fused.named_parameters()), dict(eager.named_parameters())
    for k in planes:
        d = 2 * tols[k] + 2 * 2.0 ** -24 * results["eager"][k].abs()
        bound = lr * d / eps + 8 * 2.0 ** -24 * torch.clamp(named[k].detach().abs(), min=lr)
        diff = (after_f[k].detach() - after_e[k].detach()).abs()
        print(f"\n[tv adam {k}] max diff {float(diff.max()):.3e} (largest bound {float(bound.max()):.3e})")
        assert bool((diff <= bound).all()), k
        assert not torch.equal(after_f[k].detach(), named[k].detach())           # the step moved the plane
    for k in lines:
        assert torch.equal(after_f[k].detach(), after_e[k].detach()), k


def RR_tv64(x):
    """the restated expression in torch float64 (for autograd): 2 (Sh / nh + Sw / nw)"""
    nh, nw = RR.counts(x)
    return 2 * ((x[:, :, 1:, :] - x[:, :, :-1, :]).pow(2).sum() / nh + (x[:, :, :, 1:] - x[:, :, :, :-1]).pow(2).sum() / nw)
