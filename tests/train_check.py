"""One whole training step on the GPU against the oracle's autograd (shared by tests/test_gpu_train.py and
tests/test_gpu_config_matrix.py): Renderer_TensoIR_train with is_train=True fed the oracle's random draws, the loss of
train_tensoIR.py, its backward, and every parameter gradient that is non-zero in the oracle.

Gradient tolerance: max |hip - ref| / max |ref| per tensor < GTOL = 2e-3 (fp32 atomics reorder the sums; the reference's own
CUDA grid_sampler backward has the same property), the loss 1e-5, forward maps the 1e-4 bar."""
import numpy as np
import torch

GTOL = 2e-3


def gerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-20))


def _golden_batch(env):
    """The batch of tests/golden/train_grads.npz: its rays, light indices and targets, draws under seed 21."""
    T = lambda g, k: torch.from_numpy(np.array(g[k]))
    rays, lidx = T(env.g, "rays/rays"), T(env.g, "rays/light_idx")
    S = int(env.tg["train/n_samples"][0])
    gen = torch.Generator().manual_seed(21)
    jitter = torch.rand(rays.shape[0], 1, generator=gen)
    noise = torch.randn(rays.shape[0], S, 3, generator=gen)
    return dict(rays=rays, lidx=lidx, gt=T(env.tg, "train/rgb_gt"), S=S, jitter=jitter, noise=noise)


def _hip_step(env, m, b, relight, normal_gt=None, idx=None):
    """The product's training forward on the batch (or its rays `idx`) fed the batch's draws -> (ret, loss); the caller calls
    loss.backward().  forward() takes the ray jitter from torch.rand(B, 1) on the CPU generator and the BRDF noise from
    _brdf_jitter_dense."""
    from tensoir_amd import Renderer_TensoIR_train
    sel = (lambda t: t) if idx is None else (lambda t: t[idx].contiguous())
    rays, lidx, gt, jitter, noise = (sel(b[k]) for k in ("rays", "lidx", "gt", "jitter", "noise"))
    ngt = None if normal_gt is None else sel(normal_gt)
    B = rays.shape[0]
    state = torch.get_rng_state()
    torch.manual_seed(0)
    orig_rand = torch.rand

    def fake_rand(*a, **k):
        if tuple(a) == (B, 1) or (len(a) == 1 and tuple(a[0]) == (B, 1)):
            return jitter.clone()
        return orig_rand(*a, **k)
    torch.rand = fake_rand
    try:
        orig_fwd = type(m).forward

        def fwd(self, r, l, **k):
            return orig_fwd(self, r, l, _brdf_jitter_dense=noise, **k)
        type(m).forward = fwd
        try:
            ret = Renderer_TensoIR_train(rays, ngt, lidx, m, N_samples=b["S"], white_bg=True, is_train=True,
                                         is_relight=relight, sample_method="fixed_envirmap", device="cuda",
                                         args=env.args)
        finally:
            type(m).forward = orig_fwd
    finally:
        torch.rand = orig_rand
        torch.set_rng_state(state)
    return ret, env.O.training_loss(ret, gt.cuda(), relight)


def _oracle_step(env, sc, b, relight, normal_gt=None, idx=None):
    sel = (lambda t: t) if idx is None else (lambda t: t[idx].contiguous())
    return env.O.train_step_grads(sc, sel(b["rays"]), sel(b["lidx"]), sel(b["gt"]), is_relight=relight, n_samples=b["S"],
                                  ray_jitter=sel(b["jitter"]), brdf_jitter=sel(b["noise"]),
                                  second_n_sample=env.args.second_nSample, second_near=env.args.second_near,
                                  second_far=env.args.second_far, normal_gt=None if normal_gt is None else sel(normal_gt))


def _all_but_one_ray(env, m, sc, b, relight, gtol, report):
    """DESIGN 5, the rule of the bench's gradient gate, unchanged: after a strict miss the rays are bisected (the loss is a mean
    over rays, so a deviation is a sum of per-ray deviations; benchlib.train.single_ray_bisect) down to ONE ray -- a ReLU mask
    that differs on one of its records -- and ALL THE OTHER rays together must keep the strict bound on every tensor; the
    excluded ray's own deviation is bounded too (beyond 2x its gradient is not that mechanism)."""
    from benchlib.train import grad_deviation, single_ray_bisect

    def grads_of(idx):
        m.zero_grad(set_to_none=True)
        _, loss = _hip_step(env, m, b, relight, idx=idx)
        loss.backward()
        gh = {n: p.grad.detach().cpu() for n, p in m.named_parameters() if p.grad is not None}
        m.zero_grad(set_to_none=True)
        return gh, _oracle_step(env, sc, b, relight, idx=idx)[1]

    n = b["rays"].shape[0]
    ray, alone, _ = single_ray_bisect(n, lambda idx: grad_deviation(*grads_of(idx)))
    rest = torch.arange(n)[torch.arange(n) != ray]
    gh, gr = grads_of(rest)
    worst = {k: gerr(gh[k], v) for k, v in gr.items() if k in gh and float(v.abs().max()) != 0.0}
    if report is not None:
        report["single_ray"] = {"ray": ray, "alone": alone, "rest": dict(worst)}
    bad = {k: round(v, 5) for k, v in worst.items() if v > gtol}
    assert not bad, ("all rays but", ray, bad)
    assert alone is not None and alone["dense"] < 2.0 and alone["l2"] < 2.0, (ray, alone)


def check_training_step(env, m, sc, relight, t_stop, min_checked, normal_gt=None, batch=None, report=None, gtol=GTOL,
                        single_ray=False):
    """env: O (the oracle module), args (second_* settings) and -- without `batch` -- g / tg (the golden batch).
    batch: dict(rays, lidx, gt, S, jitter [B,1], noise [B,S,3]).  min_checked: how many parameters must have been compared;
    None takes the count of the oracle's own non-zero gradients.  gtol: the gradient bound (GTOL).  single_ray: on a strict
    miss of the gradients apply the all-rays-but-one rule (_all_but_one_ray) instead of failing at once.  report: a dict that
    receives every measured figure (filled before the assertions)."""
    b = _golden_batch(env) if batch is None else batch
    loss_ref, grads_ref, ret_ref = _oracle_step(env, sc, b, relight, normal_gt)
    if min_checked is None:
        min_checked = sum(1 for name, _ in m.named_parameters() if float(grads_ref[name].abs().max()) != 0.0)
        assert min_checked >= (18 if not relight else 25), min_checked
    m.zero_grad(set_to_none=True)
    m.march_t_stop = t_stop          # 1e-6 = the product default: rays stop marching once T < 1e-6 (gradients there are < 1e-6)
    ret, loss = _hip_step(env, m, b, relight, normal_gt)
    maps = ("rgb_map", "acc_map", "depth_map") + (("rgb_with_brdf_map", "normal_map", "albedo_map", "normals_diff_map",
                                                   "normals_orientation_loss_map") if relight else ())
    if report is not None:
        report["loss"] = abs(float(loss.detach()) - float(loss_ref.detach()))
        report["maps"] = {k: float((ret[k].detach().cpu() - ret_ref[k]).abs().max()) for k in maps}
    assert abs(float(loss.detach()) - float(loss_ref.detach())) < 1e-5
    for k in maps:
        assert float((ret[k].detach().cpu() - ret_ref[k]).abs().max()) < 1e-4, k
    loss.backward()
    worst = {}
    try:
        for name, p in m.named_parameters():
            ref = grads_ref[name]
            if float(ref.abs().max()) == 0.0:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
                continue
            assert p.grad is not None, name
            worst[name] = gerr(p.grad, ref)
        if report is not None:
            report["grads"] = dict(worst)
        assert len(worst) >= min_checked
        bad = {k: round(v, 5) for k, v in worst.items() if v > gtol}
        if bad and single_ray and normal_gt is None:
            _all_but_one_ray(env, m, sc, b, relight, gtol, report)
        else:
            assert not bad, (bad, {k: round(v, 6) for k, v in worst.items() if k.startswith("density") or k.startswith("app")})
    finally:
        m.zero_grad(set_to_none=True)
        m.march_t_stop = 0.0
