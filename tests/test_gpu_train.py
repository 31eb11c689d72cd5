"""Training path on the GPU: every backward kernel (through the C ABI) against the CPU oracle's autograd,
which tests/test_oracle_train.py pins to the imported reference's own backward (tests/golden/train_grads.npz).

Gradient tolerance: max |hip - ref| / max |ref| per tensor < 2e-3 (fp32 atomics reorder the sums; the
reference's own CUDA grid_sampler backward has the same property), forward maps keep the 1e-4 bar."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.train_check import GTOL, gerr
from tests.train_check import check_training_step as _check_training_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env(golden):
    import tensoir_amd
    from oracle import tensoir_oracle as O
    from tests.helpers import golden_checkpoint, scene_from_checkpoint
    assert torch.cuda.is_available()
    from tensoir_amd import _lib
    assert _lib.lib().tir_device_check() == 0
    ckpt = golden_checkpoint(golden)
    eh, ew = [int(x) for x in golden["scene/envmap_hw"]]
    model = tensoir_amd.model_from_checkpoint(ckpt, "cuda", envmap_h=eh, envmap_w=ew)
    model.march_t_stop = 0.0
    sc = scene_from_checkpoint(ckpt, eh, ew)
    tg = np.load(os.path.join(ROOT, "tests", "golden", "train_grads.npz"))
    return types.SimpleNamespace(model=model, sc=sc, g=golden, tg=tg, O=O, dev="cuda",
                                 args=types.SimpleNamespace(second_nSample=24, second_near=0.05, second_far=1.5))


def T(g, k):
    return torch.from_numpy(np.array(g[k]))


# ------------------------------------------------------------------ building blocks
@pytest.mark.parametrize("impl,tol", [("mfma", 1e-5), ("bf16x3", 3e-5)])
def test_gemm_tn(env, impl, tol):
    """Weight-gradient product C += A^T B: exact fp32 MFMA, and the split-bf16 (3-product) version whose error per
    product is ~2^-16 (the tolerance is relative to max |C|)."""
    from tensoir_amd import ops
    gen = torch.Generator().manual_seed(3)
    for n, M, N, lda, ldb, ones in ((1000, 128, 150, 128, 160, True), (777, 27, 144, 32, 144, False),
                                    (5, 4, 128, 4, 128, True), (70000, 128, 128, 128, 128, True),
                                    (33, 100, 7, 100, 8, True), (4097, 128, 150, 132, 152, False),
                                    (1000, 27, 288, 32, 288, True), (777, 27, 290, 32, 296, False)):      # wider than one launch
        A = torch.randn(n, lda, generator=gen)
        B = torch.randn(n, ldb, generator=gen)
        A[:, M:] = float("nan")                 # row padding must never leak into C
        B[:, N:] = float("nan")
        C = torch.zeros(M, N + (1 if ones else 0) + 3).cuda()
        ops.gemm_tn(A.cuda(), M, B.cuda(), N, C, ones, impl=impl)
        ref = A[:, :M].double().T @ B[:, :N].double()
        assert gerr(C[:, :N], ref) < tol, (n, M, N)
        if ones:
            assert gerr(C[:, N], A[:, :M].double().sum(0)) < tol
            # the same with the bias column kept apart: C is the exact [M, N] weight gradient
            Cw, cb = torch.zeros(M, N).cuda(), torch.zeros(M).cuda()
            ops.gemm_tn(A.cuda(), M, B.cuda(), N, Cw, True, impl=impl, bias_out=cb)
            assert gerr(Cw, ref) < tol and gerr(cb, A[:, :M].double().sum(0)) < tol, (n, M, N)
        assert float(C[:, N + (1 if ones else 0):].abs().max()) == 0.0


def _torch_decoder(w, feat, aux, act):
    O_ = __import__("oracle.tensoir_oracle", fromlist=["x"])
    x = O_.mlp_input(feat, aux, 2, 2)
    y = O_.mlp3(w, x)
    return torch.tanh(y) if act == 1 else torch.sigmoid(y)


@pytest.mark.parametrize("which", ["rgb", "brdf", "normal"])
def test_decoder_backward(env, which):
    from tensoir_amd import ops, training
    m, sc = env.model, env.sc
    dec, w, act = {"rgb": (m.renderModule, sc.mlp_rgb, 0), "brdf": (m.renderModule_brdf, sc.mlp_brdf, 0),
                   "normal": (m.renderModule_normal, sc.mlp_normal, 1)}[which]
    gen = torch.Generator().manual_seed(7)
    n = 700
    feat = torch.randn(n, 27, generator=gen) * 0.7
    aux = torch.randn(n, 3, generator=gen)
    od = w["w2"].shape[0]
    g_out = torch.randn(n, od, generator=gen)
    wr = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    fr = feat.clone().requires_grad_(True)
    y = _torch_decoder(wr, fr, aux, act)
    (y * g_out).sum().backward()
    fpad = torch.zeros(n, 32)
    fpad[:, :27] = feat
    for impl in ("mfma", "bf16x3"):      # forward with saved activations: exact fp32 and split-bf16 matrix cores
        call = training._DecoderCall(feat=fpad.cuda(), aux=aux.cuda(), aux_map=None, g_out=g_out.cuda())
        call.out, call.h1, call.h2 = ops.mlp_train(dec.packed(), call.feat, call.aux, impl=impl)
        assert gerr(call.out, y) < 2e-5, impl
        (g_feat,), grads = training._decoder_backward(dec, [call], impl=impl)     # exact fp32 / all split-bf16
        if impl == "mfma":
            assert gerr(g_feat[:, :27], fr.grad) < 1e-4, impl
        else:
            # the split-bf16 forward rounds pre-activations differently (~1e-6): a hidden unit sitting within that of
            # zero flips its ReLU mask, which changes ONE sample's gradient by a few percent (the backward is exact for
            # the forward that was run).  Everything else agrees to 1e-4.
            d = (g_feat[:, :27].cpu().double() - fr.grad.double()).abs().amax(-1) / fr.grad.double().abs().max()
            assert float((d > 1e-4).double().mean()) < 5e-3 and float(d.max()) < 0.2, impl
        assert float(g_feat[:, 27:].abs().max()) == 0.0
        for got, name in zip(grads, ("w0", "b0", "w1", "b1", "w2", "b2")):
            if impl == "mfma":
                assert gerr(got, wr[name].grad) < 1e-4, (impl, name)
            else:      # a flipped unit moves one row of the 700-sample weight gradient by ~1 %; the bulk agrees to 1e-4
                ref = wr[name].grad.double()
                d = (got.detach().cpu().double() - ref).abs() / ref.abs().max()
                assert float(d.max()) < 5e-2 and float((d > 1e-4).double().mean()) < 2e-2, (impl, name, float(d.max()))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 70001])
def test_small_gemm_tn(env, n):
    """tir_gemm_tn_small_bf16x3: C[27, 144] += sum_j A_j^T B_j (the basis-matrix gradient of several gathers in one launch)
    against fp64; padded A rows carry NaN beyond column M, ragged row counts, 1-3 operand pairs, other shapes."""
    from tensoir_amd import ops
    gen = torch.Generator().manual_seed(200 + n)
    # N = 48 / 72: the basis-matrix gradient of 16 / 24 appearance components per plane (k_gemm_tn_small<2> / <3>)
    for M, N, lda, ldb, k in ((27, 144, 32, 144, 3), (27, 144, 32, 144, 1), (4, 30, 4, 40, 2), (32, 160, 32, 160, 2),
                              (27, 48, 32, 48, 3), (27, 72, 32, 72, 3), (27, 72, 32, 72, 1)):
        ref = torch.zeros(M, N, dtype=torch.float64)
        pairs = []
        for _ in range(k):
            A = torch.randn(n, lda, generator=gen)
            B = torch.randn(n, ldb, generator=gen)
            ref += A[:, :M].double().T @ B[:, :N].double()
            A[:, M:] = float("nan")
            B[:, N:] = float("nan")
            pairs.append((A.cuda(), B.cuda()))
        C0 = torch.randn(M, N + 3, generator=gen)
        Cd = C0.cuda()
        ops.gemm_tn_small(pairs, M, N, Cd)
        assert torch.isfinite(Cd).all()
        assert gerr(Cd[:, :N].cpu().double() - C0[:, :N].double(), ref) < 3e-5, (n, M, N, k)
        assert torch.equal(Cd[:, N:].cpu(), C0[:, N:])


@pytest.mark.parametrize("stride", [32, 29, -32])        # 32: the LDS-staged kernel; 29 (rows not float4-addressable) and
                                                           # -32 (stride 32, base pointer off by one float): direct loads
@pytest.mark.parametrize("n", [1, 15, 16, 17, 700, 4099, 70001])
def test_fused_weight_gradients(env, n, stride):
    """tir_mlp_wgrad_multi: dW0 = dz1^T x, dW1 = dz2^T h1, dW2 = dz3^T h2 and the three bias gradients of several decoder
    invocations in one launch, x rebuilt in registers from feat + aux (no tir_mlp_inputs buffer, no per-layer GEMM):
    against fp64 products with the oracle's input rows (models/tensorBase_rotated_lights.py:137-142, :12-17).  Ragged row
    counts (tails of 16-row steps, fewer steps than workgroups), an aux index map, two jobs accumulating into the same
    outputs (the BRDF decoder's two invocations), NaN poison in the feature padding."""
    from tensoir_amd import ops
    O = env.O
    gen = torch.Generator().manual_seed(100 + n)
    jobs, refs = [], []
    outs = [[torch.zeros(128, 150), torch.zeros(128), torch.zeros(128, 128), torch.zeros(128), torch.zeros(4, 128), torch.zeros(4)]
            for _ in range(2)]
    dev_outs = [[t.cuda() for t in o] for o in outs]
    R = max(3, n // 5)                                    # rows of the aux table of the mapped job (rays)
    for ji, (oi, mapped) in enumerate(((0, True), (1, False), (1, False))):
        dz1, dz2 = torch.randn(n, 128, generator=gen), torch.randn(n, 128, generator=gen)
        dz3 = torch.randn(n, 4, generator=gen)
        if ji == 0:
            dz3[:, 3] = 0.0                               # a 3-output decoder: the 4th cotangent column is zero
        h1, h2 = torch.relu(torch.randn(n, 128, generator=gen)), torch.relu(torch.randn(n, 128, generator=gen))
        feat = torch.randn(n, 27, generator=gen) * 1.5
        misaligned, stride_ = stride < 0, abs(stride)
        fpad = torch.full((n, stride_), float("nan"))     # the padding columns must never be read into a product
        fpad[:, :27] = feat
        fpad[:, 27] = 0.0                                 # (column 27 is the forward's zero pad)
        if mapped:
            table = torch.randn(R, 3, generator=gen)
            amap = torch.randint(0, R, (n,), generator=gen).int()
            aux_rows = table[amap.long()]
            aux_dev, map_dev = table.cuda(), amap.cuda()
        else:
            aux_rows = torch.randn(n, 3, generator=gen)
            aux_dev, map_dev = aux_rows.cuda(), None
        x = O.mlp_input(feat.double(), aux_rows.double(), 2, 2)
        refs.append((oi, dz1.double().T @ x, dz1.double().sum(0), dz2.double().T @ h1.double(), dz2.double().sum(0),
                     dz3.double().T @ h2.double(), dz3.double().sum(0)))
        fdev = fpad.cuda()
        if misaligned:                                    # the same rows one float into a larger allocation
            hold = torch.empty(fdev.numel() + 1, device="cuda")
            hold[1:] = fdev.reshape(-1)
            fdev = hold[1:].view(n, stride_)
            assert fdev.data_ptr() % 16 == 4
        jobs.append((dz1.cuda(), dz2.cuda(), dz3.cuda(), h1.cuda(), h2.cuda(), fdev, aux_dev, map_dev) + tuple(dev_outs[oi]))
    ops.mlp_wgrad_multi(jobs)
    want = [[torch.zeros_like(t, dtype=torch.float64) for t in o] for o in outs]
    for oi, *parts in refs:
        for acc, part in zip(want[oi], parts):
            acc += part
    for oi in range(2):
        for got, ref, name in zip(dev_outs[oi], want[oi], ("dW0", "db0", "dW1", "db1", "dW2", "db2")):
            assert torch.isfinite(got).all(), (oi, name)
            assert gerr(got, ref) < 3e-5, (n, oi, name, gerr(got, ref))


def _field_grads(env, fn_hip, fn_oracle, names):
    """run fn_hip(field, grad_desc) / fn_oracle(scene with leaf params) and compare the named gradients"""
    from tensoir_amd import training
    O = env.O
    m = env.model
    f = m.packed_field()
    bufs = training._grad_buffers(m, f)
    extra = fn_hip(f, bufs["desc"])
    work = O.Scene(**env.sc.__dict__)
    for nm in ("density_plane", "density_line", "app_plane", "app_line"):
        setattr(work, nm, [t.detach().clone().requires_grad_(True) for t in getattr(env.sc, nm)])
    work.basis_mat = env.sc.basis_mat.detach().clone().requires_grad_(True)
    work.light_line = env.sc.light_line.detach().clone().requires_grad_(True)
    fn_oracle(work).backward()
    ps = O.scene_parameters(work)
    short = {"density_plane": "dp", "density_line": "dl", "app_plane": "ap", "app_line": "al"}
    errs = {}
    for nm in names:
        ref = ps[nm].grad
        if nm == "light_line.weight":
            got = bufs["ll"] + bufs["lm"][None] / m.light_num
        elif nm == "basis_mat.weight":
            got = extra
        else:
            base, i = nm.split(".")
            got = training._to_param_layout(bufs[f"{short[base]}{i}"])
        errs[nm] = gerr(got, ref)
    assert max(errs.values()) < GTOL, errs


def test_density_normal_backward(env):
    from tensoir_amd import ops
    xyz = T(env.g, "normals/xyz")
    gn = torch.randn(xyz.shape[0], 3, generator=torch.Generator().manual_seed(11))

    def hip(f, gd):
        ops.density_grad_bwd(f, gd, xyz.cuda(), gn.cuda())

    def orc(work):
        return (env.O.density_grad(work, xyz)[2] * gn).sum()
    _field_grads(env, hip, orc, [f"density_plane.{i}" for i in range(3)] + [f"density_line.{i}" for i in range(3)])


def test_march_backward(env):
    """raw2alpha + softplus + density gather backward in isolation: random cotangents on weight / acc / depth."""
    from tensoir_amd import ops
    O, g = env.O, env.g
    rays = T(g, "rays/rays")
    B, S = rays.shape[0], 57
    gen = torch.Generator().manual_seed(31)
    jitter = torch.rand(B, 1, generator=gen)
    gw = torch.randn(B, S, generator=gen)
    ga, gd = torch.randn(B, generator=gen), torch.randn(B, generator=gen)

    def hip(f, gdesc):
        r = rays.cuda()
        weight, sigma, acc, depth, _t, _c = ops.march_primary_train(f, r, jitter.cuda(), S, 0.0)
        ops.march_primary_bwd(f, gdesc, r, jitter.cuda(), sigma, weight, gw.cuda(), ga.cuda(), gd.cuda())

    def orc(work):
        pts, z, valid = O.sample_ray(work, rays[:, :3], rays[:, 3:6], S, jitter)
        z = z.expand(B, S)
        dists = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), dim=-1)
        sigma, valid, xyz = O.march_sigma(work, pts, valid, "explicit")
        _, weight, _ = O.raw2alpha(sigma, dists * work.distance_scale)
        return (weight * gw).sum() + (weight.sum(-1) * ga).sum() + ((weight * z).sum(-1) * gd).sum()
    _field_grads(env, hip, orc, [f"density_plane.{i}" for i in range(3)] + [f"density_line.{i}" for i in range(3)])



def test_app_feature_backward(env):
    from tensoir_amd import ops
    xyz, li = T(env.g, "feat/xyz"), T(env.g, "feat/light_idx").int()
    gen = torch.Generator().manual_seed(12)
    n = xyz.shape[0]
    gr, gi = torch.zeros(n, 32), torch.zeros(n, 32)
    gr[:, :27] = torch.randn(n, 27, generator=gen)
    gi[:, :27] = torch.randn(n, 27, generator=gen)

    def hip(f, gd):
        y_rad, y_int = ops.vm_app_bwd(f, gd, xyz.cuda(), li.cuda().view(-1), None, gr.cuda(), gi.cuda())
        dB = torch.zeros(27, 3 * f.n_acomp).cuda()
        ops.gemm_tn(gr.cuda(), 27, y_rad, 3 * f.n_acomp, dB)
        ops.gemm_tn(gi.cuda(), 27, y_int, 3 * f.n_acomp, dB)
        return dB

    def orc(work):
        r, i = env.O.both_feature(work, xyz, li, "explicit")
        return (r * gr[:, :27]).sum() + (i * gi[:, :27]).sum()
    _field_grads(env, hip, orc, [f"app_plane.{i}" for i in range(3)] + [f"app_line.{i}" for i in range(3)] +
                 ["basis_mat.weight", "light_line.weight"])


def test_shading_backward(env):
    """ShadeFn / EnvSGFn against autograd through the oracle's render_with_brdf on identical vis/indirect."""
    from tensoir_amd import relight
    O, m, g = env.O, env.model, env.g
    rays, lidx = T(g, "rays/rays"), T(g, "rays/light_idx")
    with torch.no_grad():
        out = O.forward_primary(env.sc, rays, lidx.int(), brdf_jitter=torch.zeros(rays.shape[0], m.nSamples, 3))
    depth, normal, albedo, rough, fres, acc = out[1], out[2], out[3], out[4], out[5], out[6]
    mask = acc > 0.5
    leaves = [t[mask].clone().requires_grad_(True) for t in (normal, albedo, rough, fres)]
    sgs = env.sc.lgtSGs.clone().requires_grad_(True)
    work = O.Scene(**env.sc.__dict__)
    work.lgtSGs = sgs
    gout = torch.randn(int(mask.sum()), 3, generator=torch.Generator().manual_seed(13))
    ref = O.render_with_brdf(work, depth[mask], leaves[0], leaves[1], leaves[2].repeat(1, 3), leaves[3], rays[mask],
                             lidx[mask].int(), 24, 0.05, 1.5)
    (ref * gout).sum().backward()
    hl = [t.detach().clone().cuda().requires_grad_(True) for t in leaves]
    m.lgtSGs.grad = None
    got = relight.render_with_BRDF(depth[mask].cuda(), hl[0], hl[1], hl[2].repeat(1, 3), hl[3], rays[mask].cuda(), m,
                                   lidx[mask].cuda(), "fixed_envirmap", args=env.args)
    assert gerr(got, ref) < 1e-4
    (got * gout.cuda()).sum().backward()
    for a, b, nm in zip(hl, leaves, ("normal", "albedo", "roughness", "fresnel")):
        assert gerr(a.grad, b.grad) < GTOL, (nm, gerr(a.grad, b.grad))
    assert gerr(m.lgtSGs.grad, sgs.grad) < GTOL
    m.lgtSGs.grad = None


# ------------------------------------------------------------------ whole training step
@pytest.mark.parametrize("relight,t_stop", [(False, 0.0), (True, 0.0), (True, 1e-6)])
def test_training_step_vs_oracle(env, relight, t_stop):
    _check_training_step(env, env.model, env.sc, relight, t_stop, 18 if not relight else 30)


@pytest.mark.parametrize("kind", ["purely_predicted", "purely_derived", "gt_normals", "residue_prediction"])
def test_normals_kinds_vs_reference(env, kind):
    """normals_kind 'purely_predicted' (the reference's class default) and 'purely_derived': forward maps against the
    imported reference (tests/golden/normals_kinds.npz) -- normals_diff and normals_orientation_loss are ZERO in both
    (only the derived_plus_predicted branch fills them, tensorBase_rotated_lights.py:946-960) -- and one training step
    against the oracle (pinned to the reference's gradients for these kinds by tests/test_oracle_kinds.py)."""
    import tensoir_amd
    from tests.helpers import golden_checkpoint, scene_from_checkpoint
    kg = np.load(os.path.join(ROOT, "tests", "golden", "normals_kinds.npz"))
    ck = golden_checkpoint(env.g)
    ck["kwargs"]["normals_kind"] = kind
    if kind in ("purely_derived", "gt_normals"):
        ck["state_dict"] = {k: v for k, v in ck["state_dict"].items() if not k.startswith("renderModule_normal")}
    if kind == "residue_prediction":        # MLPNormal_normal_and_PExyz (:236-262): layer 1 also takes the derived normal (153 columns)
        ck["state_dict"]["renderModule_normal.mlp.0.weight"] = T(kg, "residue_prediction/w0_normal_decoder")
    eh, ew = [int(x) for x in env.g["scene/envmap_hw"]]
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=eh, envmap_w=ew)
    m.march_t_stop = 0.0
    sc = scene_from_checkpoint(ck, eh, ew)
    assert sc.normals_kind == kind
    rays, lidx = T(env.g, "rays/rays").cuda(), T(env.g, "rays/light_idx").cuda()
    names = ["rgb_map", "depth_map", "normal_map", "albedo_map", "roughness_map", "fresnel_map", "acc_map",
             "normals_diff_map", "normals_orientation_loss_map"]
    with torch.no_grad():
        out = m(rays, lidx)
    for n, a in zip(names, out):
        ref = torch.from_numpy(kg[f"{kind}/fwd/{n}"])
        if kind == "gt_normals" and n == "normal_map":
            # the model's own map is (0, 0, 1 - acc) / max(1 - acc, 1e-6) here (:1004-1028: no sample contributes a normal):
            # for opaque rays 1 ulp of acc moves it by 0.1 -- a placeholder the caller replaces, compared where it is defined
            sel = torch.from_numpy(kg[f"{kind}/fwd/acc_map"]) < 0.999
            assert float((a.cpu()[sel] - ref[sel]).abs().max()) < 1e-4, (kind, n)
            continue
        assert float((a.cpu() - ref).abs().max()) < 1e-4, (kind, n)
    if kind == "residue_prediction":        # like derived_plus_predicted it fills the two normal losses (:966-968)
        assert float(out[7].abs().max()) > 0.0
    else:
        assert float(out[7].abs().max()) == 0.0 and float(out[8].abs().max()) == 0.0
    # the boundary call against the reference's own (renderer.py:57-127); 'gt_normals': the ground-truth normals replace the
    # zero map before the shading stage and in the returned dict (:82-83)
    from tensoir_amd import Renderer_TensoIR_train
    ngt = T(kg, "normal_gt") if kind == "gt_normals" else None
    with torch.no_grad():
        ret = Renderer_TensoIR_train(rays, ngt, lidx, m, N_samples=-1, white_bg=True, is_train=False, is_relight=True,
                                     sample_method="fixed_envirmap", device="cuda", args=env.args)
    for k in ("rgb_map", "depth_map", "normal_map", "albedo_map", "roughness_map", "acc_map", "rgb_with_brdf_map"):
        ref = torch.from_numpy(kg[f"{kind}/eval_render/{k}"])
        assert float((ret[k].cpu() - ref).abs().max()) < 1e-4, (kind, k)
    _check_training_step(env, m, sc, True, 0.0, 19 if kind == "gt_normals" else 25, normal_gt=ngt)
    if kind == "residue_prediction":        # the stand-alone decoder call of the reference interface (pts, normal, features)
        n = 257
        gen = torch.Generator().manual_seed(3)
        pts, nrm = torch.rand(n, 3, generator=gen) * 2 - 1, torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
        feat = torch.randn(n, 27, generator=gen)
        with torch.no_grad():
            got = m.renderModule_normal(pts.cuda(), nrm.cuda(), feat.cuda()).cpu()
        want = env.O.render_normal_residue(sc, pts, nrm, feat)
        assert float((got - want).abs().max()) < 1e-5


def test_training_step_with_no_hits(env):
    """Rays that miss the volume: no records, every stage of the backward must cope (zero / absent gradients)."""
    from tensoir_amd import Renderer_TensoIR_train
    m = env.model
    m.zero_grad(set_to_none=True)
    rays = torch.tensor([[0.0, 0.0, 4.0, 0.9, 0.0, -0.43589]] * 5)
    rays[:, 3:] = rays[:, 3:] / rays[:, 3:].norm(dim=-1, keepdim=True)
    lidx = torch.zeros(5, 1, dtype=torch.int32)
    ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=32, white_bg=True, is_train=True, is_relight=True,
                                 sample_method="fixed_envirmap", device="cuda", args=env.args)
    loss = env.O.training_loss(ret, torch.zeros(5, 3, device="cuda"), True)
    loss.backward()
    assert torch.isfinite(loss)
    for name, p in m.named_parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), name
    m.zero_grad(set_to_none=True)
    # second call: the record buffers are now sized from the (empty) previous step -- the capacity-hint route
    ret2 = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=32, white_bg=True, is_train=True, is_relight=True,
                                  sample_method="fixed_envirmap", device="cuda", args=env.args)
    loss2 = env.O.training_loss(ret2, torch.zeros(5, 3, device="cuda"), True)
    loss2.backward()
    assert abs(float(loss2.detach()) - float(loss.detach())) < 1e-6
    for name, p in m.named_parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), name
    m.zero_grad(set_to_none=True)


def test_optimizer_steps_reduce_loss(env):
    """A few Adam steps on the HIP training path lower the image loss (end-to-end sanity of sign/scale)."""
    import tensoir_amd
    from tensoir_amd import Renderer_TensoIR_train
    from tests.helpers import golden_checkpoint
    eh, ew = [int(x) for x in env.g["scene/envmap_hw"]]
    m = tensoir_amd.model_from_checkpoint(golden_checkpoint(env.g), "cuda", envmap_h=eh, envmap_w=ew)
    rays, lidx = T(env.g, "rays/rays").cuda(), T(env.g, "rays/light_idx").cuda()
    gt = torch.full((rays.shape[0], 3), 0.25, device="cuda")
    opt = torch.optim.Adam(m.get_optparam_groups(0.02, 0.001), betas=(0.9, 0.99))
    losses = []
    for it in range(6):
        ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=64, white_bg=True, is_train=True,
                                     is_relight=True, sample_method="stratified_sampling", device="cuda", args=env.args)
        loss = env.O.training_loss(ret, gt, True)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_general_multi_light_variant(env):
    """one SG set per light.  Environment radiance, a full render and the SG gradients of a
    training step against the oracle (lgtSGs_list branch of oracle.light_rgbs)."""
    import tensoir_amd
    from tensoir_amd.general_multi_lights import TensorVMSplit as General
    from tensoir_amd import Renderer_TensoIR_train
    from tests.helpers import golden_checkpoint
    O, g = env.O, env.g
    ckpt = golden_checkpoint(g)
    kw = dict(ckpt["kwargs"])
    for k in ("light_num", "light_rotation"):
        kw.pop(k, None)
    eh, ew = [int(x) for x in g["scene/envmap_hw"]]
    m = General(device="cuda", light_name_list=["a", "b", "c"], envmap_h=eh, envmap_w=ew, **kw)
    sd = {k: v for k, v in ckpt["state_dict"].items() if k != "lgtSGs"}
    m.load_state_dict(sd, strict=False)
    m.alphaMask = env.model.alphaMask
    m._field_key = None
    m.march_t_stop = 0.0
    gen = torch.Generator().manual_seed(41)
    sgs = []
    for i, sg in enumerate(m.lgtSGs_list):
        with torch.no_grad():
            sg.copy_((env.sc.lgtSGs + 0.3 * torch.randn(env.sc.lgtSGs.shape, generator=gen)).cuda())
        sgs.append(sg.detach().cpu().clone())
    sc = O.Scene(**env.sc.__dict__)
    sc.lgtSGs_list = sgs
    dirs = torch.nn.functional.normalize(torch.randn(50, 3, generator=gen), dim=-1)
    with torch.no_grad():
        assert gerr(m.get_light_rgbs(dirs.cuda(), device="cuda"), O.light_rgbs(sc, dirs)) < 1e-5
    rays, lidx = T(g, "rays/rays"), T(g, "rays/light_idx")
    S, B = 64, rays.shape[0]
    jitter = torch.rand(B, 1, generator=gen)
    noise = torch.randn(B, S, 3, generator=gen)
    gt = T(env.tg, "train/rgb_gt")
    # oracle gradients w.r.t. the three SG sets
    leaves = [s_.clone().requires_grad_(True) for s_ in sgs]
    sc.lgtSGs_list = leaves
    ret_ref = O.renderer_train(sc, rays, lidx, S, True, True, 24, 0.05, 1.5, jitter, noise)
    O.training_loss(ret_ref, gt, True).backward()
    orig_rand, orig_fwd = torch.rand, type(m).forward

    def fake_rand(*a, **k):
        if tuple(a) == (B, 1):
            return jitter.clone()
        return orig_rand(*a, **k)

    def fwd(self, r, l, **k):
        return orig_fwd(self, r, l, _brdf_jitter_dense=noise, **k)
    torch.rand, type(m).forward = fake_rand, fwd
    try:
        ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=S, white_bg=True, is_train=True, is_relight=True,
                                     sample_method="fixed_envirmap", device="cuda", args=env.args)
    finally:
        torch.rand, type(m).forward = orig_rand, orig_fwd
    assert float((ret["rgb_with_brdf_map"].detach().cpu() - ret_ref["rgb_with_brdf_map"].detach()).abs().max()) < 1e-4
    O.training_loss(ret, gt.cuda(), True).backward()
    for sg, ref in zip(m.lgtSGs_list, leaves):
        assert gerr(sg.grad, ref.grad) < GTOL


def test_general_multi_light_variant_vs_reference_golden(env):
    """The general multi-light model against tests/golden/general_lights.npz, written by the IMPORTED REFERENCE
    (oracle/make_golden_general.py; models/tensoRF_general_multi_lights.py, tensorBase_general_multi_lights.py:463-479,
    :566-582): environment radiance of the three SG sets, the maps of an eval render, and one training step -- rendered
    maps, loss-relevant outputs and the gradient of every SG set and of the field / decoder parameters."""
    from tensoir_amd.general_multi_lights import TensorVMSplit as General
    from tensoir_amd import Renderer_TensoIR_train
    from tests.helpers import golden_checkpoint
    O, g = env.O, env.g
    gg = np.load(os.path.join(ROOT, "tests", "golden", "general_lights.npz"))
    ckpt = golden_checkpoint(g)
    kw = dict(ckpt["kwargs"])
    for k in ("light_num", "light_rotation"):
        kw.pop(k, None)
    eh, ew = [int(x) for x in g["scene/envmap_hw"]]
    m = General(device="cuda", light_name_list=["sunset", "snow", "courtyard"], envmap_h=eh, envmap_w=ew, **kw)
    m.load_state_dict({k: v for k, v in ckpt["state_dict"].items() if k != "lgtSGs"}, strict=False)
    m.alphaMask = env.model.alphaMask
    m._field_key = None
    m.march_t_stop = 0.0
    with torch.no_grad():
        for i, sg in enumerate(m.lgtSGs_list):
            sg.copy_(T(gg, f"sg/{i}").cuda())
        got = m.get_light_rgbs(T(gg, "env/dirs").cuda(), device="cuda")
    assert got.shape == (3, 50, 3) and gerr(got, T(gg, "env/light_rgbs")) < 1e-5
    rays, lidx = T(g, "rays/rays"), T(g, "rays/light_idx")
    B, S = rays.shape[0], int(gg["train/n_samples"][0])
    with torch.no_grad():
        ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=-1, white_bg=True, is_train=False, is_relight=True,
                                     sample_method="fixed_envirmap", device="cuda", args=env.args)
    for k in ("rgb_map", "depth_map", "normal_map", "albedo_map", "roughness_map", "acc_map", "rgb_with_brdf_map"):
        ref = T(gg, f"eval/out/{k}")
        err = float(((ret[k].cpu() - ref).abs() / ref.abs().clamp(min=1.0)).max())
        assert err < 1e-4, (k, err)
    # one training step: the reference's ray jitter replayed (rand [B,1], :717); the BRDF jitter draw (:937) only feeds
    # the two smoothness losses, on which neither the rendered maps nor the SG / radiance-decoder gradients depend
    jitter = T(gg, "train/ray_jitter")
    orig_rand = torch.rand

    def fake_rand(*a, **k):
        if tuple(a) == (B, 1):
            return jitter.clone().to(k.get("device", "cpu"))
        return orig_rand(*a, **k)
    torch.rand = fake_rand
    try:
        ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=S, white_bg=True, is_train=True, is_relight=True,
                                     sample_method="fixed_envirmap", device="cuda", args=env.args)
    finally:
        torch.rand = orig_rand
    for k in ("rgb_map", "acc_map", "rgb_with_brdf_map", "normals_diff_map"):
        ref = T(gg, f"train/out/{k}")
        assert float((ret[k].detach().cpu() - ref).abs().max()) < 1e-4, k
    O.training_loss(ret, T(gg, "train/rgb_gt").cuda(), True).backward()
    for i, sg in enumerate(m.lgtSGs_list):
        assert gerr(sg.grad, T(gg, f"train/grad/lgtSGs_list.{i}")) < GTOL, i
    params = dict(m.named_parameters())
    for name in ("renderModule.mlp.0.weight", "renderModule.mlp.0.bias", "renderModule.mlp.2.weight", "renderModule.mlp.4.weight"):
        # the radiance decoder's gradient comes from rgb_map alone (the secondary pass is no_grad, relight_utils.py:344):
        # independent of the BRDF jitter, so it must match the reference's
        assert gerr(params[name].grad, T(gg, f"train/grad/{name}")) < GTOL, name


def test_gt_probe_light_vs_reference_golden(env):
    """light_kind == 'gt' (:592-593): `dataset.lights_probes` looked up as it is (tir_env_pixel_fwd, softplus = 0); no light
    parameter in the optimizer groups; a training step still differentiates everything else."""
    import types
    import tensoir_amd
    from tensoir_amd import Renderer_TensoIR_train
    from tests.helpers import golden_checkpoint
    g = env.g
    pg = np.load(os.path.join(ROOT, "tests", "golden", "pixel_light.npz"))
    ck = golden_checkpoint(g)
    ck["kwargs"]["light_kind"] = "gt"
    ck["kwargs"]["dataset"] = types.SimpleNamespace(lights_probes=T(pg, "gt/probe"))
    ck["state_dict"] = {k: v for k, v in ck["state_dict"].items() if k != "lgtSGs"}
    eh, ew = [int(x) for x in g["scene/envmap_hw"]]
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=eh, envmap_w=ew)
    m.march_t_stop = 0.0
    assert m.light_kind == "gt" and not hasattr(m, "lgtSGs") and m.light_parameters() == []
    with torch.no_grad():
        got = m.get_light_rgbs(T(pg, "env/dirs").cuda(), device="cuda")
    assert got.shape == (3, 60, 3) and gerr(got, T(pg, "gt/light_rgbs")) < 1e-5
    rays, lidx = T(g, "rays/rays"), T(g, "rays/light_idx")
    with torch.no_grad():
        ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=-1, white_bg=True, is_train=False, is_relight=True,
                                     sample_method="fixed_envirmap", device="cuda", args=env.args)
    for k in ("rgb_map", "normal_map", "albedo_map", "acc_map", "rgb_with_brdf_map"):
        assert float((ret[k].cpu() - T(pg, f"gt/eval/out/{k}")).abs().max()) < 1e-4, k
    ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=64, white_bg=True, is_train=True, is_relight=True,
                                 sample_method="fixed_envirmap", device="cuda", args=env.args)
    ret["rgb_with_brdf_map"].mean().backward()
    assert m.renderModule_brdf.mlp[0].weight.grad is not None and float(m.renderModule_brdf.mlp[0].weight.grad.abs().max()) > 0


def test_pixel_environment_light_vs_reference_golden(env):
    """light_kind == 'pixel' (tir_env_pixel_fwd / _bwd; models/tensorBase_rotated_lights.py:459-460, :585-605) against
    tests/golden/pixel_light.npz, written by the IMPORTED REFERENCE: environment radiance incl. the poles and the +-pi seam, three
    light rotations; an eval render; one training step -- rendered maps and the gradient of the map parameters themselves."""
    import tensoir_amd
    from tensoir_amd import Renderer_TensoIR_train
    from tests.helpers import golden_checkpoint
    O, g = env.O, env.g
    pg = np.load(os.path.join(ROOT, "tests", "golden", "pixel_light.npz"))
    ck = golden_checkpoint(g)
    ck["kwargs"]["light_kind"] = "pixel"
    ck["state_dict"] = {k: v for k, v in ck["state_dict"].items() if k != "lgtSGs"}
    ck["state_dict"]["_light_rgbs"] = T(pg, "light_rgbs_raw")
    eh, ew = [int(x) for x in g["scene/envmap_hw"]]
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=eh, envmap_w=ew)
    m.march_t_stop = 0.0
    assert m.light_kind == "pixel" and not hasattr(m, "lgtSGs")
    assert any(p is m._light_rgbs for grp in m.get_optparam_groups() for p in (grp["params"] if isinstance(grp["params"], (list, tuple)) else [grp["params"]]))
    with torch.no_grad():
        got = m.get_light_rgbs(T(pg, "env/dirs").cuda(), device="cuda")
        fixed = m.get_light_rgbs(m.fixed_viewdirs, device="cuda")
    assert got.shape == (3, 60, 3) and gerr(got, T(pg, "env/light_rgbs")) < 1e-5
    assert gerr(fixed, T(pg, "env/light_rgbs_fixed")) < 1e-5
    rays, lidx = T(g, "rays/rays"), T(g, "rays/light_idx")
    B, S = rays.shape[0], int(pg["train/n_samples"][0])
    with torch.no_grad():
        ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=-1, white_bg=True, is_train=False, is_relight=True,
                                     sample_method="fixed_envirmap", device="cuda", args=env.args)
    for k in ("rgb_map", "normal_map", "albedo_map", "acc_map", "rgb_with_brdf_map"):
        assert float((ret[k].cpu() - T(pg, f"eval/out/{k}")).abs().max()) < 1e-4, k
    jitter = T(pg, "train/ray_jitter")
    orig_rand = torch.rand

    def fake_rand(*a, **k):
        return jitter.clone() if tuple(a) == (B, 1) else orig_rand(*a, **k)
    torch.rand = fake_rand
    try:
        ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=S, white_bg=True, is_train=True, is_relight=True,
                                     sample_method="fixed_envirmap", device="cuda", args=env.args)
    finally:
        torch.rand = orig_rand
    for k in ("rgb_map", "acc_map", "rgb_with_brdf_map"):
        assert float((ret[k].detach().cpu() - T(pg, f"train/out/{k}")).abs().max()) < 1e-4, k
    O.training_loss(ret, T(pg, "train/rgb_gt").cuda(), True).backward()
    assert gerr(m._light_rgbs.grad, T(pg, "train/grad/_light_rgbs")) < GTOL
    params = dict(m.named_parameters())
    for name in ("renderModule.mlp.0.weight", "renderModule.mlp.4.weight"):
        assert gerr(params[name].grad, T(pg, f"train/grad/{name}")) < GTOL, name


def test_training_record_capacity_hints(env):
    """Second and later training steps size their record buffers from the previous step (no mid-pass host read);
    gradients equal those of the exact (first-call) route, also after a forced capacity overflow (pass re-run)."""
    import tensoir_amd
    from tensoir_amd import Renderer_TensoIR_train
    from tests.helpers import golden_checkpoint
    eh, ew = [int(x) for x in env.g["scene/envmap_hw"]]
    m = tensoir_amd.model_from_checkpoint(golden_checkpoint(env.g), "cuda", envmap_h=eh, envmap_w=ew)
    m.march_t_stop = 0.0
    rays, lidx = T(env.g, "rays/rays").cuda(), T(env.g, "rays/light_idx").cuda()
    B, S = rays.shape[0], 64
    gt = torch.full((B, 3), 0.25, device="cuda")

    def grads():
        m.zero_grad(set_to_none=True)
        torch.manual_seed(7)
        ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=S, white_bg=True, is_train=False, is_relight=False,
                                     device="cuda", args=env.args)
        loss = torch.mean((ret["rgb_map"] - gt) ** 2)
        loss.backward()
        return float(loss), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}

    l0, g0 = grads()                                   # exact route, learns the capacity
    assert (B, S) in m._train_cap_hints
    l1, g1 = grads()                                   # capacity-hint route
    m._train_cap_hints[(B, S)] = 64                    # far too small: overflow -> the pass is re-run exactly
    l2, g2 = grads()
    assert (B, S) in m._train_cap_hints and m._train_cap_hints[(B, S)] > 64
    for l, g in ((l1, g1), (l2, g2)):
        assert abs(l - l0) < 1e-6
        assert set(g) == set(g0)
        for n in g0:
            assert gerr(g[n], g0[n]) < 2e-5, n


def test_grid_400_training_and_inference_smoke(env):
    """The largest shipped resolution (ficus: N_voxel_final = 400^3): one inference pass and one
    training step run, agree with each other on the rendered maps, and give finite gradients for every parameter."""
    import types
    import tensoir_amd
    from tensoir_amd import Renderer_TensoIR_train, synth
    ck = synth.make_checkpoint(grid=(400, 400, 400), seed=11)
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=4, envmap_w=8)
    rays = synth.make_rays(32, 32).cuda()
    lidx = torch.zeros(rays.shape[0], 1, dtype=torch.int32, device="cuda")
    args = types.SimpleNamespace(second_nSample=96, second_near=0.05, second_far=1.5)
    with torch.no_grad():
        ref = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=256, white_bg=True, is_train=False, is_relight=True,
                                     sample_method="fixed_envirmap", device="cuda", args=args)
    ret = Renderer_TensoIR_train(rays, None, lidx, m, N_samples=256, white_bg=True, is_train=False, is_relight=True,
                                 sample_method="fixed_envirmap", device="cuda", args=args)
    for k in ("rgb_map", "acc_map", "normal_map", "albedo_map"):
        assert gerr(ret[k], ref[k]) < 2e-5, k                    # training forward == inference forward
    assert float(ref["acc_map"].max()) > 0.5                     # the scene is hit
    loss = torch.mean((ret["rgb_map"] - 0.3) ** 2) + 0.2 * torch.mean((ret["rgb_with_brdf_map"] - 0.3) ** 2) \
        + 1e-3 * ret["normals_diff_map"].mean()
    loss.backward()
    n_grad = 0
    for name, p in m.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), name
            n_grad += int(p.grad.abs().sum() > 0)
    assert n_grad >= 18


def test_full_size_training_properties():
    """BASELINE size (4096 rays x 512 samples, R = 300, 128 directions x 96 secondary samples): size-independent
    properties of the training step -- (1) the training forward renders the inference forward's maps, (2) the backward
    is linear in the loss (gradients of 2 L are 2 x gradients of L up to the order of the atomic adds), (3) the
    capacity-hint route (second call) reproduces the exact route (first call), (4) every gradient is finite and every
    field parameter receives one."""
    import types
    import tensoir_amd
    from tensoir_amd import Renderer_TensoIR_train, synth
    ck = synth.make_checkpoint(grid=(300, 300, 300), seed=20211202)
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=8, envmap_w=16)
    with torch.no_grad():
        m.updateAlphaMask((128, 128, 128))
    rays = synth.make_rays(64, 64).cuda()
    lidx = torch.zeros(4096, 1, dtype=torch.int32, device="cuda")
    args = types.SimpleNamespace(second_nSample=96, second_near=0.05, second_far=1.5)
    kw = dict(N_samples=512, white_bg=True, is_train=False, is_relight=True, sample_method="fixed_envirmap",
              device="cuda", args=args)
    with torch.no_grad():
        ref = Renderer_TensoIR_train(rays, None, lidx, m, **kw)

    def run(scale):
        m.zero_grad(set_to_none=True)
        ret = Renderer_TensoIR_train(rays, None, lidx, m, **kw)
        loss = scale * (torch.mean((ret["rgb_map"] - 0.3) ** 2) + 0.2 * torch.mean((ret["rgb_with_brdf_map"] - 0.3) ** 2)
                        + 1e-3 * ret["normals_diff_map"].mean())
        loss.backward()
        return ret, float(loss.detach()), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}

    ret1, l1, g1 = run(1.0)                               # exact route (learns the record capacities)
    for k in ("rgb_map", "depth_map", "normal_map", "albedo_map", "acc_map", "rgb_with_brdf_map"):
        assert gerr(ret1[k], ref[k]) < 2e-5, k            # (1)
    ret2, l2, g2 = run(2.0)                               # capacity-hint route, doubled loss
    assert abs(l2 - 2.0 * l1) < 1e-6 * max(1.0, abs(l1))   # (3) same forward
    assert set(g1) == set(g2) and len(g1) >= 30
    for n in g1:
        assert bool(torch.isfinite(g1[n]).all()), n       # (4)
        assert gerr(g2[n], 2.0 * g1[n]) < 2e-4, n         # (2)
    for n in ("density_plane.0", "density_line.2", "app_plane.1", "app_line.0", "basis_mat.weight"):
        assert float(g1[n].abs().sum()) > 0.0, n


def test_single_launch_adam_matches_torch_adam():
    """tensoir_amd.optim.Adam.step (tir_adam_step, one launch) against torch.optim.Adam on the same gradients for 25 steps:
    per-tensor groups with different learning rates (train_tensoIR.py:196-197), channel-last parameters (the model's
    plane storage), odd sizes (scalar tail), an lr rescale mid-run (:321-322) and a parameter whose grad is None."""
    from tensoir_amd import optim
    g = torch.Generator().manual_seed(5)
    shapes = [(1, 16, 37, 41), (1, 48, 29, 1), (27, 144), (128, 150), (128,), (3,), (1, 7, 5, 3)]
    base = [torch.randn(s, generator=g) for s in shapes]
    def make():
        ps = []
        for i, b in enumerate(base):
            t = b.clone().cuda()
            if t.dim() == 4 and i != 6:
                t = t.contiguous(memory_format=torch.channels_last)
            ps.append(torch.nn.Parameter(t))
        return ps
    pa, pb = make(), make()
    lrs = [0.02, 0.02, 0.001, 0.001, 0.001, 0.0005, 0.02]
    oa = optim.Adam([{"params": p, "lr": lr} for p, lr in zip(pa, lrs)], betas=(0.9, 0.99))
    ob = optim._TorchAdam([{"params": p, "lr": lr} for p, lr in zip(pb, lrs)], betas=(0.9, 0.99))
    for step in range(25):
        for i, (a, b) in enumerate(zip(pa, pb)):
            if i == 5 and step < 3:
                a.grad = b.grad = None                   # joins later: its own step count / bias correction
                continue
            gr = torch.randn(a.shape, generator=g).cuda() * (10.0 ** ((i % 3) - 1))
            if i == 0:
                gr = gr.contiguous(memory_format=torch.channels_last)
            a.grad, b.grad = gr.clone(), gr.clone()
        if step == 10:
            for o in (oa, ob):
                for grp in o.param_groups:
                    grp["lr"] = grp["lr"] * 0.7
        v0 = pa[0]._version
        oa.step(); ob.step()
        assert pa[0]._version > v0                       # caches keyed by Tensor._version see the raw-pointer update
    for a, b in zip(pa, pb):
        assert a.stride() == b.stride()
        assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max()))
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"])
        assert torch.allclose(sa["state"][k]["exp_avg_sq"], sb["state"][k]["exp_avg_sq"], rtol=1e-5, atol=1e-12)
    # ---- the steady state of a training loop: every gradient in its parameter's own layout (what autograd hands back) -> after
    # one fully checked step the optimizer keeps a plan and a step costs identity checks only (Adam._fast_step); it must
    # notice everything that invalidates the plan: an lr change (no invalidation, new value used), a missing gradient, a
    # reloaded state
    def grads(step):
        for i, (a, b) in enumerate(zip(pa, pb)):
            gr = torch.empty_like(a).copy_(torch.randn(a.shape, generator=g).cuda() * (10.0 ** ((i % 3) - 1)))
            assert gr.stride() == a.stride()
            a.grad, b.grad = gr.clone(), gr.clone()
    fast = []
    for step in range(15):
        grads(step)
        if step == 5:
            for o in (oa, ob):
                for grp in o.param_groups:
                    grp["lr"] = grp["lr"] * 0.5
        if step == 7:
            pa[3].grad = pb[3].grad = None               # back to the checked path for this step, then a fresh plan
        if step == 9:
            oa.load_state_dict(oa.state_dict())          # new state tensors: the plan's identities no longer hold
        if step == 12:                                   # the SAME moment tensor object on other storage: the plan holds raw pointers
            mom = oa.state[pa[1]]["exp_avg"]
            mom.data = mom.data.clone()
        had_plan = oa.__dict__.get("_tir_plan") is not None
        v0, s0 = pa[0]._version, float(oa.state[pa[0]]["step"])
        if step == 13:                                   # a launch that fails must leave the step counts where they were
            from tensoir_amd import ops as _ops
            real = _ops.adam_step_tables
            def boom(*a, **k):
                raise RuntimeError("launch failed")
            _ops.adam_step_tables = boom
            try:
                with pytest.raises(RuntimeError):
                    oa.step()
            finally:
                _ops.adam_step_tables = real
            assert float(oa.state[pa[0]]["step"]) == s0 and pa[0]._version == v0
        oa.step(); ob.step()
        fast.append(had_plan and oa.__dict__.get("_tir_plan") is not None and step not in (7, 9, 12))
        assert pa[0]._version > v0 and float(oa.state[pa[0]]["step"]) == s0 + 1
    assert fast == [False, True, True, True, True, True, True, False, False, False, True, True, False, True, True], fast
    for a, b in zip(pa, pb):
        assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max()))
    sa, sb = oa.state_dict(), ob.state_dict()
    for k in sa["state"]:
        assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"])
        ea, eb = sa["state"][k]["exp_avg"], sb["state"][k]["exp_avg"]
        assert float((ea - eb).abs().max()) <= 2e-6 * float(eb.abs().max())
        assert torch.allclose(sa["state"][k]["exp_avg_sq"], sb["state"][k]["exp_avg_sq"], rtol=1e-5, atol=1e-12)
    ob2 = optim.Adam([{"params": p, "lr": lr} for p, lr in zip(pb, lrs)], betas=(0.9, 0.99))
    ob2.load_state_dict(sb)                               # a torch.optim.Adam state continues under ours
    for b in pb:
        b.grad = torch.ones_like(b)
    ob2.step()


@pytest.mark.timeout(300)
def test_dp_training_step_on_one_rank_rccl_group(env):
    """SURVEY 8(f)-4 / VERDICT r2 item 9a: the data-parallel step -- shard_batch + backward + allreduce_gradients (bucketed,
    forced through the collective although the group has one rank) -- on an RCCL process group, inside a real training step
    on the GPU: the gradients that come back from the all-reduce equal the single-process step's (sum over one rank, / 1),
    every bucket really went through RCCL, and the optimizer step after it matches.  (More ranks need more GPUs: the
    multi-rank flow is covered on gloo by tests/test_dist_gloo.py.)"""
    import torch.distributed as dist
    import tensoir_amd
    from tensoir_amd import Renderer_TensoIR_train, optim
    from tensoir_amd import dist as tdist
    from tests.helpers import golden_checkpoint
    eh, ew = [int(x) for x in env.g["scene/envmap_hw"]]
    rays, lidx = T(env.g, "rays/rays").cuda(), T(env.g, "rays/light_idx").cuda()
    gt = T(env.tg, "train/rgb_gt").cuda()
    B = rays.shape[0]
    mine = tdist.shard_batch(B, 0, 1)
    assert torch.equal(mine, torch.arange(B))
    jitter = torch.rand(B, 1, generator=torch.Generator().manual_seed(5))
    noise = torch.randn(B, 64, 3, generator=torch.Generator().manual_seed(6))

    def one_step(reduce):
        m = tensoir_amd.model_from_checkpoint(golden_checkpoint(env.g), "cuda", envmap_h=eh, envmap_w=ew)
        opt = optim.Adam(m.get_optparam_groups(0.02, 0.001), betas=(0.9, 0.99))
        params = [p for g in opt.param_groups for p in g["params"]]
        orig_rand, orig_fwd = torch.rand, type(m).forward

        def fake_rand(*a, **k):
            return jitter.clone() if tuple(a) == (B, 1) else orig_rand(*a, **k)

        def fwd(self, r, l, **k):
            return orig_fwd(self, r, l, _brdf_jitter_dense=noise, **k)
        torch.rand, type(m).forward = fake_rand, fwd
        try:
            ret = Renderer_TensoIR_train(rays[mine.cuda()], None, lidx[mine.cuda()], m, N_samples=64, white_bg=True, is_train=True,
                                         is_relight=True, sample_method="fixed_envirmap", device="cuda", args=env.args)
        finally:
            torch.rand, type(m).forward = orig_rand, orig_fwd
        env.O.training_loss(ret, gt, True).backward()
        buckets = tdist.allreduce_gradients(params, bucket_mb=0.25, force=True) if reduce else 0
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        opt.step()
        return grads, {n: p.detach().clone() for n, p in m.named_parameters()}, buckets

    g0, p0, _ = one_step(False)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29571")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
        g1, p1, buckets = one_step(True)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert buckets >= 3                      # 0.25 MB buckets: the planes, lines and decoders travel in several collectives
    assert set(g0) == set(g1) and len(g0) >= 30
    for n in g0:                             # atomics reorder the sums between two runs of the same step: same tolerance as the
        assert gerr(g1[n], g0[n]) < GTOL, n  # backward tests; the all-reduce itself adds nothing on one rank
        assert g1[n].stride() == g0[n].stride(), n          # the parameter's own (channel-last) layout survives the bucket copy
    for n in p0:
        assert gerr(p1[n], p0[n]) < 5e-3, n
