"""Parity tests proper: the HIP path (through the C ABI) against (a) the golden vectors produced by the
imported reference and (b) the CPU oracle on seeded inputs; plus size-independent properties at
BASELINE.json's full size.  Tolerance: north_star's 1e-4 relative on rendered maps, asserted two ways: |hip - ref| / max(|ref|, 1) on every
map (`rel`: the maps live in [0,1] / unit normals / depth ~4) AND the true per-pixel relative error
||hip - ref|| / ||ref|| over pixels with ||ref|| > 1e-2 on the rendered RGB / normal maps (`relpix`, `check_map`)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
NAMES = ["rgb_map", "depth_map", "normal_map", "albedo_map", "roughness_map", "fresnel_map", "acc_map",
         "normals_diff_map", "normals_orientation_loss_map", "acc_mask", "albedo_smoothness_loss",
         "roughness_smoothness_loss"]


def rel(a, b, floor=1.0):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(((a - b).abs() / b.abs().clamp(min=floor)).max()) if a.numel() else 0.0


@pytest.fixture(scope="module")
def env(golden):
    import tensoir_amd
    from tests.helpers import golden_checkpoint, scene_from_checkpoint
    assert torch.cuda.is_available()
    from tensoir_amd import _lib
    assert _lib.lib().tir_device_check() == 0           # fails loudly if the HIP library cannot run
    ckpt = golden_checkpoint(golden)
    eh, ew = [int(x) for x in golden["scene/envmap_hw"]]
    model = tensoir_amd.model_from_checkpoint(ckpt, "cuda", envmap_h=eh, envmap_w=ew)
    model.march_t_stop = 0.0
    sc = scene_from_checkpoint(ckpt, eh, ew)
    return types.SimpleNamespace(model=model, sc=sc, g=golden, dev="cuda",
                                 args=types.SimpleNamespace(second_nSample=24, second_near=0.05, second_far=1.5))


@pytest.fixture(params=["bf16x3", "mfma"])
def decoder(request):
    """Run a test once per decoder mode: split-bf16 matrix cores (product default) and exact fp32."""
    from tensoir_amd import ops
    old = ops.MLP_IMPL
    ops.MLP_IMPL = request.param
    yield request.param
    ops.MLP_IMPL = old


def G(env, key):
    return torch.from_numpy(np.array(env.g[key])).to(env.dev)


def relpix(a, b):
    """True per-pixel relative error: max over pixels with ||ref|| > 1e-2 of ||hip - ref|| / ||ref|| (vector maps: L2 over channels)."""
    from tests.helpers import parity_metrics
    return parity_metrics(a, torch.as_tensor(b))["max_rel_pixel"]


RELATIVE_MAPS = ("rgb_map", "normal_map", "albedo_map", "rgb_with_brdf_map")      # north_star: "1e-4 relative on rendered RGB / normals"


def check_map(name, a, b, tol=TOL):
    """The floor-1 metric on every map, and the per-pixel relative metric on the rendered RGB / normal maps."""
    assert rel(a, b) < tol, (name, rel(a, b))
    if name in RELATIVE_MAPS:
        assert relpix(a, b) < tol, (name, "per-pixel relative", relpix(a, b))


# ---------------------------------------------------------------- golden vectors (reference outputs)
@torch.no_grad()
def test_density_and_app_features_vs_reference(env):
    m = env.model
    xyz, li = G(env, "feat/xyz"), G(env, "feat/light_idx")
    assert rel(m.compute_densityfeature(xyz), env.g["feat/density"]) < 2e-5
    assert rel(m.compute_appfeature(xyz, li), env.g["feat/app"]) < 2e-5
    r, i = m.compute_bothfeature(xyz, li)
    assert rel(r, env.g["feat/both_rad"]) < 2e-5 and rel(i, env.g["feat/both_int"]) < 2e-5
    assert rel(m.compute_intrinfeature(xyz), env.g["feat/intrin"]) < 2e-5
    hit = m.alphaMask.sample_alpha(G(env, "occ/xyz_world")) > 0
    assert bool((hit.cpu() == (torch.from_numpy(env.g["occ/alpha"]) > 0)).all())
    assert rel(m.compute_derived_normals(G(env, "normals/xyz")), env.g["normals/derived"]) < TOL


@torch.no_grad()
@pytest.mark.parametrize("impl", ["mfma", "valu", "bf16x3"])
def test_decoders_vs_reference(env, impl):
    from tensoir_amd import ops
    m = env.model
    xyz, vd = G(env, "feat/xyz"), G(env, "mlp/viewdirs")
    r, i = G(env, "feat/both_rad"), G(env, "feat/both_int")
    assert rel(ops.mlp(m.renderModule.packed(), r, vd, None, impl), env.g["mlp/rgb"]) < 1e-5
    assert rel(ops.mlp(m.renderModule_brdf.packed(), i, xyz, None, impl), env.g["mlp/brdf"]) < 1e-5
    assert rel(ops.mlp(m.renderModule_normal.packed(), i, xyz, None, impl), env.g["mlp/normal"]) < 1e-5


@torch.no_grad()
def test_decoder_large_biases(env):
    """Layer 1's bias rides as the weight of a constant-1 input in the split-bf16 decoders (~16 mantissa bits of it in
    bf16x3; ONE bf16 rounding, 8 bits, in the reduced-precision `bf16` entry) and as an exact fp32 start value in the aux-table
    variant.  With biases 20x their initial size (|b| up to ~1.6): bf16x3 and the aux-table variant stay at the parity grade
    against the exact decoder; the single-product mode keeps ITS documented precision class (include/tensoir_hip.h) --
    no worse than with small biases, since every operand of that mode is an 8-bit bf16 anyway."""
    import copy
    import tensoir_amd
    from tensoir_amd import ops
    from tests.helpers import golden_checkpoint
    ck = golden_checkpoint(env.g)
    sd = dict(ck["state_dict"])
    for k in list(sd):
        if k.startswith("renderModule.") and k.endswith(".bias"):
            sd[k] = sd[k] * 20.0 + 0.37
    ck = dict(ck, state_dict=sd)
    eh, ew = [int(x) for x in env.g["scene/envmap_hw"]]
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=eh, envmap_w=ew)
    pm = m.renderModule.packed()
    gen = torch.Generator().manual_seed(5)
    n, D = 6000, 24
    feat = torch.zeros(n, 32)
    feat[:, :27] = torch.randn(n, 27, generator=gen) * 0.8
    dirs = torch.nn.functional.normalize(torch.randn(D, 3, generator=gen), dim=-1).cuda()
    amap = torch.randint(0, D, (n,), generator=gen).int().cuda()
    f_d = feat.cuda()
    exact = ops.mlp(pm, f_d, dirs, amap, "mfma")
    assert float(exact.std()) > 0.05                                   # the large biases do not saturate the sigmoid everywhere
    old = ops.AUX_TABLE
    try:
        ops.AUX_TABLE = False
        full = ops.mlp(pm, f_d, dirs, amap, "bf16x3")
        one = ops.mlp(pm, f_d, dirs, amap, "bf16")
        ops.AUX_TABLE = True
        tab = ops.mlp(pm, f_d, dirs, amap, "bf16x3")
    finally:
        ops.AUX_TABLE = old
    assert rel(full, exact) < 1e-5 and rel(tab, exact) < 1e-5
    small = env.model.renderModule.packed()
    base = rel(ops.mlp(small, f_d, dirs, amap, "bf16"), ops.mlp(small, f_d, dirs, amap, "mfma"))
    assert rel(one, exact) < max(2e-2, 3 * base), (rel(one, exact), base)


@torch.no_grad()
def test_high_precision_fused_indirect_kernel(env):
    """tir_indirect_fused_hp_fwd (the auto policy's first fallback, models/relight_utils.py:818-829 in one launch): against the
    exact route it stands in for -- fp32 gather + exact fp32 decoder -- on random records incl. points near / outside the borders,
    a multi-light index map, ragged and device-side counts.  Its deviation is the fp16 rounding of the ACTIVATIONS (random, zero
    mean: |max| < 3e-4, |mean| < 3e-6 per channel); the weight rounding of the fp16 kernel (a fixed perturbation) is gone: with the
    decoder's weights x8 (where the fp16 kernel's error grows ~8^2-fold) the mean deviation stays below the fp16 kernel's by > 4x."""
    import tensoir_amd
    from tensoir_amd import ops
    from tests.helpers import golden_checkpoint
    m = env.model
    gen = torch.Generator().manual_seed(12)
    D, npt = 16, 40
    dirs = torch.nn.functional.normalize(torch.randn(D, 3, generator=gen), dim=-1).cuda()
    lpt = torch.randint(0, m.light_num, (npt,), generator=gen).int().cuda()

    def routes(model, npts):
        fld, pm = model.packed_field(), model.renderModule.packed()
        pts = (torch.rand(npts, 3, generator=gen) * 1.9 - 0.95).cuda()
        pair = torch.randint(0, npt * D, (npts,), generator=gen).int().cuda()            # pair id: point = id // D, direction = id % D
        exact = ops.mlp(pm, ops.vm_app(fld, pts, lpt, pair, True, False, None, D)[0], dirs, pair, "mfma", D)
        hp = ops.indirect_fused_hp(fld, pm, pts, lpt, pair, D, dirs, D)
        return fld, pm, pts, pair, exact, hp
    for npts in (1, 37, 255, 5003, 70001):
        fld, pm, pts, pair, exact, hp = routes(m, npts)
        assert hp.shape == (npts, 3) and bool(torch.isfinite(hp).all())
        # bit-reproducible from launch to launch (a packed-fp32 form of the product chains was not: a few records of the last 16
        # lanes of a wave changed from run to run)
        assert torch.equal(hp, ops.indirect_fused_hp(fld, pm, pts, lpt, pair, D, dirs, D)), npts
        d = (hp - exact).double()
        assert float(d.abs().max()) < 3e-4, (npts, float(d.abs().max()))
        if npts > 1000:
            assert float(d.mean(0).abs().max()) < 3e-6, (npts, d.mean(0))
        if npts > 10:
            n_dev = torch.tensor([npts - 7], dtype=torch.int32, device="cuda")
            part = ops.indirect_fused_hp(fld, pm, pts, lpt, pair, D, dirs, D, n_dev)
            assert torch.equal(part[:npts - 7], hp[:npts - 7])
    # larger decoder weights: the fp16 kernel's systematic part (weight rounding) against the hp kernel's
    ck = golden_checkpoint(env.g)
    for layer in (0, 2):
        ck["state_dict"][f"renderModule.mlp.{layer}.weight"] = ck["state_dict"][f"renderModule.mlp.{layer}.weight"] * 8.0
    eh, ew = [int(x) for x in env.g["scene/envmap_hw"]]
    m8 = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=eh, envmap_w=ew)
    fld, pm, pts, pair, exact, hp = routes(m8, 70001)
    f16 = ops.indirect_fused(fld, m8.packed_field_half(), pm, pts, lpt, pair, D, dirs, D)
    e_hp, e_16 = (hp - exact).double(), (f16 - exact).double()
    assert float(e_hp.pow(2).mean().sqrt()) < float(e_16.pow(2).mean().sqrt())
    assert float(e_hp.mean(0).abs().max()) * 4 < max(float(e_16.mean(0).abs().max()), 4e-6), (e_hp.mean(0), e_16.mean(0))


@torch.no_grad()
def test_indirect_precision_policy_kernels(env):
    """The two launches of the indirect-light precision policy, each against the parity-grade kernel it replaces
    on the secondary-ray records:
    * tir_mlp_fwd_auxtab_f16 (single-product fp16 decoder, operands rounded to 11 bits): |rgb - exact| < 2e-4 on every row
      (measured ~4e-5 max, 7e-6 rms), unbiased (|mean| < 2e-6), finite for feature / activation magnitudes beyond the fp16
      range (operands saturate at 65504 instead of turning into inf), ragged and device-side row counts;
    * tir_vm_app_fwd_h16 (fp16 shadow of the appearance planes / lines, interpolation and products on the packed fp16 pipe,
      fp16 basis contraction): |feat - fp32 gather| < 4e-3 of the feature scale on every element (measured 1e-3), padding
      columns zero, index-map / idx_div / n_dev forms;
    and the policy switch itself: `full` reproduces the primary-stage kernels bit for bit."""
    from tensoir_amd import ops
    m = env.model
    pm = m.renderModule.packed()
    gen = torch.Generator().manual_seed(11)
    for n, D in ((255, 3), (4099, 16), (70001, 128)):
        feat = torch.zeros(n, 32)
        feat[:, :27] = torch.randn(n, 27, generator=gen) * 0.8
        dirs = torch.nn.functional.normalize(torch.randn(D, 3, generator=gen), dim=-1).cuda()
        amap = torch.randint(0, 10 * D, (n,), generator=gen).int().cuda()
        f_d = feat.cuda()
        exact = ops.mlp(pm, f_d, dirs, amap, "mfma", D)
        half = ops.mlp(pm, f_d, dirs, amap, "f16", D)
        d = (half - exact).double()
        assert float(d.abs().max()) < 2e-4 and abs(float(d.mean())) < 2e-6, (n, D, float(d.abs().max()), float(d.mean()))
        n_dev = torch.tensor([max(1, n - 5)], dtype=torch.int32, device="cuda")
        part = ops.mlp(pm, f_d, dirs, amap, "f16", D, n_dev)
        assert torch.equal(part[:n - 5], half[:n - 5])
    big = f_d * 1.0e6                                                  # far outside fp16: operands saturate, nothing turns into NaN / inf
    assert bool(torch.isfinite(ops.mlp(pm, big, dirs, amap, "f16", D)).all())
    # ---- the gather
    xyz, li = G(env, "feat/xyz"), G(env, "feat/light_idx")
    fld, fh = m.packed_field(), m.packed_field_half()
    assert fh is not None
    r32 = ops.vm_app(fld, xyz, li, None, True, False)[0]
    r16 = ops.vm_app_h16(fld, fh, xyz, li)
    scale = float(r32[:, :27].abs().max())
    assert float((r16 - r32)[:, :27].abs().max()) < 4e-3 * scale and bool((r16[:, 27:] == 0).all())
    assert rel(r16[:, :27], env.g["feat/app"]) < 4e-3 * max(1.0, scale)          # and against the reference's own features
    pts = (torch.rand(5003, 3, generator=gen) * 1.9 - 0.95).cuda()              # incl. points near / outside the borders
    npt = 40
    lpt = torch.randint(0, m.light_num, (npt,), generator=gen).int().cuda()
    imap = torch.randint(0, npt * 7, (5003,), generator=gen).int().cuda()        # pair ids: light index of point id // 7
    a32 = ops.vm_app(fld, pts, lpt, imap, True, False, None, 7)[0]
    a16 = ops.vm_app_h16(fld, fh, pts, lpt, imap, 7)
    assert float((a16 - a32).abs().max()) < 4e-3 * max(float(a32.abs().max()), 1e-6)
    n_dev = torch.tensor([4000], dtype=torch.int32, device="cuda")
    assert torch.equal(ops.vm_app_h16(fld, fh, pts, lpt, imap, 7, n_dev)[:4000], a16[:4000])
    # ---- the fused launch (gather -> basis contraction -> decoder, features in registers) against the two launches it replaces
    D = 16
    dirs = torch.nn.functional.normalize(torch.randn(D, 3, generator=gen), dim=-1).cuda()
    for npts in (1, 255, 5003):
        pts_f = (torch.rand(npts, 3, generator=gen) * 1.9 - 0.95).cuda()
        pair = torch.randint(0, npt * D, (npts,), generator=gen).int().cuda()            # pair id: point = id // D, direction = id % D
        two = ops.mlp(pm, ops.vm_app_h16(fld, fh, pts_f, lpt, pair, D), dirs, pair, "f16", D) if D * 8 <= npts else None
        one = ops.indirect_fused(fld, fh, pm, pts_f, lpt, pair, D, dirs, D)
        assert one.shape == (npts, 3) and bool(torch.isfinite(one).all())
        if two is not None:
            assert float((one - two).abs().max()) < 1e-5, (npts, float((one - two).abs().max()))
        exact = ops.mlp(pm, ops.vm_app(fld, pts_f, lpt, pair, True, False, None, D)[0], dirs, pair, "mfma", D)
        assert float((one - exact).abs().max()) < 5e-4, (npts, float((one - exact).abs().max()))      # the policy's precision class
        if npts > 10:
            n_dev = torch.tensor([npts - 7], dtype=torch.int32, device="cuda")
            part = ops.indirect_fused(fld, fh, pm, pts_f, lpt, pair, D, dirs, D, n_dev)
            assert torch.equal(part[:npts - 7], one[:npts - 7])
    # ---- the switch: `full` = the primary-stage kernels
    from tensoir_amd import Renderer_TensoIR_train
    rays, lidx = G(env, "rays/rays"), G(env, "rays/light_idx")
    kw = dict(N_samples=-1, white_bg=True, is_train=False, is_relight=True, sample_method="fixed_envirmap", device="cuda", args=env.args)
    old = ops.SECONDARY_MLP_IMPL, ops.SECONDARY_APP_IMPL
    try:
        ops.SECONDARY_MLP_IMPL, ops.SECONDARY_APP_IMPL = "f16", "h16"
        old_fused = ops.FUSED_INDIRECT
        try:
            ops.FUSED_INDIRECT = False
            unfused = Renderer_TensoIR_train(rays, None, lidx, m, **kw)
            ops.FUSED_INDIRECT = True
            pol = Renderer_TensoIR_train(rays, None, lidx, m, **kw)
        finally:
            ops.FUSED_INDIRECT = old_fused
        assert float((pol["rgb_with_brdf_map"] - unfused["rgb_with_brdf_map"]).abs().max()) < 2e-6
        ops.SECONDARY_MLP_IMPL, ops.SECONDARY_APP_IMPL = None, None
        full = Renderer_TensoIR_train(rays, None, lidx, m, **kw)
    finally:
        ops.SECONDARY_MLP_IMPL, ops.SECONDARY_APP_IMPL = old
    for k in ("rgb_map", "normal_map", "albedo_map", "acc_map", "depth_map"):
        assert torch.equal(pol[k], full[k]), k                         # the policy touches indirect light only
    assert float((pol["rgb_with_brdf_map"] - full["rgb_with_brdf_map"]).abs().max()) < 1e-5


@torch.no_grad()
def test_decoder_aux_table_variant(env):
    """The aux-table variant of the radiance decoder (tir_mlp_aux_table + tir_mlp_fwd_auxtab_bf16x3: the view direction's 15
    input columns and the bias as a per-direction start value of the layer-1 accumulators, 9 k-blocks of matrix work instead
    of 10): (a) against the reference's own outputs (tests/golden mlp/rgb) when every row has its own aux row; (b) through an
    index map and through `aux_mod` (rows >> distinct directions: what the renderer launches) against the exact-fp32 decoder
    and the full split-bf16 one; (c) inside the multi-decoder launch; ragged row counts, a device-side row count."""
    from tensoir_amd import ops
    m = env.model
    pm = m.renderModule.packed()
    r, vd = G(env, "feat/both_rad"), G(env, "mlp/viewdirs")
    n0 = r.shape[0]
    assert ops.AUX_TABLE
    # (a) one table row per decoder row (identity map)
    table = ops.mlp_aux_table(pm, vd)
    assert table.shape == (n0, 128)
    out = torch.empty((n0, 3), dtype=torch.float32, device="cuda")
    ops._call("tir_mlp_fwd_auxtab_bf16x3", C.byref(pm.desc), ops._ptr(r.contiguous()), r.shape[1], ops._ptr(table), None, 0,
              ops._ptr(out), n0, None, ops._stream())
    assert rel(out, env.g["mlp/rgb"]) < 1e-5
    # (b) many rows, few directions
    gen = torch.Generator().manual_seed(77)
    for n, D in ((1, 1), (255, 3), (4099, 16), (70001, 128)):
        feat = torch.zeros(n, 32)
        feat[:, :27] = torch.randn(n, 27, generator=gen) * 0.8
        dirs = torch.nn.functional.normalize(torch.randn(D, 3, generator=gen), dim=-1)
        amap = torch.randint(0, 10 * D, (n,), generator=gen).int()          # pair ids: direction = id mod D
        f_d, d_d, a_d = feat.cuda(), dirs.cuda(), amap.cuda()
        exact = ops.mlp(pm, f_d, d_d, a_d, "mfma", D)
        old = ops.AUX_TABLE
        try:
            ops.AUX_TABLE = False
            full = ops.mlp(pm, f_d, d_d, a_d, "bf16x3", D)
            ops.AUX_TABLE = True
            tab = ops.mlp(pm, f_d, d_d, a_d, "bf16x3", D) if D * 8 <= n else None
            n_dev = torch.tensor([max(1, n - 3)], dtype=torch.int32, device="cuda")
            part = ops.mlp(pm, f_d, d_d, a_d, "bf16x3", D, n_dev) if D * 8 <= n else None
        finally:
            ops.AUX_TABLE = old
        assert rel(full, exact) < 1e-5
        if tab is not None:
            assert rel(tab, exact) < 1e-5 and rel(tab, full) < 1e-5, (n, D)
            k = max(1, n - 3)
            assert torch.equal(part[:k], tab[:k])
    # (c) the multi-decoder launch: job 0 mapped (table variant), the others with per-row aux
    n = 3001
    feat = torch.zeros(n, 32)
    feat[:, :27] = torch.randn(n, 27, generator=gen) * 0.8
    rays_d = torch.nn.functional.normalize(torch.randn(40, 3, generator=gen), dim=-1).cuda()
    rmap = torch.randint(0, 40, (n,), generator=gen).int().cuda()
    pts = (torch.rand(n, 3, generator=gen) * 2 - 1).cuda()
    f_d = feat.cuda()
    jobs = [(pm, f_d, rays_d, rmap), (m.renderModule_brdf.packed(), f_d, pts, None), (m.renderModule_normal.packed(), f_d, pts, None)]
    old_multi = ops.AUX_TABLE_MULTI
    try:
        ops.AUX_TABLE_MULTI = True
        got = ops.mlp_multi(jobs)
    finally:
        ops.AUX_TABLE_MULTI = old_multi
    want = [ops.mlp(pm, f_d, rays_d, rmap, "mfma"), ops.mlp(jobs[1][0], f_d, pts, None, "mfma"), ops.mlp(jobs[2][0], f_d, pts, None, "mfma")]
    for a, b in zip(got, want):
        assert rel(a, b) < 1e-5


@torch.no_grad()
def test_forward_vs_reference(env, decoder):
    rays, lidx = G(env, "rays/rays"), G(env, "rays/light_idx")
    out = env.model(rays, lidx)
    for n, a in zip(NAMES, out):
        if n == "acc_mask":
            assert bool((a.cpu().numpy() == env.g["fwd/acc_mask"]).all())
        elif not n.endswith("smoothness_loss"):        # those depend on the (device) jitter noise draw
            check_map(n, a, env.g["fwd/" + n])
    o = env.model(rays, lidx, is_relight=False)
    assert rel(o[0], env.g["fwd_norelight/rgb_map"]) < TOL and rel(o[1], env.g["fwd_norelight/depth_map"]) < TOL
    assert all(x is None for k, x in enumerate(o) if k not in (0, 1, 6))
    o = env.model(rays, lidx, white_bg=False, N_samples=57)
    for n, a in zip(NAMES, o):
        if n not in ("acc_mask", "albedo_smoothness_loss", "roughness_smoothness_loss"):
            check_map(n, a, env.g["fwd_blackbg57/" + n])


@torch.no_grad()
def test_smoothness_losses_vs_reference_golden(env):
    """albedo / roughness smoothness losses (models/tensorBase_rotated_lights.py:937-943, :858-863) against the reference's own
    values in the golden file, with the reference's jitter draw REPLAYED: its forward draws `torch.randn_like(xyz[app_mask])`
    from the CPU generator seeded SEED + 3 (oracle/make_golden.py) as the first RNG use of the pass, one row per w > 1e-4
    sample in (ray, sample) order -- the order of the HIP path's record list -- so the same rows scattered to the records'
    (ray, sample) positions feed `_brdf_jitter_dense`.  (The product draws its jitter on the device: Philox, another stream.)"""
    from tensoir_amd import ops
    m = env.model
    rays, lidx = G(env, "rays/rays"), G(env, "rays/light_idx")
    B, S = rays.shape[0], m.nSamples
    f = m.packed_field()
    weight, _acc, _depth, _tend, cnt = ops.march_primary(f, rays, None, S, 0.0)
    offsets = ops.exclusive_scan(cnt)
    A = int(offsets[-1])
    rec_ray, rec_k, _w, _xyz = ops.compact_primary(f, rays, None, weight, offsets, A)
    torch.manual_seed(20211202 + 3)
    sparse = torch.randn(A, 3)
    dense = torch.zeros(B, S, 3)
    dense[rec_ray.cpu().long(), rec_k.cpu().long()] = sparse
    for impl in ("bf16x3", "mfma"):
        old = ops.MLP_IMPL
        ops.MLP_IMPL = impl
        try:
            out = m(rays, lidx, _brdf_jitter_dense=dense)
        finally:
            ops.MLP_IMPL = old
        for name, got in (("albedo_smoothness_loss", out[10]), ("roughness_smoothness_loss", out[11])):
            ref = float(env.g["fwd/" + name])
            assert abs(float(got) - ref) <= 1e-4 * abs(ref) + 1e-9, (impl, name, float(got), ref)


@torch.no_grad()
def test_secondary_env_ggx_vs_reference(env, decoder):
    from tensoir_amd import relight
    m = env.model
    p, d, l = G(env, "sec/pts"), G(env, "sec/dirs"), G(env, "sec/light_idx")
    v, nf = relight.compute_transmittance(m, p, d, nSample=96, vis_near=0.05, vis_far=1.5)
    assert rel(v, env.g["sec/trans_vis"]) < TOL and rel(nf, env.g["sec/trans_nerfactor"]) < TOL
    v, nf, ind = relight.compute_radiance(m, p, d, l, nSample=96, vis_near=0.05, vis_far=1.5)
    assert rel(v, env.g["sec/rad_vis"]) < TOL and rel(ind, env.g["sec/rad_indirect"]) < TOL
    assert rel(m.get_light_rgbs(G(env, "env/dirs"), device=env.dev), env.g["env/light_rgbs"]) < 1e-5
    spec = relight.GGX_specular(G(env, "ggx/normal"), G(env, "ggx/v"), G(env, "ggx/l"), G(env, "ggx/rough"),
                                G(env, "ggx/fresnel"))
    assert rel(spec, env.g["ggx/spec"], 1e-3) < 1e-4


@torch.no_grad()
def test_renderer_boundary_vs_reference(env, decoder):
    from tensoir_amd import Renderer_TensoIR_train
    rays, lidx = G(env, "rays/rays").cpu(), G(env, "rays/light_idx").cpu()   # host tensors, as the reference passes
    ret = Renderer_TensoIR_train(rays, None, lidx, env.model, args=env.args, device=env.dev)
    assert sorted(ret) == sorted(k.split("/")[1] for k in env.g.files if k.startswith("render_fixed/"))
    for k, v in ret.items():
        if not k.endswith("smoothness_loss"):
            check_map(k, v, env.g["render_fixed/" + k])
    # stratified light directions: same CPU generator draws as the reference (randn on device differs,
    # it only feeds the smoothness losses)
    # The golden run had the reference on the CPU, where its randn_like [A,3] (:937) also consumed the
    # CPU generator before the two rand_like draws of gen_light_incident_dirs (:520); replay that.
    from tensoir_amd import ops
    cnt = ops.march_primary(env.model.packed_field(), rays.to(env.dev), None, env.model.nSamples, 0.0)[4]
    torch.manual_seed(20211202 + 5)
    torch.randn(int(cnt.sum()), 3)
    ret = Renderer_TensoIR_train(rays, None, lidx, env.model, args=env.args, device=env.dev,
                                 sample_method="stratified_sampling")
    assert rel(ret["rgb_with_brdf_map"], env.g["render_strat/rgb_with_brdf_map"]) < TOL


@torch.no_grad()
def test_importance_sampled_light_directions(env):
    """gen_light_incident_dirs(method='importance_sample') (models/tensorBase_rotated_lights.py:547-572) against
    tests/golden/importance_sample.npz (the reference's own tables, oracle/make_golden_importance.py).  The jitter of the
    128 x 256 direction table comes from the CPU generator -> same seed, same table; the indices are drawn on the device
    (torch.multinomial on a CUDA tensor, as the reference does on a GPU), so what is pinned is: every returned direction is a
    row of the reference's table, its radiance and pdf are the reference's values for that row, and the drawn rows follow the
    reference's sampling pdf (chi-square over 16 x 16-cell blocks)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "importance_sample.npz"))
    m = env.model
    n = 1 << 16
    torch.manual_seed(int(g["seed"][0]))
    torch.cuda.manual_seed(11)
    d, rgb, pdf = m.gen_light_incident_dirs(sample_number=n, method="importance_sample", device="cuda")
    assert d.shape == (n, 3) and rgb.shape == (n, 3) and pdf.shape == (n, 1) and d.is_cuda
    vd = torch.from_numpy(g["view_dirs"]).cuda()
    # nearest table row in fp64: next to the poles neighbouring rows are 1.5e-4 apart, closer than the noise of an fp32 GEMM whose
    # kernel choice varies from box to box (an fp32 product picked the neighbour on one box of the pool: 1.3e-4 "error")
    idx = torch.cat([(c.double() @ vd.double().T).argmax(dim=1) for c in torch.split(d, 4096)])
    assert float((d - vd[idx]).abs().max()) < 2e-6                       # rows of the reference's jittered table
    env_ref = torch.from_numpy(g["envir_map"]).cuda()[idx]
    assert float(((rgb - env_ref).abs() / env_ref.abs().clamp(min=1.0)).max()) < 1e-5
    pc = torch.from_numpy(g["pdf_to_compute"]).cuda()[idx]
    assert float(((pdf.view(-1) - pc).abs() / pc.clamp(min=1e-6)).max()) < 1e-4
    # distribution of the drawn rows: counts per block of 16 x 16 cells vs n * (block mass of the reference's pdf_to_sample)
    blk = lambda t: t.view(8, 16, 16, 16).sum(dim=(1, 3)).reshape(-1)
    expect = blk(torch.from_numpy(g["pdf_to_sample"]).double()) * n
    counts = blk(torch.bincount(idx.cpu(), minlength=128 * 256).double())
    keep = expect > 20
    chi = float((((counts - expect) ** 2 / expect)[keep]).sum() / max(1, int(keep.sum()) - 1))
    assert chi < 1.4, chi
    d2, _, _ = m.gen_light_incident_dirs(sample_number=64, method="importance_sample", device="cuda")
    assert d2.shape == (64, 3)


@torch.no_grad()
def test_hdr_relight_vs_reference(env):
    from tensoir_amd import relight
    out = relight.relight_with_envmap(env.model, G(env, "hdr/surf"), G(env, "hdr/normal"), G(env, "hdr/albedo"),
                                      G(env, "hdr/rough"), G(env, "hdr/fresnel"), G(env, "hdr/rays_d"),
                                      G(env, "hdr/light_dir"), G(env, "hdr/light_rgb"), G(env, "hdr/light_pdf"))
    assert rel(out, env.g["hdr/relit"]) < TOL
    el = relight.Environment_Light(hdr_maps={"syn": env.g["hdr/map"]}, device=env.dev)
    assert rel(el.hdr_pdf_return["syn"], env.g["hdr/pdf_return"], 1e-3) < 1e-4
    d, rgb, pdf = el.sample_light("syn", 7, 64)
    assert d.shape == (7, 64, 3) and rgb.shape == (7, 64, 3) and pdf.shape == (7, 64, 1)
    assert rel(el.get_light("syn", G(env, "rays/rays")[:, 3:]), env.g["hdr/bg"], 1e-2) < 1e-4
    # sample_type="uniform" (models/relight_utils.py:144-146, :174-188): cells drawn uniformly in SOLID ANGLE, returned pdf 1 / 4 pi
    # (exactly: 1 / (2 pi^2 mean(sin theta)) on the map's rows); directions average to zero, z^2 to 1/3
    torch.manual_seed(0)
    d, rgb, pdf = el.sample_light("syn", 64, 512, sample_type="uniform")
    assert d.shape == (64, 512, 3) and rgb.shape == (64, 512, 3) and pdf.shape == (64, 512, 1)
    H = int(env.g["hdr/map"].shape[0])
    want = 1.0 / (2.0 * np.pi ** 2 * float(torch.sin(torch.linspace(0.5 / H, np.pi - 0.5 / H, H)).mean()))      # -> 1 / 4 pi as H grows
    assert float((pdf - want).abs().max()) < 1e-5 * want and abs(want - 1.0 / (4.0 * np.pi)) < 0.06 / (4.0 * np.pi)
    assert float(d.mean(dim=(0, 1)).abs().max()) < 2e-2 and abs(float(d[..., 2].pow(2).mean()) - 1.0 / 3.0) < 3e-2
    with pytest.raises(ValueError):
        el.sample_light("syn", 1, 1, sample_type="nope")


# ---------------------------------------------------------------- oracle on seeded inputs (mid size)
@pytest.fixture(scope="module")
def mid():
    import tensoir_amd
    from oracle import tensoir_oracle as O
    from tensoir_amd import synth
    from tests.helpers import scene_from_checkpoint
    ck = synth.make_checkpoint(grid=(96, 96, 96), seed=11, light_rotation=("000", "120", "240"))
    sc = scene_from_checkpoint(ck, 8, 16)
    O.update_alpha_mask(sc, (48, 48, 48))
    vol = sc.alpha_volume
    ck["alphaMask.shape"] = tuple(vol.shape)
    ck["alphaMask.mask"] = np.packbits(vol.bool().numpy().reshape(-1))
    ck["alphaMask.aabb"] = sc.alpha_aabb
    model = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=8, envmap_w=16)
    return types.SimpleNamespace(model=model, sc=sc, O=O, synth=synth)


@torch.no_grad()
@pytest.mark.parametrize("t_stop", [0.0, 1e-6])
def test_renderer_vs_oracle_mid_size(mid, t_stop, decoder):
    """Ragged batch (B not a multiple of 4, S not a multiple of 64), three lights, with and without
    early ray termination."""
    from tensoir_amd import Renderer_TensoIR_train, relight
    m = mid.model
    m.march_t_stop = t_stop
    rays = mid.synth.make_rays(21, 19)
    lidx = (torch.arange(rays.shape[0]) % 3).view(-1, 1).int()
    S = 200
    noise = torch.randn(rays.shape[0], S, 3, generator=torch.Generator().manual_seed(5))
    args = types.SimpleNamespace(second_nSample=96, second_near=0.05, second_far=1.5)
    out, maps = m(rays.cuda(), lidx.cuda(), N_samples=S, _brdf_jitter_dense=noise, _return_maps=True)
    mask = out[9]
    brdf = relight.shade_from_maps(m, maps, rays.cuda(), lidx.cuda(), "fixed_envirmap", args, acc_thres=0.5)[mask]
    ref = mid.O.renderer_train(mid.sc, rays, lidx, n_samples=S, brdf_jitter=noise)
    for n, a in zip(NAMES, out):
        if n == "acc_mask":
            assert bool((a.cpu() == (ref["acc_map"] > 0.5)).all())
        elif n.endswith("smoothness_loss"):
            assert rel(a, ref[n], 1e-9) < 1e-2
        else:
            check_map(n, a, ref[n])
    check_map("rgb_with_brdf_map", brdf, ref["rgb_with_brdf_map"][ref["acc_map"] > 0.5])
    m.march_t_stop = 1e-6


# ---------------------------------------------------------------- edge cases
@torch.no_grad()
def test_edge_cases(env):
    from tensoir_amd import Renderer_TensoIR_train, relight
    m, dev = env.model, env.dev
    # empty batch
    ret = Renderer_TensoIR_train(torch.zeros(0, 6), None, torch.zeros(0, 1, dtype=torch.int32), m, args=env.args, device=dev)
    assert ret["rgb_map"].shape == (0, 3) and ret["rgb_with_brdf_map"].shape == (0, 3)
    # rays that miss the volume: white background everywhere, no surface points, no records
    rays = torch.tensor([[0.0, 0.0, 4.0, 0.0, 0.0, 1.0], [5.0, 5.0, 5.0, 1.0, 0.0, 0.0], [0, 0, 4.0, 0.0, 1.0, 0.0]])
    ret = Renderer_TensoIR_train(rays, None, torch.zeros(3, 1, dtype=torch.int32), m, args=env.args, device=dev)
    assert torch.all(ret["acc_map"] == 0) and torch.allclose(ret["rgb_map"], torch.ones(3, 3, device=dev))
    assert torch.all(ret["rgb_with_brdf_map"] == 1) and torch.allclose(ret["normal_map"][:, 2], torch.ones(3, device=dev))
    # zero direction component (the vec==0 -> 1e-6 substitution of sample_ray) stays finite
    r = G(env, "rays/rays")[:5].clone(); r[:, 3] = 0.0
    out = m(r, torch.zeros(5, 1, dtype=torch.int32, device=dev))
    assert all(torch.isfinite(o).all() for o in out if torch.is_tensor(o) and o.dtype.is_floating_point)
    # secondary march limits: n_sample 1, 256 (max) and 257 (rejected)
    p, d = G(env, "sec/pts")[:9], G(env, "sec/dirs")[:9]
    for n in (1, 33, 256):
        v, nf = relight.compute_transmittance(m, p, d, nSample=n, vis_near=0.05, vis_far=1.5)
        assert v.shape == (9,) and torch.isfinite(v).all() and (v <= 1.0 + 1e-6).all()
    from tensoir_amd._lib import TensoirHipError
    with pytest.raises(TensoirHipError):
        relight.compute_transmittance(m, p, d, nSample=257, vis_near=0.05, vis_far=1.5)
    with pytest.raises(TensoirHipError):
        m.compute_densityfeature(torch.zeros(4, 3))          # CPU tensor: no fallback


@torch.no_grad()
def test_record_overflow_recovers(env):
    """Secondary records larger than the first capacity guess trigger a re-march, not a wrong answer."""
    from tensoir_amd import relight
    m = env.model
    p, d, l = G(env, "sec/pts"), G(env, "sec/dirs"), G(env, "sec/light_idx")
    m._rec_cap_hints = {p.shape[0]: 1}
    v, nf, ind = relight.compute_radiance(m, p, d, l, nSample=96, vis_near=0.05, vis_far=1.5)
    assert rel(ind, env.g["sec/rad_indirect"]) < TOL


@torch.no_grad()
@pytest.mark.parametrize("tier", ["f16", "hp", "full", "auto"])
def test_every_capacity_route_renders_the_same(env, tier):
    """The record-capacity protocol of relight._secondary never changes the result: the synchronising first call, the hinted
    call, the deferred check, an overflow that re-marches and a deferred overflow that makes the caller re-run all render
    bit-identical rows, under each forced tier and under auto (whose first call also establishes the verdict)."""
    from tensoir_amd import indirect, relight
    from tests import precision_cases as P
    m = env.model
    rays, lidx = G(env, "rays/rays"), G(env, "rays/light_idx")
    _, maps = m(rays, lidx, _return_maps=True)
    key = maps.shape[0] * m.fixed_viewdirs.shape[0]          # M * D secondary rays

    def shade(**kw):
        return relight.shade_from_maps(m, maps, rays, lidx, "fixed_envirmap", env.args, acc_thres=0.5, **kw)

    with P.policy(*{"f16": (False,), "hp": (False, "hp", None), "full": (False, None, None), "auto": (True,)}[tier]):
        indirect.reset(m)
        m.__dict__.pop("_rec_cap_hints", None)
        renders = {"first": shade()}                         # no hint: reads the count back, then sizes the buffers
        assert m._rec_cap_hints[key] > 1
        renders["hinted"] = shade()
        renders["deferred"] = shade(_defer_check=True)
        assert relight.finish_pending(m) is True
        m._rec_cap_hints[key] = 1
        renders["overflow"] = shade()                        # far too small: re-marches with room
        assert m._rec_cap_hints[key] > 1
        m._rec_cap_hints[key] = 1
        shade(_defer_check=True)                             # ... found by the deferred check: the caller re-runs
        assert relight.finish_pending(m) is False and key not in m._rec_cap_hints
        renders["re-run"] = shade()
        if tier == "auto":
            assert m.indirect_precision()["probes_run"] == 1
    assert torch.isfinite(renders["first"]).all() and float(renders["first"].min()) < 1.0      # (some ray hit the object)
    for name, r in renders.items():
        assert torch.equal(r, renders["first"]), (tier, name)


# ---------------------------------------------------------------- full size (BASELINE C2/C3) properties
@pytest.fixture(scope="module")
def full():
    import tensoir_amd
    from tensoir_amd import synth
    ck = synth.make_checkpoint(grid=(300, 300, 300), seed=20211202)
    model = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=8, envmap_w=16)
    with torch.no_grad():
        model.updateAlphaMask((128, 128, 128))
    rays = synth.make_rays(64, 64).cuda()
    return types.SimpleNamespace(model=model, rays=rays, lidx=torch.zeros(4096, 1, dtype=torch.int32, device="cuda"),
                                 args=types.SimpleNamespace(second_nSample=96, second_near=0.05, second_far=1.5))


@torch.no_grad()
def test_full_size_properties(full):
    """4096 rays x 512 samples, R=300: conservation, sharding invariance, determinism, decoder cross-check."""
    from tensoir_amd import Renderer_TensoIR_train, ops
    m, rays, lidx = full.model, full.rays, full.lidx
    f = m.packed_field()
    # (1) sum of weights + final transmittance == 1 (telescoping product; 1e-10 fudge aside)
    w, acc, depth, tend, cnt = ops.march_primary(f, rays, None, 512, 0.0)
    assert float((acc + tend - 1.0).abs().max()) < 2e-5
    assert float((w.sum(-1) - acc).abs().max()) < 2e-5
    assert int((cnt != (w > m.rayMarch_weight_thres).sum(-1)).sum()) == 0
    # (2) early termination changes nothing above its bound
    w2, acc2, depth2, _, cnt2 = ops.march_primary(f, rays, None, 512, 1e-6)
    assert float((acc2 - acc).abs().max()) < 3e-6 and float((depth2 - depth).abs().max()) < 2e-5
    assert torch.equal(cnt, cnt2)
    # (3) rays are independent: rendering two halves == rendering the batch, bit for bit; and repeatable
    noise = torch.randn(4096, 512, 3, generator=torch.Generator().manual_seed(1)).cuda()
    kw = dict(N_samples=512, args=full.args, device="cuda")
    import tensoir_amd.field_model as FM
    orig = FM.TensorVMSplit.forward
    def fwd(self, r, l, **k):
        sel = k.pop("_sel")
        return orig(self, r, l, _brdf_jitter_dense=noise[sel], **k)
    whole = orig(m, rays, lidx, N_samples=512, _brdf_jitter_dense=noise)
    again = orig(m, rays, lidx, N_samples=512, _brdf_jitter_dense=noise)
    lo = orig(m, rays[:2048], lidx[:2048], N_samples=512, _brdf_jitter_dense=noise[:2048])
    hi = orig(m, rays[2048:], lidx[2048:], N_samples=512, _brdf_jitter_dense=noise[2048:])
    for k in range(10):
        if whole[k] is None or whole[k].dim() == 0:
            continue
        assert torch.equal(whole[k], again[k]), NAMES[k]
        assert torch.equal(whole[k], torch.cat([lo[k], hi[k]])), NAMES[k]
    # (4) MFMA decoder == VALU decoder on the real sample set
    offsets = ops.exclusive_scan(cnt)
    A = int(offsets[-1])
    assert A > 100000
    rec_ray, rec_k, rec_w, rec_xyz = ops.compact_primary(f, rays, None, w, offsets, A)
    assert bool((rec_ray[1:] >= rec_ray[:-1]).all())                       # (ray, sample) order
    rad, intr = ops.vm_app(f, rec_xyz[:20000], lidx.view(-1), rec_ray[:20000], True, True)
    a = ops.mlp(m.renderModule_brdf.packed(), intr, rec_xyz[:20000], None, "mfma")
    b = ops.mlp(m.renderModule_brdf.packed(), intr, rec_xyz[:20000], None, "valu")
    c3 = ops.mlp(m.renderModule_brdf.packed(), intr, rec_xyz[:20000], None, "bf16x3")
    assert float((a - b).abs().max()) < 2e-6
    assert float((a - c3).abs().max()) < 2e-5          # split-bf16 matrix cores vs exact fp32
    # appearance gather: matrix-core kernel == one-sample-per-lane kernel
    r2, i2 = ops.vm_app(f, rec_xyz[:20000], lidx.view(-1), rec_ray[:20000], True, True, "valu")
    assert float((rad - r2).abs().max()) < 2e-6 and float((intr - i2).abs().max()) < 2e-6
    # (5) full boundary call: finite, in range, background white
    ret = Renderer_TensoIR_train(rays, None, lidx, m, **kw)
    for k, v in ret.items():
        assert torch.isfinite(v).all(), k
    assert float(ret["rgb_with_brdf_map"].min()) >= 0 and float(ret["rgb_with_brdf_map"].max()) <= 1.0 + 1e-6
    n = ret["normal_map"].norm(dim=-1)
    assert float((n[ret["acc_map"] > 0.5] - 1).abs().max()) < 1e-4


@torch.no_grad()
def test_record_capacity_hint_overflow_recovers(env):
    """Inference calls size the record buffers from the previous call's count and check afterwards; a hint that
    is too small must be detected and the pass redone (identical results, hint repaired)."""
    from tensoir_amd import Renderer_TensoIR_train
    m = env.model
    rays, lidx = G(env, "rays/rays"), G(env, "rays/light_idx")
    B, S = rays.shape[0], m.nSamples
    m.__dict__.pop("_app_cap_hints", None)
    kw = dict(N_samples=-1, white_bg=True, is_train=False, is_relight=True, sample_method="fixed_envirmap",
              device="cuda", args=env.args)
    first = Renderer_TensoIR_train(rays, None, lidx, m, **kw)            # exact route, learns the count
    assert (B, S) in m._app_cap_hints
    second = Renderer_TensoIR_train(rays, None, lidx, m, **kw)           # hinted route
    m._app_cap_hints[(B, S)] = 8                                         # far too small
    third = Renderer_TensoIR_train(rays, None, lidx, m, **kw)            # overflow -> redone
    assert m._app_cap_hints[(B, S)] > 8
    for k in ("rgb_map", "depth_map", "normal_map", "albedo_map", "acc_map", "rgb_with_brdf_map", "normals_diff_map"):
        assert torch.equal(first[k], second[k]), k
        assert torch.equal(first[k], third[k]), k


@torch.no_grad()
def test_occupancy_maintenance_on_device(env):
    """getDenseAlpha / updateAlphaMask / filtering_rays as device kernels vs the oracle / the
    reference's own formulation."""
    import copy
    import tensoir_amd
    from tests.helpers import golden_checkpoint
    O = __import__("oracle.tensoir_oracle", fromlist=["x"])
    eh, ew = [int(x) for x in env.g["scene/envmap_hw"]]
    m = tensoir_amd.model_from_checkpoint(golden_checkpoint(env.g), "cuda", envmap_h=eh, envmap_w=ew)
    sc = O.Scene(**env.sc.__dict__)
    grid = (22, 26, 30)
    # dense alpha lattice (with the existing mask culling)
    alpha, dense = m.getDenseAlpha(grid)
    a_ref, d_ref = O.dense_alpha(sc, grid)
    assert rel(dense, d_ref, 1.0) < 1e-6 and rel(alpha, a_ref, 1e-3) < 1e-3
    # new mask + bounding box
    aabb_new = m.updateAlphaMask(grid)
    ref_aabb = O.update_alpha_mask(sc, grid, thres=m.alphaMask_thres)
    vol = m.alphaMask.alpha_volume[0, 0].cpu()
    mism = int((vol != sc.alpha_volume).sum())
    assert mism <= max(2, vol.numel() // 2000), mism      # voxels within rounding of the 1e-3 threshold may flip
    if mism == 0:
        assert rel(aabb_new, ref_aabb, 1.0) < 1e-6
    # filtering_rays: both modes, vs the reference's formulation on the same model
    gen = torch.Generator().manual_seed(51)
    o = torch.randn(3000, 3, generator=gen) * 0.5 + torch.tensor([0.0, 0.0, 4.0])
    d = torch.nn.functional.normalize(torch.randn(3000, 3, generator=gen) * torch.tensor([0.6, 0.6, 0.3]) - torch.tensor([0, 0, 1.0]), dim=-1)
    rays = torch.cat([o, d], -1)
    rays[:5, 3] = 0.0                                      # zero direction components
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        kept, mask = m.filtering_rays(rays, N_samples=80, bbox_only=False)
        kept_b, mask_b = m.filtering_rays(rays, bbox_only=True)
    r = rays.cuda()
    xyz, _, _ = m.sample_ray(r[:, :3], r[:, 3:6], N_samples=80, is_train=False)
    ref = (m.alphaMask.sample_alpha(xyz).view(xyz.shape[:-1]) > 0).any(-1).cpu()
    assert torch.equal(mask, ref) and kept.shape[0] == int(ref.sum())
    vec = torch.where(r[:, 3:6] == 0, torch.full_like(r[:, 3:6], 1e-6), r[:, 3:6])
    ra, rb = (m.aabb[1] - r[:, :3]) / vec, (m.aabb[0] - r[:, :3]) / vec
    ref_b = (torch.maximum(ra, rb).amin(-1) > torch.minimum(ra, rb).amax(-1)).cpu()
    assert torch.equal(mask_b, ref_b)


@torch.no_grad()
def test_occupancy_maintenance_vs_reference_golden(env):
    """The same device kernels against tests/golden/mask_maintenance.npz, which the IMPORTED REFERENCE wrote
    (oracle/make_golden_general.py; models/tensorBase_rotated_lights.py:737-811): getDenseAlpha with and without an
    existing mask, updateAlphaMask (new volume, returned aabb, mask aabb), filtering_rays in both modes on the new mask,
    and a second update on top of the first (train_tensoIR.py:385-399)."""
    import contextlib
    import io
    import os
    import tensoir_amd
    from tests.helpers import golden_checkpoint
    mg = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_maintenance.npz"))
    R = lambda k: torch.from_numpy(np.array(mg[k]))
    eh, ew = [int(x) for x in env.g["scene/envmap_hw"]]
    ck = golden_checkpoint(env.g)
    grid = tuple(int(x) for x in mg["grid"])
    nomask = {k: v for k, v in ck.items() if not k.startswith("alphaMask")}
    m0 = tensoir_amd.model_from_checkpoint(nomask, "cuda", envmap_h=eh, envmap_w=ew)
    assert m0.alphaMask is None
    a, d = m0.getDenseAlpha(grid)
    assert rel(d, R("dense_xyz"), 1.0) < 1e-6 and float((a.cpu() - R("nomask/alpha")).abs().max()) < 2e-5
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=eh, envmap_w=ew)
    a, _ = m.getDenseAlpha(grid)
    assert float((a.cpu() - R("masked/alpha")).abs().max()) < 2e-5
    with contextlib.redirect_stdout(io.StringIO()):
        aabb = m.updateAlphaMask(grid)
    vol = m.alphaMask.alpha_volume[0, 0].cpu()
    assert vol.shape == R("update/volume").shape and int((vol != R("update/volume")).sum()) == 0
    assert rel(aabb, R("update/aabb"), 1.0) < 1e-6
    assert float((m.alphaMask.aabb.cpu() - R("update/mask_aabb")).abs().max()) == 0.0
    rays = R("filter/rays")
    with contextlib.redirect_stdout(io.StringIO()):
        kept, mask = m.filtering_rays(rays, N_samples=80, bbox_only=False)
        _, mask_b = m.filtering_rays(rays, bbox_only=True)
    assert torch.equal(mask.cpu(), R("filter/mask_alpha")) and torch.equal(kept.cpu(), R("filter/kept_alpha"))
    assert torch.equal(mask_b.cpu(), R("filter/mask_bbox"))
    with contextlib.redirect_stdout(io.StringIO()):
        aabb2 = m.updateAlphaMask((33, 29, 31))
    assert int((m.alphaMask.alpha_volume[0, 0].cpu() != R("update2/volume")).sum()) == 0
    assert rel(aabb2, R("update2/aabb"), 1.0) < 1e-6


@torch.no_grad()
def test_hip_graph_replay_matches_eager(env):
    """GraphedRenderer: one captured HIP graph per batch shape; identical maps to the eager path, also for a second
    batch of different rays, and an artificially small captured capacity is detected and re-captured."""
    from tensoir_amd import Renderer_TensoIR_train
    from tensoir_amd.graph import GraphedRenderer
    m = env.model
    rays, lidx = G(env, "rays/rays"), G(env, "rays/light_idx")
    kw = dict(N_samples=-1, white_bg=True, is_train=False, is_relight=True, sample_method="fixed_envirmap",
              device="cuda", args=env.args)
    gr = GraphedRenderer(m, rays.shape[0], args=env.args)
    keys = ("rgb_map", "depth_map", "normal_map", "albedo_map", "acc_map", "rgb_with_brdf_map", "normals_diff_map")
    for trial in range(3):
        r = rays.clone()
        if trial == 1:
            r[:, 3:6] = torch.nn.functional.normalize(r[:, 3:6] + 0.02 * torch.randn_like(r[:, 3:6]), dim=-1)
        if trial == 2:                                   # capture with too small a capacity -> overflow -> re-capture
            gr._test_shrink_capacity = 16
            gr.invalidate()
        want = Renderer_TensoIR_train(r, None, lidx, m, **kw)
        got = gr(r, lidx)
        for k in keys:
            assert torch.equal(got[k], want[k]), (trial, k)
    assert gr.captures >= 3
    # static-buffer use: inputs written straight into the graph's buffers, outputs returned without copies
    gr.rays.copy_(rays)
    gr.lidx.copy_(lidx.view(-1, 1))
    want = Renderer_TensoIR_train(rays, None, lidx, m, **kw)
    got = gr(clone_outputs=False)
    assert got["rgb_map"].data_ptr() == gr.out["rgb_map"].data_ptr()
    for k in keys:
        assert torch.equal(got[k], want[k]), k
    # deferred capacity check: replays are queued without a host wait, validate() reports on all of them
    for _ in range(3):
        got = gr(clone_outputs=False, defer_check=True)
    assert gr.validate()
    for k in keys:
        assert torch.equal(got[k], want[k]), k
    gr._test_shrink_capacity = 16                        # a capture whose capacity is too small: validate() must say so
    gr.invalidate()
    gr(clone_outputs=False, defer_check=True)
    gr(clone_outputs=False, defer_check=True)
    assert not gr.validate()
    got = gr(clone_outputs=False)                        # re-captured with room
    for k in keys:
        assert torch.equal(got[k], want[k]), k
    # staleness: a parameter update after the capture (optimizer step, upsample, new mask ...) is detected at the next
    # call and the graph is captured again -- a replay never reads freed or outdated tables
    caps = gr.captures
    saved = m.density_plane[0].detach().clone()
    try:
        m.density_plane[0].mul_(1.5)
        want2 = Renderer_TensoIR_train(rays, None, lidx, m, **kw)
        got2 = gr(rays, lidx)
        assert gr.captures == caps + 1
        for k in keys:
            assert torch.equal(got2[k], want2[k]), k
        assert not torch.equal(want2["acc_map"], want["acc_map"])
    finally:
        m.density_plane[0].copy_(saved)
    got3 = gr(rays, lidx)
    for k in keys:
        assert torch.equal(got3[k], want[k]), k


@torch.no_grad()
def test_boundary_call_replays_a_cached_graph(env, monkeypatch):
    """Renderer_TensoIR_train itself (renderer.py:57-127, what the unmodified scripts' evaluation loops call chunk after chunk,
    :225-249): from the second call of a shape on, an inference call replays a cached HIP graph -- identical maps, fresh output
    tensors, host rays accepted; small / training / gradient-enabled calls never use it; a parameter update re-captures; the
    switch turns it off."""
    from tensoir_amd import Renderer_TensoIR_train, renderer
    m = env.model
    m.__dict__.pop("_boundary_graphs", None)
    rays0, lidx0 = G(env, "rays/rays"), G(env, "rays/light_idx")
    rep = (1100 + rays0.shape[0] - 1) // rays0.shape[0]
    rays = rays0.repeat(rep, 1)[:1100].clone()
    gen = torch.Generator().manual_seed(3)
    rays[:, 3:6] = torch.nn.functional.normalize(rays[:, 3:6] + 0.01 * torch.randn(1100, 3, generator=gen).cuda(), dim=-1)
    lidx = lidx0.repeat(rep, 1)[:1100].contiguous()
    kw = dict(N_samples=-1, white_bg=True, is_train=False, is_relight=True, sample_method="fixed_envirmap", device="cuda", args=env.args)
    keys = ("rgb_map", "depth_map", "normal_map", "albedo_map", "acc_map", "rgb_with_brdf_map", "normals_diff_map")
    want = Renderer_TensoIR_train(rays, None, lidx, m, _no_graph=True, **kw)
    assert "_boundary_graphs" not in m.__dict__
    outs = [Renderer_TensoIR_train(rays.cpu(), None, lidx.cpu(), m, **kw) for _ in range(3)]      # host rays, as the scripts pass them
    cache = m.__dict__["_boundary_graphs"]
    (entry,) = cache.values()
    assert entry[0] is not None and entry[0].captures == 1 and entry[2] == 3
    for o in outs:
        for k in keys:
            assert torch.equal(o[k], want[k]), k
    assert outs[1]["rgb_map"].data_ptr() != outs[2]["rgb_map"].data_ptr()                          # a caller may keep what it got
    Renderer_TensoIR_train(rays[:100], None, lidx[:100], m, **kw)                                  # too small to be worth a graph
    with torch.enable_grad():
        Renderer_TensoIR_train(rays, None, lidx, m, **kw)                                          # gradient mode: the eager route
    assert len(cache) == 1 and entry[2] == 3
    saved = m.density_plane[0].detach().clone()
    try:
        m.density_plane[0].mul_(1.5)                                                               # new parameter version: captured again
        want2 = Renderer_TensoIR_train(rays, None, lidx, m, _no_graph=True, **kw)
        got2 = Renderer_TensoIR_train(rays, None, lidx, m, **kw)
        assert entry[0].captures == 2
        for k in keys:
            assert torch.equal(got2[k], want2[k]), k
    finally:
        m.density_plane[0].copy_(saved)
    monkeypatch.setattr(renderer, "BOUNDARY_GRAPHS", False)
    off = Renderer_TensoIR_train(rays, None, lidx, m, **kw)
    assert entry[2] == 4
    for k in keys:
        assert torch.equal(off[k], want[k]), k
    m.__dict__.pop("_boundary_graphs", None)


@torch.no_grad()
@pytest.mark.parametrize("impl", ["mfma", "valu", "bf16x3", "x3"])
def test_app_feature_implementations_vs_reference(env, impl):
    """All three appearance-contraction kernels (exact fp32 MFMA, VALU, split-bf16 MFMA) against the golden features,
    with both outputs, one output, an index map and ragged sizes."""
    from tensoir_amd import ops
    f = env.model.packed_field()
    xyz, li = G(env, "feat/xyz"), G(env, "feat/light_idx").view(-1).int()
    for n in (600, 599, 17, 1):
        r, i = ops.vm_app(f, xyz[:n], li[:n], None, True, True, impl)
        assert rel(r[:, :27], env.g["feat/both_rad"][:n]) < 2e-5 and rel(i[:, :27], env.g["feat/both_int"][:n]) < 2e-5
        assert float(r[:, 27:].abs().max()) == 0.0
    r = ops.vm_app(f, xyz, li, None, True, False, impl)[0]
    i = ops.vm_app(f, xyz, None, None, False, True, impl)[1]
    assert rel(r[:, :27], env.g["feat/app"]) < 2e-5 and rel(i[:, :27], env.g["feat/intrin"]) < 2e-5
    perm = torch.randperm(600, generator=torch.Generator().manual_seed(3)).int().cuda()
    r = ops.vm_app(f, xyz, li[perm.long()].contiguous(), torch.argsort(perm).int(), True, False, impl)[0]   # light_idx[idx_map[p]]
    assert rel(r[:, :27], env.g["feat/app"]) < 2e-5


@torch.no_grad()
def test_split_bf16_decoder_large_arguments(env):
    """The split-bf16 decoder's own sincos (Cody-Waite + polynomials, double-precision pre-reduction beyond |x| = 8192)
    against the exact-fp32 kernel (library sinf/cosf) on features far outside the usual range."""
    from tensoir_amd import ops
    m = env.model
    gen = torch.Generator().manual_seed(61)
    n = 3000
    feat = torch.zeros(n, 32)
    feat[:, :27] = torch.randn(n, 27, generator=gen) * torch.tensor([1.0, 10.0, 30.0]).repeat(9)
    feat[:100, :27] *= torch.tensor([30.0, 300.0, 3000.0]).repeat(9)   # up to ~3e5: incl. the double-precision pre-reduction
    aux = torch.randn(n, 3, generator=gen) * 3.0
    for dec in (m.renderModule, m.renderModule_brdf, m.renderModule_normal):
        a = ops.mlp(dec.packed(), feat.cuda(), aux.cuda(), None, "bf16x3")
        b = ops.mlp(dec.packed(), feat.cuda(), aux.cuda(), None, "mfma")
        # |feature| <~ 100: the split keeps 16 mantissa bits of every input -> 1e-4 * 100 * 2^-17 ... measured << 5e-5
        assert float((a[100:] - b[100:]).abs().max()) < 5e-5
        # huge raw features: the hi+lo split itself (2^-17 relative on inputs of 1e5) bounds the agreement, not the sincos
        assert torch.isfinite(a).all() and float((a[:100] - b[:100]).abs().max()) < 0.2


# ---------------------------------------------------------------- BASELINE configs C4 / C5 at full size (properties)
@pytest.fixture(scope="module")
def full3():
    """300^3 field with the three light rotations of configs[3] (multi_light_rotated)."""
    import tensoir_amd
    from tensoir_amd import synth
    ck = synth.make_checkpoint(grid=(300, 300, 300), seed=20211202, light_rotation=("000", "120", "240"))
    model = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=8, envmap_w=16)
    with torch.no_grad():
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            model.updateAlphaMask((128, 128, 128))
    return types.SimpleNamespace(model=model, args=types.SimpleNamespace(second_nSample=96, second_near=0.05, second_far=1.5))


@torch.no_grad()
def test_c4_full_image_800x800_sharded_render(full3):
    """configs[3]: 800x800 image = 640 000 rays in 157 chunks, light index = pixel mod 3, rendered through
    dist.render_sharded (the per-image record path of the 8-GPU layout; world = 1 here).  Properties: every map
    finite and in range, background white, the assembled image equals direct chunk renders bit for bit (first, a
    middle and the last, ragged, chunk), rotating the light changes the relit colour but not the geometry maps."""
    from tensoir_amd import Renderer_TensoIR_train, synth
    from tensoir_amd import dist as tdist
    m, args = full3.model, full3.args
    rays = synth.make_rays(800, 800, narrow=1.0).cuda()          # full field of view: the corners miss the object
    n = rays.shape[0]
    lidx = (torch.arange(n, device="cuda") % 3).to(torch.int32).view(-1, 1)
    kw = dict(N_samples=-1, white_bg=True, is_train=False, is_relight=True, sample_method="fixed_envirmap",
              device="cuda", args=args)

    def render(r, l):
        return Renderer_TensoIR_train(r, None, l, m, **kw)
    img = tdist.render_sharded(render, rays, lidx, rank=0, world=1, chunk=4096)
    for k, v in img.items():
        assert v.shape[0] == n and bool(torch.isfinite(v).all()), k
    acc = img["acc_map"]
    assert float(acc.min()) >= 0.0 and float(acc.max()) <= 1.0 + 1e-5
    for k in ("rgb_map", "rgb_with_brdf_map", "albedo_map"):
        assert float(img[k].min()) >= 0.0 and float(img[k].max()) <= 1.0 + 1e-6, k
    bgd = acc < 1e-6
    assert int(bgd.sum()) > 1000 and float((img["rgb_map"][bgd] - 1.0).abs().max()) < 1e-6     # corners: white background
    assert float((img["rgb_with_brdf_map"][acc <= 0.5] - 1.0).abs().max()) == 0.0
    hit = acc > 0.5
    assert int(hit.sum()) > 100000
    assert float((img["normal_map"][hit].norm(dim=-1) - 1).abs().max()) < 1e-4
    chunks = list(torch.split(torch.arange(n, device="cuda"), 4096))
    assert len(chunks) == 157 and chunks[-1].numel() == 640000 - 156 * 4096
    for ci in (0, 78, 156):
        c = chunks[ci]
        direct = render(rays[c], lidx[c])
        for k in ("rgb_map", "depth_map", "normal_map", "acc_map", "rgb_with_brdf_map"):
            assert torch.equal(img[k][c], direct[k]), (ci, k)
    # a different light rotation: same geometry / material maps, different shading
    c = chunks[78]
    other = render(rays[c], (lidx[c] + 1) % 3)
    for k in ("depth_map", "normal_map", "albedo_map", "roughness_map", "acc_map"):
        assert torch.equal(img[k][c], other[k]), k
    assert float((img["rgb_with_brdf_map"][c] - other["rgb_with_brdf_map"]).abs().max()) > 1e-4


@torch.no_grad()
def test_c5_hdr_relight_2048x1024_importance_512(full3):
    """configs[4]: relighting with a 2048x1024 HDR environment map and 512 importance samples per surface point
    (scripts/relight_importance.py:115-171) on a 4096-ray chunk.  Properties: pdf tables normalised, sampled
    directions unit length and concentrated on the bright disc, output finite / in [0,1] / deterministic for fixed
    samples, exactly black under a black map, non-decreasing when the map is scaled up."""
    from tensoir_amd import relight, synth
    m, args = full3.model, full3.args
    gen = torch.Generator().manual_seed(71)
    H, W = 1024, 2048
    hdr = torch.exp(torch.randn(H // 8, W // 8, 3, generator=gen) * 1.5)
    hdr = torch.nn.functional.interpolate(hdr.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).contiguous()
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sun = ((yy - 300) ** 2 + (xx - 700) ** 2) < 20 ** 2
    hdr[sun] *= 100.0
    env = relight.Environment_Light(hdr_maps={"syn": hdr, "black": torch.zeros_like(hdr), "dim": hdr * 0.25}, device="cuda")
    assert abs(float(env.hdr_pdf_sample["syn"].sum()) - 1.0) < 1e-4
    rays = synth.make_rays(64, 64).cuda()
    lidx = torch.zeros(4096, 1, dtype=torch.int32, device="cuda")
    out = m(rays, lidx, N_samples=512)
    depth, normal, albedo, rough, fres, acc = out[1], out[2], out[3], out[4], out[5], out[6]
    mask = acc > 0.5
    M, Ns = int(mask.sum()), 512
    assert M > 3000
    surf = (rays[:, :3] + depth.unsqueeze(-1) * rays[:, 3:])[mask]
    torch.manual_seed(5)
    ldir, lrgb, lpdf = env.sample_light("syn", M, Ns)
    assert ldir.shape == (M, Ns, 3) and float((ldir.norm(dim=-1) - 1).abs().max()) < 1e-5
    # importance sampling: the sun disc holds ~1e-4 of the pixels but a large share of the energy
    sun_dir = env.hdr_dir["syn"][300, 700]
    frac_sun = float(((ldir * sun_dir).sum(-1) > 0.995).float().mean())
    assert frac_sun > 0.02

    def relit(rgb, pdf):
        return relight.relight_with_envmap(m, surf, normal[mask], albedo[mask], rough[mask], fres[mask], rays[:, 3:][mask],
                                           ldir, rgb, pdf, nSample=96, vis_near=0.05, vis_far=1.5)
    a = relit(lrgb, lpdf)
    b = relit(lrgb, lpdf)
    assert a.shape == (M, 3) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 + 1e-6 and float(a.mean()) > 0.01
    assert float(relit(torch.zeros_like(lrgb), lpdf).abs().max()) == 0.0          # black map -> black (linear2srgb(0) = 0)
    dim = relit(lrgb * 0.25, lpdf)
    assert bool((dim <= a + 1e-6).all()) and float((a - dim).max()) > 1e-3
    bg = env.get_light("syn", rays[:, 3:])
    assert bg.shape == (4096, 3) and bool(torch.isfinite(bg).all()) and float(bg.min()) >= 0.0


@torch.no_grad()
@pytest.mark.parametrize("ns", [512, 100])
def test_c5_pair_list_orders_are_bit_identical(full3, monkeypatch, ns):
    """scripts/relight_importance.py:127-131 queries visibility for the pairs that pass the cosine mask only.  The device
    path hands them to the march as a compacted, direction-binned list (tir_env_sample_setup_list): same cells as the
    masked sampler (same Philox counters), the list = exactly the unmasked pair ids, zeros in vis where masked, and relit
    colours bit-identical between the masked march, the plain compaction and binned lists of several block sizes
    (ragged tail: M * Ns is not a multiple of the block)."""
    from tensoir_amd import relight, synth
    m = full3.model
    gen = torch.Generator().manual_seed(72)
    H, W = (256, 512) if ns == 512 else (200, 300)     # the second: guide tables larger than the map (256 / 512 thresholds)
    hdr = torch.exp(torch.randn(H // 8, W // 4, 3, generator=gen) * 1.5)
    hdr = torch.nn.functional.interpolate(hdr.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).contiguous()
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    hdr[((yy - 70) ** 2 + (xx - 200) ** 2) < 6 ** 2] *= 300.0         # a sun: long plateaus and one steep step in the CDFs
    hdr[150:160] = 0.0                                                  # rows without mass
    env = relight.Environment_Light(hdr_maps={"syn": hdr}, device="cuda")
    assert env.hdr_cdf_guide["syn"] is not None       # the listed sampler searches from guide tables, sample_cells does not
    rays = synth.make_rays(64, 64).cuda()[::3].contiguous()
    lidx = torch.zeros(rays.shape[0], 1, dtype=torch.int32, device="cuda")
    out = m(rays, lidx, N_samples=512)
    depth, normal, albedo, rough, fres, acc = out[1], out[2], out[3], out[4], out[5], out[6]
    mask = acc > 0.5
    M = int(mask.sum())
    assert M > 500
    surf = (rays[:, :3] + depth.unsqueeze(-1) * rays[:, 3:])[mask]
    nrm = normal[mask].contiguous()
    torch.manual_seed(9)
    draws = env._draws
    cell, active = env.sample_cells("syn", nrm, ns)
    assert float((((cell // W) - 70).abs() <= 6).float().mean()) > 0.02          # the sun's rows are drawn often
    for bins, block in (((8, 8), 4096), ((1, 1), 256), ((15, 17), 32768), ((4, 16), 1000)):
        env._draws = draws
        cell_b, vis0, pair_ids, n_active = env.sample_cells_listed("syn", nrm, ns, bins, block)
        torch.cuda.synchronize()
        n = int(n_active.item())
        assert torch.equal(cell_b, cell)
        assert n == int(active.sum())
        want = torch.nonzero(active.view(-1)).view(-1).to(torch.int32)
        assert torch.equal(torch.sort(pair_ids[:n]).values, want)
        assert bool((vis0.view(-1)[~active.view(-1).bool()] == 0).all())
        if bins == (8, 8):                 # inside a block the list is bin-major
            ids = pair_ids[:n].long()
            c = cell.view(-1)[ids].long()
            key = ((c // W) * 8 // H) * 8 + ((c % W) * 8 // W)
            blk = ids // block
            same = blk[1:] == blk[:-1]
            assert bool((key[1:][same] >= key[:-1][same]).all())
    cols = {}
    for mode, extra in (("mask", {}), ("compact", {}), ("binned", {}), ("binned", {"TENSOIR_C5_BLOCK_PAIRS": "1000", "TENSOIR_C5_BINS": "3x5"}),
                        ("binned", {"TENSOIR_ENV_RECORDS": "0"})):      # the last: direction / radiance / pdf from three tables
        monkeypatch.setenv("TENSOIR_C5_PAIRS", mode)
        for k in ("TENSOIR_C5_BLOCK_PAIRS", "TENSOIR_C5_BINS", "TENSOIR_ENV_RECORDS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in extra.items():
            monkeypatch.setenv(k, v)
        env._draws = draws
        cols[(mode, tuple(extra))] = relight.relight_importance_sampled(m, env, "syn", surf, nrm, albedo[mask], rough[mask], fres[mask],
                                                                       rays[:, 3:][mask], num_samples=ns)
    base = cols[("mask", ())]
    assert base.shape == (M, 3) and bool(torch.isfinite(base).all()) and float(base.mean()) > 0.01
    for k, v in cols.items():
        assert torch.equal(v, base), k


@torch.no_grad()
def test_c5_chunk_call_is_bit_identical_to_host_masking(full3):
    """relight.relight_chunk (device-side compaction of the acc > 0.5 rows, kernels bounded by the device-side point count,
    colours and background composed into one buffer: no host round trip) against the script's own sequence around
    relight_importance_sampled -- boolean-mask indexing, per-map relight, get_light + index_put_ (scripts/relight_importance.py:
    99-113, :166-171) -- on a chunk with hit and background rows, two maps: bit-identical, also for an all-background chunk."""
    from tensoir_amd import ops, relight, synth
    m = full3.model
    env = relight.Environment_Light("synthetic:h=64,w=128", device="cuda")
    names = list(env.hdr_rgbs)[:2]
    rays = synth.make_rays(48, 48, narrow=1.0).cuda()            # full field of view: about half of the rays miss the object
    lidx = torch.zeros(rays.shape[0], 1, dtype=torch.int32, device="cuda")
    for case in ("mixed", "background"):
        r = rays.clone()
        if case == "background":
            r[:, 3:] = torch.tensor([0.0, 1.0, 0.0], device="cuda")          # every ray leaves the box sideways
        draws = env._draws
        out = m(r, lidx, N_samples=-1)
        depth, normal, albedo, rough, fres, acc = out[1:7]
        mask = acc > 0.5
        if case == "mixed":
            assert 100 < int(mask.sum()) < r.shape[0] - 100
        else:
            assert int(mask.sum()) == 0
        surf = (r[:, :3] + depth.unsqueeze(-1) * r[:, 3:])[mask]
        rows = mask.nonzero()[:, 0]
        want = []
        for name in names:
            rgb = relight.relight_importance_sampled(m, env, name, surf, normal[mask], albedo[mask], rough[mask], fres[mask], r[:, 3:][mask],
                                                     num_samples=128)
            want.append(env.get_light(name, r[:, 3:]).index_put_((rows,), rgb))
        want = torch.cat(want, dim=1)
        env._draws = draws
        got, prim, c = relight.relight_chunk(m, env, names, r, lidx, num_samples=128)
        assert int(c["n_hit"].item()) == int(mask.sum())
        assert torch.equal(c["slot"][mask].long(), torch.arange(int(mask.sum()), device="cuda")) and bool((c["slot"][~mask] == -1).all())
        assert torch.equal(c["surf"][:surf.shape[0]], surf)
        assert torch.equal(got, want), case
        assert torch.equal(prim[6], acc)


@torch.no_grad()
def test_graphed_chunk_renderer_matches_eager_image(env):
    """render_sharded through GraphedChunkRenderer (one captured graph replayed per full chunk, capacity checks
    deferred to one validate() per image, ragged tail eager) gives the image of the eager per-chunk renderer, also
    when the chunks differ a lot in record count (the capacity converges to the heaviest chunk)."""
    from tensoir_amd import Renderer_TensoIR_train
    from tensoir_amd import dist as tdist
    m = env.model
    rays, lidx = G(env, "rays/rays"), G(env, "rays/light_idx")
    n0 = rays.shape[0]
    # an "image": three copies of the batch with perturbed directions, the first one mostly missing the volume
    parts = []
    for i, spread in enumerate((0.8, 0.02, 0.05)):
        r = rays.clone()
        r[:, 3:6] = torch.nn.functional.normalize(r[:, 3:6] + spread * torch.randn_like(r[:, 3:6]), dim=-1)
        parts.append(r)
    img_rays = torch.cat(parts + [rays[: n0 // 3]])                  # ragged last chunk
    img_lidx = torch.cat([lidx] * 3 + [lidx[: n0 // 3]])
    kw = dict(N_samples=-1, white_bg=True, is_train=False, is_relight=True, sample_method="fixed_envirmap",
              device="cuda", args=env.args)
    eager = lambda r, l: Renderer_TensoIR_train(r, None, l, m, **kw)
    want = tdist.render_sharded(eager, img_rays, img_lidx, rank=0, world=1, chunk=n0)
    for lanes in (2, 1, 3):                                           # chunks in flight (own graph + stream per lane)
        fn = tdist.GraphedChunkRenderer(m, n0, env.args, lanes=lanes)
        for _ in range(2):                                            # second image: no re-capture needed any more
            got = tdist.render_sharded(fn, img_rays, img_lidx, rank=0, world=1, chunk=n0)
            for k in ("rgb_map", "depth_map", "normal_map", "acc_map", "rgb_with_brdf_map"):
                assert torch.equal(got[k], want[k]), (lanes, k)
        caps = [g.captures for g in fn.grs]
        tdist.render_sharded(fn, img_rays, img_lidx, rank=0, world=1, chunk=n0)
        assert [g.captures for g in fn.grs] == caps
    # the eager renderer is untouched by the lanes' private pass state
    again = tdist.render_sharded(eager, img_rays, img_lidx, rank=0, world=1, chunk=n0)
    assert torch.equal(again["rgb_with_brdf_map"], want["rgb_with_brdf_map"])


# ---------------------------------------------------------------- fused step kernels (no framework launches inside a step)
@torch.no_grad()
def test_fused_primary_march_scan_viewdirs(full):
    """tir_march_primary_fused_fwd == tir_march_primary_fwd + tir_exclusive_scan_capped + rays[:, 3:6], bit for bit, on
    the BASELINE batch; repeated (the scan runs in whichever workgroup finishes last and reads the other workgroups'
    counts across XCDs: a stale read would show up as a wrong offset), with and without a binding capacity."""
    from tensoir_amd import ops
    m, rays = full.model, full.rays
    f = m.packed_field()
    w0, acc0, dep0, _t, cnt0 = ops.march_primary(f, rays, None, 512, m.march_t_stop)
    total = int(cnt0.sum())
    words = m._step_words(rays.device)
    for it in range(40):
        cap = total + 1000 if it % 2 == 0 else total // 3
        off_ref, tot_ref = ops.exclusive_scan_capped(cnt0, cap)
        words[1:3].fill_(7)                                  # the fused march must re-arm these
        w, acc, dep, cnt, off, tot, vd = ops.march_primary_fused(f, rays, 512, m.march_t_stop, cap, words)
        assert torch.equal(cnt, cnt0) and torch.equal(off, off_ref), it
        assert int(tot) == int(tot_ref) == total
        assert int(words[1]) == 0 and int(words[2]) == 0 and int(words[3]) == 0      # counters zeroed, ticket re-armed
        if it < 2:
            assert torch.equal(w, w0) and torch.equal(acc, acc0) and torch.equal(dep, dep0)
            assert torch.equal(vd, rays[:, 3:6])


@torch.no_grad()
def test_in_kernel_brdf_jitter_noise(env):
    """tir_vm_app_jitter_fwd: xyz_out = xyz + 0.01 * N(0,1) with Philox noise drawn in the gather kernel
    (models/tensorBase_rotated_lights.py:937); the returned features are the intrinsic features of exactly those points;
    the noise is standard normal (moments, cross-coordinate independence), repeatable for a fixed state and fresh after
    the state advances."""
    from tensoir_amd import ops
    m = env.model
    f = m.packed_field()
    n = 200_003
    g = torch.Generator().manual_seed(3)
    xyz = (torch.rand(n, 3, generator=g) * 1.6 - 0.8).cuda()
    state = torch.tensor([1234567, 5], dtype=torch.int64, device="cuda")
    xj, feat = ops.vm_app_jitter(f, xyz, 0.01, 0, 0, state)
    xj2, feat2 = ops.vm_app_jitter(f, xyz, 0.01, 0, 0, state)
    assert torch.equal(xj, xj2) and torch.equal(feat, feat2)
    ref = ops.vm_app(f, xj, None, None, False, True, "mfma")[1]
    assert torch.equal(feat, ref)                                            # same gather, same points
    z = ((xj - xyz) / 0.01).double().cpu()
    assert float(z.mean().abs()) < 0.01 and abs(float(z.var()) - 1.0) < 0.01
    assert abs(float((z ** 4).mean()) - 3.0) < 0.08 and abs(float((z ** 3).mean())) < 0.03       # kurtosis, skewness
    c = torch.corrcoef(z.T)
    assert float((c - torch.eye(3, dtype=torch.float64)).abs().max()) < 0.01
    assert abs(float((z[1:, 0] * z[:-1, 0]).mean())) < 0.01                  # neighbouring points are uncorrelated
    assert float(z.abs().max()) < 6.5
    state[1] += 1                                                            # what the compositing kernel does per pass
    xj3, _ = ops.vm_app_jitter(f, xyz, 0.01, 0, 0, state)
    z3 = ((xj3 - xyz) / 0.01).double().cpu()
    assert abs(float((z3[:, 0] * z[:, 0]).mean())) < 0.01                    # fresh, independent noise
    by_value = ops.vm_app_jitter(f, xyz, 0.01, 1234567, 5, None)[0]          # by-value state == device-side state
    assert torch.equal(by_value, xj)


@torch.no_grad()
def test_merged_primary_app_gather_equals_separate_launches(env):
    """tir_vm_app_primary_fwd (one launch) == tir_vm_app_fwd(both features) + tir_vm_app_jitter_fwd, bit for bit, with and
    without a ray -> record indirection, for a device-side point count below the buffer size; tir_vm_app_primary_x3_fwd (opt-in:
    basis_mat contraction on fp16 hi + lo operands, three products) agrees with them to 5e-6 of the feature
    scale, jittered points identical."""
    from tensoir_amd import ops
    m = env.model
    f = m.packed_field()
    g = torch.Generator().manual_seed(11)
    for n, n_live in ((230_017, 230_017), (70_001, 33_333), (5, 5)):
        xyz = (torch.rand(n, 3, generator=g) * 1.6 - 0.8).cuda()
        n_rays = 4096
        rec_ray = torch.sort(torch.randint(0, n_rays, (n,), generator=g)).values.int().cuda()
        lidx = torch.randint(0, max(int(f.n_lights), 1), (n_rays,), generator=g).int().cuda()
        n_dev = torch.tensor([n_live], dtype=torch.int32, device="cuda")
        state = torch.tensor([99, 3], dtype=torch.int64, device="cuda")
        rad0, intr0 = ops.vm_app(f, xyz, lidx, rec_ray, True, True, "mfma", 0, n_dev)
        xj0, ij0 = ops.vm_app_jitter(f, xyz, 0.01, 0, 0, state, n_dev)
        rad, intr, xj, ij = ops.vm_app_primary(f, xyz, lidx, rec_ray, 0.01, state, n_dev, exact=True)
        w = f.app_dim
        assert torch.equal(rad[:n_live, :w], rad0[:n_live, :w]) and torch.equal(intr[:n_live, :w], intr0[:n_live, :w])
        assert torch.equal(xj[:n_live], xj0[:n_live]) and torch.equal(ij[:n_live, :w], ij0[:n_live, :w])
        assert ops.app_contraction() == "fp32"                                   # x3 is opt-in (TENSOIR_APP_CONTRACTION)
        old_c = ops.APP_CONTRACTION
        try:
            ops.APP_CONTRACTION = "x3"
            rad3, intr3, xj3, ij3 = ops.vm_app_primary(f, xyz, lidx, rec_ray, 0.01, state, n_dev)
        finally:
            ops.APP_CONTRACTION = old_c
        assert torch.equal(xj3[:n_live], xj0[:n_live])
        for got, ref in ((rad3, rad0), (intr3, intr0), (ij3, ij0)):
            scale = float(ref[:n_live, :w].abs().max())
            assert float((got[:n_live, :w] - ref[:n_live, :w]).abs().max()) < 5e-6 * scale + 1e-7, (n, scale)       # (fp16 residues of small products are subnormal: an absolute floor of ~5e-8)
            assert bool((got[:n_live, w:] == 0).all())


@torch.no_grad()
def test_boundary_call_launch_budget_and_smoothness(full):
    """The hinted inference route: the smoothness losses come out of the compositing kernel (== the column means of the
    map rows), the jitter state advances once per pass (two calls -> different smoothness noise, same geometry maps)."""
    from tensoir_amd import Renderer_TensoIR_train
    m = full.model
    kw = dict(N_samples=512, args=full.args, device="cuda", _no_graph=True)  # the eager route (the cached graph owns a jitter state of its own)
    Renderer_TensoIR_train(full.rays, None, full.lidx, m, **kw)             # learns the capacity hints
    out, maps = m(full.rays, full.lidx, N_samples=512, _return_maps=True)
    want = maps[:, 17:19].double().mean(dim=0)
    assert abs(float(out[10]) - float(want[0])) <= 1e-6 * abs(float(want[0])) + 1e-12
    assert abs(float(out[11]) - float(want[1])) <= 1e-6 * abs(float(want[1])) + 1e-12
    off0 = int(m._jit_rng[1][1])
    a = Renderer_TensoIR_train(full.rays, None, full.lidx, m, **kw)
    b = Renderer_TensoIR_train(full.rays, None, full.lidx, m, **kw)
    assert int(m._jit_rng[1][1]) == off0 + 2
    for k in ("rgb_map", "depth_map", "normal_map", "albedo_map", "acc_map", "rgb_with_brdf_map"):
        assert torch.equal(a[k], b[k]), k
    assert float(a["albedo_smoothness_loss"]) != float(b["albedo_smoothness_loss"])
    assert abs(float(a["albedo_smoothness_loss"]) / float(b["albedo_smoothness_loss"]) - 1) < 0.2


@torch.no_grad()
@pytest.mark.parametrize("grid", [300, 400])
def test_lds_staged_lines_march_is_bit_identical(grid):
    """The secondary march with the density line factors staged in LDS (north_star; 512-thread blocks at 300^3, one
    1024-thread block per CU at the 400^3 of the ficus config) against the plain kernel: visibility, 1 - acc, indirect
    radiance and the record bookkeeping of compute_radiance / compute_transmittance, bit for bit, on a ragged pair count."""
    import contextlib, io
    import tensoir_amd
    from tensoir_amd import _lib, relight, synth
    ck = synth.make_checkpoint(grid=(grid,) * 3, seed=20211202)
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=8, envmap_w=16)
    with contextlib.redirect_stdout(io.StringIO()):
        m.updateAlphaMask((128, 128, 128))
    gen = torch.Generator().manual_seed(17)
    P = 40_000 + 37
    pts = (torch.rand(P, 3, generator=gen) * 2 - 1).mul(1.1).cuda()
    dirs = torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1).cuda()
    li = torch.zeros(P, 1, dtype=torch.int32, device="cuda")
    res = {}
    f = m.packed_field()                # the launch option travels in the descriptor (TirField.tune_lds_lines: 0/1 = on, 2 = off)
    prev = f.tune_lds_lines
    try:
        for on in (1, 0):
            f.tune_lds_lines = 1 if on else 2
            assert m.packed_field() is f
            m.__dict__.pop("_rec_cap_hints", None)
            v, nf, ind = relight.compute_radiance(m, pts, dirs, li, nSample=96, vis_near=0.05, vis_far=1.5)
            v2, nf2, ind2 = relight.compute_radiance(m, pts, dirs, li, nSample=96, vis_near=0.05, vis_far=1.5)   # hinted route
            t, tn = relight.compute_transmittance(m, pts, dirs, nSample=57, vis_near=0.05, vis_far=1.5)
            res[on] = (v, nf, ind, v2, ind2, t, tn)
    finally:
        f.tune_lds_lines = prev
    for a, b in zip(res[1], res[0]):
        assert torch.equal(a, b)
    assert float(res[1][0].min()) < 0.01 and float(res[1][0].max()) > 0.99 and float(res[1][2].abs().max()) > 0


@torch.no_grad()
def test_multi_decoder_launch_equals_single_launches(env):
    """tir_mlp_fwd_multi_bf16x3 (the primary stage's decoders in one launch, grid split between them) == one
    tir_mlp_fwd_bf16x3 launch per decoder, bit for bit, for 1-4 jobs, ragged row counts, with an aux index map and with a
    device-side row count."""
    from tensoir_amd import ops
    m = env.model
    gen = torch.Generator().manual_seed(23)
    _multi_vs_single(ops, m, gen)


def _multi_vs_single(ops, m, gen):
    # like for like: the single launches take the full 150-input layer 1 too (their aux-table variant rounds differently and is
    # compared in test_decoder_aux_table_variant)
    old_tab = ops.AUX_TABLE
    ops.AUX_TABLE = False
    try:
        _multi_vs_single_body(ops, m, gen)
    finally:
        ops.AUX_TABLE = old_tab


def _multi_vs_single_body(ops, m, gen):
    for n in (70_001, 255, 1):
        feats = [torch.zeros(n, 32) for _ in range(3)]
        for f in feats:
            f[:, :27] = torch.randn(n, 27, generator=gen)
        feats = [f.cuda() for f in feats]
        xyz = (torch.rand(n, 3, generator=gen) * 2 - 1).cuda()
        vd = torch.nn.functional.normalize(torch.randn(37, 3, generator=gen), dim=-1).cuda()
        amap = torch.randint(0, 37, (n,), generator=gen).int().cuda()
        jobs = [(m.renderModule.packed(), feats[0], vd, amap), (m.renderModule_brdf.packed(), feats[1], xyz, None),
                (m.renderModule_brdf.packed(), feats[2], xyz, None), (m.renderModule_normal.packed(), feats[1], xyz, None)]
        for k in (4, 3, 1):
            got = ops.mlp_multi(jobs[:k])
            for (pk, ft, ax, mp), g in zip(jobs[:k], got):
                want = ops.mlp(pk, ft, ax, mp, "bf16x3")
                assert torch.equal(g, want), (n, k)
        if n > 1000:
            n_dev = torch.tensor([n // 3], dtype=torch.int32, device="cuda")
            got = ops.mlp_multi(jobs, n_dev)
            for (pk, ft, ax, mp), g in zip(jobs, got):
                assert torch.equal(g[: n // 3], ops.mlp(pk, ft, ax, mp, "bf16x3")[: n // 3])


@torch.no_grad()
def test_occupied_box_step_skipping_changes_nothing():
    """TirField::occ_lo / occ_hi (the box outside of which the occupancy mask is empty) lets the secondary march skip whole
    32-sample steps.  Culled samples contribute alpha = 0, so the results must be the same BIT FOR BIT with the box
    (as the model builds it from a small off-centre blob: most of the aabb is empty), without it (zeros = not given) and
    with a box far away from every sample's cell -- primary weights / acc / depth / counts, secondary visibility,
    1 - acc and indirect radiance, transmittance."""
    import contextlib, copy, io
    import tensoir_amd
    from tensoir_amd import ops, relight, synth
    ck = synth.make_checkpoint(grid=(96,) * 3, seed=3, blob_sigma=0.18)
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=4, envmap_w=8)
    with contextlib.redirect_stdout(io.StringIO()):
        m.updateAlphaMask((64, 64, 64))
    f = m.packed_field()
    lo, hi = list(f.occ_lo), list(f.occ_hi)
    assert all(a < b for a, b in zip(lo, hi)) and max(b - a for a, b in zip(lo, hi)) < 2.4        # much tighter than the aabb
    rays = synth.make_rays(48, 48, narrow=1.0).cuda()
    gen = torch.Generator().manual_seed(5)
    P = 30_011
    pts = (torch.rand(P, 3, generator=gen) * 2 - 1).mul(1.2).cuda()
    dirs = torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1).cuda()
    li = torch.zeros(P, 1, dtype=torch.int32, device="cuda")

    def run():
        m.__dict__.pop("_rec_cap_hints", None)
        fd = m.packed_field()
        w, acc, dep, tend, cnt = ops.march_primary(fd, rays, None, 333, 0.0)
        w2 = ops.march_primary(fd, rays, None, 333, 1e-6)[0]
        v, nf, ind = relight.compute_radiance(m, pts, dirs, li, nSample=96, vis_near=0.05, vis_far=1.5)
        t, tn = relight.compute_transmittance(m, pts, dirs, nSample=57, vis_near=0.05, vis_far=1.5)
        return w, acc, dep, tend, cnt, w2, v, nf, ind, t, tn

    with_box = run()
    assert float(with_box[1].max()) > 0.9 and float(with_box[6].min()) < 0.05          # rays do hit the blob
    f.occ_lo[:], f.occ_hi[:] = [0.0] * 3, [0.0] * 3           # the cached descriptor is passed by value at every launch
    no_box = run()
    for a, b in zip(with_box, no_box):
        assert torch.equal(a, b)
    f.occ_lo[:], f.occ_hi[:] = lo, hi
