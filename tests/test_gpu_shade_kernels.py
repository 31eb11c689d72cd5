"""The shading stage's kernels on their own, through the ops wrappers, against the torch restatement (tests/shade_reference.py) in
float64, forward and backward: tir_ggx_specular, tir_shade_setup[_compact], tir_surface_compact, tir_shade_integrate[_records],
tir_accumulate_records, tir_shade_integrate_bwd (its LDS arm at its largest, its global-atomic arm, its persistent loop),
tir_env_sg_fwd / _bwd, tir_relight_importance and its two cell forms, tir_env_lookup.

Comparison rule (DESIGN 4.8's): per output tensor and case, the device's distance from the float64 restatement -- max abs
difference over the float64 result's maximum -- is at most ten times the float32 restatement's own distance on the same fixture
(and no less than ten half-ulps of 1); the factor covers the device's fused multiply-adds, exp2f, the wave reductions' and the
atomics' order against torch's separately rounded operations.  For the gradient of the map rows the distance is taken per column
group (normal, albedo, roughness, fresnel): their magnitudes differ by orders.  Nothing is excluded: tests/test_shade_cpu.py
asserts that on every fixture every branch predicate takes the same value in float32 and float64, with margins on the random
rows, and that `vis` and `indirect` are zero wherever the cosine mask is off, as in the pipeline.  Every test prints
`device d (bound b)`.

Measured on an MI355X: see DESIGN 2, "The shading stage on its own"."""
import pytest
import torch

from oracle import tensoir_oracle as O
from tests import shade_reference as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def dev(t):
    return None if t is None else t.contiguous().cuda()


def check(label, got, f32, f64):
    d, b = S.distance(got, f64), S.bound(f32, f64)
    print(f"\n[shade {label}] device {d:.2e} (bound {b:.2e})")
    assert torch.isfinite(torch.as_tensor(got)).all() and d <= b, (label, d, b)


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ---- GGX ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", S.GGX_SHAPES)
def test_ggx_specular(M, D):
    """M * D of 1, 255 and above 256 (one thread per pair, blocks of 256); roughness and fresnel distinct per channel, and the
    [M, 1] argument path against the same values repeated; rows with N.V = 0 and with the exact mirror direction."""
    from tensoir_amd import ops
    t = S.ggx_case(M, D)
    ref = lambda dt, r, f: O.ggx_specular(t.normal.to(dt), t.view.to(dt), t.l.to(dt), r.to(dt), f.to(dt))
    got = ops.ggx_specular(dev(t.normal), dev(t.view), dev(t.l), dev(t.rough), dev(t.fresnel)).cpu()
    assert got.shape == (M, D, 3)
    check(f"ggx M {M} D {D} [M,3]", got, ref(F32, t.rough, t.fresnel), ref(F64, t.rough, t.fresnel))
    r1, f1 = t.rough[:, :1].contiguous(), t.fresnel[:, :1].contiguous()
    one = ops.ggx_specular(dev(t.normal), dev(t.view), dev(t.l), dev(r1), dev(f1)).cpu()
    check(f"ggx M {M} D {D} [M,1]", one, ref(F32, r1.expand(M, 3), f1.expand(M, 3)), ref(F64, r1.expand(M, 3), f1.expand(M, 3)))
    assert torch.equal(one, ops.ggx_specular(dev(t.normal), dev(t.view), dev(t.l), dev(r1.expand(M, 3)), dev(f1.expand(M, 3))).cpu())
    print(f"[shade ggx M {M} D {D}] equal inputs per channel: channels apart by {S.distance(one[..., 2], one[..., 0]):.2e}")


# ---- forward -------------------------------------------------------------------------------------------------------------------------
def device_forward(fx, indirect, equal_area, use_srgb):
    from tensoir_amd import ops
    return ops.shade_integrate(dev(fx.maps), dev(fx.rays), dev(fx.dirs), dev(fx.light_idx), dev(fx.vis), dev(fx.indirect) if indirect else None,
                               dev(fx.env), dev(fx.weight_d), equal_area, use_srgb, fx.acc_thres).cpu()


def reference_forward(fx, indirect, equal_area, use_srgb, dtype):
    with torch.no_grad():
        return S.shade_integrate(fx.maps, fx.rays, fx.dirs, fx.light_idx, fx.vis, fx.indirect if indirect else None, fx.env, fx.weight_d,
                                 equal_area, use_srgb, fx.acc_thres, dtype)


FORWARD_CASES = [(s, False, True, True) for s in S.FORWARD_SHAPES] + \
                [(S.BASE, ea, srgb, ind) for ea in (False, True) for srgb in (False, True) for ind in (False, True) if (ea, srgb, ind) != (False, True, True)]


@pytest.mark.parametrize("shape,equal_area,use_srgb,indirect", FORWARD_CASES, ids=ident)
def test_shade_integrate_forward(shape, equal_area, use_srgb, indirect):
    """One wave per point, four per block: M of 1, 3, 4, 5, 257; lanes over directions: D of 1, 24, 63, 64, 65, 130; one light and
    three, light_idx of -1 and n_lights among them (clamped); roughness 0.02, 0.5, 1; all four (equal_area, use_srgb) and both
    indirect = None and given on the base case; the designed rows of shade_reference.surface_rows."""
    fx = S.case(*shape)
    got = device_forward(fx, indirect, equal_area, use_srgb)
    check(f"forward {shape} equal_area {int(equal_area)} srgb {int(use_srgb)} indirect {int(indirect)}", got,
          reference_forward(fx, indirect, equal_area, use_srgb, F32), reference_forward(fx, indirect, equal_area, use_srgb, F64))
    bg = ~(fx.maps[:, 14] > fx.acc_thres)
    assert (got[bg] == 1.0).all() and got.shape == (shape[0], 3)
    if "below_horizon" in fx.rows:
        assert (got[fx.rows["below_horizon"]] == 0).all() and (got[fx.rows["normal_zero"]] == 0).all()
        top = got[fx.rows["bright"]]                        # the clip's 1, through the curve when it is on (1.055 * (1 + 1e-6)^(1/2.4) - 0.055)
        assert (top == 1).all() if not use_srgb else ((top - 1).abs() < 1e-6).all() and (top == top[0]).all()
        assert bg[fx.rows["acc_at_threshold"]] and not bg[fx.rows["acc_above_threshold"]] and (got[fx.rows["acc_above_threshold"]] != 1).any()
    # light_idx past either end is the nearest light's
    from tensoir_amd import ops
    fixed = torch.clamp(fx.light_idx, 0, fx.env.shape[0] - 1)
    again = ops.shade_integrate(dev(fx.maps), dev(fx.rays), dev(fx.dirs), dev(fixed), dev(fx.vis), dev(fx.indirect) if indirect else None,
                                dev(fx.env), dev(fx.weight_d), equal_area, use_srgb, fx.acc_thres).cpu()
    assert torch.equal(again, got) and not torch.equal(fixed, fx.light_idx)


def test_horizon_row_is_exact():
    """n.l in {0, 2^-20, 2^-19, -2^-19}, exact products: only 2^-19 > 1e-6 is lit, and without the sRGB curve the result equals the
    float32 restatement bit for bit under either weighting (shade_reference.horizon_case says why it can); with the curve, within
    the rule.  The mask of the same row from both setup entries."""
    from tensoir_amd import ops
    fx = S.horizon_case()
    for ea in (False, True):
        got = device_forward(fx, False, ea, False)
        want = reference_forward(fx, False, ea, False, F32)
        assert torch.equal(got, want), (ea, got, want)
        assert (got > 0.01).all() and (got < 1).all()
        check(f"horizon srgb equal_area {int(ea)}", device_forward(fx, False, ea, True), reference_forward(fx, False, ea, True, F32),
              reference_forward(fx, False, ea, True, F64))
    active = ops.shade_setup(dev(fx.maps), dev(fx.rays), dev(fx.dirs), 0.5)[1].cpu()
    assert active.tolist() == [[0, 0, 1, 0]]
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = ops.shade_setup_compact(dev(fx.maps), dev(fx.rays), dev(fx.dirs), 0.5, n)
    assert out[1].cpu().tolist() == [[0, 0, 1, 0]] and int(n) == 1 and int(out[2][0]) == 2


def test_shade_integrate_records_equals_separate_sum():
    """The fused record sum (k_shade_integrate reading the secondary records) and tir_accumulate_records use the same fmaf chain in
    sample order: bit-identical outputs.  Per-pair record counts of 0, 1, 2, 5 and 96; accumulate_records against float64 under
    the rule; the pair counter handed in as 7 reads 0 afterwards."""
    from tensoir_amd import ops
    fx = S.case(*S.BASE)
    M, D = fx.vis.shape
    off, cnt, w, rgb = S.records_case(fx)
    ind = ops.accumulate_records(dev(off), dev(cnt), dev(w), dev(rgb), M * D)
    check("accumulate_records", ind.cpu(), S.records_sum(off, cnt, w, rgb, F32), S.records_sum(off, cnt, w, rgb, F64))
    assert (ind.cpu()[cnt == 0] == 0).all()
    for ea, srgb in ((False, True), (True, False)):
        counter = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        fused = ops.shade_integrate_records(dev(fx.maps), dev(fx.rays), dev(fx.dirs), dev(fx.light_idx), dev(fx.vis), dev(off), dev(cnt), dev(w),
                                            dev(rgb), dev(fx.env), dev(fx.weight_d), ea, srgb, fx.acc_thres, reset_counter=counter).cpu()
        apart = ops.shade_integrate(dev(fx.maps), dev(fx.rays), dev(fx.dirs), dev(fx.light_idx), dev(fx.vis), ind.view(M, D, 3), dev(fx.env),
                                    dev(fx.weight_d), ea, srgb, fx.acc_thres).cpu()
        assert torch.equal(fused, apart) and int(counter) == 0
        ref = lambda dt: S.shade_integrate(fx.maps, fx.rays, fx.dirs, fx.light_idx, fx.vis, S.records_sum(off, cnt, w, rgb, dt).view(M, D, 3), fx.env,
                                           fx.weight_d, ea, srgb, fx.acc_thres, dt)
        check(f"records equal_area {int(ea)} srgb {int(srgb)}", fused, ref(F32), ref(F64))


# ---- setup ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", S.SETUP_SHAPES)
def test_shade_setup(M, D, monkeypatch):
    """M * D of 1, 1023, 1024, 1025 and 3 * 1024 + 7 (the compact entry reserves list space once per 1024-pair block), the plain entry
    and the compact one in both pair orders.  The mask equals the float32 restatement's; the list holds exactly the active pairs
    (the order between blocks is free, so it is compared sorted); masked pairs have vis 0 and no records; surf has the bits of
    float32 o + (depth * d), rounded twice -- a single fused rounding differs on these fixtures (tests/test_shade_cpu.py)."""
    from tensoir_amd import ops
    fx = S.case(M, D, 3, 0.5)
    surf, active = S.shade_setup(fx.maps, fx.rays, fx.dirs, fx.acc_thres, F32)
    assert torch.equal(active, S.shade_setup(fx.maps, fx.rays, fx.dirs, fx.acc_thres, F64)[1])
    want_ids = torch.nonzero(active.reshape(-1)).reshape(-1)
    args = (dev(fx.maps), dev(fx.rays), dev(fx.dirs), fx.acc_thres)
    s0, a0 = ops.shade_setup(*args)
    assert torch.equal(a0.cpu().bool(), active) and a0.dtype == torch.uint8
    assert torch.equal(s0.cpu(), surf), f"surf differs in {int((s0.cpu() != surf).sum())} elements: contracted to a fused multiply-add?"
    default = ops.TUNE["pair_order"]
    lists = {}
    for order in (0, 2):
        monkeypatch.setitem(ops.TUNE, "pair_order", order)
        n = torch.zeros(1, dtype=torch.int32, device="cuda")
        s1, a1, ids, vis, rec_cnt = ops.shade_setup_compact(*args, n)
        assert torch.equal(s1.cpu(), surf) and torch.equal(a1.cpu().bool(), active)
        assert int(n) == int(active.sum())
        ids = ids.cpu()[: int(n)].long()
        assert torch.equal(torch.sort(ids).values, want_ids)
        off = ~active.reshape(-1)
        assert (vis.cpu()[off] == 0).all() and (rec_cnt.cpu()[off] == 0).all()
        lists[order] = ids
    monkeypatch.undo()
    assert ops.TUNE["pair_order"] == default
    if M * D <= 1024 and M > 1 and D > 1:               # one block: the list is in thread order, direction-major or point-major
        assert torch.equal(lists[2], want_ids)
        assert torch.equal(lists[0], torch.tensor(sorted(want_ids.tolist(), key=lambda i: (i % D, i // D))))
    print(f"\n[shade setup M {M} D {D}] active {int(active.sum())} of {M * D}")
    out = ops.surface_compact(*args[:2], fx.acc_thres)
    fg = fx.maps[:, 14] > fx.acc_thres
    k = int(out["n_hit"])
    assert k == int(fg.sum()) and torch.equal(out["surf"].cpu()[:k], surf[fg])
    assert torch.equal(out["slot"].cpu()[fg].long(), torch.arange(k)) and (out["slot"].cpu()[~fg] == -1).all()
    assert torch.equal(out["normal"].cpu()[:k], fx.maps[fg, 4:7]) and torch.equal(out["rough"].cpu()[:k], fx.maps[fg, 10])


# ---- backward ------------------------------------------------------------------------------------------------------------------------
def device_backward(fx, indirect, equal_area, use_srgb, cot):
    from tensoir_amd import ops
    g_maps, g_env = ops.shade_integrate_bwd(dev(fx.maps), dev(fx.rays), dev(fx.dirs), dev(fx.light_idx), dev(fx.vis),
                                            dev(fx.indirect) if indirect else None, dev(fx.env), dev(fx.weight_d), equal_area, use_srgb,
                                            fx.acc_thres, dev(cot))
    return g_maps.cpu(), g_env.cpu()


def check_backward(label, fx, indirect, equal_area, use_srgb, cot):
    g_maps, g_env = device_backward(fx, indirect, equal_area, use_srgb, cot)
    _, gm64, ge64 = S.shade_gradients(fx, indirect, equal_area, use_srgb, cot, F64)
    _, gm32, ge32 = S.shade_gradients(fx, indirect, equal_area, use_srgb, cot, F32)
    for name, cols in S.GROUPS.items():
        check(f"backward {label} {name}", g_maps[:, cols], gm32[:, cols], gm64[:, cols])
    check(f"backward {label} env", g_env, ge32, ge64)
    assert (g_maps[:, :4] == 0).all() and (g_maps[:, 14:] == 0).all()
    assert (g_maps[~(fx.maps[:, 14] > fx.acc_thres)] == 0).all()
    picked = torch.zeros(fx.env.shape[0], dtype=torch.bool)
    picked[fx.light_idx.long().clamp(0, fx.env.shape[0] - 1)] = True
    assert (g_env[~picked] == 0).all() and (g_env[picked] != 0).any()
    return g_maps, g_env


BACKWARD_CASES = [(ea, srgb, ind) for ea in (False, True) for srgb in (False, True) for ind in (False, True)]


@pytest.mark.parametrize("equal_area,use_srgb,indirect", BACKWARD_CASES)
def test_shade_integrate_backward(equal_area, use_srgb, indirect):
    """Gradients of (out * cotangent).sum() with respect to map columns 4-13 and to env on the base case (65 points, 33 directions,
    three lights), all four flag combinations, indirect = None and given, against float64 autograd of the restatement.  The
    designed rows put NoH on its upper clamp value exactly (inclusive pass-through), N.V on 0, the total above 1, on 0, and below
    the sRGB knee."""
    fx = S.case(*S.BASE)
    cot = S.cotangent(fx.maps.shape[0])
    g_maps, g_env = check_backward(f"base equal_area {int(equal_area)} srgb {int(use_srgb)} indirect {int(indirect)}", fx, indirect, equal_area,
                                   use_srgb, cot)
    for name in ("bright", "below_horizon", "normal_zero", "acc_at_threshold"):
        assert (g_maps[fx.rows[name]] == 0).all(), name
    assert (g_maps[fx.rows["mirror_03"], 4:7] != 0).any() and (g_maps[fx.rows["nov_zero"], 4:7] != 0).any()
    # the clipped row on its own: nothing reaches env either
    only = torch.zeros_like(cot)
    only[fx.rows["bright"]] = cot[fx.rows["bright"]]
    gm, ge = device_backward(fx, indirect, equal_area, use_srgb, only)
    assert (gm == 0).all() and (ge == 0).all()


def test_shade_integrate_backward_at_low_roughness():
    fx = S.case(65, 33, 3, 0.02)
    check_backward("roughness 0.02", fx, True, False, True, S.cotangent(65))


@pytest.mark.parametrize("arm", list(S.ARM_SHAPES))
def test_shade_integrate_backward_arms(arm):
    """The environment gradient's three dispatch arms: block LDS at its largest (43 lights x 127 directions x 12 bytes = 65532 of
    dynamic LDS), global atomics one float past it (66048 bytes), and the persistent grid's loop (2053 points: 514 blocks' worth on
    512 blocks, LDS arm).  The two 43-light cases differ by one direction and must agree with float64 alike."""
    shape = S.ARM_SHAPES[arm]
    fx = S.case(*shape)
    M, D, L, _ = shape
    assert (L * D * 12 <= 65536) == (arm != "global-atomic") and ((M + 3) // 4 > 512) == (arm == "persistent-loop")
    check_backward(arm, fx, True, False, True, S.cotangent(M))


def test_denominator_clamp_edges():
    """clamp_case(): the only pair has a raw denominator of 2.2e-13, inside the lower clamp.  The roughness gradient is the
    numerator's alone and the normal's gradient the cosine's alone: the device against the float64 closed form
    (shade_reference.clamp_gradients, which tests/test_shade_cpu.py ties to float64 autograd), under the rule."""
    fx = S.clamp_case()
    cot = torch.tensor([[0.5, -1.25, 2.0]])
    g_maps, g_env = device_backward(fx, True, False, False, cot)
    g_rough, g_normal = S.clamp_gradients(fx, cot)
    _, gm32, _ = S.shade_gradients(fx, True, False, False, cot, F32)
    check("clamped denominator roughness", g_maps[0, 10], gm32[0, 10], g_rough)
    check("clamped denominator normal", g_maps[0, 4:7], gm32[0, 4:7], g_normal)
    assert (g_env != 0).all()
    # the denominator's upper edge, 4 pi exactly: the gradient passes (held back, the roughness gradient would have the opposite sign)
    fx = S.clamp_case(top=True)
    g_maps, g_env = device_backward(fx, True, False, False, cot)
    _, gm64, ge64 = S.shade_gradients(fx, True, False, False, cot, F64)
    _, gm32, ge32 = S.shade_gradients(fx, True, False, False, cot, F32)
    check("denominator's upper edge roughness", g_maps[0, 10], gm32[0, 10], gm64[0, 10])
    check("denominator's upper edge normal", g_maps[0, 4:7], gm32[0, 4:7], gm64[0, 4:7])
    check("denominator's upper edge env", g_env, ge32, ge64)


# ---- spherical Gaussians -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sg,L,D", S.SG_CASES)
def test_env_sg(n_sg, L, D):
    """Lobe counts round the forward's block of 128 (its loop strides by 128, two waves reduce), L * D round the backward's block of
    256 (strides by 256, four waves reduce); negative lambda and mu, mu = 0 and lambda = 0 (derivative exactly 0, as torch.abs's),
    axes of length 0.1 and 10, lambda = 200."""
    from tensoir_amd import ops
    c = S.sg_case(n_sg, L, D)
    o64, g64 = S.sg_gradients(c, F64)
    o32, g32 = S.sg_gradients(c, F32)
    out = ops.env_sg(dev(c.sgs), dev(c.rot), dev(c.dirs)).cpu()
    assert out.shape == (L, D, 3)
    check(f"env_sg n_sg {n_sg} L {L} D {D} forward", out, o32, o64)
    g = ops.env_sg_bwd(dev(c.sgs), dev(c.rot), dev(c.dirs), dev(c.cot)).cpu()
    check(f"env_sg n_sg {n_sg} L {L} D {D} backward", g, g32, g64)
    if n_sg > 5:
        assert g[1, 4] == 0 and g[2, 3] == 0 and (g[1, 5:] != 0).all()
    flipped = c.sgs.clone()
    flipped[0, 3], flipped[0, 5] = -flipped[0, 3], -flipped[0, 5]
    g2 = ops.env_sg_bwd(dev(flipped), dev(c.rot), dev(c.dirs), dev(c.cot)).cpu()
    assert torch.equal(ops.env_sg(dev(flipped), dev(c.rot), dev(c.dirs)).cpu(), out)
    assert g2[0, 3] == -g[0, 3] and g2[0, 5] == -g[0, 5] and torch.equal(g2[1:], g[1:]) and torch.equal(g2[0, :3], g[0, :3])


# ---- importance-sampled relighting ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Ns", S.IMPORTANCE_CASES)
def test_relight_importance_forms(M, Ns):
    """One wave per point, lanes over samples: Ns of 1, 63, 64, 65, 100, M of 1, 4, 5; about half of the samples have a negative
    cosine and vis = 0.  The unfused entry against float64; the cell-indexed entry with three tables and with packed records:
    the same bits as each other and as the unfused entry on the gathered tables; a device-side point count of 3 of 5 writes rows
    0-2 as a call with three points does, and nothing else."""
    from tensoir_amd import ops
    t = S.importance_case(M, Ns)
    ref = lambda dt: S.relight_importance(t.normal, t.albedo, t.rough, t.fresnel, t.rays_d, t.light_dir, t.light_rgb, t.light_pdf, t.vis, dt)
    surf = [dev(x) for x in (t.normal, t.albedo, t.rough, t.fresnel, t.rays_d)]
    got = ops.relight_importance(*surf, dev(t.light_dir), dev(t.light_rgb), dev(t.light_pdf), dev(t.vis)).cpu()
    check(f"importance M {M} Ns {Ns}", got, ref(F32), ref(F64))
    tables = ops.relight_importance_cells(*surf, dev(t.cell), dev(t.env_dir), dev(t.env_rgb), dev(t.env_pdf), dev(t.vis)).cpu()
    packed_cells = ops.pack_env_cells(dev(t.env_dir), dev(t.env_rgb), dev(t.env_pdf))
    assert packed_cells.shape == (t.env_dir.shape[0], 8)
    packed = ops.relight_importance_cells(*surf, dev(t.cell), None, None, None, dev(t.vis), env_cell=packed_cells).cpu()
    assert torch.equal(tables, got) and torch.equal(packed, got)
    if M == 5:
        count = torch.tensor([3], dtype=torch.int32, device="cuda")
        part = ops.relight_importance_cells(*surf, dev(t.cell), None, None, None, dev(t.vis), env_cell=packed_cells, m_dev=count)
        three = ops.relight_importance_cells(*[x[:3].contiguous() for x in surf], dev(t.cell[:3]), None, None, None, dev(t.vis[:3]),
                                             env_cell=packed_cells).cpu()
        assert torch.equal(part.cpu()[:3], three) and torch.equal(three, got[:3])
        with pytest.raises(ValueError):
            ops.relight_importance_cells(*surf, dev(t.cell), dev(t.env_dir), dev(t.env_rgb), dev(t.env_pdf), dev(t.vis), m_dev=count)


# ---- the background lookup -----------------------------------------------------------------------------------------------------------
def test_env_lookup_edges():
    """Both poles, the +-pi seam, dz one ulp outside [-1, 1] (clamped by the kernel: the same bits as dz = +-1, and finite) and
    random directions; the in-range ones against Environment_Light.get_light in float64 under the rule."""
    from tensoir_amd import ops
    hdr, dirs = S.lookup_case()
    got = ops.env_lookup(dev(hdr), dev(dirs)).cpu()
    assert got.shape == dirs.shape and torch.isfinite(got).all()
    assert torch.equal(got[4], got[0]) and torch.equal(got[5], got[1]) and torch.equal(got[6:8], got[0:2])
    inside = torch.ones(dirs.shape[0], dtype=torch.bool)
    inside[4:6] = False
    check("env_lookup", got[inside], O.envlight_lookup(hdr, dirs[inside]), O.envlight_lookup(hdr.double(), dirs[inside].double()))
    assert (got[2] > 0).all() and (got[3] > 0).all()
