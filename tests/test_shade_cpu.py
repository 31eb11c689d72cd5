"""What needs no GPU of the shading-stage tests ("The shading stage on its own"): the restatement
(tests/shade_reference.py) tied to the pinned oracle on the golden scene, the fixtures' margins and designed rows -- the reason
the GPU tests (tests/test_gpu_shade_kernels.py) exclude nothing --, float64 autograd through every restatement on every fixture,
and the float32 restatement's own distance from float64, printed per fixture: ten times it is the device's bound."""
import numpy as np
import pytest
import torch

from oracle import tensoir_oracle as O
from tests import shade_reference as S
from tests.helpers import T, golden_scene

F32, F64 = torch.float32, torch.float64
SHAPES = list(dict.fromkeys(S.FORWARD_SHAPES + S.BACKWARD_SHAPES + [(M, D, 3, 0.5) for M, D in S.SETUP_SHAPES]))


# ---- the restatement against the pinned oracle ------------------------------------------------------------------------------------------
def test_restatement_is_the_oracles_on_the_golden_scene(golden):
    """render_with_brdf on the golden small scene, then shade_integrate in float32 on its own vis, indirect and env: the same
    operations on the same numbers (1e-6 covers the one difference, the white rows' torch.where)."""
    sc = golden_scene(golden)
    rays, lidx = T(golden, "rays/rays"), T(golden, "rays/light_idx").int()
    with torch.no_grad():
        out = O.forward_primary(sc, rays, lidx, brdf_jitter=torch.zeros(rays.shape[0], int(golden["scene/nSamples"][0]), 3))
        depth, normal, albedo, rough, fres, acc = out[1], out[2], out[3], out[4], out[5], out[6]
        m = acc > 0.5
        assert int(m.sum()) > 30
        rgb, aux = O.render_with_brdf(sc, depth[m], normal[m], albedo[m], rough[m].repeat(1, 3), fres[m], rays[m], lidx[m], 24, 0.05, 1.5,
                                      return_aux=True)
        area, dirs = O.envmap_dirs(sc.envmap_h, sc.envmap_w)
        maps = torch.zeros(int(m.sum()), S.MAP_STRIDE)
        maps[:, 3], maps[:, 4:7], maps[:, 7:10], maps[:, 10], maps[:, 11:14], maps[:, 14] = \
            depth[m], normal[m], albedo[m], rough[m].reshape(-1), fres[m], acc[m].reshape(-1)
        mine = S.shade_integrate(maps, rays[m], dirs, lidx[m], aux.vis[..., 0], aux.indirect, aux.env, area, False, True, 0.5, F32)
        assert mine.dtype == F32 and float((mine - rgb).abs().max()) < 1e-6 and float(rgb.max() - rgb.min()) > 0.01
        # the fixture invariant is the pipeline's: nothing arrives where the cosine mask is off
        off = ~(aux.cosine > 1e-6)
        assert off.any() and (aux.vis[off] == 0).all() and (aux.indirect[off] == 0).all()
        # the surface point and the mask
        surf, active = S.shade_setup(maps, rays[m], dirs, 0.5, F32)
        assert torch.equal(surf, rays[m][:, :3] + depth[m].unsqueeze(-1) * rays[m][:, 3:]) and torch.equal(active, aux.cosine > 1e-6)
        # the environment
        rot = O.light_rotation_matrices(sc.light_rotation)
        assert float((S.env_sg(sc.lgtSGs, rot, dirs, F32) - O.light_rgbs(sc, dirs)).abs().max()) < 1e-6


def test_equal_area_weighting_is_the_mean_with_four_pi():
    """models/relight_utils.py:470-471 against :474-475: with every weight 4 pi / D the two forms agree."""
    fx = S.case(*S.BASE)
    w = torch.full((fx.dirs.shape[0],), 4 * np.pi / fx.dirs.shape[0], dtype=F64)
    a = S.shade_integrate(fx.maps, fx.rays, fx.dirs, fx.light_idx, fx.vis, fx.indirect, fx.env, None, True, False, 0.5, F64)
    b = S.shade_integrate(fx.maps, fx.rays, fx.dirs, fx.light_idx, fx.vis, fx.indirect, fx.env, w, False, False, 0.5, F64)
    assert float((a - b).abs().max()) < 1e-12


def test_importance_restatement_is_the_oracles():
    t = S.importance_case(5, 64)
    mine = S.relight_importance(t.normal, t.albedo, t.rough, t.fresnel, t.rays_d, t.light_dir, t.light_rgb, t.light_pdf, t.vis, F64)
    d = lambda x: x.double()
    surf2c = O.safe_l2_normalize(-d(t.rays_d))
    spec = O.ggx_specular(d(t.normal), surf2c, d(t.light_dir), d(t.rough).reshape(-1, 1), d(t.fresnel))
    contrib = (d(t.albedo)[:, None, :] / np.pi + spec) * (d(t.vis)[..., None] * d(t.light_rgb)) * \
        torch.einsum("ijk,ik->ij", d(t.light_dir), d(t.normal))[:, :, None] / d(t.light_pdf)[..., None]
    assert torch.equal(mine, O.linear2srgb(torch.mean(contrib, dim=1).clamp(0.0, 1.0)))
    assert ((t.vis == 0) | (torch.einsum("ijk,ik->ij", d(t.light_dir), d(t.normal)) > 1e-6)).all() and (t.vis == 0).any() and (t.vis > 0).any()


# ---- no exclusions: margins and designed rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_no_fixture_needs_an_exclusion(shape):
    """Every branch predicate -- the cosine mask, the four [1e-6, 1] clamps, both denominator clamps, the sign of N.V, the clip,
    the sRGB knee, the acc threshold -- takes the same value in float32 and float64 on every row, in all four variants (weighting x
    indirect light); every random row keeps the module's margins; the invariant holds; the designed rows take their branches."""
    fx = S.case(*shape)
    M, D = fx.vis.shape
    tot64, tot32 = {}, {}
    p64, p32 = S.fixture_predicates(fx, F64, tot64), S.fixture_predicates(fx, F32, tot32)
    assert len(p64) == 9 + 2 * len(S.VARIANTS) and S.same(p64, p32)
    q = S.geometry(fx.maps[:, 4:7], fx.rays[:, 3:6], fx.dirs, fx.maps[:, 10], F64)
    rnd = fx.random
    assert S.geometry_margins_ok(q)[rnd].all() and all(S.total_margins_ok(t)[rnd].all() for t in tot64.values())
    assert int((~rnd).sum()) == len(fx.rows) == sum(i < M for i in S.DESIGNED.values())
    off = q["cos"] <= S.COS_THRESHOLD
    assert (fx.vis[off] == 0).all() and (fx.indirect[off] == 0).all()
    assert fx.light_idx[0] == -1 and (M == 1 or fx.light_idx[-1] == fx.env.shape[0])
    fg = p64["fg"].bool()
    r = fx.rows
    if "acc_at_threshold" in r:
        assert fx.maps[r["acc_at_threshold"], 14] == 0.5 and not fg[r["acc_at_threshold"]]
    if "flip" in r:
        assert p64["sign"][r["flip"]] == -1 and p64["sign"][0] != 0
    if "nov_zero" in r:
        assert q["nov0"][r["nov_zero"]] == 0 and p32["sign"][r["nov_zero"]] == 0 and p64["nov"][r["nov_zero"]] == 0
    if "normal_double" in r:
        n = fx.maps[:, 4:7].double().norm(dim=1)
        assert abs(float(n[r["normal_half"]]) - 0.5) < 1e-6 and abs(float(n[r["normal_double"]]) - 2) < 1e-6 and n[r["normal_zero"]] == 0
    if "ray_zero" in r:
        assert abs(float(fx.rays[r["ray_long"], 3:6].double().norm()) - 3) < 1e-6 and (fx.rays[r["ray_zero"], 3:6] == 0).all()
    if "mirror_1" in r:
        for name, low in (("mirror_002", True), ("mirror_03", False), ("mirror_1", False)):
            i = r[name]
            for p, dt in ((p64, F64), (p32, F32)):
                qq = S.geometry(fx.maps[i:i + 1, 4:7], fx.rays[i:i + 1, 3:6], fx.dirs[0:1], fx.maps[i:i + 1, 10], dt)
                assert qq["noh"][0, 0] == 1 and p["noh"][i, 0] == 1                     # exactly 1: inside the clamp, inclusively
                assert (p["nom"][i, 0, 0] == 0) == low
        assert float(q["nom"][r["mirror_002"], 0, 0]) < 1e-12                          # 2.2e-13 against the clamp's 1e-6
    if "nom_top" in r and D > 1:
        for p, dt in ((p64, F64), (p32, F32)):
            qq = S.geometry(fx.maps[:, 4:7], fx.rays[:, 3:6], fx.dirs, fx.maps[:, 10], dt)
            top = torch.tensor(4 * np.pi, dtype=dt)
            assert qq["nom"][r["nom_top"], 1, 0] == top and p["nom"][r["nom_top"], 1, 0] == 1         # on the upper edge: passes
        assert fx.vis[r["nom_top"], 1] > 0
    if "acc_above_threshold" in r:
        assert fg[r["acc_above_threshold"]] and fx.maps[r["acc_above_threshold"], 14] == np.nextafter(np.float32(0.5), np.float32(1))
        for v in S.VARIANTS:
            for tot in (tot64, tot32):
                assert (tot[v][r["bright"]] > 1).all()
                assert (tot[v][r["below_horizon"]] == 0).all() and (tot[v][r["normal_zero"]] == 0).all()
                assert ((tot[v][r["srgb_linear"]] > 0) & (tot[v][r["srgb_linear"]] <= S.KNEE)).all()
    if M >= 65:
        assert (~fg[rnd]).any() and fg[rnd].any()
        lit = q["cos"] > S.COS_THRESHOLD
        assert (fx.vis[lit] == 0).any()                                                # the backward's v != 0 branch, both ways


def test_small_fixtures_need_no_exclusion_either():
    for M, D in S.GGX_SHAPES:
        t = S.ggx_case(M, D)
        q = S.geometry(t.normal, -t.view, t.l, t.rough, F64)
        assert S.same(S.geometry_predicates(q), S.geometry_predicates(S.geometry(t.normal, -t.view, t.l, t.rough, F32)))
        if M > 2:
            assert q["nov0"][1] == 0 and q["noh"][2, 0] == 1 and S.geometry_margins_ok(q)[3:].all()
    for M, Ns in S.IMPORTANCE_CASES:
        t = S.importance_case(M, Ns)
        assert S.same(S.importance_predicates(t, F64), S.importance_predicates(t, F32))
        q = S.geometry(t.normal, t.rays_d, t.light_dir, t.rough, F64)
        assert S.geometry_margins_ok(q).all() and (q["cos"] < 0).any() and (M == 1 or q["nov0"][1] != 0)
    for fx in (S.horizon_case(), S.clamp_case()):
        assert S.same(S.fixture_predicates(fx, F64), S.fixture_predicates(fx, F32))
    fx = S.horizon_case()
    assert S.geometry(fx.maps[:, 4:7], fx.rays[:, 3:6], fx.dirs, fx.maps[:, 10], F32)["cos"][0].tolist() == [0.0, 2.0 ** -20, 2.0 ** -19, -(2.0 ** -19)]
    assert S.shade_setup(fx.maps, fx.rays, fx.dirs, 0.5, F32)[1][0].tolist() == [False, False, True, False]


def test_horizon_row_in_float32_is_a_chain_of_single_roundings():
    """The float32 restatement on horizon_case() equals ((albedo / pi * (vis * env)) * cosine) * weight in numpy float32, one
    rounding per operation -- what the device must reproduce bit for bit -- and only direction 2 contributes."""
    fx = S.horizon_case()
    f = np.float32
    alb, env, wd = fx.maps[0, 7:10].numpy(), fx.env[0, 2].numpy(), fx.weight_d.numpy()
    light = f(fx.vis[0, 2].item()) * env
    want = (((alb / f(np.pi)) * light) * f(2.0 ** -19)) * wd[2]
    got = S.shade_integrate(fx.maps, fx.rays, fx.dirs, fx.light_idx, fx.vis, None, fx.env, fx.weight_d, False, False, 0.5, F32)
    assert np.array_equal(got[0].numpy(), want.astype(f)) and (want > 0.01).all() and (want < 0.9).all()
    want_ea = (((f(4 * np.pi) * (alb / f(np.pi))) * light) * f(2.0 ** -19)) / f(4)
    got = S.shade_integrate(fx.maps, fx.rays, fx.dirs, fx.light_idx, fx.vis, None, fx.env, None, True, False, 0.5, F32)
    assert np.array_equal(got[0].numpy(), want_ea.astype(f))
    one = S.horizon_case()
    one.dirs, one.vis, one.env, one.weight_d = fx.dirs[2:3], fx.vis[:, 2:3], fx.env[:, 2:3], fx.weight_d[2:3]
    assert torch.equal(S.shade_integrate(one.maps, one.rays, one.dirs, one.light_idx, one.vis, None, one.env, one.weight_d, False, False, 0.5, F32),
                       S.shade_integrate(fx.maps, fx.rays, fx.dirs, fx.light_idx, fx.vis, None, fx.env, fx.weight_d, False, False, 0.5, F32))


def test_surface_point_rounded_twice_differs_from_a_fused_one():
    """So that the GPU test's bit comparison of surf can fail: on every setup fixture with more than a handful of rows some element of
    o + depth * d differs between two roundings and one."""
    for M, D in S.SETUP_SHAPES:
        fx = S.case(M, D, 3, 0.5)
        twice = S.shade_setup(fx.maps, fx.rays, fx.dirs, 0.5, F32)[0]
        once = S.surf_fused(fx.maps, fx.rays)
        n = int((twice != once).sum())
        print(f"\n[shade surf M {M} D {D}] elements that a fused multiply-add changes: {n} of {3 * M}")
        assert twice.dtype == F32 and (n > 0 or M < 7)
        assert float((twice.double() - once.double()).abs().max()) <= 2.0 ** -19          # one ulp below 32


def test_clamped_denominator_passes_no_gradient():
    """clamp_case(): float64 autograd equals the hand-written gradient with the denominator held at 1e-6."""
    fx = S.clamp_case()
    q = S.geometry(fx.maps[:, 4:7], fx.rays[:, 3:6], fx.dirs, fx.maps[:, 10], F64)
    assert float(q["nom"][0, 0, 0]) < 1e-12 and q["noh"][0, 0] == 1
    cot = torch.tensor([[0.5, -1.25, 2.0]])
    out, gm, ge = S.shade_gradients(fx, True, False, False, cot, F64)
    assert ((out > S.KNEE) & (out < 1)).all()
    g_rough, g_normal = S.clamp_gradients(fx, cot)
    assert abs(float(gm[0, 10] / g_rough) - 1) < 1e-12 and float((gm[0, 4:7] - g_normal).abs().max()) < 1e-12 * float(g_normal.abs().max())
    assert float(g_rough) != 0 and (ge != 0).all()
    # the upper edge: the raw value is 4 pi exactly, the gradient passes, and a roughness gradient without it would have the opposite sign
    fx = S.clamp_case(top=True)
    for dt in (F64, F32):
        q = S.geometry(fx.maps[:, 4:7], fx.rays[:, 3:6], fx.dirs, fx.maps[:, 10], dt)
        assert q["nom"][0, 0, 0] == torch.tensor(4 * np.pi, dtype=dt) and q["nov"][0] == 1 and q["noh"][0, 0] == 1 and q["nol"][0, 0] == 1
    assert S.same(S.fixture_predicates(fx, F64), S.fixture_predicates(fx, F32))
    out, gm, _ = S.shade_gradients(fx, True, False, False, cot, F64)
    held, g_normal = S.clamp_gradients(fx, cot, 4 * np.pi)
    print(f"\n[shade upper edge] roughness gradient {float(gm[0, 10]):.6f}, with the denominator held {float(held):.6f}")
    assert ((out > S.KNEE) & (out < 1)).all() and abs(float(gm[0, 10] / held) - 1) > 0.1
    assert float((gm[0, 4:7] - g_normal).abs().max()) < 1e-12 * float(g_normal.abs().max())      # what reaches N is along N: removed


# ---- float64 autograd everywhere, and the yardstick -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(dict.fromkeys(S.BACKWARD_SHAPES)), ids=lambda s: "-".join(str(v) for v in s))
def test_shading_gradients_and_float32_distances(shape):
    fx = S.case(*shape)
    M = fx.maps.shape[0]
    cot = S.cotangent(M)
    variants = [(ea, srgb, ind) for ea in (False, True) for srgb in (False, True) for ind in (False, True)] if shape == S.BASE else [(False, True, True)]
    for ea, srgb, ind in variants:
        o64, gm64, ge64 = S.shade_gradients(fx, ind, ea, srgb, cot, F64)
        o32, gm32, ge32 = S.shade_gradients(fx, ind, ea, srgb, cot, F32)
        assert all(torch.isfinite(x).all() for x in (o64, gm64, ge64, o32, gm32, ge32)) and gm32.dtype == F32
        d = {"out": S.distance(o32, o64), "env": S.distance(ge32, ge64), **{k: S.distance(gm32[:, c], gm64[:, c]) for k, c in S.GROUPS.items()}}
        print(f"\n[shade float32 {shape} equal_area {int(ea)} srgb {int(srgb)} indirect {int(ind)}] " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
        assert max(d.values()) < 1e-2 and (gm64[:, :4] == 0).all() and (gm64[:, 14:] == 0).all()
        bg = ~(fx.maps[:, 14] > 0.5)
        assert (o64[bg] == 1).all() and (gm64[bg] == 0).all()
        if "bright" in fx.rows:
            assert (gm64[fx.rows["bright"]] == 0).all() and (gm64[fx.rows["below_horizon"]] == 0).all()
            assert (gm64[fx.rows["mirror_03"], 4:7] != 0).any()
        picked = torch.zeros(fx.env.shape[0], dtype=torch.bool)
        picked[fx.light_idx.long().clamp(0, fx.env.shape[0] - 1)] = True
        assert (ge64[~picked] == 0).all() and (ge64[picked] != 0).any()


def test_forward_float32_distances():
    for shape in S.FORWARD_SHAPES:
        fx = S.case(*shape)
        for ea, srgb in ((False, True), (True, False)):
            run = lambda dt: S.shade_integrate(fx.maps, fx.rays, fx.dirs, fx.light_idx, fx.vis, fx.indirect, fx.env, fx.weight_d, ea, srgb, 0.5, dt)
            d = S.distance(run(F32), run(F64))
            print(f"\n[shade float32 forward {shape} equal_area {int(ea)} srgb {int(srgb)}] {d:.2e}")
            assert np.isfinite(d) and d < 1e-3
    for M, D in S.GGX_SHAPES:
        t = S.ggx_case(M, D)
        a, b = (O.ggx_specular(t.normal.to(dt), t.view.to(dt), t.l.to(dt), t.rough.to(dt), t.fresnel.to(dt)) for dt in (F32, F64))
        print(f"\n[shade float32 ggx M {M} D {D}] {S.distance(a, b):.2e}")
        assert torch.isfinite(b).all() and S.distance(a, b) < 1e-2
    for M, Ns in S.IMPORTANCE_CASES:
        t = S.importance_case(M, Ns)
        a, b = (S.relight_importance(t.normal, t.albedo, t.rough, t.fresnel, t.rays_d, t.light_dir, t.light_rgb, t.light_pdf, t.vis, dt) for dt in (F32, F64))
        print(f"\n[shade float32 importance M {M} Ns {Ns}] {S.distance(a, b):.2e}")
        assert torch.isfinite(b).all() and S.distance(a, b) < 1e-3 and float(b.max() - b.min()) > 0


@pytest.mark.parametrize("n_sg,L,D", S.SG_CASES)
def test_env_sg_gradients_and_float32_distances(n_sg, L, D):
    """abs() on lambda and mu: the derivative carries their sign, and is exactly 0 at 0, as torch.abs's."""
    c = S.sg_case(n_sg, L, D)
    o64, g64 = S.sg_gradients(c, F64)
    o32, g32 = S.sg_gradients(c, F32)
    print(f"\n[shade float32 env_sg n_sg {n_sg} L {L} D {D}] out {S.distance(o32, o64):.2e}, grad {S.distance(g32, g64):.2e}")
    assert torch.isfinite(g64).all() and torch.isfinite(g32).all() and o64.shape == (L, D, 3) and S.distance(g32, g64) < 1e-3
    flipped = c.sgs.clone()
    flipped[0, 3], flipped[0, 5] = -flipped[0, 3], -flipped[0, 5]
    c2 = S.sg_case(n_sg, L, D)
    c2.sgs = flipped
    o2, g2 = S.sg_gradients(c2, F64)
    assert torch.equal(o2, o64) and g2[0, 3] == -g64[0, 3] and g2[0, 5] == -g64[0, 5] and g2[0, 4] == g64[0, 4]
    if n_sg > 5:
        assert g64[1, 4] == 0 and g64[2, 3] == 0 and (g64[1, 5:] != 0).all()
        assert abs(float(c.sgs[3, :3].norm()) - 0.1) < 1e-6 and abs(float(c.sgs[4, :3].norm()) - 10) < 1e-5
        if D >= 85:
            far = S.env_sg(c.sgs[5:6], c.rot, c.dirs, F32)
            assert (far == 0).any() and (S.env_sg(c.sgs[5:6], c.rot, c.dirs, F64) > 0).all()      # underflow in float32 only


def test_records_and_lookup_restatements():
    fx = S.case(*S.BASE)
    off, cnt, w, rgb = S.records_case(fx)
    assert sorted(set(cnt.tolist())) == [0, 1, 2, 5, 96] and int(cnt.sum()) == w.shape[0]
    on = S.shade_setup(fx.maps, fx.rays, fx.dirs, -1e30, F64)[1].reshape(-1)
    assert (cnt[~on] == 0).all()
    ref = S.records_sum(off, cnt, w, rgb, F64)
    k = int(torch.nonzero(cnt == 96)[0])
    seg = slice(int(off[k]), int(off[k]) + 96)
    assert torch.allclose(ref[k], (w[seg].double()[:, None] * rgb[seg].double()).sum(0), rtol=1e-13, atol=0)
    print(f"\n[shade float32 records] {S.distance(S.records_sum(off, cnt, w, rgb, F32), ref):.2e}")
    hdr, dirs = S.lookup_case()
    inside = torch.ones(dirs.shape[0], dtype=torch.bool)
    inside[4:6] = False
    a, b = O.envlight_lookup(hdr, dirs[inside]), O.envlight_lookup(hdr.double(), dirs[inside].double())
    print(f"\n[shade float32 lookup] {S.distance(a, b):.2e}")
    assert torch.isfinite(b).all() and S.distance(a, b) < 1e-4 and dirs[4, 2] > 1 and dirs[5, 2] < -1
