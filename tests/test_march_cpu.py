"""CPU leg of the march and compositing suite (tests/test_gpu_march_kernels.py): the fixtures' margins and redraw caps, the kernel
each scene selects (from the launchers' own arithmetic), and the tie of the restatement (tests/march_reference.py) to the pinned
oracle.  Prints the float32 restatement's own distance from float64 per fixture -- a tenth of what the GPU tests allow."""
import pytest
import torch

from oracle import tensoir_oracle as O
from tests import march_reference as M
from tests.helpers import T, golden_scene

F32, F64 = torch.float32, torch.float64
PRIMARY_CASES = list(dict.fromkeys(M.PRIMARY_FORWARD + M.PRIMARY_BACKWARD))


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)


def caps_hold(fx, n, what):
    """The redraw is capped: the fixture came out clean, in at most REDRAW_ROUNDS rounds, with at most REDRAW_SHARE of its rays
    drawn again."""
    assert fx.clean, (what, "rays still break a margin after the last round")
    assert fx.rounds <= M.REDRAW_ROUNDS, (what, fx.rounds)
    assert int(fx.redrawn.sum()) <= M.REDRAW_SHARE * n, (what, int(fx.redrawn.sum()), n)


def march_margins(label, sc, r64, r32, t_stops):
    """Every discrete decision of a march fixture, with its margin, from the un-stopped float64 and float32 runs."""
    thres = sc.weight_thres
    rel = (r64.weight / thres - 1).abs()
    assert float(rel.min()) > M.W_MARGIN, (label, "weight threshold", float(rel.min()))
    assert torch.equal(r64.keep, r32.keep) and torch.equal(r64.cnt, r32.cnt), label
    for t in t_stops:
        if t > 0:
            rel_t = (r64.T_ends / t - 1).abs()
            assert float(rel_t.min()) > M.T_MARGIN, (label, "early stop", t, float(rel_t.min()))
            assert torch.equal(r64.T_ends < t, r32.T_ends < t), (label, t)
    assert torch.equal(M.occupancy(sc, r64.pts32, r64.inside, F64), r64.valid) and torch.equal(r64.valid, r32.valid), (label, "validity")
    if O.density_act(sc) == "relu":
        assert float(r64.feat[r64.valid].abs().min()) > M.RELU_MARGIN and torch.equal(r64.feat > 0, r32.feat > 0), (label, "relu")
    print(f"\n[march cpu {label}] weights {float(rel.min()):.1e} relative from the threshold at the nearest; records {int(r64.cnt.sum())}; "
          f"float32 restatement: weight {M.distance(r32.weight, r64.weight):.2e} acc {M.distance(r32.acc, r64.acc):.2e} "
          f"depth {M.distance(r32.depth, r64.depth):.2e}")


@pytest.mark.parametrize("case", PRIMARY_CASES, ids=ident)
def test_primary_fixture_margins(case):
    name, B, S, _j = case
    fx = M.primary_case(*case)
    caps_hold(fx, B, case)
    assert not bool(fx.redrawn[:min(B, M.N_DESIGNED + 1)].any()), "a designed ray broke a margin and was replaced"
    assert fx.rays.shape == (B, 6) and fx.rays.dtype == F32
    sc = fx.scene.sc
    march_margins(f"primary {ident(case)}", sc, M.primary_reference(fx, 0.0, F64), M.primary_reference(fx, 0.0, F32), M.PRIMARY_T_STOPS)
    # what the designed rays are for
    r = M.primary_reference(fx, 0.0, F64)
    lo, hi = sc.aabb[0], sc.aabb[1]
    if B >= M.N_DESIGNED + 1 and S >= 63:
        d0, inside_start, miss, side, one_zero = 0, 2, 3, 4, 5           # base_rays puts a fan ray second
        assert int((fx.rays[d0, 3:6] == 0).sum()) == 2 and int((fx.rays[one_zero, 3:6] == 0).sum()) == 1
        assert bool(((fx.rays[inside_start, :3] > lo) & (fx.rays[inside_start, :3] < hi)).all())
        assert not bool(r.inside[miss].any()) and float(r.acc[miss]) == 0
        assert bool(r.inside[side, 0]) or bool(r.inside[side].any())
        assert bool(r.inside[side].any()) and not bool(r.inside[side, -1]), "the ray does not leave the box before its last sample"
        # ray 0 crosses an opaque stretch, where 1 - alpha + 1e-10 is 1e-10 (on the fine grid 65 samples end before the middle)
        assert fx.scene.grid == M.FINE_GRID or M.least_pass(sc, r) < 1e-16, M.least_pass(sc, r)


@pytest.mark.parametrize("route,n_sample", M.SECONDARY_CASES, ids=ident)
def test_secondary_fixture_margins(route, n_sample):
    name = M.SECONDARY_ROUTES[route][0]
    fx = M.secondary_case(name, n_sample)
    n = fx.origins.shape[0]
    caps_hold(fx, n, (route, n_sample))
    assert not bool(fx.redrawn[:3].any())
    sc = fx.scene.sc
    march_margins(f"secondary {route} n_sample {n_sample}", sc, M.secondary_reference(fx, 0.0, F64), M.secondary_reference(fx, 0.0, F32),
                  M.SECONDARY_T_STOPS)
    r = M.secondary_reference(fx, 0.0, F64)
    assert not bool(r.inside[2].any()) and not bool(r.inside[1, 0])
    if n_sample >= 31:
        assert bool(r.inside[1].any()), "ray 1 does not enter the box"
        stopped = ~M.secondary_reference(fx, 1e-4, F64).live
        assert bool(stopped.any()) == (n_sample > M.SECONDARY_STEP), "1e-4 stops rays exactly where there is a second step"
        assert bool(((r.t_end > 0.01) & (r.t_end < 0.99)).any()) and bool((r.t_end > 0.99).any())


@pytest.mark.parametrize("name", sorted({v[0] for v in M.SECONDARY_ROUTES.values()}))
def test_secondary_grid_fixture_margins(name):
    fx = M.secondary_grid_case(name, 33)
    caps_hold(fx, fx.origins.shape[0], name)
    march_margins(f"secondary grid {name}", fx.scene.sc, M.secondary_reference(fx, 0.0, F64), M.secondary_reference(fx, 0.0, F32),
                  M.SECONDARY_T_STOPS)
    for n_dirs in (1, 3, 24):
        sub = M.grid_subset(fx, n_dirs)
        assert torch.equal(sub.origins, fx.points[:, None, :].expand(-1, n_dirs, 3).reshape(-1, 3))
        assert torch.equal(sub.dirs, fx.table[:n_dirs][None].expand(M.GRID_POINTS, -1, 3).reshape(-1, 3))


@pytest.mark.parametrize("B", M.COMPOSITE_B)
def test_composite_fixture_margins(B):
    fx = M.composite_case(B)
    caps_hold(fx, B, B)
    assert not bool(M.composite_bad_rays(fx)[~fx.designed].any())
    s64, s32 = M.composite_states(fx, F64), M.composite_states(fx, F32)
    for k in s64:
        assert torch.equal(s64[k], s32[k]), k                               # the designed rays included
    cnt = (fx.offsets[1:] - fx.offsets[:-1])
    assert int(cnt.max()) < fx.S and bool((fx.acc >= 0).all()) and bool((fx.acc <= 1).all())
    if B == 257:
        assert sorted(set(cnt.tolist())) == sorted(M.RECORD_COUNTS)
    for r in range(B):                                                      # rec_k: distinct, increasing samples of the ray
        k = fx.rec_k[int(fx.offsets[r]):int(fx.offsets[r + 1])]
        assert bool((k[1:] > k[:-1]).all()) and (k.numel() == 0 or (int(k[0]) >= 0 and int(k[-1]) < fx.S))
    if fx.rows:
        e, one, clip = fx.rows["empty"], fx.rows["acc_one"], fx.rows["clipped"]
        assert int(cnt[e]) == 0 and float(fx.acc[e]) == 0 and float(fx.acc[one]) == 1
        for wb in (0, 1):
            aux = {}
            with torch.no_grad():
                maps = M.composite(*M.composite_inputs(fx), wb, 1, F32, aux=aux)
            assert bool((aux["rgb"][clip] > 1).all())
            assert maps[e, 4:7].tolist() == ([0.0, 0.0, 1.0] if wb else [0.0, 0.0, 0.0])
    for wb in (0, 1):
        for rl in (0, 1):
            with torch.no_grad():
                m64, m32 = M.composite(*M.composite_inputs(fx), wb, rl, F64), M.composite(*M.composite_inputs(fx), wb, rl, F32)
            print(f"\n[march cpu composite B {B} white_bg {wb} relight {rl}] float32 restatement " +
                  " ".join(f"{g} {M.distance(m32[:, c], m64[:, c]):.1e}" for g, c in M.COLUMN_GROUPS.items()))


def test_scenes_select_the_arms():
    """From the launchers' arithmetic (tir_train.hip: tir_march_primary_bwd; tir_march.hip: tir_march_secondary_ids_fwd): the
    small scenes take the LDS-lines backward and the 512-thread secondary kernel, `long_axis` the global-atomic backward,
    `lds_1024` the 1024-thread secondary kernel; the thin grids stay within tir_plane_index_ok."""
    for name in M.SCENES:
        s = M.scene(name)
        assert M.plane_index_ok(s.grid, s.n_dcomp), name
        assert s.sc.grid == s.grid and s.sc.density_plane[0].shape[1] == s.n_dcomp
        assert (M.primary_bwd_arm(s.grid, s.n_dcomp) == "global-atomic") == (name == "long_axis"), name
    g = M.scene("long_axis").grid
    assert sum(g) * 16 * 4 > 96 * 1024 >= (sum(g) - 7) * 16 * 4                # just past the LDS arm
    for route, (name, lds) in M.SECONDARY_ROUTES.items():
        s = M.scene(name)
        for n in M.SECONDARY_SAMPLES:
            assert M.secondary_arm(s.grid, s.n_dcomp, n, lds) == (route if route.startswith("lds") else "plain"), (route, n)
    s = M.scene("d16_a48")
    for n in M.SECONDARY_SAMPLES_PLAIN:
        assert M.secondary_arm(s.grid, s.n_dcomp, n, True) == "plain"           # more than 96 samples: the plain kernel whatever the option
    assert M.scene("d16_a48").sc.alpha_volume is not None and M.scene("d16_a48_open").sc.alpha_volume is None
    vol = M.scene("d16_a48").sc.alpha_volume
    assert 0 < float(vol.mean()) < 1, "the mask culls nothing or everything"


# ---- the restatement against the pinned oracle -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sc(golden):
    return golden_scene(golden)


def test_primary_restatement_equals_oracle(golden, sc):
    """On the golden rays the float32 restatement of the march has the bits of O.forward_primary's weights (the same tensor
    operations), and composite() on the oracle's own per-record decoder outputs gives its maps: the sums run over the records in
    another order than the oracle's dense sums, so float32 agrees to 2e-6 of each map's maximum and float64 to 1e-13."""
    rays, lidx = T(golden, "rays/rays"), T(golden, "rays/light_idx")
    B = rays.shape[0]
    S = O.step_geometry(sc.aabb, sc.grid, sc.step_ratio).n_samples
    noise = torch.randn(B, S, 3, generator=torch.Generator().manual_seed(7))
    for dtype, tol in ((F32, 2e-6), (F64, 1e-13)):
        scd = sc.to(dtype)
        for wb, rl in ((True, True), (False, True), (True, False), (False, False)):
            with torch.no_grad():
                out, aux = O.forward_primary(scd, rays.to(dtype), lidx, white_bg=wb, is_relight=rl, brdf_jitter=noise, backend="explicit",
                                             return_aux=True)
            if dtype == F32 and wb and rl:
                r = M.march_primary(sc, rays, S, None, 0.0, F32)
                assert torch.equal(r.weight, aux.weight) and torch.equal(r.sigma, aux.sigma) and torch.equal(r.valid, aux.valid)
                assert torch.equal(r.xyz32, aux.xyz) and torch.equal(r.keep, aux.app_mask)
                assert torch.equal(r.acc, out[6])
            keep = aux.app_mask
            ray, _k = torch.nonzero(keep, as_tuple=True)
            xa = aux.xyz[keep]
            with torch.no_grad():
                rad_f, int_f = O.both_feature(scd, xa, lidx.view(-1, 1)[ray], "explicit")
                rgb = O.render_rgb(scd, rays[ray, 3:6].to(dtype), rad_f)
                brdf = O.render_brdf(scd, xa, int_f)
                xj = xa + noise[keep].to(dtype) * 0.01
                brdf_j = O.render_brdf(scd, xj, O.intrin_feature(scd, xj, "explicit"))
                der, pred = O.density_grad(scd, xa)[2], O.render_normal(scd, xa, int_f)
                off = torch.cat([torch.zeros(1, dtype=torch.int64), keep.sum(1).cumsum(0)]).int()
                maps = M.composite(rays, off, aux.weight[keep], rgb, brdf, brdf_j, pred, der, aux.weight.sum(-1), (aux.weight * aux.z).sum(-1),
                                   wb, rl, dtype, fixed_fresnel=sc.fixed_fresnel)
            want = {"rgb": out[0], "depth": out[1], "acc": out[6]}
            if rl:
                want.update(normal=out[2], albedo=out[3], roughness=out[4], fresnel=out[5], normals_diff=out[7], normals_orientation=out[8])
                assert abs(float(maps[:, 17].mean()) - float(out[10])) <= tol * max(float(out[10]), 1e-30) * 100
                assert abs(float(maps[:, 18].mean()) - float(out[11])) <= tol * max(float(out[11]), 1e-30) * 100
            worst = 0.0
            for group, ref in want.items():
                d = M.distance(maps[:, M.COLUMN_GROUPS[group]], ref.reshape(B, -1))
                worst = max(worst, d)
                assert d <= tol, (dtype, wb, rl, group, d)
            print(f"\n[march cpu oracle tie {dtype} white_bg {int(wb)} relight {int(rl)}] composite() from the oracle's maps: {worst:.1e}")


def test_secondary_restatement_equals_oracle(golden, sc):
    """On the golden secondary inputs the float32 restatement has the bits of O.compute_transmittance and of O.compute_radiance's
    visibility and 1 - acc (the same tensor operations); its records, decoded and summed, give compute_radiance's indirect light
    to 1e-6 (another order of the sum)."""
    p, d, l = T(golden, "sec/pts"), T(golden, "sec/dirs"), T(golden, "sec/light_idx")
    with torch.no_grad():
        r = M.march_secondary(sc, p, d, 96, 0.0, F32)
        v, nf = O.compute_transmittance(sc, p, d, 96, M.NEAR, M.FAR, "explicit")
        assert torch.equal(r.t_end, v) and torch.equal(r.one_minus_acc, nf)
        v2, nf2, ind = O.compute_radiance(sc, p, d, l, 96, M.NEAR, M.FAR, "explicit")
        assert torch.equal(r.t_end, v2) and torch.equal(r.one_minus_acc, nf2)
        ray, _k = torch.nonzero(r.keep, as_tuple=True)
        rgb = O.render_rgb(sc, d[ray], O.app_feature(sc, r.xyz32[r.keep], l.view(-1, 1)[ray], "explicit"))
        mine = torch.zeros_like(ind).index_add(0, ray, r.weight[r.keep][:, None] * rgb)
    dist = M.distance(mine, ind)
    print(f"\n[march cpu oracle tie secondary] records {int(r.keep.sum())}, indirect light from them {dist:.1e}")
    assert dist <= 1e-6 and int(r.keep.sum()) > 0
    # the early stop per 32-sample step, on these rays: the restatement against a march cut by hand
    r_stop = M.march_secondary(sc, p, d, 96, 1e-4, F32)
    T_full = torch.cumprod(1.0 - O.raw2alpha(r.sigma, torch.cat((r.z[:, 1:] - r.z[:, :-1], torch.zeros_like(r.z[:, :1])), -1) * sc.distance_scale)[0] + 1e-10, -1)
    for i in range(p.shape[0]):
        stop = next((e for e in (31, 63, 95) if float(T_full[i, e]) < 1e-4), 95)
        assert torch.equal(r_stop.weight[i, :stop + 1], r.weight[i, :stop + 1]) and bool((r_stop.weight[i, stop + 1:] == 0).all())
        assert float(r_stop.t_end[i]) == float(T_full[i, stop])
