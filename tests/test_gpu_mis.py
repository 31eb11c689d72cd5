"""Relighting with multiple importance sampling on the GPU (tir_env_mis_setup, tir_relight_mis, relight.*(mis=...))
against the restatement of tests/mis_reference.py.

Comparison rule (DESIGN 4.8's, as tests/test_gpu_shade_kernels.py): the device's distance from the float64 restatement -- max abs
difference over the float64 result's maximum -- is at most ten times the float32 restatement's own distance on the same fixture
and never less than ten half-ulps of 1.  `cell` and `active` are branches on rounded values: they are compared exactly on every
pair that is not exempt (tests/mis_reference.py says which; tests/test_mis_cpu.py asserts that they are at most 1 % and that the
float32 and float64 restatements agree on all others).  The device returns no lobe choice; a pair drawn from another lobe than the
restatement's has a direction that is off by the lobes' distance, which the rule on `dirs` does not pass.  Every test prints
`device d (bound b)`."""
import numpy as np
import pytest
import torch

from tests import mis_reference as R
from tests import shade_reference as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENTINEL = -7.0


def dev(t):
    return None if t is None else t.contiguous().cuda()


def check(label, got, f32, f64):
    d, b = S.distance(got, f64), S.bound(f32, f64)
    print(f"\n[mis {label}] device {d:.2e} (bound {b:.2e})")
    assert torch.isfinite(torch.as_tensor(got)).all() and d <= b, (label, d, b)


@pytest.fixture(scope="module")
def envs():
    from tensoir_amd import relight
    return {name: relight.Environment_Light(hdr_maps={name: R.light(name).hdr}, device="cuda") for name in R.MAPS}


def device_setup(env, name, pts, n_l, n_b, block_pairs=256, m_dev=None, buffers=None, guide=True, records=True, offset=R.OFFSET):
    from tensoir_amd import ops
    table = env.cell_records(name) if records else env.hdr_dir[name].view(-1, 3)
    return ops.env_mis_setup(env.hdr_row_cdf[name], env.hdr_col_cdf[name], table, env.hdr_row_sin[name], dev(pts.normal), dev(pts.rays_d),
                             dev(pts.rough), n_l, n_b, R.SELECT, R.SEED, offset, block_pairs, env.hdr_cdf_guide[name] if guide else None, m_dev,
                             env_pdf=None if records else env.hdr_pdf_return[name].view(-1), buffers=buffers)


def listed(pair_ids, n_active, total):
    ids = pair_ids.cpu()[: int(n_active)].long()
    mask = torch.zeros(total, dtype=torch.bool)
    mask[ids] = True
    assert int(mask.sum()) == ids.numel(), "a pair is listed twice"
    return ids, mask


CASES = [(name, M, n_l, n_b) for name in R.MAPS for M in R.POINTS for n_l, n_b in R.SPLITS]


# ---- setup ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,n_l,n_b", CASES, ids=lambda v: str(v))
def test_setup(envs, name, M, n_l, n_b):
    """M of 1, 5, 67; one pair per point of either kind, 63 and 64 pairs of one kind, 64 and 130 of both; both maps; blocks of 256
    pairs, so that 67 x 130 pairs span 35 blocks with six pairs in the last."""
    from tensoir_amd import ops
    env, pts, N = envs[name], R.points(M), n_l + n_b
    a64, a32 = R.case(name, M, n_l, n_b, F64), R.case(name, M, n_l, n_b, F32)
    keep = ~a64.exempt
    dirs, cell, pdf_mix, vis, pair_ids, n_active = device_setup(env, name, pts, n_l, n_b)
    assert dirs.shape == (M, N, 3) and cell.shape == pdf_mix.shape == vis.shape == (M, N) and cell.dtype == torch.int32
    _, active = listed(pair_ids, n_active, M * N)
    active = active.view(M, N)
    print(f"\n[mis setup {name} M {M} n_l {n_l} n_b {n_b}] {int(active.sum())} of {M * N} pairs active, {int((~keep).sum())} exempt")
    assert torch.equal(cell.cpu().long()[keep], a64.cell[keep])
    assert torch.equal(active[keep], a64.active[keep])
    assert (pdf_mix.cpu()[~active] == 1).all() and (vis.cpu()[~active] == 0).all()
    check(f"setup dirs {name} M {M} n_l {n_l} n_b {n_b}", dirs.cpu()[keep], a32.dirs[keep], a64.dirs[keep])
    check(f"setup pdf_mix {name} M {M} n_l {n_l} n_b {n_b}", pdf_mix.cpu()[keep], a32.pdf_mix[keep], a64.pdf_mix[keep])
    if n_b == 0:            # the light strategy alone: tir_env_sample_setup's cells at Ns = N, bit for bit, no pair exempt
        cell0, _ = ops.env_sample_setup(env.hdr_row_cdf[name], env.hdr_col_cdf[name], env.hdr_dir[name].view(-1, 3), dev(pts.normal), N, R.SEED,
                                        R.OFFSET)
        assert torch.equal(cell, cell0)
    if M == 5:              # the same bits from the full search and from the direction table + pdf_return
        for kw in (dict(guide=False), dict(records=False)):
            other = device_setup(env, name, pts, n_l, n_b, **kw)
            for x, y in zip(other[:3], (dirs, cell, pdf_mix)):
                assert torch.equal(x, y), kw
            assert int(other[5]) == int(n_active) and (other[3].cpu()[~active] == 0).all()


# ---- the pair list -------------------------------------------------------------------------------------------------------------------
def fresh_buffers(M, N):
    return (torch.full((M, N, 3), SENTINEL, device="cuda"), torch.full((M, N), int(SENTINEL), dtype=torch.int32, device="cuda"),
            torch.full((M, N), SENTINEL, device="cuda"), torch.full((M, N), SENTINEL, device="cuda"),
            torch.full((M * N,), int(SENTINEL), dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("block_pairs", [256, 512, 1000, 32768])
@pytest.mark.parametrize("name", list(R.MAPS))
def test_pair_list(envs, name, block_pairs):
    """67 points x 130 pairs = 8710 pairs in blocks of 256 (35, the last with six pairs), 512 (two iterations per thread), 1000 (no
    multiple of the block's 256 threads) and 32768 (one block): the sorted list is exactly the active pairs -- those the
    restatement calls active, over the pairs that are not exempt --, vis is 0 on every other pair and untouched on the listed ones,
    and inside a block the ids come in pair order."""
    M, (n_l, n_b) = 67, (100, 30)
    N = n_l + n_b
    a64 = R.case(name, M, n_l, n_b, F64)
    keep = ~a64.exempt.view(-1)
    bufs = fresh_buffers(M, N)
    dirs, cell, pdf_mix, vis, pair_ids, n_active = device_setup(envs[name], name, R.points(M), n_l, n_b, block_pairs, buffers=bufs)
    assert vis.data_ptr() == bufs[3].data_ptr()
    ids, mask = listed(pair_ids, n_active, M * N)
    assert torch.equal(torch.sort(ids).values[keep[torch.sort(ids).values]], torch.nonzero(a64.active.view(-1) & keep).view(-1))
    assert torch.equal(mask[keep], a64.active.view(-1)[keep])
    v = vis.cpu().view(-1)
    assert (v[~mask] == 0).all() and (v[mask] == SENTINEL).all()
    assert (pair_ids.cpu()[int(n_active):] == int(SENTINEL)).all()
    blk = ids // block_pairs
    same = blk[1:] == blk[:-1]
    assert (ids[1:][same] > ids[:-1][same]).all()                         # pair order within a block
    assert len(torch.unique_consecutive(blk)) == len(torch.unique(blk))   # a block's ids are one segment of the list
    if block_pairs == 32768:
        assert torch.equal(ids, torch.nonzero(mask).view(-1))
    first = device_setup(envs[name], name, R.points(M), n_l, n_b, 256)
    for x, y in zip(first[:3], (dirs, cell, pdf_mix)):                    # the grouping enters no per-pair output
        assert torch.equal(x, y)


@pytest.mark.parametrize("count", [40, 0, 67, 90])
def test_device_side_point_count(envs, count):
    """m_dev = 40 of 67 rows: the rows up to it are those of a call with 40 points, the rows past it are untouched; m_dev = 0 writes
    nothing; a count beyond the capacity is clamped to it."""
    name, M, (n_l, n_b) = "m5x12", 67, (32, 32)
    N, k = n_l + n_b, min(count, 67)
    pts = R.points(M)
    m_dev = torch.tensor([count], dtype=torch.int32, device="cuda")
    bufs = fresh_buffers(M, N)
    dirs, cell, pdf_mix, vis, pair_ids, n_active = device_setup(envs[name], name, pts, n_l, n_b, m_dev=m_dev, buffers=bufs)
    for t in (dirs, cell, pdf_mix, vis):
        assert (t[k:] == SENTINEL).all()
    ids, mask = listed(pair_ids, n_active, M * N)
    assert (pair_ids.cpu()[int(n_active):] == int(SENTINEL)).all() and (count > 0 or int(n_active) == 0)
    if k:
        part = device_setup(envs[name], name, R.take(pts, slice(0, k)), n_l, n_b)
        for x, y in zip(part[:3], (dirs, cell, pdf_mix)):
            assert torch.equal(x, y[:k])
        assert int(part[5]) == int(n_active) and torch.equal(torch.sort(part[4][: int(n_active)]).values.cpu().long(), torch.sort(ids).values)
        assert (ids < k * N).all()


# ---- integration ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,n_l,n_b", [c for c in CASES if c[0] == "m8x16" or c[1:] == (67, 100, 30)], ids=lambda v: str(v))
def test_relight_mis(envs, name, M, n_l, n_b):
    """tir_relight_mis on the device's own dirs, cell and pdf_mix with random vis on EVERY pair, both output modes, against float64:
    no pair is exempt, the kernel has no branch.  N of 1, 63, 64 and 130: a partial wave, one full pass, a third pass."""
    from tensoir_amd import ops
    env, pts, lt, N = envs[name], R.points(M), R.light(name), n_l + n_b
    dirs, cell, pdf_mix, _, _, _ = device_setup(env, name, pts, n_l, n_b)
    vis = R.random_vis(M, N, seed=M + N)
    surf = [dev(x) for x in (pts.normal, pts.albedo, pts.rough, pts.fresnel, pts.rays_d)]
    for linear in (True, False):
        got = ops.relight_mis(*surf, dirs, cell, pdf_mix, env.cell_records(name), dev(vis), linear=linear).cpu()
        assert got.shape == (M, 3)
        ref = lambda dt: R.relight(lt, pts, dirs.cpu(), cell.cpu(), pdf_mix.cpu(), vis, linear, dt)
        check(f"relight {'linear' if linear else 'srgb'} {name} M {M} n_l {n_l} n_b {n_b}", got, ref(F32), ref(F64))
        if not linear:
            assert float(got.min()) >= 0 and float(got.max()) <= 1.0 + 1e-6
        if M == 5:
            count = torch.tensor([3], dtype=torch.int32, device="cuda")
            part = ops.relight_mis(*surf, dirs, cell, pdf_mix, env.cell_records(name), dev(vis), linear=linear, m_dev=count).cpu()
            three = ops.relight_mis(*[x[:3].contiguous() for x in surf], dirs[:3].contiguous(), cell[:3].contiguous(),
                                    pdf_mix[:3].contiguous(), env.cell_records(name), dev(vis[:3]), linear=linear).cpu()
            assert torch.equal(part[:3], three) and torch.equal(three, got[:3])
    zero = torch.zeros((1,), dtype=torch.int32, device="cuda")
    ops.relight_mis(*surf, dirs, cell, pdf_mix, env.cell_records(name), dev(vis), m_dev=zero)        # no point: nothing to do


# ---- the pipeline on the small field -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field(golden):
    """The small test field of tests/helpers.py and eight of its own surface points (every sixth ray that hit, from the recorded
    primary pass); roughness from 0.15 to 0.85; the second four with the normal turned to the camera's side."""
    import tensoir_amd
    from tests.helpers import T, golden_checkpoint
    eh, ew = [int(x) for x in golden["scene/envmap_hw"]]
    model = tensoir_amd.model_from_checkpoint(golden_checkpoint(golden), "cuda", envmap_h=eh, envmap_w=ew)
    model.march_t_stop = 0.0
    rows = torch.nonzero(T(golden, "fwd/acc_mask").reshape(-1).bool()).view(-1)[::6][:8]
    assert rows.numel() == 8
    rays = T(golden, "rays/rays").float()[rows]
    normal = T(golden, "fwd/normal_map").float()[rows]
    normal[4:] = -normal[4:]
    pts = dict(surf=rays[:, :3] + T(golden, "fwd/depth_map").float()[rows, None] * rays[:, 3:], normal=normal,
               albedo=T(golden, "fwd/albedo_map").float()[rows], rough=torch.linspace(0.15, 0.85, 8).reshape(8, 1),
               fresnel=T(golden, "fwd/fresnel_map").float()[rows], rays_d=rays[:, 3:])
    return model, {k: v.contiguous().cuda() for k, v in pts.items()}


def fresh_env(name="m8x16", seed=4321):
    from tensoir_amd import relight
    torch.manual_seed(seed)
    return relight.Environment_Light(hdr_maps={name: R.light(name).hdr}, device="cuda")


def relit(model, env, p, name="m8x16", **kw):
    from tensoir_amd import relight
    return relight.relight_importance_sampled(model, env, name, p["surf"], p["normal"], p["albedo"], p["rough"], p["fresnel"], p["rays_d"],
                                              nSample=24, **kw)


@torch.no_grad()
def test_pipeline_is_the_three_ops(field):
    """relight_importance_sampled(mis=cfg) is setup -> march on the explicit directions with the id list -> tir_relight_mis, bit for
    bit, with one draw counter; and mis=None gives the same bits before and after a mis call once seed and counter are restored."""
    from tensoir_amd import ops, relight
    model, p = field
    name, N = "m8x16", 96
    env = fresh_env()
    before = relit(model, env, p, num_samples=N)
    assert env._draws == 1
    for cfg in (relight.MisConfig(), relight.MisConfig(0.25, 0.3, linear=True), relight.MisConfig(1.0), relight.MisConfig(0.0)):
        draws = env._draws
        got = relit(model, env, p, num_samples=N, mis=cfg)
        assert env._draws == draws + 1 and got.shape == (8, 3) and torch.isfinite(got).all()
        env._draws = draws
        dirs, cell, pdf_mix, vis0, pair_ids, n_active = env.sample_mis(name, p["normal"], p["rays_d"], p["rough"], N, cfg)
        assert env._draws == draws + 1 and dirs.shape == (8, N, 3)
        org = torch.arange(8 * N, dtype=torch.int32, device="cuda") // N
        vis, _, _ = ops.march_secondary(model.packed_field_dense(), p["surf"], dirs.view(-1, 3), relight._z_table(24, 0.05, 1.5, p["surf"].device),
                                        8 * N, org.to(torch.int32), None, None, model.march_t_stop, False, 0, False, ray_ids=pair_ids,
                                        n_ids_dev=n_active, vis=vis0.view(-1))
        hand = ops.relight_mis(p["normal"], p["albedo"], p["rough"], p["fresnel"], p["rays_d"], dirs, cell, pdf_mix, env.cell_records(name),
                               vis.view(8, N), linear=cfg.linear)
        assert torch.equal(got, hand), cfg
        print(f"\n[mis pipeline {cfg}] mean {float(got.mean()):.4f}, visible share of the active pairs "
              f"{float(vis.view(-1)[pair_ids[: int(n_active)].long()].mean()):.3f}")
    env._draws = 0
    after = relit(model, env, p, num_samples=N)
    assert torch.equal(before, after) and float(before.mean()) > 0
    # an empty chunk consumes its draw counter too
    empty = {k: v[:0] for k, v in p.items()}
    draws = env._draws
    assert relit(model, env, empty, num_samples=N, mis=relight.MisConfig()).shape == (0, 3) and env._draws == draws + 1


@torch.no_grad()
def test_strategies_agree(field):
    """Linear output, eight points of the small field, 16 calls of 256 samples for light only, BRDF only and half and half: the three
    means agree pairwise within 5 standard errors of their difference, taken from the 16-call spread.  Seeds are fixed."""
    from tensoir_amd import relight
    model, p = field
    env = fresh_env(seed=99)
    means, errs = {}, {}
    for label, fraction in (("light", 0.0), ("brdf", 1.0), ("half", 0.5)):
        cfg = relight.MisConfig(fraction, linear=True)
        runs = torch.stack([relit(model, env, p, num_samples=256, mis=cfg) for _ in range(16)]).double().cpu()      # [16, 8, 3]
        means[label], errs[label] = runs.mean(0), runs.std(0, unbiased=True) / 4.0
        print(f"\n[mis agreement {label}] mean per point {[round(float(v), 4) for v in means[label].mean(1)]}, "
              f"relative standard error {float((errs[label] / means[label].clamp(min=1e-12)).max()):.2e}")
    assert env._draws == 48 and (means["light"] > 1e-4).any()
    for a, b in (("light", "brdf"), ("light", "half"), ("brdf", "half")):
        se = torch.sqrt(errs[a] ** 2 + errs[b] ** 2)
        z = (means[a] - means[b]).abs() / se.clamp(min=1e-300)
        print(f"[mis agreement {a} vs {b}] max |difference| / se {float(z.max()):.2f}")
        assert ((means[a] - means[b]).abs() <= 5.0 * se).all(), (a, b, z)


# ---- a view --------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_view_with_mis():
    """relight_view(mis=cfg) on a 16 x 16 view with background: the documented shapes, the background rows those of mis=None (the
    environment lookup does not depend on the estimator), the hit rows relit by the other estimator, and the chunk loop's bits."""
    import contextlib
    import io
    import tensoir_amd
    from tensoir_amd import relight, synth
    model = tensoir_amd.model_from_checkpoint(synth.make_checkpoint(grid=(96,) * 3), "cuda")
    with contextlib.redirect_stdout(io.StringIO()):
        model.updateAlphaMask((48,) * 3)
    maps = synth.make_hdr_maps(["one", "two"], 32, 64)
    rays = synth.make_rays(16, 16, narrow=1.0).cuda()
    names, cfg = list(maps), relight.MisConfig()

    def env():
        torch.manual_seed(7)
        return relight.Environment_Light(hdr_maps=maps, device="cuda")
    plain = relight.relight_view(model, env(), names, rays, 16, 16, num_samples=32, chunk=100)
    e = env()
    view = relight.relight_view(model, e, names, rays, 16, 16, num_samples=32, chunk=100, mis=cfg)
    assert e._draws == 2 * 3                                             # two maps, three chunks
    assert view["rgb"] is view["raw"] and view["rgb"].shape == (2, 16, 16, 3) and view["guide"].shape == (16, 16, 12)
    assert view["acc"].shape == (16, 16) and torch.equal(view["acc"], plain["acc"]) and torch.equal(view["guide"], plain["guide"])
    hit = view["acc"] > 0.5
    print(f"\n[mis view] {int(hit.sum())} hit pixels of 256")
    assert 0 < int(hit.sum()) < 256
    assert torch.equal(view["rgb"][:, ~hit], plain["rgb"][:, ~hit])
    assert not torch.equal(view["rgb"][:, hit], plain["rgb"][:, hit]) and torch.isfinite(view["rgb"]).all()
    e, parts = env(), []
    lidx = torch.zeros((256, 1), dtype=torch.int32, device="cuda")
    for r0 in range(0, 256, 100):
        parts.append(relight.relight_chunk(model, e, names, rays[r0:r0 + 100], lidx[r0:r0 + 100], num_samples=32, mis=cfg)[0])
    assert torch.equal(view["rgb"], torch.cat(parts).view(16, 16, 2, 3).permute(2, 0, 1, 3))
