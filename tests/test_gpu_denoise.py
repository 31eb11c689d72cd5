"""The guided a-trous denoiser on the GPU (tensoir_amd/csrc/tir_denoise.hip, tensoir_amd/denoise.py, relight.relight_view)
against its float64 restatement (tests/denoise_reference.py), its bit-level promises, and one small view end to end.

Tolerance of one level, colours in [0, 1]: max abs 4e-5.  Taps whose exponent argument exceeds 88 vanish on both sides; below
that the fp32 argument and exp are off by about 1e-5 relative per weight at the most; the output is a convex combination, so
the bound is twice that times max c, plus the accumulation of 24 terms.  Three levels without the colour term: three times that.
With the colour term a colour error feeds the next level's weights, so the levels are compared one by one, each fed the
restatement's previous output; the end-to-end difference is printed, not bounded."""
import numpy as np
import pytest
import torch

from tests import denoise_reference as R

pytestmark = pytest.mark.gpu

TOL = 4e-5
SIGMAS = dict(sigma_n=0.05, sigma_p=0.02, sigma_a=0.1, sigma_r=0.1)


def inv32(sigma_c):
    """the five inverses as the fp32 values the kernel is handed"""
    return tuple(float(np.float32(v)) for v in R.inverses(sigma_c=sigma_c, **SIGMAS))


def make_guide(H, W, seed):
    """A bumpy height field seen from above (fp32 values, [H, W, 12]): smooth normals, a few albedo levels, smooth roughness; where
    the image is large enough an all-invalid 9 x 9 block, a valid pixel alone in an invalid 9 x 9 block, a quarter whose normals
    are flipped and a depth cliff of one unit."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = 0.05 * np.sin(0.31 * xs) * np.cos(0.23 * ys)
    n = np.stack([-0.05 * 0.31 * np.cos(0.31 * xs) * np.cos(0.23 * ys) / 0.02, 0.05 * 0.23 * np.sin(0.31 * xs) * np.sin(0.23 * ys) / 0.02,
                  np.ones_like(xs)], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    g = np.zeros((H, W, R.GUIDE))
    g[..., 0], g[..., 1], g[..., 2] = 0.02 * xs, 0.02 * ys, z
    g[..., 3] = rng.random((H, W)) > 0.08                               # scattered invalid pixels
    g[..., 4:7] = n
    g[..., 7] = 0.5 + 0.2 * np.sin(0.11 * xs + 0.07 * ys)
    g[..., 8:11] = 0.2 + 0.1 * rng.integers(0, 4, (H, W, 1)) * (rng.random((H, W, 1)) > 0.7) + 0.02 * rng.random((H, W, 3))
    if H >= 30 and W >= 30:
        g[2:11, 3:12, 3] = 0.0                                          # all invalid
        g[14:23, 3:12, 3] = 0.0
        g[18, 7, 3] = 1.0                                               # alone: every tap of steps 1 and 2 is invalid
        g[:H // 2, W // 2:, 4:7] *= -1.0                                # the normal flip
        g[H // 2:, W // 2:, 2] += 1.0                                   # the depth cliff
    return g.astype(np.float32)


def make_colour(H, W, K, seed):
    rng = np.random.default_rng(seed + 1000)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 0.5 + 0.3 * np.sin(0.2 * xs[..., None] + 0.15 * ys[..., None] + np.arange(K))
    return np.clip(base * (1.0 + 0.4 * rng.standard_normal((H, W, K))), 0.0, 1.0).astype(np.float32)


def gpu_level(c, g, step, inv):
    from tensoir_amd import ops
    H, W, K = c.shape
    cin = torch.from_numpy(c).cuda()
    out = torch.full_like(cin, -7.0)
    ops.atrous_level(cin.view(H * W, K), out.view(H * W, K), torch.from_numpy(g).cuda().view(H * W, R.GUIDE), H, W, step, *inv)
    assert torch.equal(cin.cpu(), torch.from_numpy(c))
    return out.cpu().numpy()


def rel_err(got, want):
    """max |got - want| / |want| per element; where want is 0, |got|"""
    rel = np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))
    return float(rel.max()) if rel.size else 0.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


SHAPES = [(1, 3, 1), (3, 1, 1), (5, 5, 4), (37, 53, 1), (37, 53, 2), (37, 53, 8), (64, 64, 32)]


@pytest.mark.parametrize("sigma_c", [0.5, 0.0], ids=["colour", "no-colour"])
@pytest.mark.parametrize("K", [3, 15, 24])
@pytest.mark.parametrize("H,W,step", SHAPES, ids=[f"{h}x{w}-step{s}" for h, w, s in SHAPES])
def test_one_level_matches_the_restatement(H, W, step, K, sigma_c):
    g, c = make_guide(H, W, 7 * H + W), make_colour(H, W, K, H + step)
    inv = inv32(sigma_c)
    got = gpu_level(c, g, step, inv)
    want = R.atrous_level(c, g, step, *inv)
    err = float(np.abs(got - want).max())
    print(f"{H}x{W} step {step} K {K} sigma_c {sigma_c}: max abs {err:.3e}")
    assert err <= TOL
    invalid = g[..., 3] < 0.5
    assert np.array_equal(bits(got)[invalid], bits(c)[invalid])       # copies, bit for bit
    if H >= 30 and step <= 2:
        assert g[18, 7, 3] == 1.0 and np.array_equal(bits(got)[18, 7], bits(c)[18, 7])       # the valid pixel with no valid tap
    if min(H, W) > 2 * step:
        assert np.abs(got - c).max() > 1e-3                            # (and the level does filter)


def test_three_levels_without_the_colour_term():
    from tensoir_amd import denoise
    H, W, K = 37, 53, 15
    g, c = make_guide(H, W, 11), make_colour(H, W, K, 12)
    cfg = denoise.AtrousConfig(levels=3, sigma_c=0.0, **SIGMAS)
    cin = torch.from_numpy(c).cuda()
    got = denoise.atrous(cin, torch.from_numpy(g).cuda(), cfg).cpu().numpy()
    assert torch.equal(cin.cpu(), torch.from_numpy(c))                 # the caller's tensor is never written
    want = R.atrous(c, g, levels=3, inv=tuple(float(np.float32(v)) for v in cfg.inverses()))
    err = float(np.abs(got - want).max())
    print(f"three levels, no colour term: max abs {err:.3e}")
    assert err <= 3 * TOL
    # the stacked layout is the same image
    stacked = cin.view(H, W, 5, 3).permute(2, 0, 1, 3).contiguous()
    got4 = denoise.atrous(stacked, torch.from_numpy(g).cuda(), cfg)
    assert got4.shape == (5, H, W, 3) and np.array_equal(bits(got4.permute(1, 2, 0, 3).reshape(H, W, K).cpu().numpy()), bits(got))


def test_three_levels_with_the_colour_term_level_by_level():
    from tensoir_amd import denoise
    H, W, K = 37, 53, 15
    g, c = make_guide(H, W, 21), make_colour(H, W, K, 22)
    cfg = denoise.AtrousConfig(levels=3, sigma_c=0.5, **SIGMAS)
    inv = tuple(float(np.float32(v)) for v in cfg.inverses())
    x = c.astype(np.float64)
    for level in range(3):
        fed = x.astype(np.float32)                                     # the restatement's previous output, rounded
        want = R.atrous_level(fed, g, 1 << level, *inv)
        got = gpu_level(fed, g, 1 << level, inv)
        err = float(np.abs(got - want).max())
        print(f"colour term, level {level}: max abs {err:.3e}")
        assert err <= TOL
        x = want
    end = denoise.atrous(torch.from_numpy(c).cuda(), torch.from_numpy(g).cuda(), cfg).cpu().numpy()
    print(f"colour term, three levels end to end: max abs {float(np.abs(end - R.atrous(c, g, levels=3, inv=inv)).max()):.3e} (not bounded)")


def test_bit_level_properties():
    H, W = 37, 53
    g = make_guide(H, W, 31)
    valid = g[..., 3] > 0.5
    # a constant image stays constant
    const = np.broadcast_to(np.float32([0.1, 0.7, 1.0 / 3.0]), (H, W, 3)).copy()
    for sigma_c in (0.5, 0.0):
        out = gpu_level(const, g, 2, inv32(sigma_c))
        rel = float((np.abs(out.astype(np.float64) - const) / const).max())
        print(f"constant image, sigma_c {sigma_c}: max relative {rel:.3e}")
        assert rel <= 32 * 2.0 ** -24
    for sigma_c in (0.5, 0.0):
        inv = inv32(sigma_c)
        c = make_colour(H, W, 15, 32)
        a, b = gpu_level(c, g, 2, inv), gpu_level(c, g, 2, inv)
        assert np.array_equal(bits(a), bits(b))                        # two calls: identical bits
        assert np.array_equal(bits(a)[~valid], bits(c)[~valid])        # invalid pixels: copies
        assert not np.array_equal(a[valid], c[valid])
        for m in range(5):                                             # a map does not see the other maps of the call
            one = gpu_level(np.ascontiguousarray(c[..., 3 * m:3 * m + 3]), g, 2, inv)
            assert np.array_equal(bits(one), bits(a[..., 3 * m:3 * m + 3])), (sigma_c, m)


@pytest.mark.parametrize("B,row0", [(1, 0), (1, 5), (63, 2), (64, 1), (4097, 3)])
def test_guide_rows(B, row0):
    from tensoir_amd import ops
    rng = np.random.default_rng(B + row0)
    maps = rng.standard_normal((B, 20)).astype(np.float32)
    maps[:, 3] = np.abs(maps[:, 3]) * 3.0
    maps[:, 14] = rng.choice(np.float32([0.0, 0.3, 0.5, 0.5000001, 0.9, 1.0]), B)           # acc: around and at the threshold
    maps[::7, 4:7] = 0.0                                                # no normal at all
    maps[3::7, 4:7] *= np.float32(1e-7)                                 # shorter than the clamp
    rays = rng.standard_normal((B, 6)).astype(np.float32)
    guide = torch.full((row0 + B + 3, 12), 7.0, device="cuda")
    ops.denoise_guide(torch.from_numpy(maps).cuda(), torch.from_numpy(rays).cuda(), guide, row0)
    got = guide.cpu().numpy()
    assert (got[:row0] == 7.0).all() and (got[row0 + B:] == 7.0).all()  # no other row is touched
    got, want = got[row0:row0 + B].astype(np.float64), R.guide_rows(maps, rays)
    for cols, what in ((slice(0, 3), "position"), (slice(4, 7), "normal")):
        rel = rel_err(got[:, cols], want[:, cols])
        print(f"B {B}: {what} max relative {rel * 2 ** 24:.2f} x 2^-24")
        assert rel <= 4 * 2.0 ** -24, what
    for col in (3, 7, 8, 9, 10, 11):
        assert np.array_equal(got[:, col], want[:, col]), col
    assert 0 < got[:, 3].sum() < B or B == 1


# ---- one small view end to end ------------------------------------------------------------------------------------------------
SIDE, CHUNK, SEED = 64, 1000, 1234


@pytest.fixture(scope="module")
def view_scene():
    import contextlib
    import io
    import tensoir_amd
    from tensoir_amd import synth
    model = tensoir_amd.model_from_checkpoint(synth.make_checkpoint(grid=(96,) * 3), "cuda")
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        model.updateAlphaMask((48,) * 3)
    maps = synth.make_hdr_maps(["one", "two"], 32, 64)
    return model, maps, synth.make_rays(SIDE, SIDE).cuda()


def fresh_env(maps, seed=SEED):
    from tensoir_amd import relight
    torch.manual_seed(seed)
    return relight.Environment_Light(hdr_maps=maps, device="cuda")


@torch.no_grad()
def test_view_without_the_filter_is_the_chunk_loop(view_scene):
    from tensoir_amd import relight
    model, maps, rays = view_scene
    names, n = list(maps), SIDE * SIDE
    view = relight.relight_view(model, fresh_env(maps), names, rays, SIDE, SIDE, num_samples=16, chunk=CHUNK)
    assert view["rgb"] is view["raw"] and view["rgb"].shape == (2, SIDE, SIDE, 3)
    assert view["guide"].shape == (SIDE, SIDE, 12) and view["acc"].shape == (SIDE, SIDE)
    env = fresh_env(maps)
    lidx = torch.zeros((n, 1), dtype=torch.int32, device="cuda")
    parts, accs, guides = [], [], []
    for r0 in range(0, n, CHUNK):                                      # the last chunk is ragged: 4096 = 4 x 1000 + 96
        out, prim, _ = relight.relight_chunk(model, env, names, rays[r0:r0 + CHUNK], lidx[r0:r0 + CHUNK], num_samples=16)
        parts.append(out)
        accs.append(prim[6])
        rows = torch.zeros((out.shape[0], 20), device="cuda")          # the map rows, from the columns the chunk call hands back
        rows[:, 3], rows[:, 4:7], rows[:, 7:10], rows[:, 10:11], rows[:, 14] = prim[1], prim[2], prim[3], prim[4], prim[6]
        guides.append(R.guide_rows(rows.cpu().numpy(), rays[r0:r0 + CHUNK].cpu().numpy()))
    want = torch.cat(parts).view(SIDE, SIDE, 2, 3).permute(2, 0, 1, 3)
    assert torch.equal(view["rgb"], want)
    assert torch.equal(view["acc"].view(-1), torch.cat(accs))
    got_g, want_g = view["guide"].view(-1, 12).cpu().numpy().astype(np.float64), np.concatenate(guides)
    assert np.array_equal(got_g[:, 3], want_g[:, 3]) and np.array_equal(got_g[:, 7:], want_g[:, 7:])
    for cols in (slice(0, 3), slice(4, 7)):
        assert rel_err(got_g[:, cols], want_g[:, cols]) <= 4 * 2.0 ** -24
    hit = want_g[:, 3] > 0.5
    print(f"view: {int(hit.sum())} hit pixels of {n}")
    assert hit.sum() > n // 10


@torch.no_grad()
def test_view_with_the_filter(view_scene):
    from tensoir_amd import denoise, relight
    model, maps, rays = view_scene
    names = list(maps)
    cfg = denoise.AtrousConfig()
    view = relight.relight_view(model, fresh_env(maps), names, rays, SIDE, SIDE, num_samples=16, chunk=CHUNK, denoise=cfg)
    raw, rgb, guide = view["raw"], view["rgb"], view["guide"]
    assert rgb is not raw and rgb.shape == raw.shape == (2, SIDE, SIDE, 3)
    # (b) the view's filter is denoise.atrous on the raw image and the guide; the background is not touched
    assert torch.equal(rgb, denoise.atrous(raw, guide, cfg, aabb=model.aabb))
    with pytest.raises(ValueError, match="sigma_p"):
        denoise.atrous(raw, guide, cfg)                                # sigma_p = None and no model to measure
    hit = view["acc"] > 0.5
    assert torch.equal(guide[..., 3] > 0.5, hit)
    assert torch.equal(rgb[:, ~hit], raw[:, ~hit])
    # the same draws without the filter give the same raw image
    again = relight.relight_view(model, fresh_env(maps), names, rays, SIDE, SIDE, num_samples=16, chunk=CHUNK)
    assert torch.equal(again["rgb"], raw)
    # (c) against a 512-sample view the filtered 16-sample view is closer than the raw one, map by map
    ref = relight.relight_view(model, fresh_env(maps, SEED + 1), names, rays, SIDE, SIDE, num_samples=512, chunk=CHUNK)["rgb"]
    for m, name in enumerate(names):
        mse_raw = float(((raw[m][hit] - ref[m][hit]).double() ** 2).mean())
        mse_flt = float(((rgb[m][hit] - ref[m][hit]).double() ** 2).mean())
        print(f"map {name}: mse on {int(hit.sum())} hit pixels, 16 samples raw {mse_raw:.4e}, filtered {mse_flt:.4e}, "
              f"ratio {mse_raw / max(mse_flt, 1e-300):.2f}")
        assert mse_flt < mse_raw, name


@torch.no_grad()
def test_background_rows_are_not_filtered(view_scene):
    """A wider camera, so that the view has background: those rows are invalid in the guide and leave the filter as they came."""
    from tensoir_amd import denoise, relight, synth
    model, maps, _ = view_scene
    rays = synth.make_rays(40, 40, narrow=1.0).cuda()
    view = relight.relight_view(model, fresh_env(maps), list(maps), rays, 40, 40, num_samples=16, chunk=CHUNK, denoise=denoise.AtrousConfig())
    hit = view["acc"] > 0.5
    print(f"wide view: {int(hit.sum())} hit pixels of {hit.numel()}")
    assert 100 < int(hit.sum()) < hit.numel() - 100
    assert torch.equal(view["guide"][..., 3] > 0.5, hit)
    assert torch.equal(view["rgb"][:, ~hit], view["raw"][:, ~hit])
    assert not torch.equal(view["rgb"][:, hit], view["raw"][:, hit])
