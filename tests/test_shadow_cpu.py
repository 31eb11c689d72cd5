"""The shadow-map restatement (tests/shadow_reference.py) on its own, no GPU: the frames, the maps against the analytic shadow of
the ground-and-quad scene, the two criteria the default bias was chosen by, the lookup grid's excluded share, and the float32 -
float64 distances the GPU tests' bounds are made from (tests/test_gpu_shadow.py)."""
import numpy as np
import pytest

from tests import light_reference as L
from tests import shadow_reference as SR

TIE_DIRS = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (1, 1, 1), (1, -1, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (0.3, 0.3, 0.9),
            (0.9, 0.3, 0.3), (2, -3, 0.5)]


def test_frames_are_orthonormal_in_float64():
    """L = +-e_z, the axes, and every tie of |L_a| included; the shipped host arithmetic (ops.shadow_frames_f64) equals the
    restatement's, and its rows are what the contract states."""
    from tensoir_amd import ops
    rng = np.random.default_rng(3)
    dirs = np.float64(TIE_DIRS + [tuple(x) for x in rng.normal(size=(40, 3))])
    Lh, u, v = SR.frame_axes(dirs)
    B = np.stack([u, v, Lh], 1)
    assert np.abs(B @ B.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
    assert np.abs(np.linalg.det(B) - 1).max() < 1e-12                       # right-handed: v = L x u
    assert np.array_equal(u[0], [0, -1, 0]) and np.array_equal(v[0], [1, 0, 0])          # e_z: a = x (the lowest index of the tie)
    assert np.array_equal(u[2], [0, 0, -1])                                                 # e_x: a = y
    assert np.array_equal(u[5], u[5]) and abs(u[5][0]) < 1e-15                            # (1, 1, 1): a = x, u has no x component
    c, r, S = (0.3, -0.2, 0.7), 1.7, 61
    fr = SR.frames(dirs, c, r, S)
    assert np.abs(fr - ops.shadow_frames_f64(dirs, c, r, S)).max() < 1e-12
    g = S / (2 * r)
    assert np.abs(fr[:, 0:3] - g * u).max() < 1e-12 and np.abs(fr[:, 8:11] - Lh / (4 * r)).max() < 1e-12
    x, y, w = (fr[:, 4 * k:4 * k + 3] @ np.float64(c) + fr[:, 4 * k + 3] for k in range(3))
    assert np.abs(x - S / 2).max() < 1e-12 and np.abs(y - S / 2).max() < 1e-12 and np.abs(w - 0.5).max() < 1e-12
    edge = np.float64(c) + r * Lh                                          # the sphere's point nearest to the light: w = 0.75
    assert np.abs((fr[:, 8:11] * edge).sum(1) + fr[:, 11] - 0.75).max() < 1e-12
    with pytest.raises(ValueError):
        ops.shadow_frames_f64([(0, 0, 0)], c, r, S)
    with pytest.raises(ValueError):
        ops.shadow_frames_f64(dirs, c, 0.0, S)


@pytest.mark.parametrize("light", list(SR.LIGHTS))
@pytest.mark.parametrize("S", [64, 61])
def test_map_equals_the_analytic_shadow(light, S):
    """Every texel centre, carried back along L: it meets the occluder where the point at height h lies in the quad, else the
    ground where the point at height 0 lies in [-1, 1]^2, else nothing.  The map's depth is that point's w.  Texel centres
    within 1/128 texel of a projected border are left out (the corners are snapped to 1/256 texel); the depth tolerance is what
    that snap moves w by on the slanted light's faces, 1/256 texel x 1/(2S) per texel, plus float32 frames (1e-6)."""
    h = 0.25
    pos = SR.ground_quad(h)
    c, r = SR.mesh_bounds(pos)
    l = np.float64(SR.LIGHTS[light]) / np.linalg.norm(SR.LIGHTS[light])
    fr64 = SR.frames([l], c, r, S)
    fr = fr64.astype(np.float32)
    depth, counts = SR.maps(pos, fr, S)
    assert counts == dict.fromkeys(SR.R.DROPS, 0)
    Lh, u, v = SR.frame_axes([l])
    g = S / (2 * r)
    jj, ii = np.meshgrid(np.arange(S) + 0.5, np.arange(S) + 0.5, indexing="ij")
    base = c + ((ii - S / 2) / g)[..., None] * u[0] + ((jj - S / 2) / g)[..., None] * v[0]          # on the plane through the centre
    want = np.zeros((S, S))
    sure = np.ones((S, S), bool)
    hit = np.zeros((S, S), bool)
    for z, half in ((h, SR.QUAD_HALF), (0.0, 1.0)):                      # nearest to the light first
        p = base + ((z - base[..., 2]) / l[2])[..., None] * l
        margin = (half - np.abs(p[..., 0:2])) * np.sqrt(1 - l[0:2] ** 2) * g                      # in texels, per axis
        inside = (margin > 0).all(-1) & ~hit
        sure &= hit | (np.abs(margin) > 1 / 128).all(-1)
        want[inside] = (p[inside] @ l) / (4 * r) + (0.5 - (l @ c) / (4 * r))
        hit |= inside
    assert sure.mean() > 0.9 and hit[sure].sum() > 0.3 * S * S
    assert np.array_equal(depth[0][sure] != 0, hit[sure])
    tol = (1 / 256) / (2 * S) + 1e-6
    err = np.abs(depth[0] - want)[sure].max()
    print(f"\n[shadow analytic {light} S {S}] texels compared {int(sure.sum())} of {S * S}, occluder texels "
          f"{int((want[sure] > want[sure][want[sure] > 0].min() + 1e-3).sum())}, depth error {err:.2e} (tolerance {tol:.2e})")
    assert err < tol


def test_default_bias_meets_both_criteria():
    """The shipped default is the smallest candidate (by constant + slope, the bias at 45 degrees; then by the constant) that
    leaves no pair with c >= 0.25 of the sphere self-shadowed and keeps every contact point more than two texels inside the
    shadow of the quad at 0.05 r shadowed.  The whole table is printed (DESIGN 4.10 quotes it)."""
    from tensoir_amd import raster
    pos = SR.ground_quad(SR.CONTACT_HEIGHT)
    assert abs(SR.CONTACT_HEIGHT / SR.mesh_bounds(pos)[1] - 0.05) < 1e-3
    table = {(c, s): SR.bias_criteria(c, s) for c in SR.CONSTS for s in SR.SLOPES}
    for (c, s), (self_shadowed, facing, contact_lit, contact) in table.items():
        print(f"[shadow bias {c} + {s} tan] self-shadowed {self_shadowed} of {facing} pairs, contact points lit {contact_lit} of {contact}")
    assert min(t[1] for t in table.values()) > 100000 and min(t[3] for t in table.values()) > 1000
    passing = sorted((c + s, c, s) for (c, s), t in table.items() if t[0] == 0 and t[2] == 0)
    assert passing and passing[0][1:] == tuple(raster.SHADOW_BIAS)
    assert table[tuple(raster.SHADOW_BIAS)][0] == 0 and table[tuple(raster.SHADOW_BIAS)][2] == 0


def _lookup_case(light):
    pos = SR.scene()
    dirs = [SR.LIGHTS[light]]
    fr = SR.scene_frames(pos, dirs, 64, SR.SCENE_BOUNDS)
    pts, nrm = SR.ground_grid()
    return pos, SR.cells_of(dirs), fr, pts, nrm


@pytest.mark.parametrize("light", list(SR.LIGHTS))
def test_lookup_grid_stays_inside_the_exclusion_cap(light):
    """The 41 x 41 grid of the GPU lookup test: the float64 restatement flags at most 1 % of its pairs as too close to call, the
    float32 mode agrees with it on all others, and both shadowed and lit points are there."""
    pos, cells, fr, pts, nrm = _lookup_case(light)
    depth = SR.maps(pos, fr, 64)[0]
    near = {}
    ref = SR.lookup(pts, nrm, cells, fr, depth, (0.5, 1.0), np.float64, near)
    excluded = near["depth"] | near["texel"]
    f32 = SR.lookup(pts, nrm, cells, fr, SR.maps(pos, fr, 64, dtype=np.float32)[0], (0.5, 1.0), np.float32)
    print(f"\n[shadow lookup grid {light}] excluded {int(excluded.sum())} of {excluded.size}, shadowed {int((ref == 1).sum())}, lit {int((ref == 2).sum())}")
    assert excluded.mean() <= 0.01
    assert np.array_equal(f32[~excluded], ref[~excluded])
    assert (ref == 1).sum() > 100 and (ref == 2).sum() > 100 and (ref == 0).sum() == 0


def test_float32_distances_behind_the_gpu_bounds():
    """What tests/test_gpu_shadow.py multiplies by ten: the float32 mode's distance from the float64 mode for the maps of the
    scene (over the texels occupied in both) and for the shadowed lighting sum.  Printed; the maps' occupancy agrees between the
    modes except where a corner's snap differs."""
    pos = SR.scene()
    for D in (1, 3, 33):
        for S in (8, 61, 64):
            fr = SR.scene_frames(pos, SR.cell_dirs(D), S, SR.SCENE_BOUNDS)
            a, b = SR.maps(pos, fr, S, dtype=np.float32)[0], SR.maps(pos, fr, S)[0]
            both = (a != 0) & (b != 0)
            print(f"[shadow distance maps D {D} S {S}] float32 - float64 {L.distance(a[both], b[both]):.2e}, occupancy differs at "
                  f"{int(((a != 0) != (b != 0)).sum())} of {a.size} texels")
            assert both.sum() > 0 and ((a != 0) != (b != 0)).mean() < 0.01
    g, v, cells = L.surface_rows(65, 33)
    codes = np.random.default_rng(5).integers(1, 3, (65, 33)).astype(np.uint8)
    ref = SR.light_gbuffer_shadowed(g, v, cells, 0.04, 3, codes)
    d = L.distance(SR.light_gbuffer_shadowed(g, v, cells, 0.04, 3, codes, np.float32), ref)
    print(f"[shadow distance lighting M 65 D 33] float32 - float64 {d:.2e}")
    assert 0 < d < 1e-4
    everything = np.full((65, 33), 2, np.uint8)
    assert np.array_equal(SR.light_gbuffer_shadowed(g, v, cells, 0.04, 3, everything), L.light_gbuffer(g, v, cells, 0.04, 3))
    assert (SR.light_gbuffer_shadowed(g, v, cells, 0.04, 0, np.ones((65, 33), np.uint8))[:, :3] == 0).all()
