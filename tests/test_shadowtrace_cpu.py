"""The traced-shadow restatement (tests/shadowtrace_reference.py) on the CPU: brute force against closed forms, its packing, the
rule that chooses raster.SHADOW_EPS, and the occluded lighting sum against light_reference."""
import numpy as np

from tests import light_reference as L
from tests import shadow_reference as SR
from tests import shadowtrace_reference as ST


def test_brute_force_against_the_analytic_shadow():
    """Ground + quad (h = 0.25) under e_z, -e_z, e_x and the slanted light: a ground point with an up normal is occluded under
    e_z and normalize(1, 0, 1) exactly where it lies inside the quad's analytic shadow, never under -e_z (no contribution) or e_x
    (c = 0); a point with a non-finite coordinate and a zero direction give False."""
    pos = SR.ground_quad()
    pts, nrm = SR.ground_grid(21)
    cells = SR.cells_of([(0, 0, 1), (0, 0, -1), (1, 0, 0), (1, 0, 1)])
    occ = ST.shadow_trace(pts, nrm, cells, pos, ST.unwelded_faces(pos), t0=1e-3)
    assert occ.shape == (len(pts), 4) and not occ[:, 1].any() and not occ[:, 2].any()
    for d, l in ((0, (0, 0, 1)), (3, (1, 0, 1))):
        inset = SR.shadow_inset(pts, l, 0.25, 0.0, 64, 1.0)
        assert np.array_equal(occ[:, d], inset > 0) and occ[:, d].sum() > 20 and (~occ[:, d]).sum() > 20
    # t0 beyond the occluder: nothing is met;  t0 = 0 on the ground itself: the ground's own face is met at t = 0
    assert not ST.shadow_trace(pts, nrm, cells[:1], pos, ST.unwelded_faces(pos), t0=0.5).any()
    assert ST.shadow_trace(pts, nrm, cells[:1], SR.ground_quad()[:6], ST.unwelded_faces(pos[:6]), t0=0.0).all()
    bad = pts[:3].copy()
    bad[0, 1], bad[1, 0] = np.nan, np.inf
    zero = cells[:1].copy()
    zero[0, 0:3] = 0
    assert not ST.shadow_trace(bad[:2], nrm[:2], cells[:1], pos, ST.unwelded_faces(pos)).any()
    assert not ST.shadow_trace(pts, nrm, zero, pos, ST.unwelded_faces(pos)).any()


def test_pack_and_unpack_round_trip():
    rng = np.random.default_rng(3)
    for M in (1, 63, 64, 65, 257):
        for D in (1, 17):
            mask = rng.uniform(size=(M, D)) < 0.4
            mask[M - 1, :] = True                            # the last row's bit, bit 63 when M is a multiple of 64
            w = ST.pack(mask)
            assert w.shape == (D, (M + 63) // 64) and w.dtype == np.uint64
            assert np.array_equal(ST.unpack(w, M), mask) and np.array_equal(ST.unpack(w.view(np.int64), M), mask)
            assert int(w[0, 0]) & 1 == int(mask[0, 0])
            tail = 64 * w.shape[1] - M                       # the bits beyond M are 0
            assert tail == 0 or int(w[0, -1]) >> (64 - tail) == 0
    import torch
    from tensoir_amd import ops
    mask = rng.uniform(size=(130, 5)) < 0.5
    mask[63], mask[127] = True, True
    packed = ops.pack_occlusion(torch.from_numpy(mask))
    assert packed.dtype == torch.int64 and np.array_equal(packed.numpy().view(np.uint64), ST.pack(mask))
    assert np.array_equal(ops.occlusion_bits(packed, 130).numpy(), mask)


def test_the_shadow_eps_rule():
    """DESIGN 4.17's table on every 100th point of condition (i) (281 points, 3 388 pairs with c >= 0.25), all 5 618 points of
    condition (ii) and every 7th covered pixel of condition (iii), the rasterised points (232 pixels, 2 840 pairs).  Face points:
    at 0 the sphere shadows itself through the faces its points lie on (2 774 pairs), at 1e-7 of the radius 41 pairs still do, from
    1e-6 on none.  The contact shadow is whole up to 1e-2.  The rasterised points lie off their faces by up to 1.1e-4 of the
    radius (the rasteriser snaps corners to 1 / 256 pixel): they still shadow themselves at 1e-4 and no longer at 1e-3.  The
    rule gives 1e-2, raster.SHADOW_EPS."""
    from tensoir_amd import raster
    rows = {eps: ST.eps_criteria(eps) for eps in (0.0,) + ST.EPS_CANDIDATES}
    print("\n[shadow eps] eps: (self-shadowed (i), pairs, contact lit (ii), points, self-shadowed (iii), pairs) " + ", ".join(f"{e:g}: {r}" for e, r in rows.items()))
    assert rows[0.0][1] > 3000 and rows[0.0][3] > 5000
    assert rows[0.0][0] > rows[0.0][1] // 2 and rows[1e-7][0] > 0
    assert all(rows[e][0] == 0 for e in ST.EPS_CANDIDATES[1:])
    assert all(rows[e][2] == 0 for e in (0.0,) + ST.EPS_CANDIDATES)
    assert rows[0.0][5] > 2000 and rows[1e-5][4] > rows[1e-5][5] // 10 and rows[1e-4][4] > 0
    assert rows[1e-3][4] == 0 and rows[1e-2][4] == 0
    assert ST.eps_rule() == 1e-2 and raster.SHADOW_EPS == ST.eps_rule()
    # the one-pass shortcut (the farthest meeting t against t0) is the brute-force answer
    pts, nrm, pos = ST.sphere_rows(16)
    cells = L.env_cells(np.ones((4, 8, 3), np.float32), 4, 8).astype(np.float32)
    r = SR.mesh_bounds(pos)[1]
    for eps in (0.0, 1e-7):
        t0 = np.float32(eps * r)
        on, _ = ST.contributing(nrm, cells)
        far = ST.farthest_meeting(np.repeat(pts, len(cells), 0), np.tile(cells[:, 0:3], (len(pts), 1)), pos, ST.unwelded_faces(pos))
        assert np.array_equal(ST.shadow_trace(pts, nrm, cells, pos, ST.unwelded_faces(pos), t0), on & (far.reshape(on.shape) >= np.float64(t0)))


def test_occluded_lighting_without_bits_is_the_plain_lighting():
    for M, D in ((65, 33), (257, 7)):
        g, v, cells = L.surface_rows(M, D)
        for flags in range(4):
            for dtype in (np.float64, np.float32):
                assert np.array_equal(ST.light_gbuffer_occluded(g, v, cells, 0.04, flags, np.zeros((M, D), bool), dtype),
                                      L.light_gbuffer(g, v, cells, 0.04, flags, dtype))
        occ = np.random.default_rng(M).uniform(size=(M, D)) < 0.5
        assert L.distance(ST.light_gbuffer_occluded(g, v, cells, 0.04, 0, occ), L.light_gbuffer(g, v, cells, 0.04, 0)) > 1e-3
