"""The occupancy-mask kernels on their own, through the ops wrappers, against the restatement of tests/occupancy_reference.py in
float64: tir_pack_occupancy, tir_alpha_pool, tir_occupancy_query, tir_dense_alpha, tir_filter_rays, and the host glue of
tensoir_amd/field_model.py (getDenseAlpha, updateAlphaMask, shrink between two updates, filtering_rays, AlphaGridMask.occupied_box).

What is compared how.  Bytes, volumes, bbox words, lookups and ray masks are exact.  Alpha follows the suite's rule
(shade_reference.distance / bound): the device's distance from float64 -- max abs difference over the float64 result's maximum -- is
at most ten times the float32 restatement's own on the same lattice, and no less than ten half-ulps of 1; where the float64 mask
lookup culls a lattice point alpha is exactly 0.  Nothing is excluded: tests/test_occupancy_cpu.py asserts on every fixture used
here the margins that make each lookup, threshold and slab decision the same in float32 and float64.  Every test prints
`device d (bound b)`; for exact comparisons d counts the mismatches and b is 0.

What the kernels do with input the reference never sees, stated in include/tensoir_hip.h and asserted here: tir_alpha_pool reads a
NaN alpha as 0 (fmaxf; max_pool3d would propagate it); a point with a NaN or far-away coordinate is a miss.

Measured on an MI355X: see DESIGN 2, "The occupancy-mask kernels on their own"."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import occupancy_reference as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def dev(t):
    return None if t is None else torch.as_tensor(t).contiguous().cuda()


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)


def exact(label, got, want):
    got, want = torch.as_tensor(got).cpu(), torch.as_tensor(want).cpu()
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = int((got != want).sum())
    print(f"\n[occupancy {label}] device {bad} mismatches of {want.numel()} (bound 0)")
    assert bad == 0, (label, bad)


def check(label, got, f32, f64):
    got = torch.as_tensor(got).detach().cpu()
    assert torch.isfinite(got).all(), label
    if not bool((f64 != 0).any()):
        print(f"\n[occupancy {label}] device exactly zero (float64 is)")
        assert bool((got == 0).all()), (label, "float64 is identically zero")
        return
    d, b = R.distance(got, f64), R.bound(f32, f64)
    print(f"\n[occupancy {label}] device {d:.2e} (bound {b:.2e})")
    assert d <= b, (label, d, b)


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def build(ck):
    import tensoir_amd
    with quiet():
        return tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=R.CS.ENVMAP_HW[0], envmap_w=R.CS.ENVMAP_HW[1])


class World:
    """One model per scene of occupancy_reference, built on first use and never changed (tests that update a mask build their own)."""

    def __init__(self):
        from tensoir_amd import _lib
        assert torch.cuda.is_available() and _lib.lib().tir_device_check() == 0
        self.models = {}

    def model(self, s):
        if s.key not in self.models:
            m = build(s.ck)
            assert (m.alphaMask is not None) == (s.sc.alpha_volume is not None)
            assert torch.equal(m.aabb.cpu(), s.sc.aabb) and [int(g) for g in m.gridSize] == s.sc.grid
            assert float(m.stepSize) == R.step_of(s.sc)
            self.models[s.key] = m
        return self.models[s.key]

    def field(self, s):
        return self.model(s).packed_field()


@pytest.fixture(scope="module")
def world():
    return World()


# ---- 1. tir_pack_occupancy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", R.PACK_DIMS, ids=ident)
def test_pack_occupancy(world, dims):
    """One thread per byte, 256 per block: (W+1)(H+1)(D+1) of 8, 255, 256, 258 (257 is prime) and 4590, flat and thin volumes; voxel
    values 0, 1, 0.5 (not occupied) and nextafter(0.5, 1).  Exact, and a repeat has the same bytes."""
    from tensoir_amd import ops
    vol = R.pack_volume(dims)
    got = ops.pack_occupancy(dev(vol))
    exact(f"pack {ident(dims)}", got, R.pack_occupancy(vol))
    assert torch.equal(ops.pack_occupancy(dev(vol)), got)


# ---- 2. tir_alpha_pool ---------------------------------------------------------------------------------------------------------------
def pool_check(label, alpha, thres):
    from tensoir_amd import ops
    vol, bbox = ops.alpha_pool(dev(alpha), thres)
    want_vol, want_bbox = R.alpha_pool(alpha, thres)
    bad = int((vol.cpu() != want_vol).sum()) + int(bbox.cpu().tolist() != want_bbox)
    assert vol.shape == want_vol.shape and bad == 0, (label, bad, bbox.cpu().tolist(), want_bbox)
    vol2, bbox2 = ops.alpha_pool(dev(alpha), thres)
    assert torch.equal(vol2, vol) and torch.equal(bbox2, bbox), (label, "repeat")
    return int(want_vol.sum())


@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=ident)
def test_alpha_pool(shape):
    """Lattices (1,1,1), (1,1,7), (2,3,5), (16,16,1), (7,9,257); thresholds 1e-3, 0, 1 and 2 on alpha that holds negative values,
    values above 1, -0.0, +inf, the threshold itself and its float32 neighbours; one voxel at each of the eight corners; all voxels
    set.  The volume [gz, gy, gx] and the six bbox words are exact; at threshold 2 nothing passes and the bbox keeps the wrapper's
    sentinels."""
    cases = 0
    for thres in R.POOL_THRES:
        for seed in range(3):
            n = pool_check((shape, thres, seed), R.pool_values(shape, thres, seed), thres)
            assert thres != 2.0 or n == 0
            cases += 1
    for corner in range(8):
        pool_check((shape, "corner", corner), R.pool_corner(shape, corner), 1e-3)
    assert pool_check((shape, "all"), np.ones(shape, dtype=np.float32), 1e-3) == int(np.prod(shape))
    print(f"\n[occupancy alpha_pool {ident(shape)}] device 0 mismatches in {cases + 9} volumes and bbox sextets (bound 0)")


def test_alpha_pool_nan():
    """A NaN alpha counts as 0 (the kernel's fmaxf drops it; F.max_pool3d would spread it over the neighbourhood): it passes a
    threshold of 0 and fails 1e-3, and its neighbours are decided by the other values."""
    shape = (7, 9, 33)
    a = R.pool_values(shape, 1e-3, 5)
    a.reshape(-1)[::7] = np.nan
    for thres in (1e-3, 0.0):
        pool_check((shape, "nan", thres), a, thres)
    only = np.full((3, 3, 3), np.nan, dtype=np.float32)
    from tensoir_amd import ops
    vol, bbox = ops.alpha_pool(dev(only), 1e-3)
    assert float(vol.sum()) == 0 and bbox.cpu().tolist() == R.BBOX_SENTINEL
    vol, bbox = ops.alpha_pool(dev(only), 0.0)
    assert float(vol.sum()) == 27 and bbox.cpu().tolist() == [0, 0, 0, 2, 2, 2]
    print("\n[occupancy alpha_pool nan] device 0 mismatches (bound 0)")


# ---- 3. tir_occupancy_query ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,kind", R.QUERY_SCENES, ids=ident)
def test_occupancy_query(world, row, kind):
    """1, 255, 256, 257 and 3001 points: in the mask's box, in its one-cell skirt (hits there on the POW2 mask, whose y faces hold
    occupied voxels), up to two cells beyond, coordinates of +-1e30 and +-3e38; a mask on the field's box and one on a larger box.
    Exact against the float64 sample > 0; NaN coordinates are misses."""
    from tensoir_amd import ops
    s = R.scene(row, kind)
    f = world.field(s)
    for n in R.QUERY_COUNTS:
        pts = R.query_points(s, n)
        got = ops.occupancy_query(f, dev(pts))
        exact(f"query {s.name} n {n}", got.bool(), R.occupancy(s.sc, pts, F64))
        assert torch.equal(ops.occupancy_query(f, dev(pts)), got)
    pts = R.query_points(s, 257).clone()
    want = R.occupancy(s.sc, pts, F64)
    for i in range(0, 257, 3):
        pts[i, i % 3] = float("nan")
        want[i] = False
    exact(f"query {s.name} nan", ops.occupancy_query(f, dev(pts)).bool(), want)
    got = world.model(s).alphaMask.sample_alpha(dev(R.query_points(s, 3001)))
    exact(f"sample_alpha {s.name}", got > 0, R.occupancy(s.sc, R.query_points(s, 3001), F64))


def test_occupancy_query_on_lattice(world):
    """The POW2 mask (power-of-two box, dims 17 x 9 x 33: the float32 index arithmetic is exact): every node of the mask and of its
    skirt, points on edges and faces of the lattice and inside cells, the six faces of the box -- the zero-fraction masks 0x55,
    0x33 and 0x0F, the -1 base cell, the last cell.  Exact."""
    from tensoir_amd import ops
    s = R.scene("pow2", "masked")
    lp = R.lattice_points(s)
    want = R.occupancy(s.sc, lp.pts, F64)
    got = ops.occupancy_query(world.field(s), dev(lp.pts))
    exact(f"query lattice ({int(want.sum())} hits)", got.bool(), want)
    assert torch.equal(ops.occupancy_query(world.field(s), dev(lp.pts)), got)


# ---- 4. tir_dense_alpha --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,kind", R.DENSE_CASES, ids=ident)
def test_dense_alpha(world, row, kind):
    """Lattices (1,1,1), (2,3,5), (4,8,8), (7,9,257) at two step lengths, per density width (4, 8, 16, 32) and activation: without a
    mask, with a mask on the field's box, with a mask on a larger box (the field shrunk after the mask was made).  Alpha under the
    rule; exactly 0 wherever the float64 lookup culls; getDenseAlpha's dense_xyz has the bits of the float32 torch formula."""
    from tensoir_amd import ops
    s = R.scene(row, kind)
    m, f = world.model(s), world.field(s)
    for grid in R.LATTICES:
        for length in R.dense_lengths(s.sc):
            r64, r32 = R.dense_alpha(s.sc, grid, length, F64), R.dense_alpha(s.sc, grid, length, F32)
            alpha, lins = ops.dense_alpha(f, grid, length)
            assert alpha.shape == tuple(grid) and all(torch.equal(l.cpu(), torch.linspace(0, 1, g)) for l, g in zip(lins, grid))
            check(f"dense_alpha {s.name} {ident(grid)} length {length:.4g}", alpha, r32.alpha, r64.alpha)
            assert bool((alpha.cpu()[~r64.kept] == 0).all()), (grid, "a culled point has alpha")
            assert torch.equal(ops.dense_alpha(f, grid, length)[0], alpha)
        alpha, xyz = m.getDenseAlpha(grid)
        assert torch.equal(xyz.cpu(), R.lattice(s.sc, grid)), grid
        assert torch.equal(alpha, ops.dense_alpha(f, grid, R.step_of(s.sc))[0])


# ---- 5. tir_filter_rays --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,kind", R.FILTER_SCENES, ids=ident)
def test_filter_rays(world, row, kind):
    """One wave per ray, four per block, 64 samples per pass: 1, 3, 4, 5 and 257 rays at 129 samples, 257 rays at 1, 63, 64, 65, 129
    and 256 samples.  The designed rays (occupancy_reference.filter_case): the only hits from the second and from the third chunk
    on, a hit at index n_samples - 1, a hit at index n_samples that must not count, an origin inside the box, the box missed, a
    zero direction component, near_ and far_ each the binding clamp.  A mask on the field's box and one on a larger box.  Exact."""
    from tensoir_amd import ops
    s = R.filter_scene(row, kind)
    f = world.field(s)
    for n, S in R.FILTER_CASES:
        fx = R.filter_case(s, n, S)
        got = ops.filter_rays(f, dev(fx.rays), S, False)
        exact(f"filter_rays {s.name} rays {n} samples {S} ({int(fx.want.sum())} kept; designed {sorted(fx.designed)})", got, fx.want)
        assert torch.equal(ops.filter_rays(f, dev(fx.rays), S, False), got)


@pytest.mark.parametrize("row,kind", R.FILTER_SCENES, ids=ident)
def test_filter_rays_bbox(world, row, kind):
    """bbox_only: 1, 3, 4, 5 and 257 generic rays (origins inside and outside, the box missed, zero direction components), each with
    |tmax - tmin| at least 1e-4 of the larger.  Exact against the float64 slab test."""
    from tensoir_amd import ops
    s = R.filter_scene(row, kind)
    for n in R.SLAB_COUNTS:
        rays = R.slab_rays(s, n)
        got = ops.filter_rays(world.field(s), dev(rays), 7, True)
        exact(f"filter_rays bbox {s.name} rays {n}", got, R.filter_rays(s.sc, rays, 7, True, F64))
        assert torch.equal(ops.filter_rays(world.field(s), dev(rays), 7, True), got)


def test_filter_rays_bbox_ties(world):
    """Constructed ties at the POW2 box, tmax == tmin in exactly representable numbers (through an edge, through a corner, with zero
    direction components): 0, as the reference's strict > gives; each tie's neighbour passes."""
    from tensoir_amd import ops
    s = R.scene("pow2", "masked")
    rays, want = R.slab_ties()
    exact("filter_rays bbox ties", ops.filter_rays(world.field(s), dev(rays), 1, True), want)


@pytest.mark.parametrize("row,kind", R.FILTER_SCENES, ids=ident)
def test_model_filtering_rays(world, row, kind):
    """TensorVMSplit.filtering_rays with rays on the host and a chunk that forces five launches (64 rays each): the mask and the kept
    rays, in both modes (bbox_only on the slab rays, which have their margin)."""
    s = R.filter_scene(row, kind)
    fx = R.filter_case(s, 257, 129)
    slab = R.slab_rays(s, 257)
    m = world.model(s)
    with quiet():
        kept, mask = m.filtering_rays(fx.rays, N_samples=129, chunk=R.CHUNKED_RAYS)
        kept_b, mask_b = m.filtering_rays(slab, chunk=R.CHUNKED_RAYS, bbox_only=True)
    assert not mask.is_cuda and not kept.is_cuda
    exact(f"filtering_rays {s.name}", mask, fx.want)
    assert torch.equal(kept, fx.rays[fx.want])
    want_b = R.filter_rays(s.sc, slab, 256, True, F64)
    exact(f"filtering_rays bbox {s.name}", mask_b, want_b)
    assert torch.equal(kept_b, slab[want_b])


# ---- 6. updateAlphaMask composed -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,kind", R.UPDATE_CASES, ids=ident)
def test_update_alpha_mask(row, kind):
    """updateAlphaMask on a (10,12,8) lattice, shrink to the returned box, updateAlphaMask on (12,8,10), alphaMask_thres each time in
    a gap of the float64 pooled alpha (occupancy_reference.threshold_for): the volume equals the float64 reference in every
    voxel, the returned box has the bits of the float32 formula at the index bbox, the mask keeps the field's box, the shrunk
    field is the restated one; in the second update the mask's box differs from the field's."""
    u = R.update_case(row, kind, *R.UPDATE_GRIDS)
    m = build(u.scene.ck)
    m.alphaMask_thres = u.thres1
    with quiet():
        box = m.updateAlphaMask(u.grid1)
    exact(f"update {u.scene.name} {ident(u.grid1)} volume", m.alphaMask.alpha_volume[0, 0], u.first.vol)
    assert torch.equal(box.cpu(), u.first.aabb) and torch.equal(m.alphaMask.aabb.cpu(), u.scene.sc.aabb)
    with quiet():
        m.shrink(box)
    assert torch.equal(m.aabb.cpu(), u.sc2.aabb) and [int(g) for g in m.gridSize] == u.sc2.grid
    for i in range(3):
        assert torch.equal(m.density_plane[i].detach().cpu(), u.sc2.density_plane[i]) and torch.equal(m.density_line[i].detach().cpu(), u.sc2.density_line[i])
    assert float(m.stepSize) == R.step_of(u.sc2) and not torch.equal(m.alphaMask.aabb, m.aabb)
    old = m.alphaMask.aabb.clone()
    alpha, _ = m.getDenseAlpha(u.grid2)
    r32 = R.dense_alpha(u.sc2, u.grid2, R.step_of(u.sc2), F32)
    check(f"update {u.scene.name} second lattice alpha", alpha, r32.alpha, u.second.alpha)
    assert bool((alpha.cpu()[~u.second.kept] == 0).all())
    m.alphaMask_thres = u.thres2
    with quiet():
        box2 = m.updateAlphaMask(u.grid2)
    exact(f"update {u.scene.name} {ident(u.grid2)} volume after shrink", m.alphaMask.alpha_volume[0, 0], u.second.vol)
    assert torch.equal(box2.cpu(), u.second.aabb) and torch.equal(m.alphaMask.aabb, m.aabb) and not torch.equal(m.alphaMask.aabb, old)


def test_update_alpha_mask_empty_scene(world):
    """No voxel passes (alphaMask_thres 2): updateAlphaMask raises before it assigns anything -- the mask object, packed_field() and a
    march are what they were; the same on a model without a mask."""
    from tensoir_amd import ops
    from tensoir_amd._lib import TensoirHipError
    for kind in ("masked", "open"):
        s = R.scene("d16_a48", kind)
        m = build(s.ck)
        rays = dev(R.M.base_rays(40))
        mask, f = m.alphaMask, m.packed_field()
        before = [t.clone() for t in ops.march_primary(f, rays, None, 65, 0.0)]
        m.alphaMask_thres = 2.0
        with pytest.raises(TensoirHipError), quiet():
            m.updateAlphaMask((6, 7, 8))
        assert m.alphaMask is mask and m.packed_field() is f
        after = ops.march_primary(m.packed_field(), rays, None, 65, 0.0)
        assert all(torch.equal(a, b) for a, b in zip(before, after))
        m.alphaMask_thres = 1e-3
        with quiet():
            m.updateAlphaMask((6, 7, 8))
        assert m.alphaMask is not mask and m.packed_field() is not f
    print("\n[occupancy update empty scene] device 0 mismatches (bound 0)")


# ---- 7. occupied_box -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,kind", R.BOX_SCENES, ids=ident)
def test_occupied_box(world, row, kind):
    """AlphaGridMask.occupied_box is the restated box, and no point outside it is reported occupied by the kernel or by the float64
    reference: a shell just outside every face (1e-4 of the box's size) and points up to a box size further out."""
    from tensoir_amd import ops
    s = R.scene(row, kind)
    m = world.model(s)
    lo, hi = m.alphaMask.occupied_box()
    want_lo, want_hi = R.occupied_box(s.sc.alpha_volume, s.sc.alpha_aabb)
    assert np.allclose(lo, want_lo, rtol=0, atol=1e-6) and np.allclose(hi, want_hi, rtol=0, atol=1e-6), (lo, want_lo, hi, want_hi)
    pts = R.outside_box_points(lo, hi, 2000, torch.Generator().manual_seed(12))
    got = ops.occupancy_query(world.field(s), dev(pts))
    ref = R.occupancy(s.sc, pts, F64)
    print(f"\n[occupancy occupied_box {s.name}] device {int(got.sum())} hits, float64 {int(ref.sum())} hits among {pts.shape[0]} points outside (bound 0)")
    assert int(got.sum()) == 0 and int(ref.sum()) == 0
