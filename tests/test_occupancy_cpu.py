"""CPU leg of the occupancy-mask suite (tests/test_gpu_occupancy_kernels.py): ties the restatement (tests/occupancy_reference.py) to
the pinned oracle and to the recorded tests/golden/mask_maintenance.npz, asserts on every fixture of the GPU file the margins that
make each discrete decision the same in float32 and float64, and shows that each seeded mistake of the restatement lands outside
what the GPU file accepts (the tests it breaks are named in each docstring).  Prints the float32 restatement's own distance from
float64 per dense-alpha fixture -- a tenth of what the GPU tests allow."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import tensoir_oracle as O
from tests import occupancy_reference as R
from tests.helpers import T, golden_scene

F32, F64 = torch.float32, torch.float64


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)


# ---- the restatement against the pinned oracle -----------------------------------------------------------------------------------------
def brute_pack(vol):
    """tir_pack_occupancy, voxel by voxel from the header's sentence."""
    D, H, W = vol.shape
    out = np.zeros((D + 1, H + 1, W + 1), dtype=np.uint8)
    for z0 in range(-1, D):
        for y0 in range(-1, H):
            for x0 in range(-1, W):
                for c in range(8):
                    x, y, z = x0 + (c & 1), y0 + ((c >> 1) & 1), z0 + (c >> 2)
                    if 0 <= x < W and 0 <= y < H and 0 <= z < D and vol[z, y, x] > 0.5:
                        out[z0 + 1, y0 + 1, x0 + 1] |= 1 << c
    return out.reshape(-1)


@pytest.mark.parametrize("dims", R.PACK_DIMS[:6], ids=ident)
def test_pack_restatement(dims):
    vol = R.pack_volume(dims)
    if vol.size >= 30:
        assert len(set(vol.reshape(-1).tolist())) == 4, "0, 1, 0.5 and nextafter(0.5, 1) are not all there"
    assert np.array_equal(R.pack_occupancy(vol), brute_pack(vol))


def test_pack_sizes():
    sizes = sorted((w + 1) * (h + 1) * (d + 1) for w, h, d in R.PACK_DIMS)
    assert {255, 256, 258} <= set(sizes) and sizes[-1] > 4000 and sizes[0] == 8


@pytest.mark.parametrize("row,kind", [("d16_a48", "masked"), ("d8_a48", "shrunk"), ("relu_d16_a48", "open"), ("d4_a48", "masked")], ids=ident)
def test_restatement_equals_oracle(row, kind):
    """In float32 the restatement is the oracle's explicit backend operation for operation: the lattice, the mask sample, the new
    volume and box, both modes of filtering_rays, the sample positions -- equal bits; dense alpha to one ulp of 1, with the same
    culled points.  Against the aten backend (F.grid_sample)
    alpha agrees to 2e-6 and the lookup's decision is the same on points with margin."""
    s = R.scene(row, kind)
    sc = s.sc
    grid = (7, 9, 13)
    with torch.no_grad():
        a_exp, d_exp = O.dense_alpha(sc, grid, "explicit")
        a_aten, _ = O.dense_alpha(sc, grid, "aten")
    mine = R.dense_alpha(sc, grid, R.step_of(sc), F32)
    # the oracle evaluates the lattice slice by slice: torch's channel sum then runs in another order on a few points (one ulp of 1)
    assert torch.equal(mine.xyz, d_exp) and float((mine.alpha - a_exp).abs().max()) <= 2.0 ** -23 and torch.equal(mine.alpha == 0, a_exp == 0)
    assert float((mine.alpha - a_aten).abs().max()) <= 2e-6
    sc2 = copy.deepcopy(sc)
    with torch.no_grad():
        aabb = O.update_alpha_mask(sc2, grid, thres=1.1e-3, backend="explicit")
    u = R.update_alpha_mask(sc, grid, 1.1e-3, F32)
    assert torch.equal(u.vol, sc2.alpha_volume) and torch.equal(u.aabb, aabb) and torch.equal(sc2.alpha_aabb, sc.aabb)
    pooled = (u.pooled >= np.float32(1.1e-3)).float()
    assert torch.equal(pooled, u.vol), "max_pool3d and the restated pool disagree"
    if kind == "open":
        return
    pts = R.query_points(s, 3001)
    with torch.no_grad():
        v_exp, v_aten = O.sample_occupancy(sc, pts, "explicit"), O.sample_occupancy(sc, pts, "aten")
    inside = (pts.abs() < 1e3).all(-1)                   # the oracle's index arithmetic overflows on the far-away points
    v = R.sample_mask(sc.alpha_volume, sc.alpha_aabb, pts, F32)
    assert torch.equal(v[inside], v_exp[inside]) and torch.equal(v[inside] > 0, v_aten[inside] > 0)
    assert not bool((v[~inside] > 0).any()) and int((~inside).sum()) == 6
    fs = R.filter_scene("d16_a48", kind if kind != "open" else "masked")
    fx = R.filter_case(fs, 257, 129)
    with torch.no_grad():
        pts_o, _, _ = O.sample_ray(fs.sc, fx.rays[:, :3], fx.rays[:, 3:6], 129)
        assert torch.equal(R.ray_samples(fs.sc, fx.rays, 129), pts_o)
        for bbox_only in (False, True):
            assert torch.equal(R.filter_rays(fs.sc, fx.rays, 129, bbox_only, F32), O.filtering_rays(fs.sc, fx.rays, 129, bbox_only, "explicit"))


def test_restatement_equals_golden(golden):
    """tests/golden/mask_maintenance.npz, written by the reference: the lattice has the recorded bits, float32 alpha agrees to
    2e-5 without and with the golden mask, the pool of the recorded alpha IS the recorded volume and its index box the recorded
    box, and both modes of filtering_rays on the recorded mask give the recorded ray masks (the float64 run on every ray whose
    decision has margin; the others are counted)."""
    mg = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_maintenance.npz"))
    sc = golden_scene(golden)
    grid = tuple(int(x) for x in mg["grid"])
    step = R.step_of(sc)
    masked = R.dense_alpha(sc, grid, step, F32)
    assert torch.equal(masked.xyz, T(mg, "dense_xyz"))
    assert float((masked.alpha - T(mg, "masked/alpha")).abs().max()) < 2e-5
    open_sc = sc.to(F32)
    open_sc.alpha_volume = open_sc.alpha_aabb = None
    assert float((R.dense_alpha(open_sc, grid, step, F32).alpha - T(mg, "nomask/alpha")).abs().max()) < 2e-5
    vol, bbox = R.alpha_pool(np.array(mg["masked/alpha"]), 1e-3)
    assert torch.equal(vol, T(mg, "update/volume")) and torch.equal(R.index_box(sc, grid, bbox), T(mg, "update/aabb"))
    new = R.with_mask(sc, vol, T(mg, "update/mask_aabb"))
    rays = T(mg, "filter/rays")
    assert torch.equal(R.filter_rays(new, rays, 80, False, F32), T(mg, "filter/mask_alpha"))
    assert torch.equal(R.filter_rays(new, rays, 256, True, F32), T(mg, "filter/mask_bbox"))
    m64, firm = R.ray_margins(new, rays, 80)
    assert torch.equal(m64[firm], T(mg, "filter/mask_alpha")[firm])
    ok = R.slab_margin(new, rays) >= R.SLAB_MARGIN
    assert torch.equal(R.filter_rays(new, rays, 256, True, F64)[ok], T(mg, "filter/mask_bbox")[ok])
    print(f"\n[occupancy cpu golden] rays without margin: {int((~firm).sum())} (lookup), {int((~ok).sum())} (slab) of {rays.shape[0]}")
    vol2, bbox2 = R.alpha_pool(R.dense_alpha(new, (33, 29, 31), step, F32).alpha.numpy(), 1e-3)
    flips = int((vol2 != T(mg, "update2/volume")).sum())
    print(f"[occupancy cpu golden] second update: {flips} voxels differ from the recorded volume")
    assert flips == 0 and torch.equal(R.index_box(new, (33, 29, 31), bbox2), T(mg, "update2/aabb"))


# ---- the fixtures' margins -------------------------------------------------------------------------------------------------------------
def test_faces_are_integers_in_both_types():
    """On the suite's box the mask's index coordinates of the box's own corners are 0 and dim - 1 exactly in float32 and in float64
    (on config_scenes' box the far z face is 18.999998 in float32): lattice points on the faces of a mask on the field's box are
    integers by construction.  The POW2 mask: every lattice_points() coordinate has the same index coordinates in both types."""
    for row, kind in [("d16_a48", "masked"), ("d4_a48", "masked"), ("pow2", "masked")]:
        sc = R.scene(row, kind).sc
        D, H, W = sc.alpha_volume.shape
        want = torch.tensor([[0.0, 0.0, 0.0], [W - 1.0, H - 1.0, D - 1.0]], dtype=F64)
        for dt in (F32, F64):
            assert torch.equal(R.index_coords(sc.alpha_aabb, (W, H, D), sc.aabb, dt).double(), want), (row, dt)
    s = R.scene("pow2", "masked")
    lp = R.lattice_points(s)
    D, H, W = s.sc.alpha_volume.shape
    for dt in (F32, F64):
        assert torch.equal(R.index_coords(s.sc.alpha_aabb, (W, H, D), lp.pts, dt).double(), lp.ic), dt
    on = lp.ic == lp.ic.round()
    assert int(on.all(-1).sum()) >= (W + 2) * (H + 2) * (D + 2) and int((on.sum(-1) == 2).sum()) > 500 and int((on.sum(-1) == 1).sum()) > 500
    assert bool((lp.ic == -1).any()) and bool((lp.ic[:, 0] == W).any())
    hit = R.occupancy(s.sc, lp.pts, F64)
    counted = R.occupancy(s.sc, lp.pts, F64, "zero_corners")
    assert 0.2 < float(hit.float().mean()) < 0.8 and int((hit != counted).sum()) > 50, "the zero-weight corners decide nothing here"


@pytest.mark.parametrize("row,kind", R.QUERY_SCENES, ids=ident)
def test_query_point_margins(row, kind):
    s = R.scene(row, kind)
    vol, aabb = s.sc.alpha_volume, s.sc.alpha_aabb
    for n in R.QUERY_COUNTS:
        pts = R.query_points(s, n)
        assert pts.shape == (n, 3) and pts.dtype == F32
        d = R.integer_distance(vol, aabb, pts)
        assert float(d.min()) >= R.INDEX_MARGIN, (n, float(d.min()))
        assert torch.equal(R.occupancy(s.sc, pts, F32), R.occupancy(s.sc, pts, F64))
    pts = R.query_points(s, 3001)
    D, H, W = vol.shape
    ic = R.index_coords(aabb, (W, H, D), pts, F64)
    hit = R.occupancy(s.sc, pts, F64)
    skirt = ((ic < 0) | (ic > torch.tensor([W - 1.0, H - 1.0, D - 1.0], dtype=F64))).any(-1)
    assert int((hit & ~skirt).sum()) > 200 and int((~hit & ~skirt).sum()) > 200
    if row == "pow2":
        assert int((hit & skirt).sum()) > 5 and int((hit & (torch.floor(ic) == -1).any(-1)).sum()) > 3, "no hit in the skirt"
    assert int(((ic < -1) | (ic > torch.tensor([W, H, D], dtype=F64))).any(-1).sum()) > 100
    if kind == "shrunk":
        assert bool((s.sc.alpha_aabb[0] < s.sc.aabb[0]).all()) and bool((s.sc.alpha_aabb[1] > s.sc.aabb[1]).all())
        assert int((hit != R.occupancy(s.sc, pts, F64, "field_box")).sum()) > 100


@pytest.mark.parametrize("row,kind", R.DENSE_CASES, ids=ident)
def test_dense_alpha_fixture_margins(row, kind):
    """Every lattice point's index coordinates in the mask keep INDEX_MARGIN from the integers, the faces of a mask on the field's
    own box apart (integers by construction, test_faces_are_integers_in_both_types); float32 and float64 cull the same points."""
    s = R.scene(row, kind)
    sc = s.sc
    assert sc.density_plane[0].shape[1] == R.CS.ROW[row].n_dcomp and O.density_act(sc) == R.CS.ROW[row].act
    for grid in R.LATTICES:
        if kind != "open":
            pts = R.lattice(sc, grid).reshape(-1, 3)
            d = R.integer_distance(sc.alpha_volume, sc.alpha_aabb, pts)
            if kind == "masked":
                assert torch.equal(sc.aabb, sc.alpha_aabb)
                d = torch.where(R.lattice_faces(grid), torch.ones_like(d), d)
            assert float(d.min()) >= R.INDEX_MARGIN, (grid, float(d.min()))
        for length in R.dense_lengths(sc):
            r64, r32 = R.dense_alpha(sc, grid, length, F64), R.dense_alpha(sc, grid, length, F32)
            assert torch.equal(r64.kept, r32.kept), grid
            print(f"\n[occupancy cpu dense_alpha {s.name} {ident(grid)} length {length:.4g}] float32 restatement "
                  f"{R.distance(r32.alpha, r64.alpha):.2e}; culled {int((~r64.kept).sum())} of {r64.kept.numel()}")
    if kind != "open" and row != "relu_d16_a48":
        big = R.dense_alpha(sc, R.LATTICES[-1], R.step_of(sc), F64)
        assert 0.02 < float((~big.kept).float().mean()) < 0.95, "the mask culls nothing or everything"
        assert bool((big.alpha[~big.kept] == 0).all())
        if kind == "shrunk":
            assert int((big.kept != R.dense_alpha(sc, R.LATTICES[-1], R.step_of(sc), F64, "field_box").kept).sum()) > 100


@pytest.mark.parametrize("row,kind", R.UPDATE_CASES, ids=ident)
def test_update_fixture_margins(row, kind):
    """Both updates: the threshold lies within a factor of two of 1e-3 and the pooled float64 alpha keeps ten times the alpha
    bound from it; the lattice's lookups in the existing mask are firm; float32 and float64 give the same volume and box."""
    u = R.update_case(row, kind, *R.UPDATE_GRIDS)
    for sc, grid, thres, margin, res, exact in ((u.scene.sc, u.grid1, u.thres1, u.margin1, u.first, R.lattice_faces(u.grid1)),
                                                (u.sc2, u.grid2, u.thres2, u.margin2, u.second, u.exact2)):
        assert R.THRES_RANGE[0] < thres < R.THRES_RANGE[1] and thres == float(np.float32(thres))
        gap = float((res.pooled - thres).abs().min())
        assert gap >= margin >= 10 * 10 * 2.0 ** -24 * float(res.alpha.max()), (gap, margin)
        r32 = R.update_alpha_mask(sc, grid, thres, F32)
        assert torch.equal(r32.vol, res.vol) and r32.bbox == res.bbox and torch.equal(r32.aabb, res.aabb)
        assert 0.2 < float(res.vol.mean()) < 0.9
        if sc.alpha_volume is not None:
            hit, firm = R.decision_margin(sc.alpha_volume, sc.alpha_aabb, R.lattice(sc, grid).reshape(-1, 3), exact)
            assert bool(firm.all()), int((~firm).sum())
            assert torch.equal(hit.view(res.kept.shape), res.kept)
        print(f"\n[occupancy cpu update {u.scene.name} {ident(grid)}] thres {thres:.6g}, nearest pooled alpha {gap:.2e} away (required {margin:.2e}); "
              f"occupied {float(res.vol.mean()):.2f}; bbox {res.bbox}")
    assert not torch.equal(u.sc2.aabb, u.sc2.alpha_aabb), "the shrink left the box as it was"
    assert bool((u.sc2.aabb[0] >= u.sc2.alpha_aabb[0]).all()) and bool((u.sc2.aabb[1] <= u.sc2.alpha_aabb[1]).all())
    assert int((~u.second.kept).sum()) > 50


@pytest.mark.parametrize("row,kind", R.FILTER_SCENES, ids=ident)
def test_filter_fixture_margins(row, kind):
    """Every ray of every case either has a hit with margin or consists of misses with margin, at its sample count and at one
    more; the designed rays are what they are for; float32 and float64 give the same masks."""
    s = R.filter_scene(row, kind)
    sc = s.sc
    for n, S in R.FILTER_CASES:
        fx = R.filter_case(s, n, S)
        assert fx.rays.shape == (n, 6) and fx.rays.dtype == F32
        for samples in (S, S + 1):
            mask, firm = R.ray_margins(sc, fx.rays, samples)
            assert bool(firm.all()), (n, S, samples)
        assert torch.equal(R.filter_rays(sc, fx.rays, S, False, F64), fx.want) and torch.equal(R.filter_rays(sc, fx.rays, S, False, F32), fx.want)
        hits = R.ray_hits(sc, fx.rays, S + 1, F64)
        d = fx.designed
        if n == 257:
            need = {"inside", "miss_box", "zero_dir", "near", "near_skips", "far"} | ({"chunk2"} if S > 64 else set()) | \
                ({"chunk3"} if S > 128 else set()) | ({"last", "behind"} if 1 < S < 256 else set())
            assert need <= set(d), (S, sorted(need - set(d)))
        first = lambda r: int(hits[r].int().argmax())
        if "chunk2" in d:
            assert 64 <= first(d["chunk2"]) < 128 and bool(fx.want[d["chunk2"]])
        if "chunk3" in d:
            assert 128 <= first(d["chunk3"]) < S and bool(fx.want[d["chunk3"]])
        if "last" in d:
            assert first(d["last"]) == S - 1 and bool(fx.want[d["last"]])
        if "behind" in d:
            assert first(d["behind"]) == S and not bool(fx.want[d["behind"]])
        tmin, tmax = R.slab(sc, fx.rays, F32)
        if "miss_box" in d:
            assert not bool(tmax[d["miss_box"]] > tmin[d["miss_box"]])
        if "near" in d:
            assert float(tmin[d["near"]]) < sc.near_far[0] and bool(fx.want[d["near"]])
        if "near_skips" in d:
            assert float(tmin[d["near_skips"]]) < sc.near_far[0] and not bool(fx.want[d["near_skips"]])
        if "far" in d:
            assert float(tmin[d["far"]]) > sc.near_far[1]
        if "zero_dir" in d:
            assert bool((fx.rays[d["zero_dir"], 3:6] == 0).any())
        if "inside" in d:
            o = fx.rays[d["inside"], :3]
            assert bool(((o > sc.aabb[0]) & (o < sc.aabb[1])).all())
    for n in R.SLAB_COUNTS:
        rays = R.slab_rays(s, n)
        assert rays.shape == (n, 6) and float(R.slab_margin(sc, rays).min()) >= R.SLAB_MARGIN
        assert torch.equal(R.filter_rays(sc, rays, 1, True, F32), R.filter_rays(sc, rays, 1, True, F64))
    both = R.filter_rays(sc, R.slab_rays(s, 257), 1, True, F64)
    assert 20 < int(both.sum()) < 237


def test_slab_ties_are_exact():
    """tmax == tmin, in float32 and in float64, on every constructed tie; the neighbour of each passes with margin."""
    sc = R.scene("pow2", "masked").sc
    rays, want = R.slab_ties()
    for dt in (F32, F64):
        tmin, tmax = R.slab(sc, rays, dt)
        assert bool((tmin[~want] == tmax[~want]).all()) and bool((tmax[want] > tmin[want]).all()), dt
        assert torch.equal(R.filter_rays(sc, rays, 1, True, dt), want)
    assert float(R.slab_margin(sc, rays[want]).min()) >= R.SLAB_MARGIN and int((~want).sum()) == 4
    assert bool((rays[:, 3:6] == 0).any())


@pytest.mark.parametrize("row,kind", R.BOX_SCENES, ids=ident)
def test_occupied_box_reference(row, kind):
    """No point outside the restated occupied_box is a hit of the float64 lookup: on the shell just outside every face and
    further out."""
    sc = R.scene(row, kind).sc
    lo, hi = R.occupied_box(sc.alpha_volume, sc.alpha_aabb)
    pts = R.outside_box_points(lo, hi, 2000, torch.Generator().manual_seed(12))
    assert pts.shape[0] > 20000
    assert not bool(R.occupancy(sc, pts, F64).any()) and not bool(R.occupancy(sc, pts, F32).any())
    inner = R.outside_box_points([l + 0.3 * (h - l) for l, h in zip(lo, hi)], [h - 0.3 * (h - l) for l, h in zip(lo, hi)], 500,
                                 torch.Generator().manual_seed(13))
    assert bool(R.occupancy(sc, inner, F64).any()), "the box test would pass with any box"


# ---- seeded mistakes: each lands outside what the GPU file accepts (its comparisons of these outputs are exact) --------------------------
def pool_outputs(flaw=None):
    """Every (volume, bbox) test_alpha_pool* of the GPU file compares, in its order."""
    out = []
    for shape in R.POOL_SHAPES:
        for thres in R.POOL_THRES:
            for seed in range(3):
                out.append(R.alpha_pool(R.pool_values(shape, thres, seed), thres, flaw))
        for corner in range(8):
            out.append(R.alpha_pool(R.pool_corner(shape, corner), 1e-3, flaw))
        out.append(R.alpha_pool(np.ones(shape, dtype=np.float32), 1e-3, flaw))
    return out


def differs(a, b):
    return sum(1 for (va, ba), (vb, bb) in zip(a, b) if not torch.equal(va, vb) or ba != bb)


def test_pool_fixture_holds_its_values():
    """The synthetic alpha holds what the issue lists, and the four thresholds do what they are for."""
    for shape in R.POOL_SHAPES:
        seen = np.concatenate([R.pool_values(shape, 1e-3, seed).reshape(-1) for seed in range(3)])
        t = np.float32(1e-3)
        if seen.size > 100:
            for v in (t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)), np.float32(np.inf)):
                assert (seen == v).any(), (shape, v)
            assert (seen < 0).any() and ((seen > 1) & np.isfinite(seen)).any() and np.signbit(seen[seen == 0]).any()
        for seed in range(3):
            vol, bbox = R.alpha_pool(R.pool_values(shape, 2.0, seed), 2.0)
            assert float(vol.sum()) == 0 and bbox == R.BBOX_SENTINEL
            vol, bbox = R.alpha_pool(R.pool_values(shape, 0.0, seed), 0.0)
            assert float(vol.mean()) == 1 and bbox == [0, 0, 0, shape[0] - 1, shape[1] - 1, shape[2] - 1]
    truth = pool_outputs()
    assert any(0 < float(v.mean()) < 1 for v, _ in truth)


def test_flaw_pool_gt():
    """`>` for `>=` at the threshold: test_alpha_pool (values exactly at the threshold; thres 0 and 1)."""
    assert differs(pool_outputs("pool_gt"), pool_outputs()) >= 5


def test_flaw_pool_no_clamp():
    """The clamp to [0, 1] missing: test_alpha_pool at thres 2, where 7.0 and +inf would pass."""
    assert differs(pool_outputs("pool_no_clamp"), pool_outputs()) >= 3


def test_flaw_pool_border():
    """A pool that wraps round at a border, and one that skips the last layer: test_alpha_pool's corner patterns."""
    truth = pool_outputs()
    assert differs(pool_outputs("pool_wrap"), truth) >= 8 and differs(pool_outputs("pool_skip"), truth) >= 4


def test_flaw_pool_axes():
    """Swapped axes in the transposition: test_alpha_pool on every shape that is not symmetric in x and y."""
    assert differs(pool_outputs("pool_axes"), pool_outputs()) >= 10


def test_flaw_zero_corners():
    """Zero-fraction corners counted: test_occupancy_query_on_lattice (nodes, edges and faces of the POW2 mask)."""
    s = R.scene("pow2", "masked")
    lp = R.lattice_points(s)
    assert int((R.occupancy(s.sc, lp.pts, F64) != R.occupancy(s.sc, lp.pts, F64, "zero_corners")).sum()) > 50


def test_flaw_no_minus1():
    """The -1 base cell ignored: test_occupancy_query[pow2-masked] (hits in the skirt) and test_occupancy_query_on_lattice."""
    s = R.scene("pow2", "masked")
    pts = R.query_points(s, 3001)
    assert int((R.occupancy(s.sc, pts, F64) != R.occupancy(s.sc, pts, F64, "no_minus1")).sum()) > 3
    lp = R.lattice_points(s)
    assert int((R.occupancy(s.sc, lp.pts, F64) != R.occupancy(s.sc, lp.pts, F64, "no_minus1")).sum()) > 20


def test_flaw_slab_ge():
    """`>=` in the slab test: test_filter_rays_bbox_ties."""
    sc = R.scene("pow2", "masked").sc
    rays, want = R.slab_ties()
    assert int((R.filter_rays(sc, rays, 1, True, F64, "slab_ge") != want).sum()) == int((~want).sum())


def filter_cases():
    return [(R.filter_scene(row, kind), n, S) for row, kind in R.FILTER_SCENES for n, S in R.FILTER_CASES]


def designed_rows_differ(flaw, name):
    """The cases of test_filter_rays that hold the designed ray `name`, and those of them on which the flawed restatement gets that
    very ray wrong."""
    held, wrong = 0, 0
    for s, n, S in filter_cases():
        fx = R.filter_case(s, n, S)
        if name in fx.designed:
            held += 1
            r = fx.designed[name]
            wrong += int(bool(R.filter_rays(s.sc, fx.rays[r:r + 1], S, False, F64, flaw)[0]) != bool(fx.want[r]))
    return held, wrong


def test_flaw_no_near():
    """The near_ clamp dropped: test_filter_rays, every case that holds the ray `near_skips` (all those of 257 rays)."""
    held, wrong = designed_rows_differ("no_near", "near_skips")
    assert held == 12 and wrong == held


def test_flaw_off_by_one():
    """Sample index off by one: test_filter_rays, every case that holds the ray `behind` (a hit at index n_samples)."""
    held, wrong = designed_rows_differ("off_by_one", "behind")
    assert held >= 12 and wrong == held


def test_flaw_one_chunk():
    """The chunk loop stopping after 64 samples: test_filter_rays at 65, 129 and 256 samples (the rays `chunk2`, `chunk3`); no
    case of at most 64 samples changes."""
    for name, least in (("chunk2", 8), ("chunk3", 6)):
        held, wrong = designed_rows_differ("one_chunk", name)
        assert held >= least and wrong == held, name
    for s, n, S in filter_cases():
        if S <= 64:
            fx = R.filter_case(s, n, S)
            assert torch.equal(R.filter_rays(s.sc, fx.rays, S, False, F64, "one_chunk"), fx.want)


def test_flaw_field_box():
    """The mask looked up in the field's box instead of its own: on the shrunk scenes test_occupancy_query, test_dense_alpha
    (it culls many more points: alpha lands a thousand bounds away) and test_filter_rays; nothing changes where the two boxes are
    one."""
    changed = {"masked": 0, "shrunk": 0}
    for s, n, S in filter_cases():
        fx = R.filter_case(s, n, S)
        changed[s.key[1]] += int(not torch.equal(R.filter_rays(s.sc, fx.rays, S, False, F64, "field_box"), fx.want))
    assert changed["masked"] == 0 and changed["shrunk"] >= 6, changed
    for row, kind in R.DENSE_CASES:
        if kind == "shrunk" and row != "relu_d16_a48":
            sc = R.scene(row, kind).sc
            for grid in R.LATTICES[1:]:
                truth, t32 = R.dense_alpha(sc, grid, R.step_of(sc), F64), R.dense_alpha(sc, grid, R.step_of(sc), F32)
                flawed = R.dense_alpha(sc, grid, R.step_of(sc), F64, "field_box")
                assert R.distance(flawed.alpha, truth.alpha) > 100 * R.bound(t32.alpha, truth.alpha), (row, grid)
    s = R.scene("d8_a48", "shrunk")
    pts = R.query_points(s, 3001)
    assert int((R.occupancy(s.sc, pts, F64) != R.occupancy(s.sc, pts, F64, "field_box")).sum()) > 100


def test_every_flaw_has_a_test():
    """Each flaw the restatement can be seeded with is exercised by a test of this file."""
    text = open(__file__.replace(".pyc", ".py")).read()
    for flaw in R.FLAWS:
        assert text.count(f'"{flaw}"') >= 1, flaw
