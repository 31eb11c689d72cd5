"""Ray-mesh queries on the GPU (tir_ray_mesh; ops.ray_mesh / mesh_inside; mesh.raycast, mesh.distance's signed / thresholds /
normals options, the bake command line) against the numpy restatement (tests/raymesh_reference.py).

Comparison rules.  face, count and flags are discrete and must equal the float64 restatement.  t and bary are the restatement's
float64 values rounded to fp32: the kernel forms them in fp64 with the same operations in the same order, so the bound is ONE fp32
ulp of the rounded restatement (a double rounding apart at the most), and the tests print whether the bits are in fact equal.
The closed-form cases (dyadic inputs) must be exact.  Across grids, across runs and against the 1 x 1 x 1 grid (brute force on
the device) every output but `tested` must be equal bit for bit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import components_reference as CR
from tests import distance_reference as D
from tests import raymesh_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 1 << 24


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def mesh_on_device(v, f):
    return dev(v, np.float32).reshape(-1, 3), dev(f, np.int32).reshape(-1, 3)


def cast(o, d, dv, df, grid=None, mode="closest", trange=None):
    """-> {"t", "face", "bary", "count", "flags", "tested"} as numpy arrays."""
    from tensoir_amd import ops
    out = ops.ray_mesh(dev(o, np.float32).reshape(-1, 3), dev(d, np.float32).reshape(-1, 3), dv, df, grid, mode=mode,
                       trange=None if trange is None else dev(trange, np.float32).reshape(-1, 2), bary=True, count=True, flags=True,
                       tested=True)
    torch.cuda.synchronize()
    assert [x.dtype for x in out] == [torch.float32, torch.int32, torch.float32, torch.int32, torch.int32, torch.int32]
    return dict(zip(("t", "face", "bary", "count", "flags", "tested"), (x.cpu().numpy() for x in out)))


def same_bits(a, b, what):
    for k in ("t", "bary"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (what, k)
    for k in ("face", "count", "flags"):
        assert np.array_equal(a[k], b[k]), (what, k)


def ulps(got, ref64):
    """-> (the largest distance of got from fp32(ref64) in ulps of the latter, whether all bits are equal); inf and NaN must match."""
    ref = ref64.astype(np.float32)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    if not fin.any():
        return 0.0, True
    err = np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64)) / np.spacing(np.abs(ref[fin])).astype(np.float64)
    return float(err.max()), bool(np.array_equal(got[fin], ref[fin]))


def assert_equals_restatement(got, ref, what, mode="count"):
    assert np.array_equal(got["face"], ref["face"]), what
    if mode == "count":
        assert np.array_equal(got["count"], ref["count"]) and np.array_equal(got["flags"], ref["flags"]), what
    else:
        assert np.array_equal(got["count"], np.minimum(ref["count"], 1)), what
        assert np.array_equal(got["flags"] & R.INVALID, ref["flags"] & R.INVALID) and not (got["flags"] & ~ref["flags"]).any(), what
    ut, same_t = ulps(got["t"], ref["t"])
    ub, same_b = ulps(got["bary"], ref["bary"])
    print(f"[ray_mesh {what}] {len(got['t'])} rays, {int((got['face'] >= 0).sum())} hit: t within {ut:.2f} ulp of the restatement "
          f"(bits equal: {same_t}), bary within {ub:.2f} ulp (bits equal: {same_b})")
    assert ut <= 1.0 and ub <= 1.0, what


# ---- single triangle ------------------------------------------------------------------------------------------------------------------
def test_single_triangle_dyadic_rays_are_exact():
    from tensoir_amd import ops
    o, d, tr, t, face, bary, count, flags = R.triangle_rays()
    dv, df = mesh_on_device(D.TRIANGLE, R.TRIANGLE_FACE)
    for mode in ("count", "closest"):
        for grid in (None, ops.face_grid(dv, df, dims=[1, 1, 1]), ops.face_grid(dv, df, dims=[8, 4, 1])):
            got = cast(o, d, dv, df, grid, mode, tr)
            assert np.array_equal(got["t"], t.astype(np.float32)) and np.array_equal(got["face"], face), mode
            assert np.array_equal(got["bary"], bary.astype(np.float32), equal_nan=True), mode
            assert np.array_equal(got["count"], count) and np.array_equal(got["flags"], flags), mode
    # [0, +inf] is what a missing trange means
    plain = np.nonzero((tr[:, 0] == 0) & np.isinf(tr[:, 1]))[0]
    same_bits(cast(o[plain], d[plain], dv, df, None, "count"), {k: v[plain] for k, v in cast(o, d, dv, df, None, "count", tr).items()}, "trange")
    hit = ops.ray_mesh(dev(o), dev(d), dv, df, mode="any", trange=dev(tr))[0]
    assert hit.dtype == torch.bool and np.array_equal(hit.cpu().numpy(), count > 0)


# ---- unit cube ----------------------------------------------------------------------------------------------------------------------------
def test_cube_ties_counts_and_inside():
    from tensoir_amd import mesh, ops
    dv, df = mesh_on_device(R.CUBE_VERTS, R.CUBE_FACES)
    wide = ops.face_grid(dv, df, cell=0.5, origin=[-1.0, -1.0, -1.0], dims=[6, 6, 6])       # a box around the cube
    for grid in (None, wide, ops.face_grid(dv, df, dims=[1, 1, 1])):
        # along the axes through the diagonals of two opposite sides: two faces tie at each, the smaller index wins, all four count
        o = np.float32([[-1, 0.5, 0.5], [2, 0.5, 0.5], [0.5, -1, 0.5], [0.5, 0.5, 3]])
        d = np.float32([[1, 0, 0], [-2, 0, 0], [0, 1, 0], [0, 0, -1]])
        got = cast(o, d, dv, df, grid, "count")
        assert list(got["t"]) == [1.0, 0.5, 1.0, 2.0] and list(got["face"]) == [0, 2, 4, 10], got
        assert list(got["count"]) == [4, 4, 4, 4] and (got["flags"] == R.GRAZED).all()
        assert_equals_restatement(got, R.ray_mesh(o, d, R.CUBE_VERTS, R.CUBE_FACES), "cube, axis rays")
        got = cast(o, d, dv, df, grid, "closest")
        assert list(got["t"]) == [1.0, 0.5, 1.0, 2.0] and list(got["face"]) == [0, 2, 4, 10] and (got["count"] == 1).all()
        assert (got["flags"] == R.GRAZED).all()
        # generic rays: two crossings from outside, one from inside
        o = np.float32([[-1, 0.3, 0.6], [0.5, 0.3, 0.6], [0.4, 0.4, 0.7], [3, 2.6, -1.0]])
        d = np.float32([[1, 0.01, 0.02], [1, 0.01, 0.02], [-0.3, 0.2, 0.9], [-2.5, -2.25, 1.5]])
        got = cast(o, d, dv, df, grid, "count")
        assert list(got["count"]) == [2, 1, 1, 2] and (got["flags"] == 0).all()
        assert_equals_restatement(got, R.ray_mesh(o, d, R.CUBE_VERTS, R.CUBE_FACES), "cube, generic rays")
        # inside, outside, outside the cube but inside the box of the wide grid, on the far side of it
        pts = np.float32([[0.5, 0.5, 0.5], [0.1, 0.9, 0.2], [1.5, 0.5, 0.5], [-0.2, 0.3, 0.3], [0.3, 0.3, 1.0001], [7, -3, 2], [np.nan, 0, 0]])
        inside, votes, grazed = (x.cpu().numpy() for x in ops.mesh_inside(dev(pts), dv, df, grid))
        assert votes.dtype == np.uint8 and inside.dtype == bool and grazed.dtype == bool
        assert list(inside) == [True, True, False, False, False, False, False] and list(votes) == [3, 3, 0, 0, 0, 0, 0] and not grazed.any()
        ri, rv, rg = R.inside(pts[:6], R.CUBE_VERTS, R.CUBE_FACES)
        assert np.array_equal(inside[:6], ri) and np.array_equal(votes[:6], rv) and np.array_equal(grazed[:6], rg)
    # the public wrapper: point and face normal of the hit
    r = mesh.raycast((dv, df), dev(np.float32([[-1, 0.3, 0.6], [5, 5, 5]])), dev(np.float32([[2, 0, 0], [1, 0, 0]])))
    assert r["t"].tolist() == [0.5, np.inf] and r["face"].tolist()[1] == -1 and r["count"].tolist() == [1, 0]
    assert np.allclose(r["point"][0].cpu().numpy(), [0, 0.3, 0.6], rtol=0, atol=1e-7)
    assert r["normal"][0].tolist() == [-1.0, 0.0, 0.0] and torch.isnan(r["normal"][1]).all() and torch.isnan(r["point"][1]).all()
    assert torch.isnan(r["bary"][1]).all() and r["flags"].tolist() == [0, 0]


# ---- invalid and empty inputs ----------------------------------------------------------------------------------------------------------------
def test_invalid_rays_empty_inputs_and_refusals():
    import ctypes as C
    from tensoir_amd import _lib, ops
    verts = np.float32([[1, 1, 1], [2, 2, 2], [3, 3, 3], [0, 0, 0], [1, 0, 0], [0, 1, 0]])
    dv, df = mesh_on_device(verts, [[0, 1, 2], [3, 4, 5], [4, 4, 4]])
    o = np.float32([[0.25, 0.25, -1], [np.nan, 0, 0], [0, np.inf, 0], [0.25, 0.25, -1], [0.25, 0.25, -1], [0.25, 0.25, -1], [0.25, 0.25, -1]])
    d = np.float32([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, np.nan, 1], [0, 0, 1], [0, 0, 1]])
    tr = np.float32([[0, np.inf]] * 5 + [[2, 1], [np.nan, 4]])
    for mode in ("count", "closest"):
        got = cast(o, d, dv, df, None, mode, tr)
        assert got["t"][0] == 1.0 and got["face"][0] == 1 and got["count"][0] == 1 and got["flags"][0] == 0
        assert np.isnan(got["t"][1:]).all() and (got["face"][1:] == -1).all() and (got["count"][1:] == 0).all()
        assert (got["flags"][1:] == R.INVALID).all() and np.isnan(got["bary"][1:]).all() and (got["tested"][1:] == 0).all()
        assert_equals_restatement(got, R.ray_mesh(o, d, verts, [[0, 1, 2], [3, 4, 5], [4, 4, 4]], tr), "invalid rays", mode)
    hit, fl = ops.ray_mesh(dev(o), dev(d), dv, df, mode="any", trange=dev(tr), flags=True)
    assert hit.tolist() == [True] + [False] * 6 and fl.tolist() == [0] + [R.INVALID] * 6
    # a mesh with only degenerate faces: every ray misses
    for faces in ([[0, 1, 2]], [[0, 1, 2], [4, 4, 4]]):
        gv, gf = mesh_on_device(verts, faces)
        got = cast(o[:1], d[:1], gv, gf)
        assert got["t"][0] == np.inf and got["face"][0] == -1 and got["count"][0] == 0 and got["flags"][0] == 0 and np.isnan(got["bary"]).all()
        assert ops.mesh_inside(dev(o[:1]), gv, gf)[1].tolist() == [0]
    # no rays, no faces
    none = torch.zeros((0, 3), device="cuda")
    out = ops.ray_mesh(none, none, dv, df, bary=True, count=True)
    assert [tuple(x.shape) for x in out] == [(0,), (0,), (0, 2), (0,)]
    assert ops.ray_mesh(none, none, dv, df, mode="any")[0].shape == (0,) and ops.mesh_inside(none, dv, df)[0].shape == (0,)
    t, f = ops.ray_mesh(dev(o[:1]), dev(d[:1]), dv, torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    assert t.item() == np.inf and f.item() == -1
    # a face index outside [0, V): refused where the grid is built, and never followed by the kernel when it meets one in a list
    bad = dev(np.int32([[0, 1, 2], [3, 4, 6], [4, 4, 4]]))
    with pytest.raises(_lib.TensoirHipError, match="face index"):
        ops.ray_mesh(dev(o[:1]), dev(d[:1]), dv, bad)
    grid = ops.face_grid(dv, df)
    for broken in ([[0, 1, 2], [3, 4, 6], [4, 4, 4]], [[0, 1, 2], [-1, 4, 5], [4, 4, 4]], [[0, 1, 2], [3, 2 ** 31 - 1, 5], [4, 4, 4]]):
        got = cast(o[:1], d[:1], dv, dev(np.int32(broken)), grid, "count")      # the list still names face 1: its indices are checked again
        assert got["t"][0] == np.inf and got["face"][0] == -1 and got["count"][0] == 0
    # a grid of another mesh, a host tensor, the outputs mode "any" does not have
    other = mesh_on_device(R.CUBE_VERTS, R.CUBE_FACES)
    with pytest.raises(ValueError, match="grid"):
        ops.ray_mesh(dev(o), dev(d), dv, df, grid=ops.face_grid(*other))
    with pytest.raises(ValueError, match="grid"):
        ops.mesh_inside(dev(o), dv, df, grid=ops.face_grid(*other))
    with pytest.raises(Exception):
        ops.ray_mesh(torch.from_numpy(o), dev(d), dv, df)
    with pytest.raises(ValueError, match="any"):
        ops.ray_mesh(dev(o), dev(d), dv, df, mode="any", bary=True)
    do, dd, buf = dev(o), dev(d), torch.zeros(16, device="cuda")
    f3, i3, p = (C.c_float * 3), (C.c_int32 * 3), lambda x: C.c_void_p(x.data_ptr())
    args = (p(do), p(dd), None, 7, p(dv), 6, p(df), 3, f3(*grid["cell"]), f3(*grid["origin"]), i3(*grid["dims"]), p(grid["cursor"]),
            p(grid["pairs"]), grid["n_pairs"], p(grid["bounds"]), 2)
    assert _lib.lib().tir_ray_mesh(*args, p(buf), None, None, p(buf), None, None, None) == -1001        # "any" with a t buffer
    assert _lib.lib().tir_ray_mesh(*args, None, None, None, None, None, None, None) == -1001             # "any" without count
    torch.cuda.synchronize()
    assert buf.abs().sum().item() == 0


# ---- triangle soup ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soup_device():
    from tensoir_amd import ops
    v, f, _ = D.soup()
    dv, df = mesh_on_device(v, f)
    grids = {name: ops.face_grid(dv, df, max_pairs=BUDGET, **kw) for name, kw in R.SOUP_GRIDS.items()}
    grids["default"] = ops.face_grid(dv, df)
    assert grids["1"]["dims"] == [1, 1, 1] and grids["1"]["n_pairs"] == 300 and all(g["listed"] == 300 for g in grids.values())
    return dv, df, grids


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2000])
def test_soup_equals_restatement(soup_device, n):
    dv, df, grids = soup_device
    o, d, tr = R.soup_rays()
    ref = {k: x[:n] for k, x in R.soup_reference().items()}
    assert n < 2000 or ((ref["count"] >= 2).sum() > 300 and (ref["count"] == 0).sum() > 300 and (ref["t"] < 0).any())
    for mode in ("count", "closest"):
        got = cast(o[:n], d[:n], dv, df, grids["default"], mode, tr[:n])
        assert_equals_restatement(got, ref, f"soup n={n} {mode}", mode)


def test_soup_is_bit_identical_across_grids_modes_and_runs(soup_device):
    from tensoir_amd import ops
    dv, df, grids = soup_device
    o, d, tr = R.soup_rays()
    ref = R.soup_reference()
    do, dd, dt = dev(o), dev(d), dev(tr)
    for mode in ("count", "closest"):
        base = cast(o, d, dv, df, grids["1"], mode, tr)
        assert set(np.unique(base["tested"])) <= {0, 300}                  # one cell: every face, or none for a ray clipped away
        assert_equals_restatement(base, ref, f"soup 1^3 {mode}", mode)
        for name, g in grids.items():
            got = cast(o, d, dv, df, g, mode, tr)
            same_bits(got, base, f"{name} {mode}")
            same_bits(cast(o, d, dv, df, g, mode, tr), base, f"{name} {mode}, second run")
            print(f"[ray_mesh soup {name} {mode}] dims {g['dims']} pairs {g['n_pairs']}: {got['tested'].mean():.1f} faces tested per ray")
        if mode == "count":
            for name, g in grids.items():
                hit = ops.ray_mesh(do, dd, dv, df, g, mode="any", trange=dt)[0]
                assert np.array_equal(hit.cpu().numpy(), base["count"] > 0), name
    # a rebuilt grid (another fill order, perhaps) gives the same bits
    same_bits(cast(o, d, dv, df, ops.face_grid(dv, df, max_pairs=BUDGET, dims=[16] * 3), "count", tr), cast(o, d, dv, df, grids["16"], "count", tr),
              "rebuilt")


# ---- sphere -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_device():
    from tensoir_amd import ops
    v, f, scaled = D.sphere_pair()
    dv, df = mesh_on_device(v, f)
    return dv, df, dev(scaled), ops.face_grid(dv, df)


def test_sphere_inside_matches_the_analytic_radius(sphere_device):
    from tensoir_amd import mesh, ops
    dv, df, _, grid = sphere_device
    assert mesh.topology(dv, df) == {"closed": True, "boundary_edges": 0, "degenerate": 0}
    p, signed = R.sphere_points()
    inside, votes, grazed = (x.cpu().numpy() for x in ops.mesh_inside(dev(p), dv, df, grid))
    far = np.abs(signed) > 1.0
    print(f"\n[mesh_inside sphere] {len(p)} points, {int(far.sum())} more than one unit from the surface, {int(inside.sum())} inside; "
          f"not unanimous {int(((votes == 1) | (votes == 2)).sum())}, grazed {int(grazed.sum())}")
    assert far.sum() > 2700 and np.array_equal(inside[far], signed[far] < 0)
    assert ((votes[far] == 0) | (votes[far] == 3)).all() and not grazed[far].any()
    again = ops.mesh_inside(dev(p), dv, df)                                  # builds the same default grid itself
    assert np.array_equal(again[1].cpu().numpy(), votes)
    n = 100                                                                  # the restatement, brute force, on the first of them
    ri, rv, rg = R.inside(p[:n], *D.sphere_pair()[:2])
    assert np.array_equal(inside[:n], ri) and np.array_equal(votes[:n], rv) and np.array_equal(grazed[:n], rg)


def test_sphere_rays_from_the_centre(sphere_device):
    from tensoir_amd import ops
    dv, df, _, grid = sphere_device
    v, f, _ = D.sphere_pair()
    o, d = R.sphere_rays()
    got = cast(o, d, dv, df, grid, "count")
    one = ops.face_grid(dv, df, dims=[1, 1, 1])
    brute = cast(o, d, dv, df, one, "count")
    same_bits(got, brute, "default grid against 1^3")
    assert (brute["tested"] == one["listed"]).all() and (brute["count"] == 1).all()
    same_bits(cast(o, d, dv, df, grid, "closest"), brute, "closest against 1^3")
    assert (got["count"] == 1).all() and (got["flags"] == 0).sum() > 4000
    print(f"\n[ray_mesh sphere] dims {grid['dims']} pairs {grid['n_pairs']}: {got['tested'].mean():.1f} faces tested per ray "
          f"(max {got['tested'].max()}) against {len(f)}")
    n = 200
    ref = R.ray_mesh(o[:n], d[:n], v, f)
    assert_equals_restatement({k: x[:n] for k, x in got.items()}, ref, "sphere")
    radius = np.linalg.norm(o[:n].astype(np.float64) + ref["t"][:, None] * d[:n] - D.SPHERE_CENTRE, axis=1)
    mine = np.linalg.norm(o[:n].astype(np.float64) + got["t"][:n, None].astype(np.float64) * d[:n] - D.SPHERE_CENTRE, axis=1)
    print(f"[ray_mesh sphere] hit radius {mine.min():.4f} .. {mine.max():.4f} (restatement {radius.min():.4f} .. {radius.max():.4f}), "
          f"the sphere's is {D.SPHERE_RADIUS}")
    assert np.abs(radius - D.SPHERE_RADIUS).max() < 1.0                      # marching cubes stays within a cell of the sphere
    assert np.abs(mine - radius).max() <= 4 * np.spacing(np.float32(D.SPHERE_RADIUS + 1.0))      # t is one fp32 rounding of the same value


# ---- mesh.distance ------------------------------------------------------------------------------------------------------------------------
def test_mesh_distance_signed_fscore_and_normals_on_the_scaled_sphere(sphere_device, monkeypatch):
    from tensoir_amd import mesh, metrics, ops
    dv, df, ds, _ = sphere_device
    n = D.SPHERE_SAMPLES
    plain = mesh.distance((dv, df), (ds, df), samples=n)
    r = mesh.distance((dv, df), (ds, df), samples=n, signed=True, thresholds=(0.2, 0.6), normals=True)
    print(f"\n[distance sphere] a_to_b {r['a_to_b']}\n[distance sphere] b_to_a {r['b_to_a']}\n[distance sphere] fscore {r['fscore']}")
    for way, share, sign in (("a_to_b", 1.0, -1.0), ("b_to_a", 0.0, 1.0)):          # the sphere lies inside its 1.01 scaling
        x = r[way]
        assert {k: x[k] for k in plain[way]} == plain[way]                           # the magnitudes: the same bits
        assert x["inside_share"] == share and x["undecided"] == 0 and x["signed_mean"] == sign * x["mean"]
    assert r["chamfer"] == plain["chamfer"] and r["hausdorff"] == plain["hausdorff"]
    assert [x["fscore"] for x in r["fscore"]] == [0.0, 1.0] and [x["threshold"] for x in r["fscore"]] == [0.2, 0.6]
    assert r["fscore"][1] == {"threshold": 0.6, "precision": 1.0, "recall": 1.0, "fscore": 1.0}
    # the normal figures against numpy on the same faces
    v, f, scaled = D.sphere_pair()
    for way, (sv, dvv), (hv, hd) in (("a_to_b", (dv, ds), (v, scaled)), ("b_to_a", (ds, dv), (scaled, v))):
        pts, own = ops.sample_surface(sv, df, n, 0)
        near = ops.point_mesh_distance(pts, dvv, df)[1]
        want = R.normal_figures(R.face_normals(hv, f, own.cpu().numpy()), R.face_normals(hd, f, near.cpu().numpy()))
        for k, w in want.items():
            assert abs(r[way][k] - w) <= 1e-12, (way, k, r[way][k], w)
        assert r[way]["normal_consistency"] > 0.95 and r[way]["flipped_share"] == 0.0
    assert metrics.chamfer((v, f), (ds, df), samples=n, signed=True, thresholds=(0.2, 0.6), normals=True) == r
    # an open destination is refused by name, or taken as it comes
    ov, of = mesh_on_device(*R.open_cube())
    cv, cf = mesh_on_device(R.CUBE_VERTS, R.CUBE_FACES)
    with pytest.raises(ValueError, match="4 boundary edges"):
        mesh.distance((cv, cf), (ov, of), samples=256, signed=True)
    loose = mesh.distance((cv, cf), (ov, of), samples=256, signed=True, allow_open=True)
    assert loose["a_to_b"]["n"] == 256 and 0.0 <= loose["a_to_b"]["inside_share"] <= 1.0
    # without an option: the old keys and the old bits, and no ray is cast
    def refuse(*a, **k):
        raise AssertionError("a ray without the option")
    monkeypatch.setattr(ops, "ray_mesh", refuse)
    again = mesh.distance((dv, df), (ds, df), samples=n)
    assert again == plain and sorted(again) == ["a_to_b", "b_to_a", "chamfer", "hausdorff"]
    assert all(sorted(again[w]) == ["max", "mean", "n", "p95", "rms"] for w in ("a_to_b", "b_to_a"))
    for way, (sv, dvv) in (("a_to_b", (dv, ds)), ("b_to_a", (ds, dv))):              # as the parent computed it
        used = torch.unique(df.reshape(-1).long())
        q = torch.cat([sv[used], ops.sample_surface(sv, df, n, 0)[0]])
        dist = ops.point_mesh_distance(q, dvv, df, ops.face_grid(dvv, df))[0]
        assert mesh.distance_summary(dist[:used.numel()], dist[used.numel():]) == again[way]
    with pytest.raises(AssertionError, match="ray without"):
        mesh.distance((dv, df), (ds, df), samples=64, signed=True)


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def test_the_command_line_reports_what_the_api_does(tmp_path):
    import tensoir_amd
    from tensoir_amd import mesh, metrics
    m = tensoir_amd.model_from_checkpoint(CR.blob_checkpoint(), "cuda:0", envmap_h=4, envmap_w=8)
    out, cli, ckpt = (str(tmp_path / n) for n in ("api.ply", "cli.ply", "blobs.th"))
    mesh.export_mesh(m, out, attributes=True, keep_largest=1, simplify=2)
    full = mesh.extract_mesh(m, keep_largest=1)[:2]
    check = metrics.chamfer(out, full, samples=5000, thresholds=(0.001, 10.0), signed=True, normals=True)
    assert check["fscore"][1]["fscore"] == 1.0 and "signed_mean" in check["a_to_b"] and "normal_consistency" in check["b_to_a"]
    m.save(ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tensoir_amd.bake", ckpt, cli, "--simplify", "2", "--keep-largest", "1", "--envmap", "4", "8",
                        "--check-distance", "5000", "--check-fscore", "0.001", "10", "--check-signed", "--check-normals"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(cli, "rb").read() == open(out, "rb").read()
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert next(x for x in lines if "check_distance" in x)["check_distance"] == json.loads(json.dumps(check))
