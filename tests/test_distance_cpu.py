"""Surface distance without a GPU: the numpy restatement (tests/distance_reference.py) against closed forms and against the
properties the contract of include/tensoir_hip.h promises, mesh.distance_summary / mesh.choose_simplify, the option checks, and
the float32 deviation of the restatement that the tolerances of tests/test_gpu_distance.py are ten times of."""
import numpy as np
import pytest
import torch

from tests import distance_reference as D
from tests import simplify_reference as S


# ---- point to triangle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_seven_regions_in_closed_form(dtype):
    pts, want = D.region_points()
    a, b, c = (D.TRIANGLE[k].astype(dtype) for k in range(3))
    d2, closest, region = D.closest_on_triangle(pts.astype(dtype), a, b, c)
    assert list(region) == list(range(7)), [D.REGIONS[r] for r in region]
    np.testing.assert_allclose(np.sqrt(d2), want, rtol=4 * np.finfo(dtype).eps)
    dist, face, cl = D.point_mesh(pts, D.TRIANGLE, [[0, 1, 2]], dtype)
    np.testing.assert_allclose(dist, want, rtol=4 * np.finfo(dtype).eps)
    assert (face == 0).all() and np.allclose(cl, closest)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_points_in_the_plane_on_an_edge_and_on_a_corner(dtype):
    dist, face, cl = D.point_mesh(D.zero_points(), D.TRIANGLE, [[0, 1, 2]], dtype)
    assert np.isfinite(dist).all() and np.isfinite(cl).all() and (face == 0).all()
    assert (dist <= 4 * np.finfo(dtype).eps * 3).all(), dist
    # the same with the corners in another order (every corner plays every role)
    for order in ([1, 2, 0], [2, 0, 1], [0, 2, 1]):
        dist, _, _ = D.point_mesh(D.zero_points(), D.TRIANGLE, [order], dtype)
        assert np.isfinite(dist).all() and (dist <= 4 * np.finfo(dtype).eps * 3).all(), (order, dist)


def test_degenerate_and_non_finite_faces_are_ignored_and_counted():
    verts = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0],                   # a proper face
                        [1, 1, 1], [2, 2, 2], [3, 3, 3],                   # collinear
                        [5, 5, 5], [np.nan, 0, 0], [0, np.inf, 0]])
    faces = np.int32([[3, 4, 5], [0, 1, 2], [6, 6, 6], [0, 1, 7], [0, 8, 2]])
    keep, bad = D.listed_faces(verts, faces)
    assert list(keep) == [1] and bad == 4
    dist, face, _ = D.point_mesh(np.float32([[0.25, 0.25, 2.0], [3, 3, 3]]), verts, faces)
    assert list(face) == [1, 1] and dist[0] == 2.0
    # nothing but degenerate faces: +inf / -1; a non-finite point: NaN / -1
    dist, face, cl = D.point_mesh(np.float32([[0, 0, 0], [np.nan, 0, 0]]), verts, faces[[0, 2]])
    assert dist[0] == np.inf and np.isnan(dist[1]) and list(face) == [-1, -1] and np.isnan(cl).all()
    with pytest.raises(ValueError, match="face index"):
        D.listed_faces(verts, [[0, 1, 9]])
    # ... and they have no weight
    q, cdf, total = D.integer_cdf(verts, faces)
    assert list(q > 0) == [False, True, False, False, False] and total == q[1] == cdf[-1]


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------
def _box_with_zero_faces():
    v, f = S.case("box")[:2]
    f = np.concatenate([f[:100], [[0, 0, 0], [5, 5, 9]], f[100:], [[7, 7, 7]]]).astype(np.int32)
    return np.asarray(v, np.float32), f


@pytest.mark.parametrize("n", [1, 257, 5000, 40001])
def test_stratified_samples_follow_the_weight_share(n):
    v, f = _box_with_zero_faces()
    q, cdf, total = D.integer_cdf(v, f)
    assert total < 2 ** 53 and (q >= 0).all() and q.max() == 2 ** 52 // 2 ** int(np.ceil(np.log2(len(f))))
    assert q[100] == 0 and q[101] == 0 and q[-1] == 0
    pts, face = D.sample(v, f, n, seed=3)
    count = np.bincount(face, minlength=len(f))
    share = q.astype(np.float64) / float(total)
    assert (np.abs(count - n * share) < 2).all(), np.abs(count - n * share).max()
    assert (count[q == 0] == 0).all()
    assert (np.diff(face) >= 0).all()                                   # stratified positions ascend: samples come in face order
    # every point lies in its face's plane and inside it (barycentric coordinates of the restatement are a convex combination)
    tri = v[f[face]].astype(np.float64)
    d2, _, _ = D.closest_on_triangle(pts, tri[:, 0], tri[:, 1], tri[:, 2])
    assert np.sqrt(d2).max() < 1e-12


def test_the_integer_weights_follow_the_areas():
    v, f = _box_with_zero_faces()
    q, _, total = D.integer_cdf(v, f)
    area = np.sqrt(D.cross2(v, f))
    np.testing.assert_allclose(q / float(total), area / area.sum(), atol=2.0 ** -40)


def test_samples_are_reproducible_and_seeded():
    v, f = _box_with_zero_faces()
    p0, f0 = D.sample(v, f, 3000, seed=11)
    p1, f1 = D.sample(v, f, 3000, seed=11)
    p2, f2 = D.sample(v, f, 3000, seed=12)
    assert np.array_equal(p0, p1) and np.array_equal(f0, f1)
    assert not np.array_equal(p0, p2)
    # the hash: spot values of the written-out definition (python integers), and its 24-bit range
    def h(seed, i, ch):
        m = (1 << 64) - 1
        x = (seed + 0x9E3779B97F4A7C15 * (3 * i + ch + 1)) & m
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & m
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & m
        x ^= x >> 31
        return x >> 40
    for seed, i, ch in ((0, 0, 0), (11, 2999, 2), (2 ** 64 - 1, 123456789, 1)):
        assert int(D.hash24(seed, np.array([i]), ch)[0]) == h(seed, i, ch) < 2 ** 24
    u = D.hash24(5, np.arange(100000), 0).astype(np.float64) * 2.0 ** -24
    assert abs(u.mean() - 0.5) < 0.01 and u.min() >= 0 and u.max() < 1


# ---- the summary and the search policy ------------------------------------------------------------------------------------------------
def test_distance_summary_on_hand_made_tensors():
    from tensoir_amd import mesh
    dv = torch.tensor([0.5, 7.0, 0.25])
    ds = torch.tensor([1.0, 2.0, 3.0, 4.0, 10.0])
    s = mesh.distance_summary(dv, ds)
    assert s["n"] == 5 and s["mean"] == 4.0 and s["max"] == 10.0
    assert s["rms"] == pytest.approx(np.sqrt(130 / 5), rel=1e-15) and s["p95"] == pytest.approx(8.8, rel=1e-15)
    assert mesh.distance_summary(torch.tensor([11.0]), ds)["max"] == 11.0          # max sees the vertices, the mean does not
    assert mesh.distance_summary(torch.tensor([11.0]), ds)["mean"] == 4.0
    want = D.summary(dv.numpy(), ds.numpy())
    assert all(s[k] == pytest.approx(want[k], rel=1e-15) for k in want)
    # float64 sums: 2^24 + 1 float32 ones keep their count
    big = mesh.distance_summary(torch.zeros(0), torch.ones(2 ** 24 + 1, dtype=torch.float32))
    assert big["mean"] == 1.0 and big["rms"] == 1.0 and big["n"] == 2 ** 24 + 1
    empty = mesh.distance_summary(torch.tensor([2.0]), torch.zeros(0))
    assert empty["n"] == 0 and empty["max"] == 2.0 and all(np.isnan(empty[k]) for k in ("mean", "rms", "p95"))
    assert mesh.distance_summary(torch.tensor([float("inf")]), ds)["max"] == float("inf")


def test_choose_simplify_policy():
    from tensoir_amd import mesh
    calls = []

    def fake(table):
        def measure(k):
            calls.append(k)
            return table[k]
        return measure

    mono = {2: 0.2, 3: 0.4, 4: 0.7, 5: 1.1, 6: 1.6}
    assert mesh.choose_simplify(fake(mono), range(2, 7), 0.75) == (4, {2: 0.2, 3: 0.4, 4: 0.7, 5: 1.1})
    assert calls == [2, 3, 4, 5]                                        # stops at the first failure: 6 is never measured
    assert mesh.choose_simplify(fake(mono), range(2, 7), 0.1) == (None, {2: 0.2})
    assert mesh.choose_simplify(fake(mono), range(2, 7), 5.0) == (6, mono)
    assert mesh.choose_simplify(fake(mono), range(2, 7), 0.4)[0] == 3                # at most: equality passes
    bumpy = {2: 0.2, 3: 0.9, 4: 0.3, 5: 0.35}
    assert mesh.choose_simplify(fake(bumpy), range(2, 6), 0.5) == (2, {2: 0.2, 3: 0.9})      # a later k that would pass is not tried
    assert mesh.choose_simplify(fake({2: float("nan")}), [2], 1.0) == (None, pytest.approx({2: float("nan")}, nan_ok=True))
    assert mesh.choose_simplify(fake(mono), [], 1.0) == (None, {})


class _Untouchable:
    """A model whose every attribute raises: the option checks must come before anything reads it (or the device)."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the options were checked")


@pytest.mark.parametrize("entry", ["extract_mesh", "export_mesh", "export_textured"])
def test_option_validation_comes_before_the_device(entry, tmp_path):
    from tensoir_amd import mesh
    fn = getattr(mesh, entry)
    args = (_Untouchable(),) if entry == "extract_mesh" else (_Untouchable(), str(tmp_path / "out.bin"))
    with pytest.raises(ValueError, match="mutually exclusive"):
        fn(*args, simplify=2, simplify_tolerance=0.5)
    for bad in (-0.5, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="simplify_tolerance"):
            fn(*args, simplify_tolerance=bad)
    for bad in (1, 2.5, True):
        with pytest.raises(ValueError, match="simplify_max"):
            fn(*args, simplify_tolerance=0.5, simplify_max=bad)
    with pytest.raises(ValueError, match="measure_simplify"):
        fn(*args, measure_simplify=True)
    assert not (tmp_path / "out.bin").exists()


def test_entries_validate_on_the_host_before_any_device_work():
    """-1001 / -1002 for bad arguments and 0 for n = 0, without a GPU: the pointers are host addresses that are never followed."""
    import ctypes as C
    from tensoir_amd import _lib
    lib = _lib.lib()
    keep = torch.zeros(64, dtype=torch.float32)
    ptr = keep.data_ptr()
    f3, i3 = (C.c_float * 3), (C.c_int32 * 3)
    cell, org, dims = f3(1, 1, 1), f3(0, 0, 0), i3(2, 2, 2)
    assert lib.tir_distance_blocks(0) == 0 and lib.tir_distance_blocks(4097) == 2 and lib.tir_distance_blocks(-1) == -1001
    # samples
    assert lib.tir_mesh_sample_cdf(ptr, 3, ptr, 0, None, None, ptr, None) == 0
    assert lib.tir_mesh_sample_cdf(ptr, 3, ptr, 1, None, ptr, ptr, None) == -1001
    assert lib.tir_mesh_sample_cdf(ptr, 3, ptr, 1, ptr, ptr, None, None) == -1001
    assert lib.tir_mesh_sample_cdf(ptr, 3, ptr, -1, ptr, ptr, ptr, None) == -1001
    assert lib.tir_mesh_sample_cdf(ptr, 3, ptr, 2 ** 28 + 1, ptr, ptr, ptr, None) == -1002
    assert lib.tir_mesh_sample_cdf(ptr, 2 ** 31, ptr, 1, ptr, ptr, ptr, None) == -1002
    assert lib.tir_mesh_sample(ptr, 3, ptr, 1, ptr, 0, 0, None, None, None) == 0
    assert lib.tir_mesh_sample(ptr, 3, ptr, 1, ptr, 8, 0, None, ptr, None) == -1001
    assert lib.tir_mesh_sample(ptr, 3, ptr, 0, ptr, 8, 0, ptr, ptr, None) == -1001         # nothing to sample
    assert lib.tir_mesh_sample(ptr, 3, ptr, 1, ptr, -1, 0, ptr, ptr, None) == -1001
    assert lib.tir_mesh_sample(ptr, 3, ptr, 1, ptr, 2 ** 31, 0, ptr, ptr, None) == -1002
    # grid
    assert lib.tir_face_grid_count(ptr, 3, ptr, 0, cell, org, dims, ptr, None) == 0
    assert lib.tir_face_grid_count(ptr, 3, ptr, 1, cell, org, dims, None, None) == -1001
    assert lib.tir_face_grid_count(ptr, 3, None, 1, cell, org, dims, ptr, None) == -1001
    assert lib.tir_face_grid_count(ptr, 3, ptr, 1, None, org, dims, ptr, None) == -1001
    for bad in (f3(1, 0, 1), f3(1, -1, 1), f3(float("nan"), 1, 1), f3(float("inf"), 1, 1)):
        assert lib.tir_face_grid_count(ptr, 3, ptr, 1, bad, org, dims, ptr, None) == -1001
    assert lib.tir_face_grid_count(ptr, 3, ptr, 1, cell, f3(0, float("nan"), 0), dims, ptr, None) == -1001
    assert lib.tir_face_grid_count(ptr, 3, ptr, 1, cell, org, i3(2, 0, 2), ptr, None) == -1001
    assert lib.tir_face_grid_count(ptr, 3, ptr, 1, cell, org, i3(257, 1, 1), ptr, None) == -1002
    assert lib.tir_face_grid_count(ptr, 3, ptr, 1, cell, org, i3(256, 256, 256), None, None) == -1001      # the limit itself passes
    assert lib.tir_face_grid_fill(ptr, 3, ptr, 1, cell, org, dims, 0, ptr, ptr, ptr, None, None) == 0
    assert lib.tir_face_grid_fill(ptr, 3, ptr, 1, cell, org, dims, 4, ptr, ptr, ptr, None, None) == -1001
    assert lib.tir_face_grid_fill(ptr, 3, ptr, 1, cell, org, dims, 4, None, ptr, ptr, ptr, None) == -1001
    assert lib.tir_face_grid_fill(ptr, 3, ptr, 1, cell, org, dims, -1, ptr, ptr, ptr, ptr, None) == -1001
    assert lib.tir_face_grid_fill(ptr, 3, ptr, 1, cell, org, dims, 2 ** 31, ptr, ptr, ptr, ptr, None) == -1002
    assert lib.tir_face_grid_fill(ptr, 3, ptr, 1, cell, org, i3(1, 300, 1), 4, ptr, ptr, ptr, ptr, None) == -1002
    # query
    q = lambda n, **kw: lib.tir_point_mesh_distance(kw.get("points", ptr), n, ptr, 3, ptr, 1, kw.get("cell", cell), org, kw.get("dims", dims),
                                                    kw.get("cursor", ptr), ptr, kw.get("pairs", 4), kw.get("dist", ptr), ptr, None, None, None)
    assert q(0) == 0 and q(0, points=None, dist=None) == 0
    assert q(8, points=None) == -1001 and q(8, cursor=None) == -1001 and q(8, dist=None) == -1001 and q(-1) == -1001
    assert q(8, cell=f3(0, 1, 1)) == -1001 and q(8, pairs=-1) == -1001
    assert q(8, dims=i3(1, 1, 1000)) == -1002 and q(2 ** 31) == -1002 and q(8, pairs=2 ** 31) == -1002


# ---- the tolerances of the GPU tests ------------------------------------------------------------------------------------------------------
def test_float32_deviation_of_the_restatement(capsys):
    """Prints the largest deviation of the float32 restatement from the float64 one over the cases of tests/test_gpu_distance.py;
    the tolerances there are ten times these values (its docstring quotes them).  Asserted here: that those quoted tolerances
    are indeed ten times what this machine measures, to the two digits quoted."""
    from tests import test_gpu_distance as G
    dev = {}
    pts, _ = D.region_points()
    allp = np.concatenate([pts, D.zero_points()])
    d64, d32 = (D.point_mesh(allp, D.TRIANGLE, [[0, 1, 2]], t)[0] for t in (np.float64, np.float32))
    dev["triangle"] = np.abs(d32 - d64).max()
    v, f, p = D.soup()
    d64, d32 = (D.point_mesh(p, v, f, t)[0] for t in (np.float64, np.float32))
    dev["soup"] = np.abs(d32 - d64).max()
    dev["sphere"] = np.abs(D.sphere_distances(np.float32)[0] - D.sphere_distances(np.float64)[0]).max()
    dev["sphere_points"] = np.abs(D.sphere_samples(np.float32)[0].astype(np.float64) - D.sphere_samples(np.float64)[0]).max()
    with capsys.disabled():
        print("\nfloat32 restatement - float64 restatement, max abs:", {k: float(f"{x:.3g}") for k, x in dev.items()})
    for k, x in dev.items():
        assert G.TOLERANCE[k] == pytest.approx(10 * x, rel=0.01), (k, x, G.TOLERANCE[k])
