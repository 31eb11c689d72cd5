"""Surface distance on the GPU (tir_mesh_sample*, tir_face_grid_*, tir_point_mesh_distance; ops.sample_surface / face_grid /
point_mesh_distance; mesh.distance, extract_mesh's simplify_tolerance / measure_simplify, the bake command line) against the numpy
restatement (tests/distance_reference.py).

Comparison rules.  The face of a sample, the integer sums behind it and the degenerate rule are discrete and must be equal.
Distances and sample positions must agree with the float64 restatement within TEN TIMES the largest deviation of the restatement
run wholly in float32 from its float64 self on the same case (tests/test_distance_cpu.py::test_float32_deviation_of_the_restatement
measures and prints them, and asserts that TOLERANCE below is ten times what it measures):
    single triangle  dist 4.98e-8 -> 4.98e-7         triangle soup            dist 7.22e-7 -> 7.22e-6
    sphere           dist 6.24e-8 -> 6.24e-7         sphere sample positions  1.21e-5 -> 1.21e-4
The kernel finds the closest point in fp64, so it sits far inside them.  For `face` the rule is d64(point, face_device) <= d64_min +
tolerance: either side of a tie passes and nothing is excluded.  Across grids and across runs dist, face and closest must be
equal bit for bit.
mesh.distance of the sphere to itself scaled by 1.01: a_to_b.mean within 2 % of 0.01 R = 0.403; the float64 restatement's own
figure over the 500 checked samples is 0.40293 (0.02 % below: the facets lie inside the sphere), inside the margin.
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE = {"triangle": 4.98e-7, "soup": 7.22e-6, "sphere": 6.24e-7, "sphere_points": 1.21e-4}


def dev(a, dtype=None):
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a).cuda()


def mesh_on_device(v, f):
    return dev(v, np.float32).reshape(-1, 3), dev(f, np.int32).reshape(-1, 3)


def query(points, v, f, grid=None, **kw):
    from tensoir_amd import ops
    dv, df = mesh_on_device(v, f)
    out = ops.point_mesh_distance(dev(points, np.float32).reshape(-1, 3), dv, df, grid, closest=True, **kw)
    torch.cuda.synchronize()
    assert [t.dtype for t in out[:3]] == [torch.float32, torch.int32, torch.float32] and all(t.is_cuda for t in out)
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_same_bits(a, b, what=""):
    assert torch.equal(bits(a[0]), bits(b[0])), what
    assert torch.equal(a[1], b[1]), what
    assert torch.equal(bits(a[2]), bits(b[2])), what


def assert_equals_restatement(got, points, v, f, tol, what, ref=None):
    dist, face, closest = (t.cpu().numpy() for t in got[:3])
    rd, rf, rc = D.point_mesh(points, v, f) if ref is None else ref
    err = np.abs(dist.astype(np.float64) - rd)
    print(f"\n[distance {what}] {len(dist)} points: max |dist - restatement| {err.max():.3e} (tolerance {tol:.3e})")
    assert err.max() <= tol, what
    assert (face >= 0).all() and (face < len(f)).all()
    assert (D.distance_to_face(points, v, f, face) <= rd + tol).all(), what
    # the closest point lies on the face (to fp32 rounding of the coordinates) at the reported distance
    assert np.abs(np.linalg.norm(closest.astype(np.float64) - np.asarray(points, np.float64), axis=1) - rd).max() <= \
        tol + 4 * np.finfo(np.float32).eps * np.abs(closest).max(), what


# ---- single triangle ------------------------------------------------------------------------------------------------------------------
def test_single_triangle_regions_and_zero_distances():
    pts, want = D.region_points()
    allp = np.concatenate([pts, D.zero_points()])
    got = query(allp, D.TRIANGLE, [[0, 1, 2]])
    assert_equals_restatement(got, allp, D.TRIANGLE, np.int32([[0, 1, 2]]), TOLERANCE["triangle"], "single triangle")
    d = got[0].cpu().numpy()
    assert np.abs(d[:7] - want).max() <= TOLERANCE["triangle"] and not np.isnan(d).any()
    assert (d[7:] <= TOLERANCE["triangle"]).all() and (got[1] == 0).all()
    for order in ([1, 2, 0], [2, 0, 1], [0, 2, 1]):
        assert_equals_restatement(query(allp, D.TRIANGLE, [order]), allp, D.TRIANGLE, np.int32([order]), TOLERANCE["triangle"],
                                  f"single triangle {order}")


def test_degenerate_mesh_nan_point_and_empty_inputs():
    from tensoir_amd import ops
    verts = np.float32([[1, 1, 1], [2, 2, 2], [3, 3, 3], [0, 0, 0], [1, 0, 0], [0, 1, 0]])
    p = np.float32([[0.25, 0.25, 2.0], [np.nan, 0, 0], [0, np.inf, 0]])
    for faces in ([[0, 1, 2]], [[4, 4, 4]], [[0, 1, 2], [4, 4, 4]]):
        g = ops.face_grid(*mesh_on_device(verts, faces))
        assert g["degenerate"] == len(faces) and g["listed"] == 0 and g["n_pairs"] == 0
        d, f, c = (t.cpu().numpy() for t in query(p, verts, faces, g))
        assert d[0] == np.inf and np.isnan(d[1:]).all() and list(f) == [-1, -1, -1] and np.isnan(c).all()
    # a proper face among them: found, the others counted; a NaN point stays NaN
    faces = [[0, 1, 2], [3, 4, 5], [4, 4, 4]]
    g = ops.face_grid(*mesh_on_device(verts, faces))
    assert (g["degenerate"], g["listed"]) == (2, 1)
    d, f, c = (t.cpu().numpy() for t in query(p, verts, faces, g))
    assert d[0] == 2.0 and f[0] == 1 and np.isnan(d[1:]).all() and list(f[1:]) == [-1, -1]
    # a face with a non-finite corner is listed nowhere
    bad = verts.copy()
    bad[5, 1] = np.nan
    g = ops.face_grid(*mesh_on_device(bad, [[3, 4, 5]]))
    assert (g["degenerate"], g["listed"]) == (1, 0)
    # no points, no faces
    dv, df = mesh_on_device(verts, faces)
    out = ops.point_mesh_distance(torch.zeros((0, 3), device="cuda"), dv, df)
    assert out[0].shape == (0,) and out[1].shape == (0,)
    d, f = ops.point_mesh_distance(dev(p), dv, torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    assert d[0].item() == np.inf and f[0].item() == -1
    pts, fc = ops.sample_surface(dv, df, 0)
    assert pts.shape == (0, 3) and fc.shape == (0,)
    with pytest.raises(ValueError):
        ops.sample_surface(dv, torch.zeros((0, 3), dtype=torch.int32, device="cuda"), 5)
    from tensoir_amd._lib import TensoirHipError
    with pytest.raises(TensoirHipError, match="degenerate"):
        ops.sample_surface(dv, dev(np.int32([[0, 1, 2], [4, 4, 4]])), 5)


# ---- triangle soup ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soup_reference():
    v, f, p = D.soup()
    return D.point_mesh(p, v, f)


def test_soup_equals_restatement_and_is_bit_identical_across_grids(soup_reference):
    from tensoir_amd import ops
    v, f, p = D.soup()
    dv, df = mesh_on_device(v, f)
    budget = 1 << 24
    grids = {n: ops.face_grid(dv, df, max_pairs=budget, dims=[n] * 3) for n in (1, 4, 16, 64)}
    grids["anisotropic"] = ops.face_grid(dv, df, max_pairs=budget, dims=[3, 50, 11])
    grids["inside"] = ops.face_grid(dv, df, cell=[0.05, 0.07, 0.11], origin=[0.3, 0.2, 0.4], dims=[5, 6, 2])    # faces beyond it
    grids["default"] = ops.face_grid(dv, df)
    assert grids[1]["dims"] == [1, 1, 1] and grids[1]["n_pairs"] == 300 and grids[64]["dims"] == [64, 64, 64]
    assert all(g["listed"] == 300 and g["degenerate"] == 0 for g in grids.values())
    base = query(p, v, f, grids[1], tested=True)
    assert (base[3] == 300).all()                                       # the brute-force path tests every face
    assert_equals_restatement(base, p, v, f, TOLERANCE["soup"], "soup 1^3", soup_reference)
    for name, g in grids.items():
        got = query(p, v, f, g, tested=True)
        assert_same_bits(got, base, name)
        assert_same_bits(query(p, v, f, g), base, f"{name}, second run")
        print(f"[distance soup {name}] dims {g['dims']} pairs {g['n_pairs']}: {got[3].float().mean().item():.1f} faces tested per point")
    # a rebuilt grid (another fill order, perhaps) gives the same bits
    assert_same_bits(query(p, v, f, ops.face_grid(dv, df, max_pairs=budget, dims=[16] * 3)), base, "rebuilt")


# ---- sphere -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_device():
    from tensoir_amd import ops
    v, f, scaled = D.sphere_pair()
    dv, df = mesh_on_device(v, f)
    pts, face = ops.sample_surface(dv, df, D.SPHERE_SAMPLES, 0)
    torch.cuda.synchronize()
    return dv, df, dev(scaled), pts, face


def test_sphere_samples_equal_restatement(sphere_device):
    from tensoir_amd import ops
    dv, df, _, pts, face = sphere_device
    v, f, _ = D.sphere_pair()
    assert len(f) == 61236
    rp, rf = D.sphere_samples(np.float64)
    assert np.array_equal(face.cpu().numpy(), rf)
    err = np.abs(pts.cpu().numpy().astype(np.float64) - rp).max()
    print(f"\n[distance sphere samples] max |point - restatement| {err:.3e} (tolerance {TOLERANCE['sphere_points']:.3e})")
    assert err <= TOLERANCE["sphere_points"]
    q, _, total = D.integer_cdf(v, f)
    count = np.bincount(face.cpu().numpy(), minlength=len(f))
    assert (np.abs(count - D.SPHERE_SAMPLES * (q / float(total))) < 2).all() and (count[q == 0] == 0).all()
    again = ops.sample_surface(dv, df, D.SPHERE_SAMPLES, 0)
    assert torch.equal(bits(again[0]), bits(pts)) and torch.equal(again[1], face)
    other = ops.sample_surface(dv, df, D.SPHERE_SAMPLES, 1)
    assert not torch.equal(bits(other[0]), bits(pts))
    assert np.array_equal(other[1].cpu().numpy(), D.sample(v, f, D.SPHERE_SAMPLES, 1)[1])
    odd = ops.sample_surface(dv, df, 4097, 2 ** 64 - 1)                 # another n, the largest seed, more than one block
    assert np.array_equal(odd[1].cpu().numpy(), D.sample(v, f, 4097, 2 ** 64 - 1)[1])


def test_sphere_distances_equal_brute_force_and_restatement(sphere_device):
    from tensoir_amd import ops
    dv, df, ds, pts, _ = sphere_device
    _, f, scaled = D.sphere_pair()
    grid = ops.face_grid(ds, df)
    assert max(grid["dims"]) > 8 and grid["n_pairs"] <= max(16 * len(f), 1 << 20)
    got = ops.point_mesh_distance(pts, ds, df, grid, closest=True, tested=True)
    brute = ops.point_mesh_distance(pts, ds, df, ops.face_grid(ds, df, dims=[1, 1, 1]), closest=True)
    torch.cuda.synchronize()
    assert_same_bits(got, brute, "default grid against 1^3")
    print(f"\n[distance sphere] dims {grid['dims']} pairs {grid['n_pairs']}: {got[3].float().mean().item():.1f} faces tested per point")
    idx = D.sphere_checked()
    sub = tuple(t[torch.from_numpy(idx).cuda()] for t in got[:3])
    assert_equals_restatement(sub, pts.cpu().numpy()[idx], scaled, f, TOLERANCE["sphere"], "sphere", D.sphere_distances(np.float64))


def test_mesh_distance_of_a_scaled_sphere(sphere_device):
    from tensoir_amd import mesh, metrics
    dv, df, ds, _, _ = sphere_device
    want = 0.01 * D.SPHERE_RADIUS
    own = D.sphere_distances(np.float64)[0].mean()
    assert abs(own - want) <= 0.02 * want                               # the restatement's own figure is inside the margin
    r = mesh.distance((dv, df), (ds, df), samples=D.SPHERE_SAMPLES)
    print(f"\n[distance sphere] a_to_b {r['a_to_b']}, b_to_a {r['b_to_a']}; restatement mean over the checked samples {own:.5f}")
    assert abs(r["a_to_b"]["mean"] - want) <= 0.02 * want and r["a_to_b"]["n"] == D.SPHERE_SAMPLES
    assert abs(r["b_to_a"]["mean"] - want) <= 0.02 * want
    assert r["chamfer"] == r["a_to_b"]["mean"] + r["b_to_a"]["mean"] and r["hausdorff"] == max(r["a_to_b"]["max"], r["b_to_a"]["max"])
    for d in (r["a_to_b"], r["b_to_a"]):
        assert d["mean"] <= d["rms"] <= d["p95"] * 1.5 and d["p95"] <= d["max"] < 0.02 * D.SPHERE_RADIUS
    assert mesh.distance((dv, df), (ds, df), samples=D.SPHERE_SAMPLES) == r                  # every figure, bit for bit
    same = mesh.distance((dv, df), (dv, df), samples=4096)
    assert same["hausdorff"] <= TOLERANCE["sphere_points"] and same["chamfer"] <= same["hausdorff"] * 2      # samples are fp32 points
    assert metrics.chamfer((dv.cpu().numpy(), df.cpu().numpy()), (ds, df), samples=D.SPHERE_SAMPLES) == r


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_refused_not_followed_and_nothing_is_truncated():
    from tensoir_amd import ops
    from tensoir_amd._lib import TensoirHipError
    v = np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]])
    p = dev(np.float32([[0, 0, 0]]))
    for faces, verts in (([[0, 1, 2], [0, 1, 3]], v), ([[0, -1, 2]], v), ([[0, 0, 0]], np.zeros((0, 3), np.float32))):
        dv, df = mesh_on_device(verts, faces)
        with pytest.raises(TensoirHipError, match="face index"):
            ops.sample_surface(dv, df, 16)
        with pytest.raises(TensoirHipError, match="face index"):
            ops.face_grid(dv, df)
        with pytest.raises(TensoirHipError, match="face index"):
            ops.point_mesh_distance(p, dv, df)
    sv, sf, _ = D.soup()
    dv, df = mesh_on_device(sv, sf)
    true_total = ops.face_grid(dv, df, max_pairs=1 << 24, dims=[16] * 3)["n_pairs"]
    assert true_total > 300
    with pytest.raises(TensoirHipError, match=f"pairs.*{true_total}|{true_total}.*pairs"):
        ops.face_grid(dv, df, max_pairs=true_total - 1, dims=[16] * 3)
    assert ops.face_grid(dv, df, max_pairs=true_total, dims=[16] * 3)["n_pairs"] == true_total
    with pytest.raises(TensoirHipError, match="pairs"):
        ops.face_grid(dv, df, max_pairs=299)                            # not even 1 x 1 x 1 fits: refused, not truncated
    g = ops.face_grid(dv, df, max_pairs=300)                            # the chosen cell grows until the pairs fit
    assert g["n_pairs"] <= 300 and g["dims"] == [1, 1, 1]
    for cell in (0.0, -1.0, float("nan"), [0.1, 0.0, 0.1]):
        with pytest.raises(TensoirHipError):
            ops.face_grid(dv, df, cell=cell)
    with pytest.raises(TensoirHipError):
        ops.face_grid(dv, df, dims=[257, 1, 1])
    with pytest.raises(TensoirHipError):
        ops.face_grid(dv, df, cell=1e-3)                                # 1001 cells per axis: above the limit of 256
    with pytest.raises(TensoirHipError):
        ops.face_grid(dv, df, dims=[0, 1, 1])
    with pytest.raises(ValueError, match="grid"):
        ops.point_mesh_distance(p, *mesh_on_device(v, [[0, 1, 2]]), grid=ops.face_grid(dv, df))
    with pytest.raises(Exception):
        ops.point_mesh_distance(p.cpu(), dv, df)


# ---- the blob scene -----------------------------------------------------------------------------------------------------------------------
def blob_model():
    import tensoir_amd
    return tensoir_amd.model_from_checkpoint(CR.blob_checkpoint(), "cuda:0", envmap_h=4, envmap_w=8)


@pytest.fixture(scope="module")
def blobs():
    model = blob_model()
    model.march_t_stop = 0.0
    return model


@pytest.fixture(scope="module")
def blob_errors(blobs):
    """mesh.distance(simplified k, full) for k = 2 .. 8, as a loop over simplify=k measures it."""
    from tensoir_amd import mesh
    full = mesh.extract_mesh(blobs)[:2]
    out = {}
    for k in range(2, 9):
        v, f, _ = mesh.extract_mesh(blobs, simplify=k)
        out[k] = mesh.distance((v, f), full)
    return out


@pytest.mark.parametrize("k", [2, 3])
def test_vertex_clustering_moves_the_surface_by_at_most_a_cluster_diagonal(blobs, blob_errors, k):
    from tensoir_amd import mesh
    r = {}
    v, f, n = mesh.extract_mesh(blobs, simplify=k, measure_simplify=True, report=r)
    plain = mesh.extract_mesh(blobs, simplify=k)
    assert all(torch.equal(a, b) for a, b in zip((v, f, n), plain))    # measuring changes nothing
    sp = np.float64(mesh.reference_spacing(blobs.aabb.detach().cpu().float(), CR.BLOB_GRID))
    err = r["simplify_error"]
    print(f"\n[distance blobs k={k}] a_to_b {err['a_to_b']} hausdorff {err['hausdorff']:.5f}; cluster diagonal {np.linalg.norm(k * sp):.5f}")
    assert 0 < err["a_to_b"]["max"] <= np.linalg.norm(k * sp) * (1 + 1e-4)
    assert err["cell"] == min(mesh.reference_spacing(blobs.aabb.detach().cpu().float(), CR.BLOB_GRID))
    assert {x: err[x] for x in ("a_to_b", "b_to_a", "chamfer", "hausdorff")} == blob_errors[k]


def test_simplify_tolerance_takes_what_a_loop_over_k_would(blobs, blob_errors):
    from tensoir_amd import mesh
    cell = min(mesh.reference_spacing(blobs.aabb.detach().cpu().float(), CR.BLOB_GRID))
    cells = {k: e["hausdorff"] / cell for k, e in blob_errors.items()}
    print("\n[distance blobs] hausdorff in cells per k:", {k: round(c, 4) for k, c in cells.items()})
    full = mesh.extract_mesh(blobs)
    upper = next((k for k in range(3, 9) if cells[k] > cells[k - 1] and all(cells[j] <= cells[k - 1] for j in range(2, k))), None)
    assert upper is not None, cells                                     # two measured errors to aim between
    for t in (cells[2] * 0.5, (cells[upper - 1] + cells[upper]) / 2, max(cells.values()) * 1.5):
        want, tried = mesh.choose_simplify(lambda k: cells[k], range(2, 9), t)
        r = {}
        got = mesh.extract_mesh(blobs, simplify_tolerance=t, report=r)
        assert r["simplify"] == want and sorted(r["simplify_error"]) == sorted(tried)
        assert all({x: r["simplify_error"][k][x] for x in blob_errors[k]} == blob_errors[k] for k in tried)
        ref = full if want is None else mesh.extract_mesh(blobs, simplify=want)
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), t
        assert r["full"] == (full[0].shape[0], full[1].shape[0])
    assert mesh.choose_simplify(lambda k: cells[k], range(2, 9), cells[2] * 0.5)[0] is None
    assert mesh.choose_simplify(lambda k: cells[k], range(2, 9), max(cells.values()) * 1.5)[0] == 8
    r = {}
    mesh.extract_mesh(blobs, simplify_tolerance=max(cells.values()) * 1.5, simplify_max=4, report=r)
    assert r["simplify"] == 4 and sorted(r["simplify_error"]) == [2, 3, 4]


def test_no_new_option_runs_no_new_kernel_and_writes_the_same_bytes(blobs, tmp_path, monkeypatch):
    from tensoir_amd import mesh, ops

    def refuse(*a, **k):
        raise AssertionError("a distance call without the option")
    for name in ("point_mesh_distance", "face_grid", "sample_surface"):
        monkeypatch.setattr(ops, name, refuse)
    a, b, c = (str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply"))
    na = mesh.export_mesh(blobs, a)
    v, f, _ = mesh.extract_mesh(blobs)
    mesh.write_ply(b, v, f)                              # the export as it was before the options existed
    assert na == (v.shape[0], f.shape[0]) and open(a, "rb").read() == open(b, "rb").read()
    mesh.export_mesh(blobs, a, simplify=2)
    v, f, _ = mesh.extract_mesh(blobs, simplify=2, simplify_tolerance=None, measure_simplify=False)
    mesh.write_ply(c, v, f)
    assert open(a, "rb").read() == open(c, "rb").read()
    with pytest.raises(AssertionError, match="distance call"):
        mesh.extract_mesh(blobs, simplify=2, measure_simplify=True)


def test_the_command_line_agrees_with_the_api(tmp_path, blob_errors):
    from tensoir_amd import mesh, metrics
    m = blob_model()
    cell = min(mesh.reference_spacing(m.aabb.detach().cpu().float(), CR.BLOB_GRID))
    t = 0.5 * (blob_errors[2]["hausdorff"] + blob_errors[3]["hausdorff"]) / cell if blob_errors[3]["hausdorff"] > blob_errors[2]["hausdorff"] \
        else 1.01 * blob_errors[2]["hausdorff"] / cell
    out, cli, ckpt = (str(tmp_path / n) for n in ("api.ply", "cli.ply", "blobs.th"))
    report = {}
    nv, nf = mesh.export_mesh(m, out, attributes=True, keep_largest=1, simplify_tolerance=t, simplify_max=4, report=report)
    full = mesh.extract_mesh(m, keep_largest=1)[:2]
    check = metrics.chamfer(out, full, samples=5000)
    m.save(ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tensoir_amd.bake", ckpt, cli, "--simplify-tolerance", repr(t), "--simplify-max", "4",
                        "--check-distance", "5000", "--keep-largest", "1", "--envmap", "4", "8"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(cli, "rb").read() == open(out, "rb").read()
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    said = next(x for x in lines if "simplify_error" in x)
    assert said["simplify"] == report["simplify"]
    assert said["simplify_error"] == json.loads(json.dumps({str(k): v for k, v in report["simplify_error"].items()}))
    assert next(x for x in lines if "check_distance" in x)["check_distance"] == json.loads(json.dumps(check))
    assert f"simplify {report['simplify']}: " in r.stdout and f"{nv} vertices, {nf} faces" in r.stdout
