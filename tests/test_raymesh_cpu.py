"""What the ray-mesh query needs no GPU for: the numpy restatement (tests/raymesh_reference.py) against closed forms and against
itself (the grid walk against brute force), mesh.topology and the summaries of mesh.distance's new options on hand-made tensors,
option validation, and tir_ray_mesh's host validation through the built library."""
import numpy as np
import pytest
import torch

from tests import distance_reference as D
from tests import raymesh_reference as R


def test_edge_function_is_bitwise_antisymmetric():
    rng = np.random.default_rng(3)
    n = 100000
    d, P, Q = rng.normal(size=(n, 3)), rng.normal(size=(n, 3)) * 10, rng.normal(size=(n, 3)) * 10
    P[: n // 4], Q[: n // 4] = P[: n // 4].astype(np.float32), Q[: n // 4].astype(np.float32)       # (differences of fp32 inputs)
    a, b = R.edge(d, P, Q), R.edge(d, Q, P)
    assert (a != 0).all() and np.array_equal(a.view(np.int64), (-b).view(np.int64))


def test_closed_form_triangle_cases_on_the_restatement():
    o, d, tr, t, face, bary, count, flags = R.triangle_rays()
    for order in ([0, 1, 2],):
        r = R.ray_mesh(o, d, D.TRIANGLE, np.int32([order]), tr)
        assert np.array_equal(r["t"], t) and np.array_equal(r["face"], face) and np.array_equal(r["count"], count)
        assert np.array_equal(r["flags"], flags) and np.array_equal(r["bary"], bary, equal_nan=True)
    # the other corner orders and the other winding: the same t, the weights permuted
    for order, perm in (([1, 2, 0], lambda b0, b1, b2: (b2, b0)), ([0, 2, 1], lambda b0, b1, b2: (b2, b1))):
        r = R.ray_mesh(o, d, D.TRIANGLE, np.int32([order]), tr)
        assert np.array_equal(r["t"], t) and np.array_equal(r["flags"], flags)
        b0 = 1.0 - bary[:, 0] - bary[:, 1]
        want = np.stack(perm(b0, bary[:, 0], bary[:, 1]), 1)
        assert np.array_equal(r["bary"], want, equal_nan=True)


def test_invalid_rays_and_degenerate_faces_on_the_restatement():
    verts = np.float32([[1, 1, 1], [2, 2, 2], [3, 3, 3], [0, 0, 0], [1, 0, 0], [0, 1, 0]])
    o = np.float32([[0.25, 0.25, -1], [np.nan, 0, 0], [0, np.inf, 0], [0.25, 0.25, -1], [0.25, 0.25, -1], [0.25, 0.25, -1]])
    d = np.float32([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, np.nan, 1], [0, 0, 1]])
    tr = np.float32([[0, np.inf]] * 5 + [[2, 1]])
    r = R.ray_mesh(o, d, verts, [[0, 1, 2], [3, 4, 5], [4, 4, 4]], tr)
    assert r["t"][0] == 1.0 and r["face"][0] == 1 and r["count"][0] == 1 and r["flags"][0] == 0
    assert np.isnan(r["t"][1:]).all() and (r["face"][1:] == -1).all() and (r["count"][1:] == 0).all() and (r["flags"][1:] == R.INVALID).all()
    r = R.ray_mesh(o[:1], d[:1], verts, [[0, 1, 2], [4, 4, 4]])
    assert r["t"][0] == np.inf and r["face"][0] == -1 and r["count"][0] == 0


def test_cube_ties_counts_and_parity_on_the_restatement():
    v, f = R.CUBE_VERTS, R.CUBE_FACES
    # through the diagonal of the sides x = 0 and x = 1: two faces tie, the smaller index wins, both count, grazed
    r = R.ray_mesh([[-1, 0.5, 0.5]], [[1, 0, 0]], v, f)
    assert r["t"][0] == 1.0 and r["face"][0] == 0 and r["count"][0] == 4 and r["flags"][0] == R.GRAZED
    o = np.float32([[-1, 0.3, 0.6], [0.5, 0.3, 0.6], [0.4, 0.4, 0.7]])
    d = np.float32([[1, 0.01, 0.02], [1, 0.01, 0.02], [-0.3, 0.2, 0.9]])
    r = R.ray_mesh(o, d, v, f)
    assert list(r["count"]) == [2, 1, 1] and (r["flags"] == 0).all()
    pts = np.float32([[0.5, 0.5, 0.5], [0.1, 0.9, 0.2], [1.5, 0.5, 0.5], [-0.2, 0.3, 0.3], [0.3, 0.3, 1.0001]])
    ins, votes, grazed = R.inside(pts, v, f)
    assert list(ins) == [True, True, False, False, False] and list(votes) == [3, 3, 0, 0, 0] and not grazed.any()


@pytest.mark.parametrize("name", list(R.SOUP_GRIDS))
def test_the_grid_walk_reproduces_brute_force(name):
    """The scalar restatement of k_ray_mesh's walk gives brute force's nearest hit, count and flags on every grid (32 rays per
    grid: the walk is a python loop)."""
    v, f, _ = D.soup()
    o, d, tr = R.soup_rays()
    ref = R.soup_reference()
    g = R.numpy_grid(v, f, **R.SOUP_GRIDS[name])
    for i in range(0, 2000, 63):
        t, face, count, flags, _, tests = R.traverse(o[i], d[i], tr[i], v, f, g, "count")
        assert (t, face, count, flags) == (ref["t"][i], ref["face"][i], ref["count"][i], ref["flags"][i]), (name, i)
        t, face, count, _, _, fewer = R.traverse(o[i], d[i], tr[i], v, f, g, "closest")
        assert (t, face, count) == (ref["t"][i], ref["face"][i], min(ref["count"][i], 1)) and fewer <= tests, (name, i)


def test_parity_on_the_sphere_restatement():
    v, f, _ = D.sphere_pair()
    p, signed = R.sphere_points()
    p, signed = p[:R.SPHERE_POINTS], signed[:R.SPHERE_POINTS]
    ins, votes, grazed = R.inside(p, v, f)
    far = np.abs(signed) > 1.0
    assert far.sum() > 0.9 * len(p) and 0.1 < (signed < 0).mean() < 0.9
    assert np.array_equal(ins[far], signed[far] < 0)
    assert ((votes[far] == 0) | (votes[far] == 3)).all() and not grazed[far].any()


def test_topology_of_a_cube_an_open_cube_and_an_unwelded_copy():
    from tensoir_amd import mesh
    v, f = torch.from_numpy(R.CUBE_VERTS), torch.from_numpy(R.CUBE_FACES)
    assert mesh.topology(v, f) == {"closed": True, "boundary_edges": 0, "degenerate": 0}
    ov, of = R.open_cube()
    assert mesh.topology(torch.from_numpy(ov), torch.from_numpy(of)) == {"closed": False, "boundary_edges": 4, "degenerate": 0}
    uv, uf = R.unwelded(R.CUBE_VERTS, R.CUBE_FACES)
    assert len(uv) == 36 and mesh.topology(torch.from_numpy(uv), torch.from_numpy(uf))["closed"]
    uv, uf = R.unwelded(ov, of)
    assert mesh.topology(torch.from_numpy(uv), torch.from_numpy(uf)) == {"closed": False, "boundary_edges": 4, "degenerate": 0}
    flipped = R.CUBE_FACES.copy()
    flipped[5] = flipped[5, ::-1]                                       # one face wound the other way: its three edges twice, none back
    assert mesh.topology(v, torch.from_numpy(flipped)) == {"closed": False, "boundary_edges": 6, "degenerate": 0}
    sliver = np.concatenate([R.CUBE_FACES, np.int32([[0, 0, 3]])])      # a face with a repeated corner: its edges 0-3, 3-0 pair up
    assert mesh.topology(v, torch.from_numpy(sliver)) == {"closed": True, "boundary_edges": 0, "degenerate": 1}
    assert mesh.topology(v, torch.zeros((0, 3), dtype=torch.int32))["closed"]
    assert mesh.topology(v.numpy(), f.numpy())["closed"]               # arrays are taken too
    with pytest.raises(ValueError, match="face index"):
        mesh.topology(v, torch.tensor([[0, 1, 8]]))
    sv, sf, _ = D.sphere_pair()
    assert mesh.topology(sv, sf) == {"closed": True, "boundary_edges": 0, "degenerate": 0}


def test_summaries_on_hand_made_tensors():
    from tensoir_amd import mesh
    d = torch.tensor([0.5, 1.5, 2.0, 4.0])
    s = mesh.signed_summary(d, torch.tensor([True, False, True, False]), torch.tensor([3, 0, 2, 1], dtype=torch.uint8),
                            torch.tensor([False, False, True, False]))
    assert s == {"signed_mean": (-0.5 + 1.5 - 2.0 + 4.0) / 4, "inside_share": 0.5, "undecided": 2, "grazed": 1}
    s = mesh.signed_summary(d, torch.ones(4, dtype=torch.bool), torch.full((4,), 3), torch.zeros(4, dtype=torch.bool))
    assert s["signed_mean"] == -mesh.distance_summary(d[:0], d)["mean"] and s["inside_share"] == 1.0 and s["undecided"] == 0
    assert np.isnan(mesh.signed_summary(d[:0], d[:0].bool(), d[:0], d[:0].bool())["signed_mean"])
    fs = mesh.fscore_summary(d, torch.tensor([0.1, 0.2, 3.0, 9.0]), (0.05, 1.5, 10.0))
    assert fs[0] == {"threshold": 0.05, "precision": 0.0, "recall": 0.0, "fscore": 0.0}
    assert fs[1] == {"threshold": 1.5, "precision": 0.5, "recall": 0.5, "fscore": 0.5}           # <= : 1.5 itself counts
    assert fs[2] == {"threshold": 10.0, "precision": 1.0, "recall": 1.0, "fscore": 1.0}
    assert fs == R.fscore(d.numpy(), [0.1, 0.2, 3.0, 9.0], (0.05, 1.5, 10.0))
    z, x = [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]
    n_own = torch.tensor([z, z, z, x], dtype=torch.float64)
    n_near = torch.tensor([z, [0.0, 0.0, -1.0], [0.0, 0.6, 0.8], z], dtype=torch.float64)
    ns = mesh.normal_summary(n_own, n_near)
    assert ns == {"normal_consistency": (1 + 1 + 0.8 + 0) / 4, "flipped_share": 0.25}
    assert ns == R.normal_figures(n_own.numpy(), n_near.numpy())
    # face normals: fp64, unit, NaN for the index -1
    fn = mesh.face_normals(torch.from_numpy(R.CUBE_VERTS), torch.from_numpy(R.CUBE_FACES), torch.tensor([0, 2, 11, -1]))
    assert fn.dtype == torch.float64 and torch.equal(fn[:3], torch.tensor([[-1.0, 0, 0], [1.0, 0, 0], [0, 0, 1.0]], dtype=torch.float64))
    assert torch.isnan(fn[3]).all()
    assert np.allclose(fn[:3].numpy(), R.face_normals(R.CUBE_VERTS, R.CUBE_FACES, [0, 2, 11]), atol=0, rtol=0)


def test_options_are_validated_before_the_device():
    from tensoir_amd import mesh, ops
    v, f = torch.from_numpy(R.CUBE_VERTS), torch.from_numpy(R.CUBE_FACES)
    m = (v, f)
    for kw in (dict(samples=-1), dict(thresholds=()), dict(thresholds=(0.1, -1.0)), dict(thresholds=(float("nan"),)), dict(signed=1),
               dict(normals="yes"), dict(allow_open=True)):
        with pytest.raises(ValueError):
            mesh.distance(m, m, **kw)
    ov, of = (torch.from_numpy(x) for x in R.open_cube())
    with pytest.raises(ValueError, match="4 boundary edges"):
        mesh.distance(m, (ov, of), samples=16, signed=True)                # refused on the host mesh, before any kernel
    o = torch.zeros((4, 3))
    with pytest.raises(ValueError, match="mode"):
        ops.ray_mesh(o, o, v, f, mode="nearest")
    with pytest.raises(ValueError, match="any"):
        ops.ray_mesh(o, o, v, f, mode="any", bary=True)
    with pytest.raises(ValueError, match="any"):
        ops.ray_mesh(o, o, v, f, mode="any", count=True)
    with pytest.raises(ValueError, match="mode"):
        mesh.raycast(m, o, o, mode="any")
    from tensoir_amd._lib import TensoirHipError
    with pytest.raises(TensoirHipError, match="GPU"):                      # no CPU path, no fall-back
        ops.ray_mesh(o, o, v, f)
    with pytest.raises(TensoirHipError, match="GPU"):
        ops.mesh_inside(o, v, f)


def test_the_command_line_refuses_options_without_check_distance(capsys):
    from tensoir_amd import bake
    for extra in (["--check-signed"], ["--check-normals"], ["--check-fscore", "0.5"], ["--check-distance", "16", "--check-fscore", "-1"]):
        with pytest.raises(SystemExit):
            bake.main(["nowhere.th", "out.ply"] + extra)
        assert "--check-" in capsys.readouterr().err


def test_ray_entry_validates_on_the_host_before_any_device_work():
    """-1001 / -1002 for bad arguments and 0 for n = 0, without a GPU: the pointers are host addresses that are never followed."""
    import ctypes as C
    from tensoir_amd import _lib
    lib = _lib.lib()
    keep = torch.zeros(64, dtype=torch.float32)
    ptr = keep.data_ptr()
    f3, i3 = (C.c_float * 3), (C.c_int32 * 3)
    cell, org, dims = f3(1, 1, 1), f3(0, 0, 0), i3(2, 2, 2)
    base = dict(origins=ptr, dirs=ptr, trange=None, n=8, cell=cell, dims=dims, cursor=ptr, pairs=ptr, n_pairs=4, bounds=ptr, mode=0,
                t=ptr, face=ptr, bary=None, count=None, flags=None, tested=None, verts=ptr, faces=ptr)

    def q(**kw):
        a = dict(base, **kw)
        return lib.tir_ray_mesh(a["origins"], a["dirs"], a["trange"], a["n"], a["verts"], 3, a["faces"], 1, a["cell"], org, a["dims"],
                                a["cursor"], a["pairs"], a["n_pairs"], a["bounds"], a["mode"], a["t"], a["face"], a["bary"], a["count"],
                                a["flags"], a["tested"], None)
    assert q(n=0) == 0 and q(n=0, origins=None, dirs=None, t=None, face=None, bounds=None) == 0
    assert q(n=0, mode=1) == 0 and q(n=0, mode=2, t=None, face=None) == 0
    for name in ("origins", "dirs", "cursor", "bounds", "t", "face", "pairs", "verts", "faces"):
        assert q(**{name: None}) == -1001, name
    assert q(n=-1) == -1001 and q(n_pairs=-1) == -1001
    assert q(mode=3) == -1001 and q(mode=-1) == -1001 and q(n=0, mode=7) == -1001
    # mode any: count is the output, t / face / bary contradict it (whatever n is)
    assert q(mode=2) == -1001 and q(mode=2, t=None) == -1001 and q(mode=2, t=None, face=None) == -1001
    assert q(mode=2, t=None, face=None, count=ptr, bary=ptr) == -1001 and q(n=0, mode=2, count=ptr) == -1001
    assert q(mode=1, t=None, count=ptr) == -1001
    # the grid conditions of the other entries
    assert q(cell=f3(0, 1, 1)) == -1001 and q(cell=f3(1, float("nan"), 1)) == -1001 and q(dims=i3(2, 0, 2)) == -1001 and q(cell=None) == -1001
    assert q(dims=i3(1, 1, 1000)) == -1002 and q(n=2 ** 31) == -1002 and q(n_pairs=2 ** 31) == -1002
