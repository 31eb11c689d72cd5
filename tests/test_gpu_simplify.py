"""Mesh simplification on the GPU (tir_simplify_*, ops.simplify_mesh, mesh.extract_mesh / export_mesh with simplify=k, the bake
command line) against the numpy restatement (tests/simplify_reference.py).

Comparison rules.  faces' and cell_of_vertex are discrete and must be equal.  Positions must agree within 1e-4 of a cell edge per
axis: the restatement run wholly in float32 deviates from its float64 self by at most 9.9e-6 cell edges over all the cases below
(reg = 1e-2), and the limit is ten times that; the kernels form every term in fp64 and sum in integers, so they sit far inside
it.  Normals must agree within 1e-5 per component (float32 deviation 2.5e-7; every cell of these cases has |N| >= 0.82 sum |n|).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import components_reference as CR
from tests import mesh_reference as MR
from tests import simplify_reference as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS_TOL, NRM_TOL = 1e-4, 1e-5


def device_simplify(v, f, cell, origin=(0.0, 0.0, 0.0), dims=None, **kw):
    from tensoir_amd import ops
    out = ops.simplify_mesh(torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda().reshape(-1, 3),
                            torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda().reshape(-1, 3),
                            [float(c) for c in np.broadcast_to(np.asarray(cell, np.float32), (3,))], origin,
                            None if dims is None else [int(d) for d in dims], **kw)
    torch.cuda.synchronize()
    assert [t.dtype for t in out] == [torch.float32, torch.int32, torch.float32, torch.int32] and all(t.is_cuda for t in out)
    assert out[0].shape == out[2].shape and out[0].shape[1:] == (3,) and out[1].shape[1:] == (3,) and out[3].shape == (len(v),)
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_same_bits(a, b):
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(bits(a[2]), bits(b[2]))
    assert torch.equal(a[3], b[3])


def assert_equals_restatement(got, ref, cell, what=""):
    pos, faces, normals, cov = (t.cpu().numpy() for t in got)
    rpos, rfaces, rnormals, rcov = ref[:4]
    assert np.array_equal(cov, rcov), what
    assert faces.shape == rfaces.shape and np.array_equal(faces, rfaces), what
    assert pos.shape == rpos.shape
    cell = np.broadcast_to(np.asarray(cell, np.float32), (3,)).astype(np.float64)
    dp = np.abs(pos.astype(np.float64) - rpos) / cell
    dn = np.abs(normals.astype(np.float64) - rnormals)
    print(f"\n[simplify {what}] V' {len(pos)} F' {len(faces)}: max position deviation {dp.max(initial=0):.3e} cell edges, "
          f"max normal deviation {dn.max(initial=0):.3e}")
    assert dp.max(initial=0) <= POS_TOL and dn.max(initial=0) <= NRM_TOL, what


@pytest.mark.parametrize("name", S.GOLDEN_CASES + ("box", "sphere"))
def test_kernels_equal_restatement_and_repeat(name):
    v, f, cell, origin = S.case(name)
    ref = S.reference(name)
    dims = ref[4]
    a = device_simplify(v, f, cell, origin, dims)
    assert_equals_restatement(a, ref, cell, name)
    b = device_simplify(v, f, cell, origin, dims)
    assert_same_bits(a, b)
    if name in ("alpha-k2", "sphere"):                 # dims taken from the vertex maximum: the same cells, the same mesh
        c = device_simplify(v, f, cell, origin, None)
        assert_same_bits(a, c)
    if name == "sphere":
        assert len(f) == 61236 and a[0].shape[0] == 6674          # several scan blocks of faces, and of cell slots


# ---- hand-made meshes ------------------------------------------------------------------------------------------------------
def test_empty_mesh():
    z3f, z3i = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    pos, faces, normals, cov = device_simplify(z3f, z3i, 1.0, dims=[3, 3, 3])
    assert pos.shape == (0, 3) and faces.shape == (0, 3) and normals.shape == (0, 3) and cov.shape == (0,)
    pos, faces, normals, cov = device_simplify(z3f, z3i, 1.0)
    assert pos.shape == (0, 3) and faces.shape == (0, 3)
    # vertices without faces: every one at the mean of its cell's vertices, normal (0, 0, 1)
    v = np.float32([[0.25, 0.5, 0.75], [0.75, 0.5, 0.25], [2.5, 0.125, 0.0]])
    got = device_simplify(v, z3i, 1.0)
    assert_equals_restatement(got, S.simplify(v, z3i, 1.0), 1.0, "no faces")
    assert np.allclose(got[0].cpu().numpy(), [[0.5, 0.5, 0.5], [2.5, 0.125, 0.0]], atol=1e-6)
    assert got[2].cpu().tolist() == [[0, 0, 1], [0, 0, 1]] and got[3].cpu().tolist() == [0, 0, 1]


def test_all_vertices_in_one_cell():
    v = np.float32([[0.1, 0.1, 0.1], [0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.5, 0.5, 0.9]])
    f = np.int32([[0, 1, 2], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    got = device_simplify(v, f, 1.0, dims=[2, 2, 2])
    assert got[0].shape == (1, 3) and got[1].shape == (0, 3) and got[3].cpu().tolist() == [0, 0, 0, 0]
    assert_equals_restatement(got, S.simplify(v, f, 1.0, dims=[2, 2, 2]), 1.0, "one cell")


def test_one_triangle_over_three_cells_and_an_unused_vertex():
    """A single face gives every cell a rank-1 quadric: the regularisation places the vertex on the face's plane nearest the mean.
    Vertex 3 belongs to no face: its cell has t = 0 and the vertex goes to the mean."""
    v = np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.75], [2.25, 2.5, 2.75]])
    f = np.int32([[0, 1, 2]])
    ref = S.simplify(v, f, 1.0, dims=[3, 3, 3])
    got = device_simplify(v, f, 1.0, dims=[3, 3, 3])
    assert ref[1].tolist() == [[0, 2, 1]] and len(ref[0]) == 4         # kept, renumbered in key order, winding as given
    assert_equals_restatement(got, ref, 1.0, "one triangle")
    assert np.allclose(got[0].cpu().numpy()[3], [2.25, 2.5, 2.75], atol=1e-6)
    n = np.cross(v[1] - v[0], v[2] - v[0])
    assert np.allclose(got[2].cpu().numpy()[:3], n / np.linalg.norm(n), atol=1e-6)
    assert got[2].cpu().numpy()[3].tolist() == [0, 0, 1]


def test_opposite_triangles_cancel_to_the_default_normal():
    """Two coincident triangles of opposite winding whose first corner shares cell 0: N = 0 there, exactly, in integer sums."""
    v = np.float32([[0.3, 0.4, 0.5], [1.6, 0.4, 0.45], [0.3, 1.7, 0.55]])
    f = np.int32([[0, 1, 2], [0, 2, 1]])
    ref = S.simplify(v, f, 1.0, dims=[2, 2, 1])
    got = device_simplify(v, f, 1.0, dims=[2, 2, 1])
    assert (ref[2] == [0, 0, 1]).all() and len(ref[1]) == 2
    assert_equals_restatement(got, ref, 1.0, "opposite triangles")
    assert got[2].cpu().tolist() == [[0, 0, 1]] * 3


def test_vertex_on_the_upper_boundary_clamps():
    v = np.float32([[2.0, 0.5, 0.5], [0.5, 2.0, 0.5], [0.5, 0.5, 1.0], [2.0, 2.0, 1.0]])           # q = dims on some axis
    f = np.int32([[0, 1, 2], [1, 0, 3]])
    ref = S.simplify(v, f, 1.0, dims=[2, 2, 1])
    got = device_simplify(v, f, 1.0, dims=[2, 2, 1])
    assert_equals_restatement(got, ref, 1.0, "upper boundary")
    assert got[3].cpu().tolist() == [2, 1, 0, 3] and ref[1].tolist() == [[2, 1, 0], [1, 2, 3]]
    # anisotropic cells and an origin: positions and normals come back in the coordinates of verts
    cell, origin = np.float32([0.5, 1.0, 2.0]), (-1.0, 0.25, 3.0)
    w = v * cell + np.float32(origin)
    got2 = device_simplify(w, f, cell, origin, dims=[2, 2, 1])
    assert_equals_restatement(got2, S.simplify(w, f, cell, origin, dims=[2, 2, 1]), cell, "anisotropic")
    assert torch.equal(got2[1], got[1]) and torch.equal(got2[3], got[3])


def test_bad_input_is_refused_not_followed():
    """The guards' refusals.  No access leaves a buffer: the face with the index V is skipped by every kernel and reported."""
    from tensoir_amd import ops
    from tensoir_amd._lib import TensoirHipError
    v = np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]])
    with pytest.raises(TensoirHipError, match="face index"):
        device_simplify(v, np.int32([[0, 1, 2], [0, 1, 3]]), 1.0, dims=[2, 2, 1])
    with pytest.raises(TensoirHipError, match="face index"):
        device_simplify(v, np.int32([[0, -1, 2]]), 1.0, dims=[2, 2, 1])
    with pytest.raises(TensoirHipError, match="face index"):
        device_simplify(np.zeros((0, 3), np.float32), np.int32([[0, 0, 0]]), 1.0, dims=[2, 2, 1])
    far = np.float32([[0.5, 0.5, 0.5], [5.0, 0.5, 0.5], [0.5, 1.5, 0.5]])
    with pytest.raises(TensoirHipError, match="face edge"):
        device_simplify(far, np.int32([[0, 1, 2]]), 1.0, dims=[6, 2, 1])
    with pytest.raises(TensoirHipError, match="vertex"):
        device_simplify(np.float32([[-9.0, 0.5, 0.5]]), np.zeros((0, 3), np.int32), 1.0, dims=[2, 2, 1])
    dv, df = torch.from_numpy(v).cuda(), torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda")
    with pytest.raises(TensoirHipError):
        ops.simplify_mesh(dv, df, 0.0)
    with pytest.raises(TensoirHipError):
        ops.simplify_mesh(dv, df, 1.0, dims=[2, 0, 1])
    with pytest.raises(TensoirHipError):
        ops.simplify_mesh(dv, df, 1.0, dims=[2048, 2048, 2048])
    with pytest.raises(TensoirHipError):
        ops.simplify_mesh(dv, df, 1.0, dims=[2, 2, 1], reg=-1.0)
    # a NaN vertex is keyed to cell 0 (no access outside the slots) and reported
    with pytest.raises(TensoirHipError, match="vertex"):
        device_simplify(np.float32([[np.nan, 0.5, 0.5]]), np.zeros((0, 3), np.int32), 1.0, dims=[2, 2, 1])


# ---- the blob scene --------------------------------------------------------------------------------------------------------
def blob_model():
    import tensoir_amd
    return tensoir_amd.model_from_checkpoint(CR.blob_checkpoint(), "cuda:0", envmap_h=4, envmap_w=8)


@pytest.fixture(scope="module")
def blobs():
    model = blob_model()
    model.march_t_stop = 0.0
    return model


def restated(model, verts, faces, k):
    """The restatement with the clusters extract_mesh(simplify=k) uses -> (pos, faces, INDEX-space normals, cell)."""
    from tensoir_amd import mesh
    aabb = model.aabb.detach().cpu().float()
    sp = np.float32(mesh.reference_spacing(aabb, CR.BLOB_GRID))
    cell = sp * np.float32(k)
    pos, f, n, _ = S.simplify(verts.cpu().numpy(), faces.cpu().numpy(), cell, aabb[0].numpy(), [(g - 1) // k + 1 for g in CR.BLOB_GRID])
    n = n * sp.astype(np.float64)
    return pos, f, n / np.linalg.norm(n, axis=1, keepdims=True), cell


def test_extract_mesh_simplify_equals_restatement_of_the_full_mesh(blobs):
    from tensoir_amd import mesh
    v0, f0, _ = mesh.extract_mesh(blobs)
    assert MR.is_closed_and_oriented(f0.cpu().numpy())
    for k in (2, 3):
        report = {}
        v, f, n = mesh.extract_mesh(blobs, simplify=k, report=report)
        assert report["full"] == (v0.shape[0], f0.shape[0])
        pos, rf, rn, cell = restated(blobs, v0, f0, k)
        assert np.array_equal(f.cpu().numpy(), rf) and 0 < len(rf) < len(f0) / 2
        assert (np.abs(v.cpu().numpy().astype(np.float64) - pos) / cell).max() <= POS_TOL
        assert np.abs(n.cpu().numpy().astype(np.float64) - rn).max() <= NRM_TOL
        assert S.edge_balance(rf)
    # after the component filter: the filter runs first, on the lattice
    v1, f1, _ = mesh.extract_mesh(blobs, keep_largest=1)
    v, f, n = mesh.extract_mesh(blobs, keep_largest=1, simplify=2)
    pos, rf, rn, cell = restated(blobs, v1, f1, 2)
    assert np.array_equal(f.cpu().numpy(), rf) and (np.abs(v.cpu().numpy().astype(np.float64) - pos) / cell).max() <= POS_TOL
    assert S.edge_balance(rf) and len(rf) < len(f1) / 2


def test_simplify_none_leaves_the_export_byte_identical(blobs, tmp_path, monkeypatch):
    from tensoir_amd import mesh, ops

    def refuse(*a, **k):
        raise AssertionError("a simplification call without the option")
    monkeypatch.setattr(ops, "simplify_mesh", refuse)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    na = mesh.export_mesh(blobs, a)
    nb = mesh.export_mesh(blobs, b, simplify=None)
    assert na == nb and open(a, "rb").read() == open(b, "rb").read()
    v, f, _ = mesh.extract_mesh(blobs)
    plain = str(tmp_path / "plain.ply")
    mesh.write_ply(plain, v, f)                         # the export as it was before the option existed: marching cubes, written
    assert open(a, "rb").read() == open(plain, "rb").read()


def test_export_with_attributes_bakes_at_the_simplified_vertices_and_the_cli_agrees(tmp_path):
    """A model as a saved checkpoint loads it (march_t_stop at its default, which the bake's marches use and a checkpoint does
    not carry), so that the command line, a fresh child process, can be asked for the same file."""
    from tensoir_amd import bake, mesh
    m = blob_model()
    full, out, cli = (str(tmp_path / n) for n in ("full.ply", "simplified.ply", "cli.ply"))
    _, nf_full = mesh.export_mesh(m, full, keep_largest=1)
    nv, nf = mesh.export_mesh(m, out, simplify=2, attributes=True, keep_largest=1)
    pv, pf, attrs = mesh.read_ply_attributes(out)
    assert (nv, nf) == (len(pv), len(pf)) and 0 < nf < nf_full / 2
    verts, faces, normals = mesh.extract_mesh(m, simplify=2, keep_largest=1)
    assert np.array_equal(pv.view(np.uint32), verts.cpu().numpy().view(np.uint32)) and np.array_equal(pf, faces.cpu().numpy())
    pos, outward = mesh.field_positions(m.aabb, CR.BLOB_GRID, verts, normals)
    baked = bake.bake_points(m, pos.contiguous(), outward.contiguous())
    torch.cuda.synchronize()
    col = lambda *names: np.stack([attrs[n] for n in names], 1)
    same = lambda a, t: np.array_equal(a.view(np.uint32), t.cpu().numpy().reshape(a.shape).view(np.uint32))
    assert list(attrs) == [n for n, _ in mesh.ATTRIBUTE_LAYOUT[3:]]
    assert same(col("nx", "ny", "nz"), baked["normal"])
    assert same(attrs["roughness"], baked["roughness"]) and same(attrs["ao"], baked["ao"]) and same(attrs["coverage"], baked["coverage"])
    assert same(col("albedo_r", "albedo_g", "albedo_b"), baked["albedo"])
    assert same(col("irradiance_r", "irradiance_g", "irradiance_b"), baked["irradiance"])
    # the command line on the saved checkpoint
    ckpt = str(tmp_path / "blobs.th")
    m.save(ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tensoir_amd.bake", ckpt, cli, "--simplify", "2", "--keep-largest", "1", "--envmap", "4", "8"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "simplify 2: " in r.stdout and f"{nv} vertices, {nf} faces" in r.stdout, r.stdout
    assert open(cli, "rb").read() == open(out, "rb").read()
