"""Mesh simplification without a GPU: the numpy restatement (tests/simplify_reference.py) has the properties the definition
promises, the quadric placement beats the centroid where it should, and the C entries and the Python options refuse bad
arguments on the host."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import mesh_reference as MR
from tests import simplify_reference as S


@pytest.mark.parametrize("name", S.GOLDEN_CASES)
def test_restatement_on_the_golden_volumes(name):
    v, f, cell, origin = S.case(name)
    pos, faces, normals, cov, dims = S.reference(name)
    assert len(f) > 0 and 0 < len(faces) < len(f) and 0 < len(pos) < len(v)
    # one output vertex per distinct key, in ascending key order
    q, ci, _ = S.cell_indices(v, cell, origin, dims)
    key = (ci[:, 0] * dims[1] + ci[:, 1]) * dims[2] + ci[:, 2]
    uk = np.unique(key)
    assert len(pos) == len(uk) and np.array_equal(uk[cov], key)
    # every vertex inside its cell (the clamp), and the map takes each input vertex to the vertex of its own cell
    u = S.in_cell_units(pos, cell, origin)
    cidx = np.stack([uk // (dims[1] * dims[2]), (uk // dims[2]) % dims[1], uk % dims[2]], 1)
    assert (u >= cidx - 1e-9).all() and (u <= cidx + 1 + 1e-9).all()
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-12)
    # faces: the survivors of the remap, in input order, none degenerate
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    g = cov[f]
    keep = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    assert np.array_equal(faces, g[keep])
    closed = MR.is_closed_and_oriented(f)
    assert closed == (not name.startswith("open"))
    assert S.edge_balance(faces) == closed


def test_float64_cell_assignment_would_differ():
    """Why step 1 is pinned to float32: marching-cubes vertices sit on cluster boundaries, and a float64 quotient puts some of them
    in the neighbouring cell."""
    v, f, cell, origin = S.case("alpha-k2")
    q32 = S.cell_indices(v, cell, origin)[0]
    q64 = (v.astype(np.float64) - np.asarray(origin, np.float32).astype(np.float64)) / cell.astype(np.float64)
    assert (np.floor(q32) != np.floor(q64)).any()


def test_float32_restatement_stays_inside_the_gpu_tolerance():
    """Where the GPU test's position and normal limits come from: the restatement run wholly in float32 against its float64 self
    (identical faces; at most 9.9e-6 cell edges and 2.5e-7 per normal component when the limits were set, ten times below them)."""
    worst_p = worst_n = 0.0
    for name in S.GOLDEN_CASES + ("box", "sphere"):
        v, f, cell, origin = S.case(name)
        pos, faces, normals, cov, dims = S.reference(name)
        p32, f32, n32, c32 = S.simplify(v, f, cell, origin, dims, dtype=np.float32)
        assert p32.dtype == np.float32 and np.array_equal(f32, faces) and np.array_equal(c32, cov)
        worst_p = max(worst_p, float((np.abs(p32 - pos) / cell.astype(np.float64)).max()))
        worst_n = max(worst_n, float(np.abs(n32 - normals).max()))
    print(f"\n[float32 restatement] max position deviation {worst_p:.2e} cell edges, max normal deviation {worst_n:.2e}")
    assert worst_p <= 1e-4 / 5 and worst_n <= 1e-5 / 5


def test_quadric_vertices_lie_on_a_box_where_centroids_do_not():
    v, f, cell, origin = S.case("box")
    assert MR.is_closed_and_oriented(f)
    pos, faces, _, _, dims = S.reference("box")
    cen = S.simplify(v, f, cell, origin, dims, centroid=True)[0]
    rms = lambda p: float(np.sqrt((S.box_distance(p) ** 2).mean()))
    rq, rc = rms(pos), rms(cen)
    print(f"\n[box, k = 3] rms distance to the true surface: quadric {rq:.4f}, centroid {rc:.4f}")
    assert rq <= 0.5 * rc
    assert abs(rq - 0.048) < 2e-3 and abs(rc - 0.211) < 2e-3           # the figures the design records
    assert S.edge_balance(faces)


def test_hand_made_meshes():
    # all vertices in one cell: one vertex, no face; the collapsed face still counts toward the cell's quadric and normal
    v = np.float32([[0.1, 0.1, 0.1], [0.9, 0.1, 0.1], [0.1, 0.9, 0.1]])
    pos, faces, normals, cov = S.simplify(v, [[0, 1, 2]], 1.0)
    assert len(pos) == 1 and faces.shape == (0, 3) and cov.tolist() == [0, 0, 0]
    assert np.allclose(normals, [[0, 0, 1]])
    # a vertex no face uses sits at the mean of its cell's vertices
    pos, faces, normals, cov = S.simplify(np.float32([[0.25, 0.5, 0.75], [0.75, 0.5, 0.25]]), np.zeros((0, 3), np.int32), 1.0)
    assert np.allclose(pos, [[0.5, 0.5, 0.5]]) and np.allclose(normals, [[0, 0, 1]])
    # nothing at all
    pos, faces, normals, cov = S.simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0)
    assert pos.shape == (0, 3) and faces.shape == (0, 3) and normals.shape == (0, 3) and cov.shape == (0,)


# ---- the library and the options, on the host -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_entries_validate_before_any_device_work(lib):
    import torch
    keep = torch.zeros(64, dtype=torch.float32)                        # a non-null host address: never dereferenced
    ptr = keep.data_ptr()
    f3 = lambda *x: (C.c_float * 3)(*x)
    i3 = lambda *x: (C.c_int32 * 3)(*x)
    one, org, dims = f3(1, 1, 1), f3(0, 0, 0), i3(4, 4, 4)
    count = lambda *a: lib.tir_simplify_count(*a, None)
    emit = lambda *a: lib.tir_simplify_emit(*a, None)
    assert count(None, 8, None, 8, one, org, dims, None, None, None, None, None) == -1001
    assert count(ptr, 8, ptr, 8, None, org, dims, ptr, ptr, ptr, ptr, ptr) == -1001
    assert count(ptr, 8, ptr, 8, one, org, None, ptr, ptr, ptr, ptr, ptr) == -1001
    assert count(ptr, 8, ptr, 8, one, org, dims, ptr, ptr, ptr, ptr, None) == -1001            # the status words
    assert count(ptr, 8, ptr, 8, f3(1, 0, 1), org, dims, ptr, ptr, ptr, ptr, ptr) == -1001      # cell = 0
    assert count(ptr, 8, ptr, 8, f3(1, float("nan"), 1), org, dims, ptr, ptr, ptr, ptr, ptr) == -1001
    assert count(ptr, 8, ptr, 8, one, org, i3(4, 0, 4), ptr, ptr, ptr, ptr, ptr) == -1001      # dims < 1
    assert count(ptr, -1, ptr, 8, one, org, dims, ptr, ptr, ptr, ptr, ptr) == -1001
    assert count(ptr, 8, ptr, 8, one, org, i3(2048, 2048, 2048), ptr, ptr, ptr, ptr, ptr) == -1002
    assert count(ptr, 8, ptr, (1 << 28) + 1, one, org, dims, ptr, ptr, ptr, ptr, ptr) == -1002
    assert emit(ptr, 8, ptr, 8, one, org, i3(2048, 2048, 2048), 1e-2, ptr, ptr, 4, 4, ptr, ptr, ptr, ptr, ptr) == -1002
    assert emit(ptr, 8, ptr, 8, one, org, dims, -1e-3, ptr, ptr, 4, 4, ptr, ptr, ptr, ptr, ptr) == -1001      # reg < 0
    assert emit(ptr, 8, ptr, 8, one, org, dims, float("nan"), ptr, ptr, 4, 4, ptr, ptr, ptr, ptr, ptr) == -1001
    assert emit(ptr, 8, ptr, 8, f3(0, 1, 1), org, dims, 1e-2, ptr, ptr, 4, 4, ptr, ptr, ptr, ptr, ptr) == -1001
    assert emit(None, 8, ptr, 8, one, org, dims, 1e-2, ptr, ptr, 4, 4, ptr, ptr, ptr, ptr, ptr) == -1001
    assert emit(ptr, 8, ptr, 8, one, org, dims, 1e-2, ptr, ptr, 4, 4, None, ptr, ptr, ptr, ptr) == -1001      # the accumulators
    assert emit(ptr, 8, ptr, 8, one, org, dims, 1e-2, ptr, ptr, 9, 4, ptr, ptr, ptr, ptr, ptr) == -1001       # more cells than vertices
    assert emit(None, 0, None, 0, one, org, dims, 1e-2, None, None, 0, 0, None, None, None, None, None) == 0   # nothing to do
    assert lib.tir_simplify_blocks(0) == 0 and lib.tir_simplify_blocks(4097) == 2 and lib.tir_simplify_blocks(-1) == -1001
    assert lib.tir_version() == 100


def test_simplify_kernels_hold_no_scratch(lib):
    import sys
    sys.path.insert(0, os.path.join(S.ROOT, "tools"))
    import kernel_resources
    from tensoir_amd import _lib
    ks = [k for k in kernel_resources.kernels(_lib.LIB_PATH) if k["name"].startswith("k_simplify_")]
    assert len(ks) >= 8, sorted(k["name"] for k in ks)
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgpr"] + k["agpr"] <= 128, k


@pytest.mark.parametrize("bad", [1, 0, -3, 2.5, True, "2"])
def test_export_refuses_a_bad_simplify_before_touching_the_device(bad, tmp_path):
    import torch
    import tensoir_amd
    from tensoir_amd import mesh
    from tests import config_scenes as CS
    m = tensoir_amd.TensorVMSplit(torch.tensor(CS.AABB), CS.GRID, "cpu", shadingMode="MLP_Fea")       # a host-built model
    path = str(tmp_path / "never.ply")
    with pytest.raises(ValueError, match="simplify"):
        mesh.export_mesh(m, path, simplify=bad)
    with pytest.raises(ValueError, match="simplify"):
        mesh.extract_mesh(m, simplify=bad)
    assert not os.path.exists(path)
