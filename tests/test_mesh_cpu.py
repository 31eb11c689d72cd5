"""Marching-cubes mesh export without a GPU: the generated case table, the numpy restatement of the kernels' contract against
scikit-image's recorded output (tests/golden/mesh_skimage.npz), the PLY writer, the skimage / plyfile stand-ins and the
argument validation of the tir_mc_* entry points."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests import mesh_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "mesh_skimage.npz"))
CASES = [str(c) for c in G["cases"]]


def load_generator():
    spec = importlib.util.spec_from_file_location("make_mc_table", os.path.join(ROOT, "tools", "make_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case(name):
    p = name + "/"
    return G[p + "vol"], float(G[p + "level"]), G[p + "spacing"]


def test_generator_reproduces_the_committed_table():
    gen = load_generator()
    assert gen.render() == open(R.TABLE).read()


# ---- the table, case by case -------------------------------------------------------------------------------------------
CORNER = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
EOFF, EAX = R.edge_corner_axis()


def edge_ends(e):
    a = tuple(int(x) for x in EOFF[e])
    b = list(a)
    b[EAX[e]] = 1
    return a, tuple(b)


def face_rule_segments(case_bits):
    """Independent statement of the face rule: per cube face, the undirected pairs of crossing edges it joins."""
    inside = [(case_bits >> c) & 1 for c in range(8)]
    segs = set()
    for axis in range(3):
        for side in (0, 1):
            cyc = [c for c in range(8) if CORNER[c][axis] == side]
            u, w = [a for a in range(3) if a != axis]
            cyc.sort(key=lambda c: {(0, 0): 0, (1, 0): 1, (1, 1): 2, (0, 1): 3}[(CORNER[c][u], CORNER[c][w])])
            edges = []
            for i in range(4):
                a, b = cyc[i], cyc[(i + 1) % 4]
                e = next(e for e in range(12) if set(edge_ends(e)) == {CORNER[a], CORNER[b]})
                edges.append((e, inside[a] != inside[b]))
            crossing = [e for e, x in edges if x]
            if len(crossing) == 2:
                segs.add(frozenset(crossing))
            elif len(crossing) == 4:
                for i in range(4):
                    if inside[cyc[i]]:      # inside corners are separated: cut each off with its own two edges
                        segs.add(frozenset((edges[i][0], edges[(i + 3) % 4][0])))
    return segs


def test_every_case_follows_the_face_rule():
    ntri, tri = R.load_table()
    for c in range(256):
        t = tri[c, :3 * ntri[c]].reshape(-1, 3).astype(int)
        assert (tri[c, 3 * ntri[c]:] == -1).all()
        inside = [(c >> k) & 1 for k in range(8)]
        crossing = {e for e in range(12) if inside[int(np.dot(EOFF[e], [1, 2, 4]))] !=
                    inside[int(np.dot(EOFF[e], [1, 2, 4])) + (1 << EAX[e])]}
        assert set(t.reshape(-1).tolist()) == crossing, c            # every crossing edge is used, no other
        cnt = {}
        for tr in t:
            assert len(set(tr.tolist())) == 3
            for i in range(3):
                k = frozenset((tr[i], tr[(i + 1) % 3]))
                cnt[k] = cnt.get(k, 0) + 1
        boundary = {k for k, n in cnt.items() if n == 1}
        assert all(n <= 2 for n in cnt.values()), c
        # boundary segments lie on cube faces (their two edges share a face) and are exactly the face rule's
        for k in boundary:
            e0, e1 = tuple(k)
            pts = set(edge_ends(e0)) | set(edge_ends(e1))
            assert any(len({p[a] for p in pts}) == 1 for a in range(3)), (c, k)
        assert boundary == face_rule_segments(c), c


def test_table_orientation_points_from_inside_to_outside():
    """With vertices at the edge midpoints no triangle's right-hand normal points against the direction from the inside
    corners to the outside corners of its edges, and in every case their sum points along it."""
    ntri, tri = R.load_table()
    mid = np.array([np.add(*edge_ends(e)) / 2 for e in range(12)])
    for c in range(1, 255):
        total = 0.0
        for tr in tri[c, :3 * ntri[c]].reshape(-1, 3):
            p = mid[tr]
            nrm = np.cross(p[1] - p[0], p[2] - p[0])
            out = np.zeros(3)
            for e in tr:
                a, b = (np.array(x) for x in edge_ends(e))
                ia = (c >> int(np.dot(a, [1, 2, 4]))) & 1
                out += (b - a) if ia else (a - b)
            assert np.dot(nrm, out) >= 0, (c, tr)
            total += np.dot(nrm, out)
        assert total > 0, c


# ---- restatement vs scikit-image -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_against_skimage(name):
    vol, level, sp = case(name)
    v, f, n = R.marching_cubes(vol, level, sp)
    p = name + "/"
    sv, sf = G[p + "verts"], G[p + "faces"]
    ext = float((np.array(vol.shape) * sp).max())
    assert len(v) == len(sv) == R.n_crossing_edges(vol, level)
    assert np.abs(R.sorted_rows(v) - R.sorted_rows(sv)).max() <= 1e-6 * ext
    assert abs(R.area(v, f) / R.area(sv, sf) - 1) < 0.01
    if name in ("blob", "onlevel"):
        assert R.is_closed_and_oriented(f)
    if name == "blob":
        ours, sk = R.signed_volume(v, f), R.signed_volume(sv, sf)
        assert ours > 0 > sk
        assert abs(ours / -sk - 1) < 0.005


@pytest.mark.parametrize("name", [c for c in CASES if c != "onlevel"])
def test_surface_polygons_differ_only_in_ambiguous_cells(name):
    """Per cell, the polygon the triangles cover agrees with scikit-image's except where a face is ambiguous (Lewiner's
    decider is value-based).  How each polygon is split into triangles may differ: the table fans every loop from its
    lowest edge.  (The on-level case has vertices at lattice points, whose edge is not recoverable from the position.)"""
    vol, level, sp = case(name)
    v, f, _ = R.marching_cubes(vol, level, sp)
    sv, sf = G[name + "/verts"], G[name + "/faces"]
    ours_k = R.crossing_keys(vol, level)
    sk_k = R.edge_keys(sv, sp, vol.shape)
    assert np.array_equal(np.sort(sk_k), ours_k)
    a, b = R.cell_polygons(ours_k[f], vol.shape), R.cell_polygons(sk_k[sf], vol.shape)
    assert set(a) == set(b)
    differ = {c for c in a if a[c] != b[c]}
    assert differ <= R.ambiguous_cells(vol, level)


# ---- PLY -------------------------------------------------------------------------------------------------------------------
def test_write_ply_layout_and_round_trip(tmp_path):
    from tensoir_amd import mesh
    rng = np.random.default_rng(0)
    v = rng.standard_normal((17, 3)).astype(np.float32)
    f = rng.integers(0, 17, (29, 3)).astype(np.int32)
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, v, f)
    data = open(path, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 17\nproperty float x\nproperty float y\n"
              b"property float z\nelement face 29\nproperty list uchar int vertex_indices\nend_header\n")
    assert data.startswith(header)
    assert len(data) == len(header) + 17 * 12 + 29 * 13
    body = data[len(header):]
    assert np.array_equal(np.frombuffer(body[:17 * 12], "<f4").reshape(17, 3), v)
    rec = np.frombuffer(body[17 * 12:], np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    assert (rec["n"] == 3).all() and np.array_equal(rec["i"], f)
    rv, rf = mesh.read_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rf, f)
    mesh.write_ply(str(tmp_path / "e.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert mesh.read_ply(str(tmp_path / "e.ply"))[0].shape == (0, 3)


@pytest.fixture
def shimmed():
    """shims.install() with sys.modules restored afterwards (the stand-ins must not leak into other tests)."""
    from tensoir_amd import shims
    before = dict(sys.modules)
    shims.install()
    yield
    for k in list(sys.modules):
        if k not in before:
            del sys.modules[k]
    sys.modules.update(before)


def test_plyfile_stand_in_writes_what_write_ply_writes(tmp_path, shimmed):
    import plyfile
    if not getattr(plyfile, "__tensoir_shim__", False):
        pytest.skip("the real plyfile is installed")
    from tensoir_amd import mesh
    rng = np.random.default_rng(1)
    v = rng.standard_normal((11, 3)).astype(np.float32)
    f = rng.integers(0, 11, (7, 3)).astype(np.int32)
    # the arrays exactly as convert_sdf_samples_to_ply builds them (utils.py:206-219)
    verts_tuple = np.zeros((11,), dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
    for i in range(11):
        verts_tuple[i] = tuple(v[i, :])
    faces_tuple = np.array([(f[i, :].tolist(),) for i in range(7)], dtype=[("vertex_indices", "i4", (3,))])
    el_verts = plyfile.PlyElement.describe(verts_tuple, "vertex")
    el_faces = plyfile.PlyElement.describe(faces_tuple, "face")
    plyfile.PlyData([el_verts, el_faces]).write(str(tmp_path / "a.ply"))
    mesh.write_ply(str(tmp_path / "b.ply"), v, f)
    assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read()


def test_skimage_stand_in_is_installed_and_rejects_other_options(shimmed):
    import skimage.measure
    if not getattr(skimage.measure, "__tensoir_shim__", False):
        pytest.skip("the real scikit-image is installed")
    from tensoir_amd import shims
    assert skimage.measure.marching_cubes is shims.marching_cubes
    vol = np.zeros((4, 4, 4), np.float32)
    for kw in ({"level": None}, {"level": 0.5, "mask": np.ones((4, 4, 4), bool)}, {"level": 0.5, "step_size": 2},
               {"level": 0.5, "gradient_direction": "ascent"}, {"level": 0.5, "method": "lorensen"},
               {"level": 0.5, "spacing": (1.0, 1.0)}):
        with pytest.raises(ValueError):
            skimage.measure.marching_cubes(vol, **kw)      # raised on the host: no device is touched


# ---- C ABI validation --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_mc_entry_points_validate_before_any_device_work(lib):
    import torch
    keep = torch.zeros(64, dtype=torch.float32)      # a non-null host address: never dereferenced
    ptr = keep.data_ptr()
    assert lib.tir_mc_blocks(2, 2, 2) == 1
    assert lib.tir_mc_blocks(512, 512, 512) == 512 ** 3 // 4096
    assert lib.tir_mc_blocks(300, 300, 300) == -(-300 ** 3 // 4096)
    for g in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (-4, 8, 8)):
        assert lib.tir_mc_blocks(*g) == -1001, g
        assert lib.tir_mc_count(ptr, *g, 0.5, ptr, ptr, None) == -1001, g
    for g in ((2048, 1024, 1025), (1300, 1300, 1300), (1000, 1000, 1000)):   # > 2^31-1 points / worst-case totals > int32
        assert lib.tir_mc_blocks(*g) == -1002, g
        assert lib.tir_mc_count(ptr, *g, 0.5, ptr, ptr, None) == -1002, g
        assert lib.tir_mc_emit(ptr, *g, 0.5, 1, 1, 1, 0, 0, 0, ptr, 4, 4, ptr, ptr, ptr, ptr, None) == -1002, g
    assert lib.tir_mc_count(None, 8, 8, 8, 0.5, ptr, ptr, None) == -1001
    assert lib.tir_mc_count(ptr, 8, 8, 8, 0.5, None, ptr, None) == -1001
    assert lib.tir_mc_count(ptr, 8, 8, 8, 0.5, ptr, None, None) == -1001
    emit = lambda vol, off, nv, nf, vb, v, n, f: lib.tir_mc_emit(vol, 8, 8, 8, 0.5, 1, 1, 1, 0, 0, 0, off, nv, nf, vb, v, n, f,
                                                                 None)
    assert emit(None, ptr, 4, 4, ptr, ptr, ptr, ptr) == -1001
    assert emit(ptr, None, 4, 4, ptr, ptr, ptr, ptr) == -1001
    assert emit(ptr, ptr, -1, 0, ptr, ptr, ptr, ptr) == -1001
    assert emit(ptr, ptr, 4, 4, None, ptr, ptr, ptr) == -1001
    assert emit(ptr, ptr, 4, 0, ptr, None, ptr, None) == -1001
    assert emit(ptr, ptr, 4, 0, ptr, ptr, None, None) == -1001
    assert emit(ptr, ptr, 4, 4, ptr, ptr, ptr, None) == -1001
    assert emit(ptr, ptr, 0, 4, ptr, ptr, ptr, ptr) == -1001            # faces without vertices
    assert emit(ptr, ptr, 0, 0, None, None, None, None) == 0           # an empty surface: nothing to launch


def test_mc_prototypes_are_declared_and_bound():
    from tensoir_amd import _lib
    for name in ("tir_mc_blocks", "tir_mc_count", "tir_mc_emit"):
        assert name in _lib.SIGNATURES           # derived from include/tensoir_hip.h: bound means declared
    assert _lib.SIGNATURES["tir_mc_blocks"][0] is C.c_int64
