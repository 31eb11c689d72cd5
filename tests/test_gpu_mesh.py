"""Marching-cubes mesh export on the GPU (tir_mc_*, ops.marching_cubes, tensoir_amd.mesh, the skimage / plyfile stand-ins):
the kernels against the numpy restatement (tests/mesh_reference.py) exactly, and against scikit-image's recorded output
(tests/golden/mesh_skimage.npz) by the fixture criteria."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "mesh_skimage.npz"))
CASES = [str(c) for c in G["cases"]]


def case(name):
    p = name + "/"
    return G[p + "vol"], float(G[p + "level"]), G[p + "spacing"]


def kernel(vol, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    from tensoir_amd import ops
    v, f, n = ops.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), level, spacing, origin)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()


def assert_matches_restatement(got, ref):
    v, f, n = got
    rv, rf, rn = ref
    assert v.shape == rv.shape and f.shape == rf.shape and n.shape == rn.shape
    assert f.dtype == np.int32 and v.dtype == np.float32 and n.dtype == np.float32
    assert np.array_equal(f, rf)
    np.testing.assert_array_max_ulp(v, rv, maxulp=1)
    assert np.abs(n - rn).max(initial=0.0) <= 1e-5


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_restatement(name):
    vol, level, sp = case(name)
    origin = (-0.25, 0.5, 1.0)
    got = kernel(vol, level, sp, origin)
    ref = R.marching_cubes(vol, level, sp, origin)
    assert_matches_restatement(got, ref)
    # bit-identical positions are what the rounding rule promises
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_skimage(name):
    vol, level, sp = case(name)
    v, f, n = kernel(vol, level, sp)
    p = name + "/"
    sv, sf, sn = G[p + "verts"], G[p + "faces"], G[p + "normals"]
    ext = float((np.array(vol.shape) * sp).max())
    assert len(v) == len(sv) == R.n_crossing_edges(vol, level)
    assert np.abs(R.sorted_rows(v) - R.sorted_rows(sv)).max() <= 1e-6 * ext
    assert abs(R.area(v, f) / R.area(sv, sf) - 1) < 0.01
    if name in ("blob", "onlevel"):
        assert R.is_closed_and_oriented(f)
    if name == "blob":
        vol_ours, vol_sk = R.signed_volume(v, f), R.signed_volume(sv, sf)
        assert vol_ours > 0 > vol_sk                       # outward here, inward with scikit-image's winding
        assert abs(vol_ours / -vol_sk - 1) < 0.005
        # normals: match vertices through their lattice edge
        order = np.argsort(R.edge_keys(sv, sp, vol.shape))
        cos = (n * sn[order]).sum(1)
        assert np.array_equal(np.sort(R.edge_keys(sv, sp, vol.shape)), R.crossing_keys(vol, level))
        assert np.median(cos) >= 0.99 and cos.min() >= 0.9, (np.median(cos), cos.min())


def test_two_calls_are_bit_identical():
    vol, level, sp = case("alpha")
    a, b = kernel(vol, level, sp), kernel(vol, level, sp)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("fill", ["zeros", "inside", "outside", "level"])
def test_empty_surfaces(fill):
    vol = {"zeros": np.zeros((9, 7, 5), np.float32), "inside": np.full((9, 7, 5), 2.0, np.float32),
           "outside": np.full((9, 7, 5), -2.0, np.float32), "level": np.full((9, 7, 5), 0.5, np.float32)}[fill]
    level = 0.0 if fill == "zeros" else 0.5
    v, f, n = kernel(vol, level)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)


def test_rejects_bad_lattices():
    from tensoir_amd import ops
    from tensoir_amd._lib import TensoirHipError
    with pytest.raises(TensoirHipError):
        ops.marching_cubes(torch.zeros((1, 8, 8), device="cuda"), 0.5)
    with pytest.raises(ValueError):
        ops.marching_cubes(torch.zeros((8, 8), device="cuda"), 0.5)


def noisy_blob_300():
    g = torch.Generator().manual_seed(7)
    ax = torch.linspace(-1, 1, 300)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v = 1 - (x * x / 0.5 + y * y / 0.4 + z * z / 0.6) + 0.05 * torch.rand((300, 300, 300), generator=g)
    return v.float().numpy()


def test_300_cubed_lattice_equals_restatement():
    """27 M points = 6.6 K blocks: the multi-block offsets at the final grid size of a scene."""
    vol = noisy_blob_300()
    sp = np.float32([3 / 300, 3 / 300, 3 / 300])
    got = kernel(vol, 0.3, sp, (-1.5, -1.5, -1.5))
    ref = R.marching_cubes(vol, 0.3, sp, (-1.5, -1.5, -1.5))
    assert len(got[0]) > 100000
    assert_matches_restatement(got, ref)


@pytest.fixture(scope="module")
def trained():
    from tests.train_sequence import reconstruct
    return reconstruct()


def test_trained_field_300_cubed_equals_restatement(trained):
    from tensoir_amd import ops
    m = trained.model
    alpha, _ = ops.dense_alpha(m.packed_field(), [300, 300, 300], float(m.stepSize))
    vol = alpha.cpu().numpy()
    got = kernel(vol, 0.005, (0.01, 0.01, 0.01))
    ref = R.marching_cubes(vol, 0.005, (0.01, 0.01, 0.01))
    assert len(got[1]) > 1000
    assert_matches_restatement(got, ref)


def test_export_mesh_on_trained_checkpoint(trained, tmp_path):
    from tensoir_amd import mesh, ops
    m = trained.model
    path = str(tmp_path / "scene.ply")
    nv, nf = mesh.export_mesh(m, path)
    v, f = mesh.read_ply(path)
    assert (len(v), len(f)) == (nv, nf) and nf > 0
    grid = [int(g) for g in m.gridSize]
    alpha, _ = ops.dense_alpha(m.packed_field(), grid, float(m.stepSize))
    aabb = m.aabb.detach().cpu().float()
    # the reference's transform (utils.py:186-197): voxel size (aabb1 - aabb0) / shape, origin aabb0, outward faces
    sp = ((aabb[1] - aabb[0]) / torch.tensor(grid, dtype=torch.float32)).numpy()
    rv, rf, _ = R.marching_cubes(alpha.cpu().numpy(), 0.005, sp, aabb[0].numpy())
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(f, rf)


def test_skimage_stand_in_as_the_reference_calls_it():
    """convert_sdf_samples_to_ply: marching_cubes(numpy volume, level=..., spacing=list of 0-d float32 tensors)."""
    from tensoir_amd import shims
    shims.install()
    import skimage.measure
    if not getattr(skimage.measure, "__tensoir_shim__", False):
        pytest.skip("the real scikit-image is installed: the stand-in is not used")
    for name in CASES:
        vol, level, sp = case(name)
        spacing = list(torch.from_numpy(sp))
        verts, faces, normals, values = skimage.measure.marching_cubes(vol, level=level, spacing=spacing)
        want = [str(d) for d in G[name + "/dtypes"]]
        assert [verts.dtype.str, faces.dtype.str, normals.dtype.str, values.dtype.str] == want, name
        rv, rf, rn = R.marching_cubes(vol, level, sp)
        assert np.array_equal(faces, rf[:, ::-1])            # scikit-image's (inward) winding
        np.testing.assert_array_max_ulp(verts, rv, maxulp=1)
        assert np.abs(normals - rn).max(initial=0.0) <= 1e-5
        assert (values == np.float32(level)).all()
