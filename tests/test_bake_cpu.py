"""What the per-vertex bake can check without a GPU: the PLY vertex attributes, the file-to-field coordinate map, and the
qualification of the GPU tests' point sets (tests/bake_cases.py) by the restatement itself, fp32 against fp64."""
import numpy as np
import pytest
import torch

from tests import bake_cases as BC
from tests import bake_reference as BR

TOL = 1e-4                       # the GPU tests' bound (tests/test_gpu_bake.py); a point set qualifies at half of it
# ... and keeps this distance from the two discontinuities that move an output by more than TOL: no sample weight within MARGIN
# (relative) of rayMarch_weight_thres, no coverage within MARGIN of 0.5.  The figure is the restatement's own error: its fp32 weights
# differ from its fp64 weights by up to 3.4e-4 (relative) among the samples within 5 % of the threshold (measured over the six
# sets), so a sample closer than that falls on either side in fp32 arithmetic; three times that, rounded.
MARGIN = 1e-3
OUTPUTS = ("albedo", "roughness", "normal", "coverage", "surface", "ao", "irradiance")


def rel(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).abs() / b.abs().clamp(min=1.0)).max()) if a.numel() else 0.0


# ---- PLY ---------------------------------------------------------------------------------------------------------------------
def _attribute_vertices(n, seed=3):
    from tensoir_amd import mesh
    rng = np.random.default_rng(seed)
    v = np.empty(n, dtype=mesh.ATTRIBUTE_LAYOUT)
    for name, t in mesh.ATTRIBUTE_LAYOUT:
        v[name] = rng.integers(0, 256, n) if t == "u1" else rng.standard_normal(n).astype(np.float32)
    return v


def test_ply_attributes_round_trip(tmp_path):
    from tensoir_amd import mesh
    v = _attribute_vertices(37)
    f = np.empty(11, dtype=[("vertex_indices", "i4", (3,))])
    f["vertex_indices"] = np.random.default_rng(4).integers(0, 37, (11, 3))
    path = str(tmp_path / "a.ply")
    mesh.write_elements(path, [("vertex", v), ("face", f)])
    header = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii").split("\n")
    want = (["ply", "format binary_little_endian 1.0", "element vertex 37"] +
            [f"property float {n}" for n in ("x", "y", "z", "nx", "ny", "nz")] +
            [f"property uchar {n}" for n in ("red", "green", "blue")] +
            [f"property float {n}" for n in ("roughness", "ao", "coverage", "albedo_r", "albedo_g", "albedo_b", "irradiance_r",
                                             "irradiance_g", "irradiance_b")] +
            ["element face 11", "property list uchar int vertex_indices", ""])
    assert header == want
    verts, faces, attrs = mesh.read_ply_attributes(path)
    assert verts.dtype == np.float32 and faces.dtype == np.int32
    assert np.array_equal(verts.view(np.uint32), np.stack([v["x"], v["y"], v["z"]], 1).view(np.uint32))
    assert np.array_equal(faces, f["vertex_indices"])
    assert list(attrs) == [n for n, _ in mesh.ATTRIBUTE_LAYOUT[3:]]
    for name, t in mesh.ATTRIBUTE_LAYOUT[3:]:
        assert attrs[name].dtype == np.dtype(t), name
        assert np.array_equal(attrs[name].view(np.uint32 if t == "f4" else np.uint8), v[name].view(np.uint32 if t == "f4" else np.uint8)), name


def test_plain_ply_reads_both_ways(tmp_path):
    from tensoir_amd import mesh
    rng = np.random.default_rng(5)
    verts = rng.standard_normal((20, 3)).astype(np.float32)
    faces = rng.integers(0, 20, (9, 3)).astype(np.int32)
    path = str(tmp_path / "p.ply")
    mesh.write_ply(path, verts, faces)
    v, f = mesh.read_ply(path)
    assert np.array_equal(v, verts) and np.array_equal(f, faces)
    v2, f2, attrs = mesh.read_ply_attributes(path)
    assert np.array_equal(v2, verts) and np.array_equal(f2, faces) and attrs == {}
    mesh.write_ply(path, verts[:0], faces[:0])                     # an empty surface
    v3, f3, attrs = mesh.read_ply_attributes(path)
    assert v3.shape == (0, 3) and f3.shape == (0, 3) and attrs == {}


def test_vertex_colors():
    from tensoir_amd import mesh
    a = torch.tensor([[0.0, 0.5, 1.0], [0.002, 0.2, 2.0]])
    got = mesh.vertex_colors(a).numpy()
    x = a.double().clamp(0, 1).numpy()
    srgb = np.where(x <= 0.0031308, x * 12.92, 1.055 * np.power(x + 1e-6, 1 / 2.4) - 0.055)
    assert got.dtype == np.uint8 and np.abs(got - 255 * srgb).max() <= 0.5 + 1e-3
    irr = torch.full((2, 3), np.pi)
    assert np.array_equal(mesh.vertex_colors(a, irr, "diffuse").numpy(), got)
    with pytest.raises(ValueError):
        mesh.vertex_colors(a, None, "diffuse")
    with pytest.raises(ValueError):
        mesh.vertex_colors(a, irr, "specular")


# ---- file coordinates -> field coordinates -------------------------------------------------------------------------------------
def test_field_positions_undo_the_voxel_size_quirk():
    from tensoir_amd import mesh
    aabb = torch.tensor([[-1.5, -1.4, -1.3], [1.5, 1.4, 1.6]])
    grid = [20, 24, 28]
    g = torch.tensor(grid, dtype=torch.float64)
    idx = torch.stack(torch.meshgrid([torch.arange(0, n, 3) for n in grid], indexing="ij"), -1).reshape(-1, 3).double()
    idx = torch.cat([idx, g[None] - 1])                           # incl. the far corner
    size = (aabb[1] - aabb[0]).double()
    written = (aabb[0].double() + idx * size / g).float()          # where export_mesh puts lattice point idx
    true = aabb[0].double() + idx * size / (g - 1)                 # where getDenseAlpha sampled it
    pos = mesh.field_positions(aabb, grid, written)
    assert pos.dtype == torch.float32 and pos.shape == written.shape
    ulp = float(size.max()) * 2.0 ** -23
    assert float((pos.double() - true).abs().max()) <= 4 * ulp
    # normals: index space -> world
    n_idx = torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, 1.0], [0.6, 0.0, 0.8], [1.0, 1.0, 1.0]])
    n_idx = n_idx / n_idx.norm(dim=-1, keepdim=True)
    pos2, n_w = mesh.field_positions(aabb, grid, written[:5], n_idx)
    assert torch.equal(pos2, pos[:5])
    assert torch.allclose(n_w[:3], n_idx[:3], atol=1e-7)
    want = n_idx.double() / (size / (g - 1))
    want = want / want.norm(dim=-1, keepdim=True)
    assert float((n_w.double() - want).abs().max()) <= 1e-6
    assert float((n_w.norm(dim=-1) - 1).abs().max()) <= 1e-6
    assert not torch.allclose(n_w[3], n_idx[3], atol=1e-3)         # the axes' spacings differ: an oblique normal turns


# ---- the restatement against itself: which point sets the GPU tests may use -----------------------------------------------------

@pytest.mark.parametrize("name", BC.CASES)
def test_point_set_qualifies(name):
    """The threshold tests of the bake (w > weight_thres, cos > 1e-6, coverage > 0.5, in the box, occupied) are discontinuous: a
    point set is admissible for the GPU parity tests only if the restatement in fp32 stays within half their bound of the
    restatement in fp64 on every output of every point, and keeps MARGIN from the weight and coverage thresholds.  A set that
    does not qualify gets another seed in tests/bake_cases.py.
    Measured (max over all points of |fp32 - fp64| / max(|fp64|, 1); limit 5e-5), largest figure per set: golden 1.2e-5, a16 2.0e-5,
    a96 1.9e-5, purely_derived 3.0e-5 (normal), residue_prediction 1.8e-5, general 2.4e-5 -- `surface` everywhere else: the origin
    p + 16 s n carries the fp32 rounding of the step s; albedo and roughness stay below 3e-7, coverage below 4e-6, ao and
    irradiance below 1.3e-5.  No sample count differs between the two precisions."""
    c = BC.case(name)
    r64 = BR.bake(c.scene, c.points, c.outward, c.light_idx, dtype=torch.float64)
    r32 = BR.bake(c.scene, c.points, c.outward, c.light_idx, dtype=torch.float32)
    errs = {k: rel(r32[k], r64[k]) for k in OUTPUTS}
    covered = int((r64["coverage"] > 0.5).sum())
    print(f"\n[bake qualify] {name}: points {c.points.shape[0]} covered {covered} records {int(r64['records'].sum())} "
          f"pairs {r64['pairs']} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    flips = int((r32["records"] != r64["records"]).sum())
    print(f"[bake qualify] {name}: points whose record count differs between fp32 and fp64: {flips}; pairs fp32 {r32['pairs']}")
    print(f"[bake qualify] {name}: closest sample to the weight threshold {r64['margin_w']:.2e} (relative), closest coverage to 0.5 "
          f"{r64['margin_coverage']:.2e}")
    assert covered >= c.points.shape[0] // 8, "the point set hardly touches a surface"
    assert r64["margin_w"] >= MARGIN and r64["margin_coverage"] >= MARGIN
    for k, v in errs.items():
        assert v <= TOL / 2, (k, v)
    if name == "golden":
        e = c.empty
        assert c.n_surface >= 40 and float(r64["coverage"][:c.n_surface].min()) > 0.5
        assert float(r64["coverage"][e].abs().max()) == 0.0 and float(r32["coverage"][e].abs().max()) == 0.0
        assert torch.equal(r64["normal"][e], c.outward[e].double()) and float((r64["ao"][e] - 1).abs().max()) == 0.0
        assert float(r64["irradiance"][e].abs().max()) == 0.0
