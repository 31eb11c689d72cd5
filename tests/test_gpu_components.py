"""Connected-component filter on the GPU (tir_ccl_*, ops.label_components / keep_components, mesh.extract_mesh / export_mesh
with keep_largest, TensorVMSplit.prune_alpha_mask) against the numpy restatement (tests/components_reference.py), exactly."""
import os

import numpy as np
import pytest
import torch

from tests import components_reference as R
from tests import mesh_reference as MR

pytestmark = pytest.mark.gpu


def device_labels(vol, level, connectivity):
    from tensoir_amd import ops
    labels, table = ops.label_components(torch.from_numpy(vol).cuda(), level, connectivity)
    torch.cuda.synchronize()
    return labels, table


def host(table):
    return {k: v.cpu().numpy() for k, v in table.items()}


def assert_equals_restatement(labels, table, ref_labels):
    ref = R.table(ref_labels)
    got_labels, got = labels.cpu().numpy(), host(table)
    assert got_labels.dtype == np.int32 and got_labels.shape == ref_labels.shape
    assert np.array_equal(got_labels, ref_labels)
    for k in ("roots", "sizes", "boxes"):
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), k
    return ref


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", R.SMALL)
def test_labels_table_and_filter_equal_restatement(name, connectivity):
    from tensoir_amd import ops
    vol, level = R.case(name)
    ref_labels = R.label(vol, level, connectivity)
    labels, table = device_labels(vol, level, connectivity)
    ref = assert_equals_restatement(labels, table, ref_labels)
    K = len(ref["roots"])
    assert all(v.is_cuda for v in table.values()) and table["boxes"].shape == (K, 6)
    # the filter: the largest component alone, and a seeded pattern of flags; removed points become level - 1
    patterns = [R.select(ref, keep_largest=1), np.random.default_rng(K).random(K) < 0.5]
    for flags in patterns:
        fill = level - 1.0
        out = ops.keep_components(torch.from_numpy(vol).cuda(), labels, table, torch.from_numpy(flags), fill=fill, level=level)
        want = R.keep(vol, ref_labels, ref, flags, fill)
        assert out.dtype == torch.float32 and out.shape == labels.shape
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))         # NaNs included, bit for bit


def test_filter_refuses_a_fill_above_the_level():
    from tensoir_amd import ops
    from tensoir_amd._lib import TensoirHipError
    vol, level = R.case("face_diagonal")
    labels, table = device_labels(vol, level, 6)
    with pytest.raises(TensoirHipError):
        ops.keep_components(torch.from_numpy(vol).cuda(), labels, table, torch.ones(2, dtype=torch.bool), fill=0.75, level=level)
    with pytest.raises(ValueError):
        ops.keep_components(torch.from_numpy(vol).cuda(), labels, table, torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.label_components(torch.from_numpy(vol).cuda(), level, 8)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_300_cubed_equals_restatement_and_repeats(connectivity):
    """27 M points, one dominant component and thousands of single-voxel floaters."""
    from tensoir_amd import ops
    vol, level = R.noisy_blob(300)
    ref_labels = R.label(vol, level, connectivity)
    dvol = torch.from_numpy(vol).cuda()
    la, ta = ops.label_components(dvol, level, connectivity)
    ref = assert_equals_restatement(la, ta, ref_labels)
    sizes = np.sort(ref["sizes"])[::-1]
    assert len(sizes) > 1000 and sizes[0] > 1000 * sizes[1]
    flags = R.select(ref, keep_largest=1)
    oa = ops.keep_components(dvol, la, ta, torch.from_numpy(flags), fill=0.0, level=level)
    assert np.array_equal(oa.cpu().numpy().view(np.uint32), R.keep(vol, ref_labels, ref, flags, 0.0).view(np.uint32))
    lb, tb = ops.label_components(dvol, level, connectivity)
    ob = ops.keep_components(dvol, lb, tb, torch.from_numpy(flags), fill=0.0, level=level)
    assert torch.equal(la, lb) and all(torch.equal(ta[k], tb[k]) for k in ta)
    assert torch.equal(oa.view(torch.int32), ob.view(torch.int32))


# ---- the blob scene --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs():
    import tensoir_amd
    model = tensoir_amd.model_from_checkpoint(R.blob_checkpoint(), "cuda:0", envmap_h=4, envmap_w=8)
    model.march_t_stop = 0.0
    return model


def blob_alpha(model):
    from tensoir_amd import ops
    alpha, _ = ops.dense_alpha(model.packed_field(), R.BLOB_GRID, float(model.stepSize))
    return alpha.cpu().numpy()


def export_spacing(model):
    aabb = model.aabb.detach().cpu().float()
    return ((aabb[1] - aabb[0]) / torch.tensor(R.BLOB_GRID, dtype=torch.float32)).numpy(), aabb[0].numpy()


def test_blob_scene_is_what_the_plan_says(blobs):
    alpha = blob_alpha(blobs)
    for c in (6, 26):
        sizes = np.sort(R.table(R.label(alpha, 0.005, c))["sizes"])[::-1]
        assert len(sizes) == len(R.BLOBS) and sizes[0] >= 10 * sizes[1] and sizes[-1] >= 8


def test_export_keep_largest_equals_marching_cubes_of_the_filtered_lattice(blobs, tmp_path):
    from tensoir_amd import mesh
    alpha = blob_alpha(blobs)
    labels = R.label(alpha, 0.005, 6)
    tab = R.table(labels)
    filtered = R.keep(alpha, labels, tab, R.select(tab, keep_largest=1), 0.0)
    sp, origin = export_spacing(blobs)
    rv, rf, _ = MR.marching_cubes(filtered, 0.005, sp, origin)
    path = str(tmp_path / "main.ply")
    nv, nf = mesh.export_mesh(blobs, path, keep_largest=1)
    v, f = mesh.read_ply(path)
    assert (nv, nf) == (len(v), len(f)) == (len(rv), len(rf)) and nf > 100
    assert np.array_equal(f, rf)
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert MR.is_closed_and_oriented(f)
    # the unfiltered export: more surface, and every kept vertex is one of its vertices, bit for bit
    full = str(tmp_path / "full.ply")
    nv0, nf0 = mesh.export_mesh(blobs, full)
    v0, f0 = mesh.read_ply(full)
    assert nv0 > nv and nf0 > nf
    rows = lambda a: set(map(bytes, np.ascontiguousarray(a).view(np.uint8).reshape(len(a), 12)))
    assert rows(v) < rows(v0)
    # min_component_voxels just above the largest floater selects the same mesh; a 26-connectivity run as well (blobs far apart)
    biggest_floater = int(np.sort(tab["sizes"])[-2])
    for kw in (dict(min_component_voxels=biggest_floater + 1), dict(keep_largest=1, connectivity=26),
               dict(keep_largest=3, min_component_voxels=biggest_floater + 1)):
        v2, f2, _ = mesh.extract_mesh(blobs, **kw)
        assert np.array_equal(v2.cpu().numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(f2.cpu().numpy(), rf), kw
    # nothing kept: an empty mesh, as for an empty surface
    v3, f3, n3 = mesh.extract_mesh(blobs, keep_largest=0)
    assert v3.shape == (0, 3) and f3.shape == (0, 3) and n3.shape == (0, 3)
    # keep_largest=2: the main blob and the largest floater (ties to the smaller root), against the restatement again
    filtered2 = R.keep(alpha, labels, tab, R.select(tab, keep_largest=2), 0.0)
    rv2, rf2, _ = MR.marching_cubes(filtered2, 0.005, sp, origin)
    v4, f4, _ = mesh.extract_mesh(blobs, keep_largest=2)
    assert len(rf2) > len(rf)
    assert np.array_equal(v4.cpu().numpy().view(np.uint32), rv2.view(np.uint32)) and np.array_equal(f4.cpu().numpy(), rf2)


def test_options_none_leave_the_export_byte_identical(blobs, tmp_path, monkeypatch):
    """With both options None the path is the one without the feature: same bytes, and no labelling entry is called."""
    from tensoir_amd import mesh, ops
    sp, origin = export_spacing(blobs)
    rv, rf, _ = MR.marching_cubes(blob_alpha(blobs), 0.005, sp, origin)
    plain = str(tmp_path / "plain.ply")
    mesh.write_ply(plain, rv, rf)                     # what export_mesh wrote before it had the options (test_gpu_mesh.py pins that)

    def refuse(*a, **k):
        raise AssertionError("a labelling call without a component option")
    monkeypatch.setattr(ops, "label_components", refuse)
    monkeypatch.setattr(ops, "keep_components", refuse)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    mesh.export_mesh(blobs, a)
    mesh.export_mesh(blobs, b, keep_largest=None, min_component_voxels=None, connectivity=26)
    assert open(a, "rb").read() == open(b, "rb").read() == open(plain, "rb").read()


def test_attributes_with_keep_largest(blobs, tmp_path):
    from tensoir_amd import mesh
    plain, baked = str(tmp_path / "p.ply"), str(tmp_path / "b.ply")
    nv, nf = mesh.export_mesh(blobs, plain, keep_largest=1)
    report = {}
    nv2, nf2 = mesh.export_mesh(blobs, baked, attributes=True, keep_largest=1, report=report)
    v, f = mesh.read_ply(plain)
    bv, bf, attrs = mesh.read_ply_attributes(baked)
    assert (nv2, nf2) == (nv, nf) == (len(bv), len(bf))
    assert np.array_equal(bv.view(np.uint32), v.view(np.uint32)) and np.array_equal(bf, f)
    assert set(attrs) == {n for n, _ in mesh.ATTRIBUTE_LAYOUT[3:]} and all(len(a) == nv for a in attrs.values())
    assert int(report["kept"].sum()) == 1 and report["kept"].numel() == len(R.BLOBS)


def test_components_lists_the_blobs_in_world_coordinates(blobs):
    from tensoir_amd import mesh
    t = mesh.components(blobs)
    K = len(R.BLOBS)
    assert t["roots"].shape == (K,) and t["boxes_world"].shape == (K, 2, 3)
    lo, hi = t["boxes_world"][:, 0].cpu().numpy(), t["boxes_world"][:, 1].cpu().numpy()
    centres = R.blob_centres_world()
    for c in centres:                                  # every blob centre lies in exactly one box
        assert int(((lo <= c) & (c <= hi)).all(1).sum()) == 1
    ref = R.table(R.label(blob_alpha(blobs), 0.005, 6))
    assert np.array_equal(t["boxes"].cpu().numpy(), ref["boxes"]) and np.array_equal(t["sizes"].cpu().numpy(), ref["sizes"])


# ---- the occupancy mask ----------------------------------------------------------------------------------------------------
def rays_down_z(xy):
    """Axis-parallel rays from z = 4 toward -z through the world points xy [n, 2]."""
    n = len(xy)
    o = np.concatenate([np.asarray(xy, np.float32), np.full((n, 1), 4.0, np.float32)], 1)
    d = np.tile(np.float32([0, 0, -1]), (n, 1))
    return torch.from_numpy(np.concatenate([o, d], 1)).cuda()


def render(model, rays):
    lidx = torch.zeros((rays.shape[0], 1), dtype=torch.int32, device="cuda")
    noise = torch.randn(rays.shape[0], model.nSamples, 3, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        out, maps = model(rays, lidx, _brdf_jitter_dense=noise, _return_maps=True)
    torch.cuda.synchronize()
    return out, maps


def test_prune_alpha_mask(tmp_path):
    import tensoir_amd
    from tensoir_amd import ops
    from tensoir_amd._lib import TensoirHipError
    model = tensoir_amd.model_from_checkpoint(R.blob_checkpoint(), "cuda:0", envmap_h=4, envmap_w=8)
    model.march_t_stop = 0.0
    with pytest.raises(TensoirHipError):
        model.prune_alpha_mask(keep_largest=1)                                  # no mask yet
    model.updateAlphaMask(R.BLOB_GRID)
    old_mask = model.alphaMask
    old = old_mask.alpha_volume.reshape(old_mask.alpha_volume.shape[-3:]).cpu().numpy().astype(np.float32)
    ref_labels = R.label(old, 0.5, 26)
    ref = R.table(ref_labels)
    assert len(ref["roots"]) == len(R.BLOBS)                                    # the dilated blobs are still apart
    flags = R.select(ref, keep_largest=1)
    want = R.keep(old, ref_labels, ref, flags, 0.0)
    removed = (old > 0.5) & ~(want > 0.5)
    assert removed.any() and (want > 0.5).any()

    centres = R.blob_centres_world()
    main, floaters = centres[:1], centres[1:]
    cpts = torch.from_numpy(centres).cuda()
    assert ops.occupancy_query(model.packed_field(), cpts).cpu().tolist() == [1] * len(centres)
    # rays: one through every floater centre; a 5 x 5 bundle through the main blob whose columns of mask voxels stay at
    # least two voxels (in x and y) from every removed voxel
    f_rays = rays_down_z(floaters[:, :2])
    aabb = np.float32(R.BLOB_AABB)
    cell = (aabb[1] - aabb[0]) / (np.float32(R.BLOB_GRID) - 1)
    offs = np.stack(np.meshgrid(np.linspace(-0.15, 0.15, 5), np.linspace(-0.15, 0.15, 5)), -1).reshape(-1, 2).astype(np.float32)
    m_xy = main[0, :2] + offs
    rz, ry, rx = np.nonzero(removed)                                            # the volume is stored [gz, gy, gx]
    rem_xy = aabb[0, :2] + np.stack([rx, ry], 1) * cell[:2]
    gap = np.abs(m_xy[:, None, :] - rem_xy[None, :, :]) / cell[:2]
    assert float(gap.max(-1).min()) >= 2.0 + 1.0                                # two voxels beyond the lookup's own one-cell reach
    m_rays = rays_down_z(m_xy)
    before_f, before_m = render(model, f_rays), render(model, m_rays)
    assert float(before_f[0][6].min()) > 0.5 and float(before_m[0][6].min()) > 0.5          # acc_map: all of them hit something

    table = model.prune_alpha_mask(keep_largest=1)
    assert model.alphaMask is not old_mask
    new = model.alphaMask.alpha_volume
    assert new.shape == old_mask.alpha_volume.shape and new.dtype == old_mask.alpha_volume.dtype
    assert torch.equal(model.alphaMask.aabb, old_mask.aabb)
    got = new.reshape(new.shape[-3:]).cpu().numpy().astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(table["kept"].cpu().numpy(), flags) and np.array_equal(table["sizes"].cpu().numpy(), ref["sizes"])
    assert np.array_equal(table["roots"].cpu().numpy(), ref["roots"]) and np.array_equal(table["boxes"].cpu().numpy(), ref["boxes"])
    assert ops.occupancy_query(model.packed_field(), cpts).cpu().tolist() == [1] + [0] * len(floaters)

    after_f, after_m = render(model, f_rays), render(model, m_rays)
    assert float(after_f[0][6].abs().max()) == 0.0                              # exactly nothing left on the floater rays
    assert torch.equal(before_m[1].view(torch.int32), after_m[1].view(torch.int32))         # every map of the pass, bit for bit
    for a, b in zip(before_m[0], after_m[0]):
        if torch.is_tensor(a):
            assert torch.equal(a, b)

    # save / load keeps the pruned mask
    path = str(tmp_path / "pruned.th")
    model.save(path)
    ck = torch.load(path, weights_only=False)
    again = tensoir_amd.model_from_checkpoint(ck, "cuda:0", envmap_h=4, envmap_w=8)
    assert torch.equal(again.alphaMask.alpha_volume.bool(), model.alphaMask.alpha_volume.bool())
    assert ops.occupancy_query(again.packed_field(), cpts).cpu().tolist() == [1] + [0] * len(floaters)

    with pytest.raises(TensoirHipError):
        model.prune_alpha_mask(keep_largest=0)                                  # nothing would be kept: the mask stays
    with pytest.raises(TensoirHipError):
        model.prune_alpha_mask(min_voxels=10 ** 9)
    with pytest.raises(ValueError):
        model.prune_alpha_mask(keep_largest=-2)
    assert np.array_equal(model.alphaMask.alpha_volume.reshape(got.shape).cpu().numpy().astype(np.float32), want)


# ---- the trained fixture ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    from tests.train_sequence import reconstruct
    return reconstruct()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_trained_field_300_cubed_equals_restatement(trained, connectivity):
    from tensoir_amd import ops
    m = trained.model
    alpha, _ = ops.dense_alpha(m.packed_field(), [300, 300, 300], float(m.stepSize))
    labels, table = ops.label_components(alpha, 0.005, connectivity)
    ref = assert_equals_restatement(labels, table, R.label(alpha.cpu().numpy(), 0.005, connectivity))
    print(f"trained 300^3 lattice, connectivity {connectivity}: {len(ref['roots'])} components, largest {ref['sizes'].max(initial=0)}")
