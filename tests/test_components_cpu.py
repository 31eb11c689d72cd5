"""Connected-component filter, the part that needs no GPU: the numpy restatement (tests/components_reference.py) against
scipy.ndimage.label, the non-vacuity of the GPU tests' volumes, mesh.select_components, and the argument validation of the
tir_ccl_* entries through the built library."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import components_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def n_components(vol, level, connectivity):
    return len(R.table(R.label(vol, level, connectivity))["roots"])


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", R.SMALL)
def test_restatement_equals_scipy(name, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    vol, level = R.case(name)
    labels = R.label(vol, level, connectivity)
    tab = R.table(labels)
    structure = ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    theirs, k = ndi.label(R.inside(vol, level), structure=structure)
    assert k == len(tab["roots"])
    assert np.array_equal(theirs > 0, labels >= 0)
    # equal up to renaming: the pairs (our label, their label) are a bijection
    ins = labels >= 0
    pairs = np.unique(np.stack([labels[ins], theirs[ins]], 1), axis=0)
    assert len(pairs) == k and len(np.unique(pairs[:, 0])) == k and len(np.unique(pairs[:, 1])) == k
    # sizes and boxes exactly, matched through the renaming
    theirs_of = dict(pairs.tolist())
    sizes = np.bincount(theirs.reshape(-1), minlength=k + 1)
    slices = ndi.find_objects(theirs)
    for row, root in enumerate(tab["roots"].tolist()):
        t = theirs_of[root]
        assert tab["sizes"][row] == sizes[t]
        box = [s.start for s in slices[t - 1]] + [s.stop - 1 for s in slices[t - 1]]
        assert tab["boxes"][row].tolist() == box


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", R.SMALL)
def test_restatement_labels_are_canonical(name, connectivity):
    vol, level = R.case(name)
    labels = R.label(vol, level, connectivity)
    assert labels.dtype == np.int32 and labels.shape == vol.shape
    assert np.array_equal(labels >= 0, R.inside(vol, level)) and (labels[labels < 0] == -1).all()
    flat = labels.reshape(-1)
    idx = np.flatnonzero(flat >= 0)
    if len(idx):
        order = np.argsort(flat[idx], kind="stable")
        firsts = idx[order][np.r_[True, np.diff(flat[idx][order]) != 0]]      # smallest index of every label's set
        assert np.array_equal(firsts, np.unique(flat[idx]))
    tab = R.table(labels)
    assert np.array_equal(tab["roots"], np.flatnonzero(flat == np.arange(flat.size)))
    assert int(tab["sizes"].sum()) == len(idx)


def test_nan_is_outside():
    vol, level = R.case("nans")
    assert np.isnan(vol).sum() > 50
    for c in (6, 26):
        assert (R.label(vol, level, c)[np.isnan(vol)] == -1).all()


def test_restatement_filter():
    vol, level = R.case("nans")
    labels = R.label(vol, level, 6)
    tab = R.table(labels)
    flags = R.select(tab, keep_largest=1)
    out = R.keep(vol, labels, tab, flags, fill=0.25)
    big = tab["roots"][np.argmax(tab["sizes"])]
    assert np.array_equal(out[labels == big].view(np.uint32), vol[labels == big].view(np.uint32))
    assert (out[(labels >= 0) & (labels != big)] == np.float32(0.25)).all()
    assert np.array_equal(out[labels < 0].view(np.uint32), vol[labels < 0].view(np.uint32))          # NaNs included, bit for bit
    assert len(R.table(R.label(out, level, 6))["roots"]) == 1


# ---- non-vacuity of the GPU tests, on the reference alone ------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SMALL)
def test_cases_hold_what_their_descriptions_say(name):
    _, want6, want26 = R.CASES[name]
    vol, level = R.case(name)
    k6, k26 = n_components(vol, level, 6), n_components(vol, level, 26)
    assert k26 <= k6
    if want6 is not None:
        assert (k6, k26) == (want6, want26)
    if name == "smooth_noise":
        assert vol.shape == (37, 50, 91) and 200 <= k26 <= k6 <= 999                # "a few hundred", no axis a tile multiple
    if name == "nans":
        assert k6 > k26 > 1
    if name == "serpentine":
        assert vol.shape == (48, 48, 48) and int(vol.sum()) > 24 * 24 * 48          # every other row, all of it on the path
        # one voxel wide: apart from the two ends, every path voxel has exactly two face neighbours on the path
        p = np.pad(vol, 1)
        nb = sum(np.roll(p, s, a) for a in range(3) for s in (-1, 1))[1:-1, 1:-1, 1:-1]
        assert sorted(np.unique(nb[vol > 0]).tolist()) == [1.0, 2.0] and int((nb[vol > 0] == 1).sum()) == 2
    if name == "checkerboard":
        assert vol.shape == (17, 18, 19) and k6 == int(vol.sum())


def test_noisy_blob_recipe_at_64():
    vol, level = R.noisy_blob(64, speck_rate=4e-3)
    for c in (6, 26):
        tab = R.table(R.label(vol, level, c))
        sizes = np.sort(tab["sizes"])[::-1]
        assert len(sizes) > 200 and sizes[0] > 10000 and sizes[0] > 100 * sizes[1]


def test_blob_scene_plan():
    alpha = R.blob_alpha_planned()
    assert list(alpha.shape) == R.BLOB_GRID
    for c in (6, 26):
        tab = R.table(R.label(alpha, 0.005, c))
        sizes = np.sort(tab["sizes"])[::-1]
        assert len(sizes) == len(R.BLOBS) == 6
        assert sizes[0] >= 10 * sizes[1] and sizes[-1] >= 8
    # every blob's peak is opaque, the space between them empty
    assert float(alpha.max()) > 0.99 and float(np.median(alpha)) < 1e-4


# ---- mesh.select_components ------------------------------------------------------------------------------------------------
def _table(sizes):
    k = len(sizes)
    return {"roots": torch.arange(k, dtype=torch.int32) * 7, "sizes": torch.tensor(sizes, dtype=torch.int32),
            "boxes": torch.zeros((k, 6), dtype=torch.int32)}


def test_select_components():
    from tensoir_amd import mesh
    t = _table([5, 90, 5, 90, 1, 12])
    sel = lambda **kw: mesh.select_components(t, **kw).tolist()
    assert sel() == [True] * 6
    assert sel(keep_largest=1) == [False, True, False, False, False, False]                # the tie goes to the smaller root
    assert sel(keep_largest=2) == [False, True, False, True, False, False]
    assert sel(keep_largest=4) == [True, True, False, True, False, True]                   # 90, 90, 12, then the first 5
    assert sel(keep_largest=0) == [False] * 6
    assert sel(keep_largest=99) == [True] * 6
    assert sel(min_voxels=5) == [True, True, True, True, False, True]
    assert sel(min_voxels=91) == [False] * 6
    assert sel(keep_largest=4, min_voxels=12) == [False, True, False, True, False, True]   # both must hold
    assert sel(keep_largest=1, min_voxels=91) == [False] * 6
    out = mesh.select_components(t, keep_largest=1)
    assert out.dtype == torch.bool and out.shape == (6,)
    assert mesh.select_components(_table([]), keep_largest=3).shape == (0,)
    for kw in (dict(keep_largest=2), dict(min_voxels=6), dict(keep_largest=3, min_voxels=5)):
        ref = R.select({k: v.numpy() for k, v in t.items()}, **kw)
        assert sel(**kw) == ref.tolist()


@pytest.mark.parametrize("kw", [dict(keep_largest=-1), dict(min_voxels=-3), dict(keep_largest=1.5), dict(min_voxels="4"),
                                dict(keep_largest=True)])
def test_select_components_rejects(kw):
    from tensoir_amd import mesh
    with pytest.raises(ValueError):
        mesh.select_components(_table([3, 4]), **kw)


def test_extract_mesh_rejects_bad_options_before_the_device():
    """The model is never touched: a stand-in without a single attribute would raise AttributeError first otherwise."""
    from tensoir_amd import mesh
    for kw in (dict(keep_largest=-1), dict(min_component_voxels=-1), dict(keep_largest=1, connectivity=8)):
        with pytest.raises(ValueError):
            mesh.extract_mesh(object(), **kw)
        with pytest.raises(ValueError):
            mesh.export_mesh(object(), "unused.ply", **kw)


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_ccl_entries_validate_before_any_device_work(lib):
    keep = torch.zeros(64, dtype=torch.float32)                       # a non-null host address: never dereferenced
    ptr = keep.data_ptr()
    assert lib.tir_version() == 100
    assert lib.tir_ccl_blocks(300, 300, 300) == (300 ** 3 + 4095) // 4096
    assert lib.tir_ccl_blocks(1, 1, 1) == 1
    assert lib.tir_ccl_blocks(0, 8, 8) == -1001
    assert lib.tir_ccl_blocks(2048, 2048, 2048) == -1002
    # label
    assert lib.tir_ccl_label(None, 8, 8, 8, 0.5, 6, ptr, ptr, ptr, None) == -1001
    assert lib.tir_ccl_label(ptr, 8, 8, 8, 0.5, 6, None, ptr, ptr, None) == -1001
    assert lib.tir_ccl_label(ptr, 8, 8, 8, 0.5, 6, ptr, None, ptr, None) == -1001
    assert lib.tir_ccl_label(ptr, 8, 8, 8, 0.5, 6, ptr, ptr, None, None) == -1001
    assert lib.tir_ccl_label(ptr, 8, 8, 8, 0.5, 8, ptr, ptr, ptr, None) == -1001            # connectivity 8
    assert lib.tir_ccl_label(ptr, 8, 8, 8, 0.5, 18, ptr, ptr, ptr, None) == -1001
    assert lib.tir_ccl_label(ptr, 8, 0, 8, 0.5, 6, ptr, ptr, ptr, None) == -1001            # a zero dimension
    assert lib.tir_ccl_label(ptr, 8, 8, -1, 0.5, 26, ptr, ptr, ptr, None) == -1001
    assert lib.tir_ccl_label(ptr, 2048, 2048, 2048, 0.5, 6, ptr, ptr, ptr, None) == -1002
    # table
    assert lib.tir_ccl_table(None, 8, 8, 8, ptr, 3, ptr, ptr, ptr, None) == -1001
    assert lib.tir_ccl_table(ptr, 8, 8, 8, None, 3, ptr, ptr, ptr, None) == -1001
    assert lib.tir_ccl_table(ptr, 8, 8, 8, ptr, 3, None, ptr, ptr, None) == -1001
    assert lib.tir_ccl_table(ptr, 8, 8, 8, ptr, 3, ptr, None, ptr, None) == -1001
    assert lib.tir_ccl_table(ptr, 8, 8, 8, ptr, 3, ptr, ptr, None, None) == -1001
    assert lib.tir_ccl_table(ptr, 8, 8, 8, ptr, -1, ptr, ptr, ptr, None) == -1001
    assert lib.tir_ccl_table(ptr, 0, 8, 8, ptr, 3, ptr, ptr, ptr, None) == -1001
    assert lib.tir_ccl_table(ptr, 2048, 2048, 2048, ptr, 3, ptr, ptr, ptr, None) == -1002
    assert lib.tir_ccl_table(ptr, 8, 8, 8, ptr, 0, None, None, None, None) == 0             # no component: nothing to do
    # filter
    assert lib.tir_ccl_filter(None, ptr, 8, 8, 8, 0.5, ptr, ptr, 3, 0.0, ptr, None) == -1001
    assert lib.tir_ccl_filter(ptr, None, 8, 8, 8, 0.5, ptr, ptr, 3, 0.0, ptr, None) == -1001
    assert lib.tir_ccl_filter(ptr, ptr, 8, 8, 8, 0.5, None, ptr, 3, 0.0, ptr, None) == -1001
    assert lib.tir_ccl_filter(ptr, ptr, 8, 8, 8, 0.5, ptr, None, 3, 0.0, ptr, None) == -1001
    assert lib.tir_ccl_filter(ptr, ptr, 8, 8, 8, 0.5, ptr, ptr, 3, 0.0, None, None) == -1001
    assert lib.tir_ccl_filter(ptr, ptr, 8, 8, 8, 0.5, ptr, ptr, 3, 0.75, ptr, None) == -1001   # fill > level
    assert lib.tir_ccl_filter(ptr, ptr, 8, 8, 8, 0.5, ptr, ptr, 3, float("nan"), ptr, None) == -1001
    assert lib.tir_ccl_filter(ptr, ptr, 8, 8, 0, 0.5, ptr, ptr, 3, 0.0, ptr, None) == -1001
    assert lib.tir_ccl_filter(ptr, ptr, 2048, 2048, 2048, 0.5, ptr, ptr, 3, 0.0, ptr, None) == -1002


def test_ops_reject_host_tensors_and_bad_arguments():
    from tensoir_amd import _lib, ops
    with pytest.raises(_lib.TensoirHipError):
        ops.label_components(torch.zeros(4, 4, 4), 0.5)                                  # no CPU path
    if torch.cuda.is_available():
        pytest.skip("the remaining checks are written for a host without a GPU")


def test_header_documents_the_entries():
    src = open(os.path.join(ROOT, "include", "tensoir_hip.h")).read()
    for name in ("tir_ccl_blocks", "tir_ccl_label", "tir_ccl_table", "tir_ccl_filter"):
        assert src.count(name) >= 2, name                                                # the prototype and its contract text
