"""The guided a-trous denoiser without a GPU: properties of the float64 restatement (tests/denoise_reference.py), what the filter
is worth on a synthetic scene by those formulas alone, and every refusal of tir_denoise_guide, tir_atrous_level and AtrousConfig
-- all answered on the host before any device work."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import denoise_reference as R

_KEEP = torch.zeros(64, dtype=torch.float32)      # any non-null, 16-byte aligned host address: never dereferenced
P = _KEEP.data_ptr()
Q = P + 16                                        # another one
assert P % 16 == 0
ARG, UNSUP, OK = -1001, -1002, 0
INV = R.inverses(sigma_p=0.02)


def flat_guide(H, W, valid=True):
    g = np.zeros((H, W, R.GUIDE))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    g[..., 0], g[..., 1] = xs * 0.01, ys * 0.01                       # a plane z = 0 facing +z
    g[..., 3] = valid
    g[..., 6] = 1.0
    g[..., 7] = 0.5
    g[..., 8:11] = 0.6
    return g


# ---- properties of the restatement ----------------------------------------------------------------------------------------------
def test_constant_image_stays_constant():
    g = flat_guide(9, 11)
    g[4, 5, 8:11] = 0.1                                               # an albedo speck changes weights, not the result
    c = np.broadcast_to(np.array([0.25, 0.5, 0.75, 0.1, 0.2, 0.3]), (9, 11, 6)).copy()
    for step in (1, 2, 4):
        out = R.atrous_level(c, g, step, *INV)
        assert np.abs(out - c).max() < 1e-15


def test_one_valid_pixel_among_invalid_ones_is_unchanged():
    rng = np.random.default_rng(3)
    g = flat_guide(7, 7, valid=False)
    g[3, 2, 3] = 1.0
    c = rng.random((7, 7, 3))
    out = R.atrous_level(c, g, 1, *INV)
    invalid = g[..., 3] < 0.5
    assert np.array_equal(out[invalid], c[invalid])                   # copies
    assert np.abs(out[3, 2] - c[3, 2]).max() < 1e-15                  # (w c) / w


def test_albedo_step_does_not_leak():
    g = flat_guide(8, 12)
    g[..., 8:11] = 0.25
    g[:, 6:, 8:11] += 0.5                                             # every channel steps by 0.5 across the edge, sigma_a = 0.1
    c = np.zeros((8, 12, 3))
    c[:, 6:] = 1.0
    out = R.atrous_level(c, g, 1, *R.inverses(sigma_p=0.02, sigma_c=0.0))
    assert np.abs(out - c).max() < 1e-12                              # exp(-75) of weight at the most ...
    assert np.abs(out - c).max() > 0                                  # ... and not nothing: the tap is taken


def test_step_beyond_the_image_leaves_the_centre_tap():
    rng = np.random.default_rng(4)
    g = flat_guide(5, 6)
    c = rng.random((5, 6, 3))
    assert np.abs(R.atrous_level(c, g, 6, *INV) - c).max() < 1e-15
    assert np.abs(R.atrous_level(c, g, 3, *INV) - c).max() > 1e-3     # (a step inside the image does filter)


# ---- what the filter is worth, by the formulas alone ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return R.sphere_scene(96)


def _mse(a, b, valid):
    return float(np.mean((a[valid] - b[valid]) ** 2))


@pytest.mark.parametrize("rel_sigma", [0.5, 0.25])
def test_default_config_at_least_halves_the_error(scene, rel_sigma):
    clean, g = scene
    valid = g[..., 3] > 0.5
    rng = np.random.default_rng(20100625)
    noisy = clean * (1.0 + rel_sigma * rng.standard_normal(clean.shape))
    out = R.atrous(noisy, g, levels=3, sigma_p=0.005 * 6.0)           # the default config; a scene of about 6 units across
    before, after = _mse(noisy, clean, valid), _mse(out, clean, valid)
    print(f"relative sigma {rel_sigma}: mse {before:.3e} -> {after:.3e}, factor {before / after:.2f}")
    assert after <= 0.5 * before
    assert np.array_equal(out[~valid], noisy[~valid])


def test_default_config_keeps_the_clean_image(scene):
    clean, g = scene
    valid = g[..., 3] > 0.5
    out = R.atrous(clean, g, levels=3, sigma_p=0.005 * 6.0)
    mse = _mse(out, clean, valid)
    print(f"clean image: mse {mse:.3e}")
    assert mse <= 2e-3


def test_guide_rows_restatement():
    maps = np.zeros((3, 20))
    maps[:, 3] = [2.0, 0.0, 1.0]
    maps[:, 4:7] = [[0, 0, 2], [0, 0, 0], [3, 4, 0]]
    maps[:, 7:10] = [[0.1, 0.2, 0.3]] * 3
    maps[:, 10] = 0.7
    maps[:, 14] = [0.9, 0.5, 0.51]
    rays = np.array([[0, 0, 4, 0, 0, -1.0]] * 3)
    g = R.guide_rows(maps, rays)
    assert g[:, 0:3].tolist() == [[0, 0, 2], [0, 0, 4], [0, 0, 3]]
    assert g[:, 3].tolist() == [1, 0, 1]
    assert np.allclose(g[:, 4:7], [[0, 0, 1], [0, 0, 0], [0.6, 0.8, 0]])
    assert g[:, 7].tolist() == [0.7] * 3 and g[:, 8:11].tolist() == [[0.1, 0.2, 0.3]] * 3 and not g[:, 11].any()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    return _lib.lib()


_NAN, _INF = float("nan"), float("inf")


def _case_id(change):
    """A case's id with the host addresses written as P and P+4: an id must not change with where _KEEP happens to live."""
    return repr(change).replace(str(P + 4), "P+4").replace(str(P), "P")


# tir_atrous_level(color_in, color_out, guide, H, W, K, step, inv_sn, inv_sp, inv_sa2, inv_sr2, inv_sc2, stream)
_GOOD_LEVEL = dict(color_in=P, color_out=Q, guide=P, H=4, W=4, K=3, step=1, inv_sn=20.0, inv_sp=50.0, inv_sa2=100.0, inv_sr2=100.0,
                   inv_sc2=4.0, stream=None)
_LEVEL_CASES = [
    ({"color_in": None}, ARG), ({"color_out": None}, ARG), ({"guide": None}, ARG),
    ({"H": 0}, ARG), ({"W": 0}, ARG), ({"H": -3}, ARG), ({"W": -1}, ARG),
    ({"K": 0}, ARG), ({"K": 4}, ARG), ({"K": 2}, ARG), ({"K": 27}, ARG), ({"K": -3}, ARG),
    ({"step": 0}, ARG), ({"step": -1}, ARG),
    *[({k: v}, ARG) for k in ("inv_sn", "inv_sp", "inv_sa2", "inv_sr2", "inv_sc2") for v in (-1.0, _NAN, _INF)],
    ({"color_out": P}, ARG),                                          # in place
    ({"guide": P + 4}, ARG),                                          # guide rows are read as 16-byte vectors
    ({"H": 1 << 16, "W": 1 << 15}, UNSUP), ({"H": 1, "W": 1 << 29}, UNSUP),
]


@pytest.mark.parametrize("change,want", _LEVEL_CASES, ids=[_case_id(c) for c, _ in _LEVEL_CASES])
def test_atrous_level_refuses_before_any_device_work(lib, change, want):
    assert lib.tir_atrous_level(*{**_GOOD_LEVEL, **change}.values()) == want


# tir_denoise_guide(maps, rays, n, acc_thres, guide, row0, stream)
_GOOD_GUIDE = dict(maps=P, rays=P, n=8, acc_thres=0.5, guide=P, row0=0, stream=None)
_GUIDE_CASES = [
    ({"maps": None}, ARG), ({"rays": None}, ARG), ({"guide": None}, ARG), ({"n": -1}, ARG), ({"row0": -1}, ARG),
    ({"guide": P + 4}, ARG),
    ({"n": 0}, OK), ({"n": 0, "maps": None, "rays": None, "guide": None}, OK), ({"n": 0, "row0": -1}, ARG),
]


@pytest.mark.parametrize("change,want", _GUIDE_CASES, ids=[_case_id(c) for c, _ in _GUIDE_CASES])
def test_denoise_guide_refuses_before_any_device_work(lib, change, want):
    assert lib.tir_denoise_guide(*{**_GOOD_GUIDE, **change}.values()) == want


def test_config_refusals():
    from tensoir_amd.denoise import AtrousConfig
    cfg = AtrousConfig()
    assert (cfg.levels, cfg.sigma_n, cfg.sigma_p, cfg.sigma_a, cfg.sigma_r, cfg.sigma_c) == (3, 0.05, None, 0.1, 0.1, 0.5)
    for bad in (dict(levels=0), dict(levels=7), dict(levels=2.0), dict(levels=True), dict(sigma_n=0.0), dict(sigma_n=-1.0),
                dict(sigma_p=0.0), dict(sigma_p=_INF), dict(sigma_a=0.0), dict(sigma_a=_NAN), dict(sigma_r=-0.1), dict(sigma_r="x"),
                dict(sigma_c=-0.5), dict(sigma_c=_INF)):
        with pytest.raises(ValueError):
            AtrousConfig(**bad)
    with pytest.raises(ValueError, match="sigma_p"):
        cfg.inverses()                                                # no model to take the diagonal from
    inv = cfg.inverses([[-1.5] * 3, [1.5] * 3])
    assert inv[0] == 20.0 and abs(inv[1] - 1.0 / (0.005 * np.sqrt(27.0))) < 1e-12 and inv[4] == 4.0
    assert all(abs(a - b) <= 1e-12 * b for a, b in zip(inv[2:4], (100.0, 100.0)))
    assert AtrousConfig(sigma_c=0.0, sigma_p=0.1, levels=6).inverses()[4] == 0.0
    assert tuple(AtrousConfig(sigma_p=0.02).inverses()) == tuple(R.inverses(sigma_p=0.02))


def test_no_gpu_no_cpu_path():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tensoir_amd import _lib, denoise, relight
    with pytest.raises(_lib.TensoirHipError):
        denoise.atrous(torch.zeros(4, 4, 3), torch.zeros(4, 4, 12), denoise.AtrousConfig(sigma_p=0.1))
    with pytest.raises(_lib.TensoirHipError):
        relight.relight_view(None, None, ["a"], torch.zeros(16, 6), 4, 4)


def test_map_rows_from_the_primary_tuple():
    """relight_view's map rows: read in place where the tuple's columns are views of one [B, 20] block (also one that starts
    inside a larger storage), assembled from the columns the guide reads when they are copies."""
    from tensoir_amd import relight
    from tensoir_amd.field_model import TensorVMSplit
    B = 7
    store = torch.arange(5 + B * 20 + 3, dtype=torch.float32)
    for maps in (store[:B * 20].view(B, 20), store[5:5 + B * 20].view(B, 20)):
        prim = TensorVMSplit.unpack_maps(maps, want_mask=False, smooth=torch.zeros(2))
        rows = relight._map_rows(prim, B)
        assert rows.data_ptr() == maps.data_ptr() and rows.shape == (B, 20) and torch.equal(rows, maps)
        copies = tuple(t.clone() if torch.is_tensor(t) else t for t in prim)
        rows = relight._map_rows(copies, B)
        assert rows.data_ptr() != maps.data_ptr() and rows.shape == (B, 20)
        for c in (slice(3, 11), slice(14, 15)):
            assert torch.equal(rows[:, c], maps[:, c])
        assert np.array_equal(R.guide_rows(rows.numpy(), np.ones((B, 6))), R.guide_rows(maps.numpy(), np.ones((B, 6))))
    # columns of different blocks are not taken for one
    other = TensorVMSplit.unpack_maps(store[:B * 20].clone().view(B, 20), want_mask=False, smooth=torch.zeros(2))
    mixed = prim[:6] + (other[6],) + prim[7:]
    assert relight._map_rows(mixed, B).data_ptr() != maps.data_ptr()
