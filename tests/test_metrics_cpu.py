"""Image metrics, the part that needs no GPU: the float64 restatement (tests/metrics_reference.py) against what the reference's
own utils.rgb_ssim returned (tests/golden/metrics_ssim.npz), the float32-product rule, host-side validation of tir_ssim /
tir_image_error, metrics.ssim's argument errors, and the launcher's rebinding guard."""
import sys

import numpy as np
import pytest
import torch

from tests import metrics_reference as MR


@pytest.fixture(scope="module")
def golden():
    return np.load(MR.GOLDEN)


@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    return _lib.lib()


def test_cases_cover_the_tile_edges():
    from tensoir_amd import metrics
    T = metrics.SSIM_TILE
    cs = {name: (a, b, kw) for name, a, b, kw in MR.cases(T)}
    assert cs["one_pixel"][0].shape == (11, 11, 3) and cs["one_row"][0].shape == (11, 40, 3)
    H, W, _ = cs["ragged_tiles"][0].shape
    assert H - 10 == 2 * T + 5 and W - 10 == 2 * T + T // 2 + 1
    assert cs["gray"][0].shape == (33, 34, 1) and cs["rgba"][0].shape[-1] == 4
    assert cs["hdr"][0].max() > 3.0 and cs["hdr"][2] == {"max_val": 4.0}
    assert cs["filter4"][2]["filter_size"] == 4 and cs["filter5"][2]["filter_size"] == 5
    again = MR.cases(T)
    assert all(np.array_equal(a, c[1]) and np.array_equal(b, c[2]) for (_, a, b, _), c in zip(MR.cases(T), again))


def test_restatement_against_the_reference(golden):
    """Mean within 1e-12 and map within 1e-10 of the reference's rgb_ssim for every three-channel case (measured with a separable
    restatement: 4e-15 and 7e-13; the direct window sums form other tap products, the bounds leave two orders for that)."""
    seen = 0
    for name, a, b, kw in MR.cases():
        if a.shape[-1] != 3:
            continue
        m = MR.ssim_map(a, b, **kw)
        dm = abs(float(m.mean()) - float(golden["mean/" + name]))
        line = f"\n[metrics restatement {name}] mean {dm:.2e}"
        assert dm <= 1e-12, (name, dm)
        if name in MR.MAP_CASES:
            dmap = float(np.abs(m - golden["map/" + name]).max())
            line += f" map {dmap:.2e}"
            assert dmap <= 1e-10, (name, dmap)
        print(line)
        seen += 1
    assert seen == 11 and float(golden["mean/self"]) == 1.0 and float(golden["mean/anti"]) < 0
    assert {k.split("/")[1] for k in golden.files if k.startswith("map/")} == set(MR.MAP_CASES)


def test_float32_products_are_the_rule(golden):
    """Exact float64 products are NOT what the reference computes: on the smooth case that restatement is further than 1e-7 from
    the recorded map, the float32-product one within 1e-10."""
    name, a, b, kw = next(c for c in MR.cases() if c[0] == "smooth")
    exact = float(np.abs(MR.ssim_map(a, b, exact_products=True, **kw) - golden["map/smooth"]).max())
    f32 = float(np.abs(MR.ssim_map(a, b, **kw) - golden["map/smooth"]).max())
    print(f"\n[metrics products] exact float64 products {exact:.2e}, float32 products {f32:.2e}")
    assert exact > 1e-7 and f32 <= 1e-10


def test_taps_equal_the_reference_filter():
    from tensoir_amd import metrics
    for n, s in ((11, 1.5), (5, 0.8), (4, 1.0), (1, 1.5), (31, 4.0)):
        t = metrics.gaussian_taps(n, s)
        assert t.dtype == np.float64 and np.array_equal(t, t[::-1]) and abs(t.sum() - 1.0) < 1e-14
        assert np.abs(t - MR.gaussian(n, s)).max() < 1e-16


def test_entries_validate_on_the_host(lib):
    """Every refusal happens before any device work: the pointers are host addresses (or null) and nothing may be launched."""
    keep = torch.zeros(64, dtype=torch.float64)
    p = keep.data_ptr()
    ssim = lambda N=1, H=16, W=16, Cn=3, n=11, img0=p, img1=p, taps=p, ws=p, mean=p: lib.tir_ssim(img0, img1, N, H, W, Cn, taps, n, 1e-4, 9e-4, None, ws, mean, None)
    assert ssim(img0=None) == -1001 and ssim(img1=None) == -1001 and ssim(taps=None) == -1001 and ssim(ws=None) == -1001
    assert ssim(mean=None) == -1001
    assert ssim(n=0) == -1001 and ssim(n=32) == -1001 and ssim(n=17) == -1001 and ssim(H=10) == -1001
    assert ssim(N=-1) == -1001 and ssim(H=-16) == -1001 and ssim(W=0) == -1001
    assert ssim(Cn=0) == -1002 and ssim(Cn=5) == -1002
    assert ssim(N=0) == 0 and ssim(N=0, img0=None, img1=None, ws=None, mean=None) == 0
    T = 16
    assert lib.tir_ssim_workspace(3, 10 + 2 * T + 5, 10 + 2 * T + T // 2 + 1, 3, 11) == 3 * 9 + 2      # 9 tiles per image + 3 tickets
    assert lib.tir_ssim_workspace(1, 11, 11, 1, 11) == 2 and lib.tir_ssim_workspace(0, 11, 11, 1, 11) == 0
    assert lib.tir_ssim_workspace(1, 11, 11, 1, 12) == -1001 and lib.tir_ssim_workspace(1, 11, 11, 5, 11) == -1002
    err = lambda N=1, P=8, Cn=3, a=p, b=p, ws=p, out=p: lib.tir_image_error(a, b, None, N, P, Cn, 1, ws, out, None)
    assert err(a=None) == -1001 and err(b=None) == -1001 and err(ws=None) == -1001 and err(out=None) == -1001
    assert err(N=-1) == -1001 and err(P=-1) == -1001
    assert err(Cn=0) == -1002 and err(Cn=5) == -1002
    assert err(N=0) == 0 and err(N=0, a=None, b=None, ws=None, out=None) == 0
    assert lib.tir_image_error_workspace(2, 1) == 2 * 3 + 1 and lib.tir_image_error_workspace(1, 2049) == 2 * 3 + 1
    assert lib.tir_image_error_workspace(1, 10 ** 9) == 256 * 3 + 1 and lib.tir_image_error_workspace(-1, 4) == -1001


def test_ssim_argument_errors():
    """Refused before any device is looked for."""
    from tensoir_amd import metrics
    a = np.zeros((16, 16, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="one shape"):
        metrics.ssim(a, np.zeros((16, 17, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="one shape"):
        metrics.ssim(a[0], a[0])
    with pytest.raises(ValueError, match="channels"):
        metrics.ssim(np.zeros((16, 16, 5), dtype=np.float32), np.zeros((16, 16, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="does not fit"):
        metrics.ssim(a[:10], a[:10])
    for bad in (0, 32, -3):
        with pytest.raises(ValueError, match="filter_size"):
            metrics.ssim(a, a, filter_size=bad)
    with pytest.raises(AssertionError):
        metrics.rgb_ssim(np.zeros((16, 16, 1), dtype=np.float32), np.zeros((16, 16, 1), dtype=np.float32), 1)
    assert metrics.SSIM_TILE == 16 and metrics.MAX_FILTER == 31


def _fake_utils(tmp_path, monkeypatch):
    root = tmp_path / "tree"
    root.mkdir()
    (root / "utils.py").write_text("def rgb_ssim(*a, **k):\n    return 'host'\n")
    (root / "renderer.py").write_text("from utils import *\n")
    for k in ("utils", "renderer"):
        monkeypatch.delitem(sys.modules, k, raising=False)
    monkeypatch.setattr(sys, "path", [str(root)] + list(sys.path))
    return root


def test_rebinding_guard(tmp_path, monkeypatch):
    """Without a GPU nothing is rebound (the scripts keep scipy); with TENSOIR_HOST_METRICS=1 nothing is; and a `utils` that does
    not come from the reference root is left alone even where a GPU is claimed."""
    import importlib
    from tensoir_amd import run
    root = _fake_utils(tmp_path, monkeypatch)
    renderer = importlib.import_module("renderer")
    utils = importlib.import_module("utils")
    host = utils.rgb_ssim
    try:
        if not torch.cuda.is_available():
            assert run._rebind_metrics(str(root)) is False and utils.rgb_ssim is host and renderer.rgb_ssim is host
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        monkeypatch.setenv("TENSOIR_HOST_METRICS", "1")
        assert run._rebind_metrics(str(root)) is False and utils.rgb_ssim is host
        monkeypatch.setenv("TENSOIR_HOST_METRICS", "0")
        elsewhere = tmp_path / "elsewhere"
        elsewhere.mkdir()
        assert run._rebind_metrics(str(elsewhere)) is False and utils.rgb_ssim is host and renderer.rgb_ssim is host
        # the positive leg needs no device either: rebinding only stores a function
        from tensoir_amd import metrics
        assert run._rebind_metrics(str(root)) is True and utils.rgb_ssim is metrics.rgb_ssim and renderer.rgb_ssim is metrics.rgb_ssim
    finally:
        for k in ("utils", "renderer"):
            sys.modules.pop(k, None)
