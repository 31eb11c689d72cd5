"""Image metrics on the GPU (tir_ssim / tir_image_error, ops.ssim / image_error, tensoir_amd.metrics, the launcher's rebinding,
compare_asset(ssim=True)) against the reference's recorded results (tests/golden/metrics_ssim.npz) and the float64 restatement
(tests/metrics_reference.py).  Bounds: the device's double sums differ from numpy's only by order and FMA, measured on the host
between two float64 forms as 4e-15 (mean) and 7e-13 (map); 1e-10 and 1e-9 leave three orders."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import metrics_reference as MR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN_TOL, MAP_TOL, REL_TOL = 1e-10, 1e-9, 1e-12


@pytest.fixture(scope="module")
def golden():
    return np.load(MR.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    """name -> (img0, img1, kw, the restatement's map), computed once"""
    from tensoir_amd import metrics
    return {name: (a, b, kw, MR.ssim_map(a, b, **kw)) for name, a, b, kw in MR.cases(metrics.SSIM_TILE)}


@pytest.mark.parametrize("name", [c[0] for c in MR.cases()])
def test_ssim_against_reference_and_restatement(cases, golden, name):
    from tensoir_amd import metrics
    a, b, kw, want = cases[name]
    mean = metrics.ssim(a, b, **kw)
    smap = metrics.ssim(a, b, return_map=True, **kw)
    assert isinstance(mean, np.float64) and smap.dtype == np.float64 and smap.shape == want.shape
    d_mean, d_map = abs(float(mean) - float(want.mean())), float(np.abs(smap - want).max())
    line = f"\n[gpu ssim {name} {a.shape}] restatement: mean {d_mean:.2e} map {d_map:.2e}"
    ok = d_mean <= MEAN_TOL and d_map <= MAP_TOL
    if "mean/" + name in golden.files:
        g_mean = abs(float(mean) - float(golden["mean/" + name]))
        line += f"; reference: mean {g_mean:.2e}"
        ok = ok and g_mean <= MEAN_TOL
        if "map/" + name in golden.files:
            g_map = float(np.abs(smap - golden["map/" + name]).max())
            line += f" map {g_map:.2e}"
            ok = ok and g_map <= MAP_TOL
    print(line)
    assert ok, line
    if name == "self":
        assert float(mean) == 1.0 and (smap == 1.0).all()
    if name == "anti":
        assert float(mean) < 0


def test_batch_equals_single_calls_bitwise_and_launches_repeat(cases):
    """Three different-content pairs of one shape: the batched means and maps equal the three single calls bit for bit, and a
    second launch equals the first."""
    from tensoir_amd import metrics, ops
    rng = np.random.default_rng(7)
    T = metrics.SSIM_TILE
    a = rng.uniform(0, 1, size=(3, 2 * T + 15, 3 * T + 12, 3)).astype(np.float32)
    b = np.clip(a + rng.normal(0, 0.1, size=a.shape), 0, 1).astype(np.float32)
    b[1] = 1.0 - a[1]
    mean, smap = metrics.ssim(a, b), metrics.ssim(a, b, return_map=True)
    assert mean.shape == (3,) and smap.shape == (3, 2 * T + 5, 3 * T + 2, 3)
    for i in range(3):
        assert metrics.ssim(a[i], b[i]) == mean[i] and np.array_equal(metrics.ssim(a[i], b[i], return_map=True), smap[i])
        assert abs(mean[i] - MR.ssim(a[i], b[i])) <= MEAN_TOL
    da, db, taps = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), metrics.gaussian_taps()
    first = ops.ssim(da, db, taps, 0.01 ** 2, 0.03 ** 2, return_map=True)
    second = ops.ssim(da, db, taps, 0.01 ** 2, 0.03 ** 2, return_map=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert np.array_equal(first[0].cpu().numpy(), mean)


def test_input_kinds_agree(cases):
    from tensoir_amd import metrics
    a, b, kw, _ = cases["ragged_tiles"]
    want = metrics.ssim(a, b)
    assert metrics.ssim(torch.from_numpy(a), torch.from_numpy(b)) == want
    assert metrics.ssim(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) == want
    assert metrics.ssim(torch.from_numpy(a).cuda(), b) == want
    assert metrics.rgb_ssim(torch.from_numpy(a), torch.from_numpy(b), 1) == want
    # anything that is not float32 is converted to float32 first
    assert metrics.ssim(a.astype(np.float64), b.astype(np.float64)) == want


@pytest.mark.parametrize("P", [1, 255, 257, 2 * 2048 + 77, 256 * 2048 + 513])
def test_psnr_and_normal_mae_against_float64(P):
    """One pixel, one short of / one past a wave-multiple, more than one workgroup's share (ops.IMAGE_ERROR_SHARE pixels), and more
    than the 256 workgroups an image gets; a . b beyond the clamp on both sides."""
    from tensoir_amd import metrics, ops
    assert ops.IMAGE_ERROR_SHARE == 2048
    rng = np.random.default_rng(P)
    a = rng.normal(size=(P, 3)).astype(np.float32)
    a /= np.linalg.norm(a, axis=-1, keepdims=True)
    b = a + rng.normal(scale=0.2, size=(P, 3)).astype(np.float32)
    b = (b / np.linalg.norm(b, axis=-1, keepdims=True)).astype(np.float32)
    b[0] = a[0] * np.float32(1.5)                       # a . b > 1
    if P > 1:
        b[P // 2] = -a[P // 2] * np.float32(1.25)       # a . b < -1
    mask = rng.uniform(size=P) < 0.6
    mask[0] = True
    dots = (a.astype(np.float64) * b.astype(np.float64)).sum(-1)
    assert dots.max() > 1 and (P == 1 or dots.min() < -1)
    rel = lambda x, y: abs(x - y) / abs(y) if y else abs(x - y)          # (one clamped pixel: both are exactly 0)
    for m in (None, mask):
        dp, dn = rel(metrics.psnr(a, b, m), MR.psnr(a, b, m)), rel(metrics.normal_mae(a, b, m), MR.normal_mae(a, b, m))
        print(f"\n[gpu image_error P={P} mask={m is not None}] psnr rel {dp:.2e} mae rel {dn:.2e}")
        assert dp <= REL_TOL and dn <= REL_TOL
    # other channel counts, a mask as [P, 1], tensors on the device
    for Cn in (1, 2, 4):
        x, y = rng.uniform(size=(P, Cn)).astype(np.float32), rng.uniform(size=(P, Cn)).astype(np.float32)
        assert rel(metrics.psnr(torch.from_numpy(x).cuda(), torch.from_numpy(y), mask[:, None]), MR.psnr(x, y, mask)) <= REL_TOL
    assert metrics.psnr(a, a) == float("inf") and metrics.normal_mae(a[:1], a[:1] * np.float32(2)) == 0.0
    assert np.isnan(metrics.psnr(a, b, np.zeros(P, dtype=bool)))
    two = ops.image_error(torch.from_numpy(np.stack([a, b])).cuda(), torch.from_numpy(np.stack([b, b])).cuda(), None, angular=True)
    one = ops.image_error(torch.from_numpy(a[None]).cuda(), torch.from_numpy(b[None]).cuda(), None, angular=True)
    assert torch.equal(two[0], one[0]) and two[1].tolist()[:2] == [float(P), 0.0]


def test_albedo_scale_equals_cpu_medians():
    from tensoir_amd import metrics
    rng = np.random.default_rng(3)
    for n in (1, 2, 101, 4096):
        pred = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
        pred[0] = 0.0                                                   # the clamp
        gt = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
        mask = rng.uniform(size=n) < 0.7
        mask[:2] = True
        single, three = metrics.albedo_scale(pred, gt, mask)
        tp, tg, tm = torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(mask)
        r = tg[tm] / tp[tm].clamp(min=1e-6)
        assert single.is_cuda and torch.equal(single.cpu(), r[..., 0].median()) and torch.equal(three.cpu(), r.median(dim=0)[0])
        s_ref, t_ref = MR.albedo_scale(pred, gt, mask)
        assert float(single) == float(s_ref) and np.array_equal(three.cpu().numpy(), t_ref)


def _fresh_model(ds, dev):
    import tensoir_amd
    torch.manual_seed(11)
    return tensoir_amd.TensorVMSplit(ds.scene_bbox.to(dev), [32, 32, 32], dev, density_n_comp=[16, 16, 16], appearance_n_comp=[48, 48, 48],
                                     app_dim=27, near_far=ds.near_far, shadingMode="MLP_Fea", alphaMask_thres=1e-4, density_shift=-10,
                                     distance_scale=25, pos_pe=2, view_pe=2, fea_pe=2, featureC=128, step_ratio=0.5, fea2denseAct="softplus",
                                     normals_kind="derived_plus_predicted", light_kind="sg", dataset=ds, numLgtSGs=128, light_rotation=["000"])


def test_evaluate_equals_the_restatement_on_the_same_maps():
    """A freshly initialised model on the synthetic dataset (views=2, res=24): every number of the report equals the maps that
    were measured pushed through the float64 restatement -- over the whole dataset (the global rescale ratio) and over one view
    (its own ratio)."""
    import types
    from tensoir_amd import metrics
    from tensoir_amd.synth_dataset import SyntheticDataset
    dev = torch.device("cuda:0")
    ds = SyntheticDataset("synthetic:views=2,res=24", split="train")
    model = _fresh_model(ds, dev)
    args = types.SimpleNamespace(second_nSample=24, second_near=0.05, second_far=1.5)
    for views in (None, [1]):
        maps = []
        rep = metrics.evaluate(model, ds, views=views, args=args, maps=maps)
        n = 2 if views is None else 1
        assert len(rep["views"]) == n == len(maps) and sorted(rep["mean"]) == sorted(metrics.REPORT_KEYS)
        mses = []
        for v, m in zip(rep["views"], maps):
            m = {k: t.cpu().numpy() for k, t in m.items()}
            assert sorted(v) == sorted(metrics.REPORT_KEYS) and all(isinstance(x, float) for x in v.values())
            want = {"PSNR_nvs": MR.psnr(m["rgb"], m["gt_rgb"]), "PSNR_nvs_brdf": MR.psnr(m["rgb_brdf"], m["gt_rgb"]),
                    "PSNR_albedo_single_aligned": MR.psnr(m["albedo_single_gamma"], m["gt_albedo_gamma"]),
                    "PSNR_albedo_three_aligned": MR.psnr(m["albedo_three_gamma"], m["gt_albedo_gamma"]),
                    "MAE": MR.normal_mae(m["normal"], m["gt_normal"])}
            for k, w in want.items():
                assert abs(v[k] - w) <= REL_TOL * abs(w), (k, v[k], w)
            for k, x, y in (("SSIM_rgb", "rgb", "gt_rgb"), ("SSIM_rgb_brdf", "rgb_brdf", "gt_rgb"), ("SSIM_albedo_single", "albedo_single", "gt_albedo"),
                            ("SSIM_albedo_three", "albedo_three", "gt_albedo")):
                assert abs(v[k] - MR.ssim(m[x], m[y])) <= MEAN_TOL, (k, v[k])
            mses.append([10 ** (-want[k] / 10) for k in ("PSNR_albedo_single_aligned", "PSNR_albedo_three_aligned")])
            # the aligned maps are what the ratio rule says: 1 outside the mask, the clamped rescaled albedo inside
            assert (m["albedo_single"][~m["mask"]] == 1).all() and m["albedo_single"].max() <= 1 and m["albedo_single"].min() >= 0
        for k in metrics.REPORT_KEYS:
            if not k.startswith("PSNR_albedo"):
                assert abs(rep["mean"][k] - np.mean([v[k] for v in rep["views"]])) <= 1e-12 * abs(rep["mean"][k])
        for j, k in enumerate(("PSNR_albedo_single_aligned", "PSNR_albedo_three_aligned")):
            w = -10 * np.log10(np.mean([x[j] for x in mses]))
            assert abs(rep["mean"][k] - w) <= 1e-9 * abs(w), (k, rep["mean"][k], w)
        print("\n[gpu evaluate] " + ("all views" if views is None else "view 1") + " " + str(rep["mean"]))
    assert "SSIM_rgb" not in metrics.evaluate(model, ds, views=1, args=args, ssim=False)["mean"]


@pytest.fixture(scope="module")
def trained():
    from tests.train_sequence import reconstruct
    return reconstruct()


def test_compare_asset_ssim_adds_one_key(trained, tmp_path):
    from tensoir_amd import mesh, raster
    m = trained.model
    glb = str(tmp_path / "scene.glb")
    mesh.export_textured(m, glb, simplify=3, size=256)
    plain = raster.compare_asset(m, glb, H=48, W=48, n_views=2)
    with_ssim = raster.compare_asset(m, glb, H=48, W=48, n_views=2, ssim=True)
    for a, b in zip(plain["views"] + [plain["mean"]], with_ssim["views"] + [with_ssim["mean"]]):
        assert set(b) - set(a) == {"albedo_ssim"} and all(np.array(a[k]).tobytes() == np.array(b[k]).tobytes() for k in a)
        assert isinstance(b["albedo_ssim"], float) and -1.0 <= b["albedo_ssim"] <= 1.0
    assert {k: v for k, v in with_ssim.items() if k not in ("views", "mean")} == {k: v for k, v in plain.items() if k not in ("views", "mean")}
    print("\n[gpu compare_asset ssim] " + str([v["albedo_ssim"] for v in with_ssim["views"]]))


REBIND_CHILD = r"""
import importlib, os, sys
import torch
from tensoir_amd import metrics, run
root = sys.argv[1]
done = run.install(root)                    # imports renderer (from utils import *) for its own rebinding, then rebinds the metric
utils, renderer = importlib.import_module("utils"), importlib.import_module("renderer")
want = os.environ.get("TENSOIR_HOST_METRICS", "0") != "1"
assert (done.get("utils") == ["rgb_ssim"]) is want and ("utils" in done) is want, done
assert set(done) - {"utils"} == set(run.PATCHES) | {"torch.optim"}, done
assert (utils.rgb_ssim is metrics.rgb_ssim) is want and (renderer.rgb_ssim is metrics.rgb_ssim) is want
if want:
    import numpy as np
    a = np.linspace(0, 1, 16 * 16 * 3, dtype=np.float32).reshape(16, 16, 3)
    assert renderer.rgb_ssim(torch.from_numpy(a), torch.from_numpy(a), 1) == 1.0
else:
    assert utils.rgb_ssim() == "host" and renderer.rgb_ssim() == "host"
print("rebind child ok", want)
"""


@pytest.mark.parametrize("host", ["0", "1"])
def test_launcher_rebinds_rgb_ssim_in_a_fresh_process(tmp_path, host):
    """tensoir_amd.run.install against a tree of the reference's module names (placeholders, as tests/test_host_model.py builds it)
    plus a utils.py and a renderer.py that does `from utils import *`: both names resolve to metrics.rgb_ssim, and with
    TENSOIR_HOST_METRICS=1 neither does.  A fresh child process: install() rebinds process-wide state."""
    from tensoir_amd import run
    root = tmp_path / "tree"
    for name, symbols in run.PATCHES.items():
        path = root.joinpath(*name.split(".")).with_suffix(".py")
        path.parent.mkdir(parents=True, exist_ok=True)
        for d in [path.parent] + list(path.parent.parents):
            if d == root:
                break
            (d / "__init__.py").touch()
        head = "from utils import *\n" if name == "renderer" else ""
        path.write_text(head + "".join(f"{s.split(':')[0]} = None\n" for s in symbols))
    (root / "dataLoader").mkdir()
    (root / "dataLoader" / "__init__.py").write_text("dataset_dict = {}\n")
    (root / "utils.py").write_text("def rgb_ssim(*a, **k):\n    return 'host'\n")
    child = tmp_path / "child.py"
    child.write_text(REBIND_CHILD)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), TENSOIR_HOST_METRICS=host, TENSOIR_DEVICE_DATASET="0")
    r = subprocess.run([sys.executable, str(child), str(root)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rebind child ok" in r.stdout, r.stdout + r.stderr
