"""Pins the oracle on two configurations no other golden covers -- 8 density / 24 appearance components (the constructor
default) with softplus and with fea2denseAct='relu' -- against tests/golden/config_scenes.npz, recorded from the imported
reference by oracle/make_golden_configs.py: features and sigma at seeded points, derived normals, the evaluation render's maps
and one training step's loss, maps and parameter gradients.  Tolerances are those of tests/test_oracle_golden.py and
tests/test_oracle_train.py.  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import tensoir_oracle as O
from tests import config_scenes as CS
from tests.helpers import T, digest, max_err, rel_err, scene_from_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKENDS = ["aten", "explicit"]


@pytest.fixture(scope="module")
def cg():
    return np.load(os.path.join(ROOT, "tests", "golden", "config_scenes.npz"))


def golden_scene(cg, name):
    ck = CS.with_golden_mask(CS.checkpoint(CS.ROW[name]), cg, name)
    return scene_from_checkpoint(ck, *CS.ENVMAP_HW)


@pytest.mark.parametrize("name", CS.GOLDEN_ROWS)
def test_checkpoint_is_the_recorded_one(cg, name):
    """The golden stores results, not weights: the seeded checkpoint must be the one they were recorded on."""
    sd = CS.checkpoint(CS.ROW[name])["state_dict"]
    assert [f"{k}={digest(v)}" for k, v in sorted(sd.items())] == [str(s) for s in cg[f"{name}/sd_digest"]]


@pytest.mark.parametrize("name", CS.GOLDEN_ROWS)
def test_scene_carries_activation(cg, name):
    sc = golden_scene(cg, name)
    assert sc.fea2denseAct == CS.ROW[name].act
    assert sc.to(torch.float64).fea2denseAct == sc.fea2denseAct
    assert sc.density_plane[0].shape[1] == 8 and sc.app_plane[0].shape[1] == 24


def test_unknown_activation_refused(cg):
    sc = golden_scene(cg, "d8_a24")
    sc.fea2denseAct = "exp"
    with pytest.raises(ValueError, match="fea2denseAct"):
        O.feature2density(sc, torch.zeros(3))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CS.GOLDEN_ROWS)
def test_features_vs_reference(cg, name, backend):
    sc = golden_scene(cg, name)
    xyz = CS.feature_points()
    lidx = CS.light_indices(xyz.shape[0], CS.ROW[name].n_lights)
    tol = 1e-6 if backend == "aten" else 2e-5
    f = O.density_feature(sc, xyz, backend)
    ref_f = T(cg, f"{name}/feat/density")
    assert max_err(f, ref_f) < tol
    assert rel_err(O.feature2density(sc, f), cg[f"{name}/feat/sigma"], 1e-3) < 1e-4
    assert max_err(O.app_feature(sc, xyz, lidx, backend), cg[f"{name}/feat/app"]) < tol
    assert max_err(O.intrin_feature(sc, xyz, backend), cg[f"{name}/feat/intrin"]) < tol
    if CS.ROW[name].act == "relu":            # the recorded scene exercises both arms of relu, and sigma is relu(f): no shift
        assert float((ref_f > 0).float().mean()) >= 0.25 and float((ref_f < 0).float().mean()) >= 0.25
        assert np.array_equal(cg[f"{name}/feat/sigma"], np.maximum(cg[f"{name}/feat/density"], 0.0))


@pytest.mark.parametrize("name", CS.GOLDEN_ROWS)
def test_derived_normals_vs_reference(cg, name):
    sc = golden_scene(cg, name)
    x = CS.feature_points().clamp(-0.95, 0.95)
    ref = T(cg, f"{name}/feat/derived_normals")
    _, _, n = O.density_grad(sc, x)
    _, _, n64 = O.density_grad(sc.to(torch.float64), x.double())
    # as tests/test_oracle_golden.py: compared where the fp32 gradient is well conditioned (fp64 agrees with fp32)
    ok = (n.double() - n64).abs().amax(-1) < 1e-3
    assert float(ok.float().mean()) > 0.9
    assert max_err(n[ok], ref[ok]) < 2e-3
    if CS.ROW[name].act == "relu":            # relu' is 0 below zero: the normal of a zero gradient is zero on both sides
        f = T(cg, f"{name}/feat/density")
        inside = (CS.feature_points().abs() <= 0.95).all(-1)
        dead = inside & (f < 0)
        assert int(dead.sum()) > 0
        assert float(ref[dead].abs().max()) == 0.0 and float(n[dead].abs().max()) == 0.0


@pytest.mark.parametrize("name", CS.GOLDEN_ROWS)
def test_eval_render_vs_reference(cg, name):
    sc = golden_scene(cg, name)
    rays, lidx, _ = CS.rays_for(CS.ROW[name])
    torch.manual_seed(CS.SEED + 3)
    with torch.no_grad():
        ret = O.renderer_train(sc, rays, lidx, n_samples=-1, **{"second_n_sample": CS.SECOND["second_nSample"],
                               "second_near": CS.SECOND["second_near"], "second_far": CS.SECOND["second_far"]})
    for k in ("rgb_map", "depth_map", "normal_map", "albedo_map", "roughness_map", "acc_map", "rgb_with_brdf_map"):
        assert float((ret[k] - T(cg, f"{name}/eval/{k}")).abs().max()) < 3e-5, (name, k)
    acc = T(cg, f"{name}/eval/acc_map")
    assert float(acc.max()) > 0.99 and float(acc.min()) < 0.01          # rays that hit and rays that miss


@pytest.mark.parametrize("name", CS.GOLDEN_ROWS)
def test_train_grads_vs_reference(cg, name):
    sc = golden_scene(cg, name)
    rays, lidx, gt = CS.rays_for(CS.ROW[name])
    torch.manual_seed(CS.SEED + 12)
    jit = torch.rand(rays.shape[0], 1)
    assert np.array_equal(jit.numpy(), cg[f"{name}/train/ray_jitter"])
    loss, grads, ret = O.train_step_grads(sc, rays, lidx, gt, is_relight=True, n_samples=CS.N_SAMPLES, ray_jitter=jit,
                                          second_n_sample=CS.SECOND["second_nSample"], second_near=CS.SECOND["second_near"],
                                          second_far=CS.SECOND["second_far"])
    assert abs(float(loss) - float(cg[f"{name}/train/loss"][0])) < 2e-6
    for k in ("rgb_map", "acc_map", "rgb_with_brdf_map"):
        assert float((ret[k] - T(cg, f"{name}/train/out/{k}")).abs().max()) < 3e-5, k
    checked = 0
    for pname, gr in grads.items():
        ref = torch.from_numpy(cg[f"{name}/train/grad/{pname}"]).double()
        if float(ref.abs().max()) == 0:
            assert float(gr.abs().max()) == 0, pname
            continue
        err = float((gr.double() - ref).abs().max() / ref.abs().max())
        assert err < 2e-3, (pname, err)
        checked += 1
    assert checked >= 30
