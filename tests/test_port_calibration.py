"""cpu_baseline bookkeeping: bench.py times the oracle ("port") on the GPU box because the reference
checkout cannot travel there; profiles/port_over_reference.json (oracle/calibrate_port.py) relates the two on the same inputs.
Here: the committed calibration is well-formed and says the port is a fair stand-in (within 2x either way, identical maps), and
the port agrees map for map with the reference's recorded maps of a small sample of the bench scene."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_calibration():
    d = json.load(open(os.path.join(ROOT, "profiles", "port_over_reference.json")))
    for k in ("port_over_reference", "reference_rays_per_s", "port_rays_per_s", "port_vs_reference_max_rel_floor1", "sample", "threads"):
        assert k in d, k
    assert 0.5 < d["port_over_reference"] < 2.0
    assert abs(d["port_over_reference"] - d["reference_rays_per_s"] / d["port_rays_per_s"]) < 0.02
    assert d["port_vs_reference_max_rel_floor1"] < 1e-5 and "4096 rays" in d["sample"]


@pytest.mark.timeout(900)
def test_port_equals_reference_on_the_bench_scene():
    """The port on the bench scene (32 rays of the 4096-ray batch, 96^3 field, the reference-built 128^3 mask) against the maps
    the reference computed on the same inputs (tests/golden/port_reference.npz, oracle/make_golden_host.py)."""
    import time
    import numpy as np
    import torch
    from oracle import tensoir_oracle as O
    from oracle.make_golden_host import PORT_ENV, PORT_GRID, PORT_SAMPLES, PORT_SECOND
    from oracle.ref_on_gpu import MAPS, metrics
    from tensoir_amd import synth
    from tests.helpers import scene_from_checkpoint
    g = np.load(os.path.join(ROOT, "tests", "golden", "port_reference.npz"))
    ck = dict(synth.make_checkpoint(grid=(PORT_GRID,) * 3, seed=20211202))
    ck["alphaMask.shape"] = tuple(int(x) for x in g["mask/shape"])
    ck["alphaMask.mask"] = g["mask/bits"]
    ck["alphaMask.aabb"] = torch.from_numpy(g["mask/aabb"])
    rays_all = synth.make_rays(64, 64)
    rays = rays_all[::int(g["stride"])][: g["rays"].shape[0]].contiguous()
    assert torch.equal(rays, torch.from_numpy(g["rays"]))                  # the recorded inputs are the bench batch's
    sc = scene_from_checkpoint(ck, *PORT_ENV)
    t0 = time.perf_counter()
    with torch.no_grad():
        out = O.renderer_train(sc, rays, torch.from_numpy(g["light_idx"]), n_samples=PORT_SAMPLES, second_n_sample=PORT_SECOND,
                               chunk_size=160000)
    port_rays_per_s = rays.shape[0] / (time.perf_counter() - t0)
    worst = max(metrics(out[k], torch.from_numpy(g["ref/" + k]))["max_rel_floor1"] for k in MAPS)
    assert worst < 1e-5
    assert port_rays_per_s > 0


def test_bench_reports_the_relation():
    import sys
    sys.path.insert(0, ROOT)
    import bench
    v = bench.port_vs_reference(200.0)
    d = json.load(open(os.path.join(ROOT, "profiles", "port_over_reference.json")))
    assert v["port_over_reference_time"] == d["port_over_reference"]
    assert abs(v["reference_equivalent_rays_per_s"] - 200.0 * d["port_over_reference"]) < 0.01
