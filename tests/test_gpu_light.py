"""The asset lighting on the GPU (tir_env_cells, tir_light_gbuffer, ops.env_cells / light_gbuffer, raster.relight_mesh /
compare_asset(light=), mesh.export_environment, the bake command line with --check-light) against the numpy restatement
(tests/light_reference.py).

Comparison rule (DESIGN 4.8's, for device against restatement): the device's distance from the float64 restatement -- max abs
difference over the float64 result's maximum -- is at most ten times the float32 restatement's own distance on the same fixture;
the margin covers v_exp_f32, v_rsq_f32, v_rcp_f32 and fused multiply-adds against numpy's separately rounded operations.  No
fixture has a pair within 1e-6 of the horizon threshold (tests/test_light_cpu.py asserts it), so nothing is excluded.  Everything
repeats bit for bit.

Measured on an MI355X: see DESIGN 4.9."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import light_reference as L
from tests import raster_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def device_light(g, v, cells, fresnel=0.04, flags=3):
    from tensoir_amd import ops
    return ops.light_gbuffer(dev(g), dev(v), dev(cells), fresnel, bool(flags & L.OCCLUSION), bool(flags & L.SRGB)).cpu().numpy()


CASES = [(M, 33, 0.5, 3) for M in L.M_CASES] + [(65, D, 0.5, 3) for D in L.D_CASES if D != 33] + [(65, 33, 0.5, f) for f in range(3)] + \
        [(65, 33, r, f) for r in (0.02, 1.0) for f in (0, 3)]


@pytest.mark.parametrize("M,D,rough,flags", CASES)
def test_light_gbuffer_against_float64(M, D, rough, flags):
    """Wave and block edges in M, light counts round 32 and 64, all four flag combinations, roughness down to the denominator's
    lower clamp; the designed rows (light_reference.surface_rows): an empty row between covered ones, N.V zero, 1e-7, negative."""
    g, v, cells = L.surface_rows(M, D, rough)
    ref = L.light_gbuffer(g, v, cells, 0.04, flags, np.float64)
    bound = 10 * L.distance(L.light_gbuffer(g, v, cells, 0.04, flags, np.float32), ref)
    got = device_light(g, v, cells, 0.04, flags)
    d = L.distance(got, ref)
    print(f"\n[light gbuffer M {M} D {D} roughness {rough} flags {flags}] device {d:.2e} (bound {bound:.2e})")
    assert got.shape == (M, 4) and np.isfinite(got).all()
    assert d <= bound
    assert np.array_equal(got[:, 3], g[:, 8])
    if M > 2:
        assert (got[1] == 0).all() and (got[0] != 0).any()


def test_horizon_threshold_is_exact():
    """n.L in {0, 2^-20, 2^-19, -2^-19}, exact products: only 2^-19 > 1e-6 contributes, and the result equals the float32
    restatement's bit for bit (light_reference.horizon_case says why it can)."""
    g, v, cells = L.horizon_case()
    for flags in (0, 1):
        want = L.light_gbuffer(g, v, cells, 0.04, flags, np.float32)
        got = device_light(g, v, cells, 0.04, flags)
        assert np.array_equal(got, want), (flags, got, want)
        assert np.array_equal(got, device_light(g, v, cells[2:3], 0.04, flags)) and (got[0, :3] > 0).all()
    for only in (0, 1, 3):
        assert (device_light(g, v, cells[only:only + 1], 0.04, 0)[0, :3] == 0).all()


def test_light_gbuffer_repeats():
    g, v, cells = L.surface_rows(257, 67, 0.5)
    a, b = device_light(g, v, cells), device_light(g, v, cells)
    assert np.array_equal(a, b)
    perm = np.random.default_rng(0).permutation(257)
    c = device_light(g[perm], v[perm], cells)
    undone = np.empty_like(c)
    undone[perm] = c
    assert np.array_equal(undone, a)


def test_entries_validate_before_any_device_work():
    """Host addresses throughout: every call below must be refused on the host (an accepted one would launch on host memory)."""
    from tensoir_amd import _lib
    lib = _lib.lib()
    keep = torch.zeros(64, dtype=torch.float32)
    ptr = keep.data_ptr()
    assert ptr % 16 == 0
    ARG, UNSUPPORTED = -1001, -1002
    f = lib.tir_light_gbuffer
    assert f(None, ptr, ptr, 4, 8, 0.04, 0, ptr, None) == ARG
    assert f(ptr, None, ptr, 4, 8, 0.04, 0, ptr, None) == ARG
    assert f(ptr, ptr, None, 4, 8, 0.04, 0, ptr, None) == ARG
    assert f(ptr, ptr, ptr, 4, 8, 0.04, 0, None, None) == ARG
    assert f(ptr, ptr, ptr, -1, 8, 0.04, 0, ptr, None) == ARG
    assert f(ptr, ptr, ptr, 4, 0, 0.04, 0, ptr, None) == ARG
    assert f(ptr, ptr, ptr, 4, 8, 0.04, 4, ptr, None) == ARG                    # an unknown flag bit
    assert f(ptr, ptr, ptr, 4, 8, 0.04, -1, ptr, None) == ARG
    assert f(ptr + 4, ptr, ptr, 4, 8, 0.04, 0, ptr, None) == ARG                # gbuf, cells, out: 16-byte aligned
    assert f(ptr, ptr, ptr + 8, 4, 8, 0.04, 0, ptr, None) == ARG
    assert f(ptr, ptr, ptr, 4, 8, 0.04, 0, ptr + 4, None) == ARG
    assert f(ptr, ptr, ptr, 4, (1 << 20) + 1, 0.04, 0, ptr, None) == UNSUPPORTED
    assert f(None, None, None, 0, 8, 0.04, 3, None, None) == 0                  # M = 0: nothing to do
    e = lib.tir_env_cells
    assert e(None, 8, 16, ptr, 4, 8, ptr, None) == ARG
    assert e(ptr, 8, 16, None, 4, 8, ptr, None) == ARG
    assert e(ptr, 8, 16, ptr, 4, 8, None, None) == ARG
    assert e(ptr, 8, 16, ptr, 4, 8, ptr + 4, None) == ARG
    assert e(ptr, 8, 16, ptr, 3, 8, ptr, None) == ARG                           # 8 is no multiple of 3
    assert e(ptr, 8, 16, ptr, 4, 5, ptr, None) == ARG
    assert e(ptr, 8, 16, ptr, 0, 8, ptr, None) == ARG
    assert e(ptr, 0, 16, ptr, 4, 8, ptr, None) == ARG
    assert e(ptr, 1 << 15, 1 << 14, ptr, 4, 8, ptr, None) == UNSUPPORTED
    assert C.sizeof(C.c_float) == 4


@pytest.mark.parametrize("name", list(L.CELL_CASES))
def test_env_cells_against_float64(name):
    from tensoir_amd import ops
    hdr, h, w = L.cell_case(name)
    ref = L.env_cells(hdr, h, w, np.float64)
    bound = 10 * L.distance(L.env_cells(hdr, h, w, np.float32), ref)
    got = ops.env_cells(dev(hdr), h, w).cpu().numpy()
    d = L.distance(got, ref)
    print(f"\n[light cells {name}] device {d:.2e} (bound {bound:.2e}), sum of solid angles / 4 pi - 1 = "
          f"{got[:, 3].astype(np.float64).sum() / (4 * np.pi) - 1:.2e}")
    assert got.shape == (h * w, 8) and d <= bound and (got[:, 7] == 0).all()
    assert abs(got[:, 3].astype(np.float64).sum() / (4 * np.pi) - 1) < 1e-6
    assert np.abs(got[:, 0:3].astype(np.float64) - ref[:, 0:3]).max() < 5e-7          # directions on their own: sinf / cosf of an fp32 angle
    assert np.array_equal(got, ops.env_cells(dev(hdr), h, w).cpu().numpy())
    with pytest.raises(ValueError):
        ops.env_cells(dev(hdr), hdr.shape[0] + 1, w)


# ---- end to end on the sphere ---------------------------------------------------------------------------------------------------------
def _sphere():
    from tensoir_amd import raster
    pos, nrm, c2w, focal, W, H = R.sphere_case("sphere-64")
    tan, uv, images = R.shade_inputs(13)
    mesh = (dev(pos), dev(nrm), dev(tan), dev(uv), dict(zip(raster.IMAGE_NAMES, images)))
    return mesh, c2w, float(focal), W, H


def _gbuffer(out):
    n = out["coverage"].numel()
    g = np.zeros((n, L.ROW), np.float32)
    g[:, 0:3] = out["albedo"].reshape(n, 3).cpu().numpy()
    g[:, 3], g[:, 4] = out["roughness"].reshape(n).cpu().numpy(), out["ao"].reshape(n).cpu().numpy()
    g[:, 5:8] = out["normal"].reshape(n, 3).cpu().numpy()
    g[:, 8] = out["coverage"].reshape(n).cpu().numpy()
    return g


def test_relight_mesh_on_the_sphere():
    """relight_mesh equals the float64 restatement fed with the device's own G-buffer, view vectors and cells, within the bound;
    empty pixels show the environment, tone-mapped.  Pixels with a pair within 1e-6 of the horizon threshold (where float32 and
    float64 may take different pairs) are counted and left out; the sphere view has at most a handful."""
    from tensoir_amd import ops, raster
    mesh, c2w, focal, W, H = _sphere()
    hdr = dev(L.hdr_map(16, 32, 21) * np.float32(0.05))
    cells = raster.environment_cells(hdr, rows=4)
    assert cells.shape == (32, 8)
    out = raster.relight_mesh(*mesh, cells, c2w, focal, H, W, hdr=hdr)
    plain = raster.render_mesh(*mesh, c2w, focal, H, W)
    assert sorted(out) == sorted(list(plain) + ["rgb"]) and out["rgb"].shape == (H, W, 3)
    assert all(torch.equal(out[k], plain[k]) for k in plain if k != "drops")
    g = _gbuffer(out)
    rays = raster.camera_rays(c2w, focal, H, W, "cuda")
    view = (-rays[:, 3:6]).cpu().numpy()
    cl = cells.cpu().numpy()
    stats = {}
    ref = L.light_gbuffer(g, view, cl, 0.04, 3, np.float64, stats=stats)
    f32 = L.light_gbuffer(g, view, cl, 0.04, 3, np.float32)
    m = g[:, 8] > 0
    c = L._dot(g[:, None, 5:8].astype(np.float64), cl[None, :, 0:3].astype(np.float64))
    keep = m & ~(np.abs(c - L.THRESHOLD) < 1e-6).any(1)
    assert int(m.sum()) == R.SPHERE_VIEWS["sphere-64"][4] and (m & ~keep).sum() <= 0.001 * m.sum()
    got = out["rgb"].reshape(-1, 3).cpu().numpy()
    bound = 10 * L.distance(f32[keep, :3], ref[keep, :3])
    d = L.distance(got[keep], ref[keep, :3])
    print(f"\n[light relight_mesh sphere-64] device {d:.2e} (bound {bound:.2e}), pixels left out {int((m & ~keep).sum())}, "
          f"lit range {ref[keep, :3].min():.3f} .. {ref[keep, :3].max():.3f}")
    assert d <= bound
    back = ops.env_lookup(hdr, rays[:, 3:6].contiguous()).cpu().numpy().astype(np.float64)
    # torch.pow in float32 on a value in [0, 1]: a few ulp of the result, below 1e-6 absolute
    assert np.abs(got[~m] - L.linear2srgb(back)[~m]).max() < 1e-6 and (~m).sum() > 100
    linear = raster.relight_mesh(*mesh, cells, c2w, focal, H, W, hdr=hdr, srgb=False, occlusion=False)["rgb"].reshape(-1, 3).cpu().numpy()
    assert np.array_equal(linear[~m], back[~m].astype(np.float32))
    none = raster.relight_mesh(*mesh, cells, c2w, focal, H, W)["rgb"].reshape(-1, 3).cpu().numpy()
    assert (none[~m] == 0).all() and np.array_equal(none[m], got[m])


def test_one_bright_cell_leaves_the_far_side_black():
    from tensoir_amd import raster
    mesh, c2w, focal, W, H = _sphere()
    hdr = np.zeros((8, 16, 3), np.float32)
    hdr[2:4, 6:8] = (3.0, 2.0, 1.0)                          # cell (1, 3) of the 4 x 8 grid
    cells = raster.environment_cells(hdr, rows=4)
    cl = cells.cpu().numpy()
    assert (cl[:, 4:7] != 0).any(1).tolist() == [k == 1 * 8 + 3 for k in range(32)]
    out = raster.relight_mesh(*mesh, cells, c2w, focal, H, W)
    rgb, g = out["rgb"].reshape(-1, 3).cpu().numpy(), _gbuffer(out)
    m = g[:, 8] > 0
    c = (g[:, 5] * cl[11, 0] + g[:, 6] * cl[11, 1]) + g[:, 7] * cl[11, 2]
    away, facing = m & (c < -1e-5), m & (c > 1e-5)
    assert away.sum() > 50 and facing.sum() > 50
    assert (rgb[away] == 0).all() and (rgb[~m] == 0).all() and (rgb[facing] > 0).all()


def test_environment_cells_inputs(tmp_path):
    from tensoir_amd import hdr as H, raster
    x = L.hdr_map(8, 16, 4)
    p = str(tmp_path / "e.hdr")
    H.write_hdr(p, x)
    a = raster.environment_cells(H.read_hdr(p), rows=4)
    assert torch.equal(a, raster.environment_cells(p, rows=4)) and torch.equal(a, raster.environment_cells(torch.from_numpy(H.read_hdr(p)), 4))
    with pytest.raises(ValueError):
        raster.environment_cells(x, rows=3)
    with pytest.raises(ValueError):
        raster.environment_cells(x[:, :12], rows=4)


# ---- a real asset ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    from tests.train_sequence import reconstruct
    return reconstruct()


def test_export_environment(trained, tmp_path):
    """The file, read back, equals get_light_rgbs at Environment_Light's directions within the RGBE bound."""
    from tensoir_amd import hdr, mesh, relight
    m = trained.model
    p = str(tmp_path / "light.hdr")
    written = mesh.export_environment(m, p, 8, 16)
    back = hdr.read_hdr(p)
    assert back.shape == (8, 16, 3) and written.shape == (8, 16, 3)
    env = relight.Environment_Light(hdr_maps={"recovered": back})
    with torch.no_grad():
        want = m.get_light_rgbs(env.hdr_dir["recovered"].reshape(-1, 3), device="cuda")[0].detach().reshape(8, 16, 3).cpu().numpy()
    assert (want > 0).any() and np.array_equal(want, written)
    assert (np.abs(back.astype(np.float64) - want) <= want.max(-1, keepdims=True).astype(np.float64) / 128).all()
    with pytest.raises(ValueError):
        mesh.export_environment(m, p, 8, 16, light=99)


def test_compare_asset_with_a_light(trained, tmp_path):
    """export_textured(simplify=3, size=256), 4 views at 64 x 64, light_rows=8, a seeded 16 x 32 map: relit_psnr is finite in every
    view and repeats exactly, every other number equals the report's without a light, the command line prints the same report and
    writes the same bytes.  Not measured before this test ran: on an MI355X the mean relit_psnr is recorded in DESIGN 4.9."""
    import types
    from tensoir_amd import mesh, raster
    from tensoir_amd.renderer import Renderer_TensoIR_train
    m = trained.model
    glb, cli = str(tmp_path / "scene.glb"), str(tmp_path / "cli.glb")
    mesh.export_textured(m, glb, simplify=3, size=256)
    light = L.hdr_map(16, 32, 33) * np.float32(0.05)
    npy = str(tmp_path / "light.npy")
    np.save(npy, light)
    base = raster.compare_asset(m, glb, H=64, W=64, n_views=4)
    report = raster.compare_asset(m, glb, H=64, W=64, n_views=4, light=light, light_rows=8)
    print("\n[light compare_asset] " + json.dumps(report))
    for v, b in zip(report["views"] + [report["mean"]], base["views"] + [base["mean"]]):
        assert sorted(v) == sorted(list(b) + ["relit_psnr"]) and np.isfinite(v["relit_psnr"])
        assert {k: v[k] for k in b} == b
    assert {k: report[k] for k in report if k not in ("views", "mean")} == {k: base[k] for k in base if k not in ("views", "mean")}
    assert raster.compare_asset(m, glb, H=64, W=64, n_views=4, light=npy, light_rows=8) == report
    # the field's G-buffer on both sides: the images agree exactly
    c2w = raster.orbit_cameras(m.aabb, 1, distance=0.5 * (float(m.near_far[0]) + float(m.near_far[1])))[0]
    rays = raster.camera_rays(c2w, report["focal"] / 2, 32, 32, "cuda")
    args = types.SimpleNamespace(second_nSample=96, second_near=0.05, second_far=1.5)
    ret = Renderer_TensoIR_train(rays, None, torch.zeros((rays.shape[0], 1), dtype=torch.int32, device="cuda"), m, N_samples=-1,
                                 white_bg=False, is_train=False, is_relight=True, sample_method="fixed_envirmap", device="cuda",
                                 args=args, _no_graph=True)
    g = raster.field_gbuffer(ret, rays.shape[0])
    assert int((g[:, 8] > 0).sum()) > 20
    assert raster.relit_psnr(g, g, (-rays[:, 3:6]).contiguous(), raster.environment_cells(light, 8), m.fixed_fresnel) == float("inf")
    ckpt = str(tmp_path / "trained.th")
    m.save(ckpt)
    views = str(tmp_path / "views")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tensoir_amd.bake", ckpt, cli, "--simplify", "3", "--texture-size", "256", "--check-views", "4",
                        "--check-size", "64", "--check-light", npy, "--check-light-rows", "8", "--write-views", views,
                        "--environment", str(tmp_path / "cli.hdr"), "--environment-size", "8", "16"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == report
    assert open(cli, "rb").read() == open(glb, "rb").read()
    assert sorted(os.listdir(views)) == sorted(f"view_{k:02d}_{s}.png" for k in range(4) for s in ("field", "asset"))
    assert mesh.read_png(open(os.path.join(views, "view_00_asset.png"), "rb").read()).shape == (64, 64, 4)
    from tensoir_amd import hdr
    assert hdr.read_hdr(str(tmp_path / "cli.hdr")).shape == (8, 16, 3)
