"""The dense appearance-feature volume (TirField::dense_app) and the indirect-light kernels that read it.

On a field with ONE light every axis uses one tap pair for its planes and its line, so plane x line x light row is multilinear
inside a grid cell and the linear basis_mat contraction keeps it so: the 27 radiance features at a point are the trilinear
interpolation of the features at the 8 cell corners.  tir_dense_app_build stores the corner features as fp16
([z][y][x of X + 1][half 2][16]); tir_vm_app_fwd_h16 and tir_indirect_fused_fwd look them up when the descriptor carries them.
Bounds used here:
  * volume: one fp16 rounding of the fp64 value plus the fp32 accumulation error of the 144 terms (derived from the data);
  * features: the lookup may deviate from fp64 at most 1.5 x (rms) / 2 x (max) as much as today's fp16 gather does;
  * fused kernel: < 1e-5 against the two-launch route, < 5e-4 against the exact route (the bounds of tests/test_gpu_parity.py);
  * route: every map bit-equal except rgb_with_brdf_map, which stays within 2.5e-5 (the precision policy's own limit).
TENSOIR_DENSE_APP_REPORT=<file.json>: the measured figures are merged into that file (profiles/dense_app_numerics.json)."""
import contextlib
import io
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import precision_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = (20, 24, 28)                 # unequal axes: a swapped axis in the build kernel or the lookup cannot pass
POLICY_TOL = 2.5e-5
NF0, F = 14, 27
MODES = ((0, 1, 2), (0, 2, 1), (1, 2, 0))          # (m0, m1, line axis) of plane 0, 1, 2


def _report(key, value):
    print(f"[dense_app] {key}: {json.dumps(value)}")
    path = os.environ.get("TENSOIR_DENSE_APP_REPORT")
    if not path:
        return
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = value
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)


@contextlib.contextmanager
def _switch(dense_app=None, max_mb=None, dense_sigma=None):
    from tensoir_amd import ops
    old = dict(ops.TUNE)
    for k, v in (("dense_app", dense_app), ("dense_app_max_mb", max_mb), ("dense_sigma", dense_sigma)):
        if v is not None:
            ops.TUNE[k] = v
    try:
        yield
    finally:
        ops.TUNE.clear()
        ops.TUNE.update(old)


def _model(grid=GRID, seed=20211202, mask=None):
    import tensoir_amd
    from tensoir_amd import synth
    ck = synth.make_checkpoint(grid=grid, seed=seed)
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=8, envmap_w=16)
    if mask:
        with contextlib.redirect_stdout(io.StringIO()):
            m.updateAlphaMask((mask,) * 3)
    return ck, m


@pytest.fixture(scope="module")
def small():
    """The one-light, 48-component field of the kernel-level tests, its descriptors and its fp64 corner features."""
    _, m = _model()
    st = m.dense_app_state()
    assert st["on"] and st["why"] is None and abs(st["mb"] - 64 * (GRID[0] + 1) * GRID[1] * GRID[2] / 2 ** 20) < 1e-9, st
    f_dense, f_plain, fh = m.packed_field_dense(app=True), m.packed_field(), m.packed_field_half()
    assert int(f_dense.dense_app) != 0 and int(f_dense.dense_app_pitch) == GRID[0] + 1 and int(f_plain.dense_app or 0) == 0
    assert fh is not None
    planes = [p.detach().cpu().double()[0] for p in m.app_plane]              # [48, grid[m1], grid[m0]]
    lines = [ln.detach().cpu().double()[0, :, :, 0] for ln in m.app_line]      # [48, grid[line axis]]
    basis = m.basis_mat.weight.detach().cpu().double()                         # [27, 144]
    light = m.light_line.weight.detach().cpu().double()[0]                     # [144]
    return dict(m=m, f_dense=f_dense, f_plain=f_plain, fh=fh, planes=planes, lines=lines, basis=basis, light=light)


def _taps32(x, size):
    """make_tap_q on the host: every fp32 step rounded on its own, indices clamped, out-of-range weights zero."""
    ix = ((x + 1.0) * 0.5) * torch.tensor(float(size - 1), dtype=torch.float32)
    f0 = torch.floor(ix)
    t = ix - f0
    i0 = f0.long()
    i1 = i0 + 1
    w0 = torch.where((i0 >= 0) & (i0 < size), 1.0 - t, torch.zeros_like(t))
    w1 = torch.where((i1 >= 0) & (i1 < size), t, torch.zeros_like(t))
    return i0.clamp(0, size - 1), i1.clamp(0, size - 1), w0.double(), w1.double()


def _features_fp64(s, xyz):
    """basis_mat . (bilinear(plane) * linear(line) * light row) in fp64 on the fp32 taps the kernels use -> [n, 27]."""
    xyz = xyz.cpu().float()
    tp = [_taps32(xyz[:, a], GRID[a]) for a in range(3)]
    prod = []
    for k, (m0, m1, vi) in enumerate(MODES):
        x0, x1, wx0, wx1 = tp[m0]
        y0, y1, wy0, wy1 = tp[m1]
        l0, l1, wl0, wl1 = tp[vi]
        pl, ln = s["planes"][k], s["lines"][k]
        bil = (pl[:, y0, x0] * (wx0 * wy0) + pl[:, y0, x1] * (wx1 * wy0) + pl[:, y1, x0] * (wx0 * wy1) + pl[:, y1, x1] * (wx1 * wy1))
        prod.append(bil * (ln[:, l0] * wl0 + ln[:, l1] * wl1))
    x = torch.cat(prod, 0) * s["light"][:, None]                               # [144, n]
    return (s["basis"] @ x).t().contiguous()


def _points(gen, n=6000):
    """Random points, cell corners, box faces, the last cell of each axis, points slightly outside the box (index clamp)."""
    pts = [torch.rand(n, 3, generator=gen) * 2 - 1]
    node = torch.stack([torch.randint(0, GRID[a], (n // 4,), generator=gen).float() / (GRID[a] - 1) * 2 - 1 for a in range(3)], 1)
    pts.append(node)                                                           # cell corners
    for a in range(3):
        for edge in (-1.0, 1.0):
            q = torch.rand(n // 20, 3, generator=gen) * 2 - 1
            q[:, a] = edge
            pts.append(q)                                                      # box faces
        q = torch.rand(n // 20, 3, generator=gen) * 2 - 1
        q[:, a] = 1.0 - torch.rand(n // 20, generator=gen) * 2.0 / (GRID[a] - 1)
        pts.append(q)                                                          # the last cell of the axis
    pts.append((torch.rand(n // 4, 3, generator=gen) * 2 - 1) * 1.08)          # slightly outside
    pts.append(torch.tensor([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]))
    return torch.cat(pts).contiguous()


# ---- 1. the volume against the host ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@torch.no_grad()
def test_volume_holds_the_corner_features(small):
    """Every corner against fp64 from the parameters.  Allowed: the fp32 accumulation error e32 of the kernel's sum -- each of the
    144 terms is (plane * line) * light (two roundings) and enters an FMA chain of 144 steps: (144 + 2) 2^-24 sum |B| |term| --
    plus one fp16 rounding of the accumulated value, 2^-11 (|value| + e32), and 2^-25 for a result in fp16's subnormal range."""
    s = small
    X, Y, Z = GRID
    vol = s["m"]._field_cache["dense"]["app"]["vol"]
    assert vol.shape == (Z, Y, X + 1, 2, 16) and vol.dtype == torch.float16
    v = vol.cpu()
    terms = []
    for k, (m0, m1, vi) in enumerate(MODES):
        pl, ln = s["planes"][k], s["lines"][k]                                 # pl [48, grid[m1], grid[m0]]
        shape = {0: (1, 1, 1, X), 1: (1, 1, Y, 1), 2: (1, Z, 1, 1)}
        idx = {0: torch.arange(X), 1: torch.arange(Y), 2: torch.arange(Z)}
        p = pl[:, idx[m1].view(shape[m1][1:]).expand(Z, Y, X), idx[m0].view(shape[m0][1:]).expand(Z, Y, X)]
        l_ = ln[:, idx[vi].view(shape[vi][1:]).expand(Z, Y, X)]
        terms.append(p * l_)
    x = torch.cat(terms, 0) * s["light"][:, None, None, None]                  # [144, Z, Y, X]
    ref = torch.einsum("jc,czyx->zyxj", s["basis"], x)
    mag = torch.einsum("jc,czyx->zyxj", s["basis"].abs(), x.abs())
    e32 = (144 + 2) * 2.0 ** -24 * mag
    tol = e32 + 2.0 ** -11 * (ref.abs() + e32) + 2.0 ** -25
    got = torch.cat([v[:, :, :X, 0, :NF0], v[:, :, :X, 1, :F - NF0]], -1).double()
    err = (got - ref).abs()
    _report("volume", {"corners": X * Y * Z, "feature_peak": float(ref.abs().max()), "max_err": float(err.max()),
                       "max_err_over_bound": float((err / tol).max()), "e32_peak": float(e32.max())})
    assert float(ref.abs().max()) > 1e-2                    # a field with content
    assert bool((err <= tol).all()), float((err / tol).max())
    # padding: the spare corner of every row and the slots behind a half's features are exactly zero
    assert bool((v[:, :, X] == 0).all()) and bool((v[:, :, :, 0, NF0:] == 0).all()) and bool((v[:, :, :, 1, F - NF0:] == 0).all())


# ---- 2. the features ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@torch.no_grad()
def test_lookup_deviates_little_more_than_the_fp16_gather(small):
    """ops.vm_app_h16 on the dense descriptor and on the plain one (today's fp16 gather), both against fp64.  The margins (1.5 x
    rms, 2 x max) come from a CPU emulation of the packed-fp16 lookup (0.92 x rms, at most 1.36 x max)."""
    from tensoir_amd import ops
    s = small
    xyz = _points(torch.Generator().manual_seed(5))
    ref = _features_fp64(s, xyz)
    li = torch.zeros(xyz.shape[0], dtype=torch.int32, device="cuda")
    dense = ops.vm_app_h16(s["f_dense"], s["fh"], xyz.cuda(), li).cpu()
    plain = ops.vm_app_h16(s["f_plain"], s["fh"], xyz.cuda(), li).cpu()
    assert bool((dense[:, F:] == 0).all()) and dense.shape == plain.shape == (xyz.shape[0], 32)
    dd, dp = (dense[:, :F].double() - ref), (plain[:, :F].double() - ref)
    fig = {"points": int(xyz.shape[0]), "feature_peak": float(ref.abs().max()), "feature_rms": float(ref.pow(2).mean().sqrt()),
           "rms_dense": float(dd.pow(2).mean().sqrt()), "rms_plain": float(dp.pow(2).mean().sqrt()),
           "max_dense": float(dd.abs().max()), "max_plain": float(dp.abs().max())}
    fig["rms_ratio"], fig["max_ratio"] = fig["rms_dense"] / fig["rms_plain"], fig["max_dense"] / fig["max_plain"]
    _report("features", fig)
    assert fig["feature_peak"] > 1e-2
    outside = (xyz.abs() > 1).any(1)
    far = (xyz.abs() > 1 + 2.0 / (min(GRID) - 1)).any(1)
    assert int(outside.sum()) > 100
    assert float(dense[far].abs().max()) == 0.0 if bool(far.any()) else True
    assert fig["rms_dense"] <= 1.5 * fig["rms_plain"], fig
    assert fig["max_dense"] <= 2.0 * fig["max_plain"], fig


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 385, 1000])
def test_lookup_rows_do_not_depend_on_the_launch(small, n):
    """A wave is 32 records: every row count gives the rows of the 1000-point launch bit for bit; an n_dev bound below n leaves
    the rows behind it untouched."""
    from tensoir_amd import ops
    s = small
    gen = torch.Generator().manual_seed(6)
    xyz = _points(gen, 600)
    xyz = xyz[torch.randperm(xyz.shape[0], generator=gen)[:1000]].cuda().contiguous()
    li = torch.zeros(1000, dtype=torch.int32, device="cuda")
    whole = ops.vm_app_h16(s["f_dense"], s["fh"], xyz, li)
    part = ops.vm_app_h16(s["f_dense"], s["fh"], xyz[:n].contiguous(), li[:n].contiguous())
    assert part.shape == (n, 32) and torch.equal(part, whole[:n])
    if n > 1:
        k = n - max(1, n // 3)
        n_dev = torch.tensor([k], dtype=torch.int32, device="cuda")
        C = __import__("ctypes")
        out = torch.full((n, 32), -7.0, device="cuda")
        rc = ops._lib.lib().tir_vm_app_fwd_h16(C.byref(s["f_dense"]), C.byref(s["fh"]), xyz.data_ptr(), li.data_ptr(), None, out.data_ptr(),
                                               32, 0, n, n_dev.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(out[:k], whole[:k]) and bool((out[k:] == -7.0).all())


# ---- 3. the fused kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 385, 1000])
def test_fused_kernel_on_the_dense_descriptor(small, n):
    """k_indirect_fused_dense (a tile is 384 records) against the two launches on the same descriptor (1e-5) and against the
    exact route, fp32 gather + mfma decoder (5e-4); n_dev; out-of-range light indices."""
    import ctypes as C
    from tensoir_amd import ops
    s = small
    m, fd, fh = s["m"], s["f_dense"], s["fh"]
    pm = m.renderModule.packed()
    gen = torch.Generator().manual_seed(100 + n)
    D, npt = 3, 40
    dirs = torch.nn.functional.normalize(torch.randn(D, 3, generator=gen), dim=-1).cuda()
    pts = _points(gen, 600)
    pts = pts[torch.randperm(pts.shape[0], generator=gen)[:n]].cuda().contiguous()
    assert pts.shape[0] == n
    pair = torch.randint(0, npt * D, (n,), generator=gen).int().cuda()
    lpt = torch.zeros(npt, dtype=torch.int32, device="cuda")
    odd = torch.tensor([0, -1, 5, 0] * (npt // 4), dtype=torch.int32, device="cuda")
    one = ops.indirect_fused(fd, fh, pm, pts, lpt, pair, D, dirs, D)
    assert one.shape == (n, 3) and bool(torch.isfinite(one).all())
    if n == 0:
        return
    assert torch.equal(ops.indirect_fused(fd, fh, pm, pts, odd, pair, D, dirs, D), one)          # one light: every index is row 0
    exact = ops.mlp(pm, ops.vm_app(s["f_plain"], pts, lpt, pair, True, False, "mfma", D)[0], dirs, pair, "mfma", D)
    e1 = float((one - exact).abs().max())
    e2 = None
    if D * 8 <= n:                                                              # the two-launch route takes its aux-table decoder
        two = ops.mlp(pm, ops.vm_app_h16(fd, fh, pts, lpt, pair, D), dirs, pair, "f16", D)
        e2 = float((one - two).abs().max())
    _report(f"fused/n={n}", {"fused_vs_two_launches": e2, "fused_vs_exact": e1})
    assert e1 < 5e-4 and (e2 is None or e2 < 1e-5), (n, e1, e2)
    if n > 1:
        k = n - max(1, n // 3)
        n_dev = torch.tensor([k], dtype=torch.int32, device="cuda")
        table = ops._aux_table_cached(pm, dirs)
        out = torch.full((n, 3), -7.0, device="cuda")
        rc = ops._lib.lib().tir_indirect_fused_fwd(C.byref(fd), C.byref(fh), C.byref(pm.desc), pts.data_ptr(), lpt.data_ptr(), pair.data_ptr(),
                                                   D, D, table.data_ptr(), out.data_ptr(), n, n_dev.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(out[:k], one[:k]) and bool((out[k:] == -7.0).all())


# ---- 4. route level -------------------------------------------------------------------------------------------------------------------
def _scene96():
    """The scene of test_graph_replay_follows_the_verdict: 96^3, 48 x 48 rays."""
    from tensoir_amd import synth
    _, m = _model((96,) * 3, mask=96)
    rays = synth.make_rays(48, 48).cuda()
    lidx = torch.zeros(rays.shape[0], 1, dtype=torch.int32, device="cuda")
    kw = dict(N_samples=-1, white_bg=True, is_train=False, is_relight=True, sample_method="fixed_envirmap", device="cuda", args=P.ARGS)
    return m, rays, lidx, kw


@pytest.fixture(scope="module")
def scene96():
    return _scene96()


def _render(scene, dense_app):
    from tensoir_amd import Renderer_TensoIR_train, indirect
    m, rays, lidx, kw = scene
    with _switch(dense_app=dense_app), P.policy(True), torch.no_grad():
        assert m.dense_app_state()["on"] == bool(dense_app)
        indirect.reset(m)
        out = Renderer_TensoIR_train(rays, None, lidx, m, **kw)
        return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}, m.indirect_precision()


def _check_route(on, off, what):
    assert set(on) == set(off) and "rgb_with_brdf_map" in on
    for k in on:
        # (the two smoothness losses come from the device-side jitter draw, which differs from render to render: bench.py's
        #  output dump and the parity checks leave them out for the same reason)
        if k not in ("rgb_with_brdf_map", "albedo_smoothness_loss", "roughness_smoothness_loss"):
            assert torch.equal(on[k], off[k]), (what, k)
    d = float((on["rgb_with_brdf_map"] - off["rgb_with_brdf_map"]).abs().max())
    assert d <= POLICY_TOL, (what, d)
    return d


@pytest.mark.gpu
def test_render_with_and_without_the_volume(scene96):
    on, dec_on = _render(scene96, 1)
    off, dec_off = _render(scene96, 0)
    d = _check_route(on, off, "render")
    _report("route/96", {"rgb_with_brdf_map_max_abs": d, "verdict_on": dec_on["mode"], "verdict_off": dec_off["mode"],
                         "probe_on": dec_on.get("probe"), "probe_off": dec_off.get("probe")})
    assert dec_on["mode"] == "f16" and dec_off["mode"] == "f16", (dec_on, dec_off)
    assert float(on["rgb_with_brdf_map"].std()) > 1e-3


# ---- 5. switches and fallbacks --------------------------------------------------------------------------------------------------------
def _radiance(m, pts, dirs, li):
    from tensoir_amd import relight
    with P.policy(False):                                    # forced f16 tier: the route under test, no probe
        m.__dict__.pop("_rec_cap_hints", None)
        return relight.compute_radiance(m, pts, dirs, li, nSample=96, vis_near=0.05, vis_far=1.5)


def _pairs(seed, n=6000):
    gen = torch.Generator().manual_seed(seed)
    pts = (torch.rand(n, 3, generator=gen) * 1.2 - 0.6).cuda()
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1).cuda()
    return pts, dirs, torch.zeros(n, dtype=torch.int32, device="cuda")


@pytest.mark.gpu
@torch.no_grad()
def test_switch_cap_and_lights_fall_back_to_the_shadow_taps():
    import tensoir_amd
    from tensoir_amd import ops, relight
    from tests import config_scenes as CS
    _, m = _model((64,) * 3, seed=3, mask=64)
    pts, dirs, li = _pairs(1)
    z = relight._z_table(96, 0.05, 1.5, "cuda")

    def present_route():
        """Today's route spelled out: the march on the density-volume descriptor, the fused kernel on a descriptor WITHOUT the
        appearance volume."""
        f = m.packed_field_dense()
        assert int(f.dense_app or 0) == 0
        vis, _, rec = ops.march_secondary(f, pts, dirs, z, pts.shape[0], None, None, None, m.march_t_stop, True, 1 << 20, True, 0)
        n = int(rec["counter"][0])
        rgb = ops.mlp(m.renderModule.packed(), ops.vm_app_h16(f, m.packed_field_half(), rec["xyz"][:n], li, rec["ray"][:n]),
                      dirs, rec["ray"][:n], "f16", 0)
        return vis, ops.accumulate_records(rec["off"], rec["cnt"], rec["w"][:n], rgb, pts.shape[0])

    st = m.dense_app_state()
    assert st["on"] and st["why"] is None and abs(st["mb"] - 64 * 65 * 64 * 64 / 2 ** 20) < 1e-9, st
    on = _radiance(m, pts, dirs, li)
    assert float(on[2].abs().max()) > 0
    offs = []
    for kw, why in ((dict(dense_app=0), "switched off"), (dict(max_mb=16), "above the size cap"),
                    (dict(dense_sigma=0), "no dense density volume")):
        with _switch(**kw):
            st = m.dense_app_state()
            assert not st["on"] and st["why"] == why, st
            f = m.packed_field_dense(app=True)
            assert int(f.dense_app or 0) == 0 and f is m.packed_field_dense()
            offs.append(_radiance(m, pts, dirs, li))
    assert torch.equal(offs[0][0], offs[1][0]) and torch.equal(offs[0][2], offs[1][2])          # switch and cap: the same route
    vis, ind = present_route()
    assert torch.equal(offs[0][0], vis) and torch.equal(offs[0][2], ind)
    assert float((on[2] - offs[0][2]).abs().max()) < 5e-4 and not torch.equal(on[2], offs[0][2])
    assert m.dense_app_state()["on"]                         # the switches are read per call: back on
    assert torch.equal(_radiance(m, pts, dirs, li)[2], on[2])
    assert m.dense_app_state(training=True) == {"on": False, "why": "training pass", "mb": st["mb"]}
    # several lights: one volume cannot hold their features
    row = CS.ROW["d16_a48_l9"]
    ml = tensoir_amd.model_from_checkpoint(CS.checkpoint(row), "cuda", envmap_h=CS.ENVMAP_HW[0], envmap_w=CS.ENVMAP_HW[1])
    st = ml.dense_app_state()
    assert not st["on"] and st["why"] == "several lights", st
    assert ml.packed_field_dense(app=True) is ml.packed_field_dense()
    lil = torch.randint(0, 9, (pts.shape[0],), generator=torch.Generator().manual_seed(2)).int().cuda()
    a = _radiance(ml, pts, dirs, lil)
    with _switch(dense_app=0):
        b = _radiance(ml, pts, dirs, lil)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


@pytest.mark.gpu
def test_training_pass_keeps_the_shadow_taps(scene96):
    """A pass that differentiates (maps.requires_grad) takes packed_field(): same bits with the switch on and off."""
    from tensoir_amd import relight
    m, rays, lidx, _ = scene96
    res = []
    for on in (1, 0):
        with _switch(dense_app=on), P.policy(False):
            with torch.no_grad():
                noise = torch.randn(rays.shape[0], int(m.nSamples), 3, generator=torch.Generator().manual_seed(0))
                _, maps = m(rays, lidx, _brdf_jitter_dense=noise, _return_maps=True)
            maps = maps.detach().clone().requires_grad_(True)
            with torch.enable_grad():
                res.append(relight.shade_from_maps(m, maps, rays, lidx, "fixed_envirmap", P.ARGS, acc_thres=0.5).detach())
    assert torch.equal(res[0], res[1])
    assert m.dense_app_state(training=True)["why"] == "training pass"


def test_environment_switches_reach_ops_tune():
    """TENSOIR_DENSE_APP / TENSOIR_DENSE_APP_MAX_MB are read once at import, like the other launch options."""
    code = "from tensoir_amd import ops; print(ops.TUNE['dense_app'], ops.TUNE['dense_app_max_mb'])"
    for env, want in (({}, "1 4096"), ({"TENSOIR_DENSE_APP": "0"}, "0 4096"), ({"TENSOIR_DENSE_APP_MAX_MB": "64"}, "1 64")):
        e = {k: v for k, v in os.environ.items() if not k.startswith("TENSOIR_DENSE_APP")}
        e.update(env)
        out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, env=e).decode().split("\n")
        assert want in [ln.strip() for ln in out], (env, out)


# ---- 6. staleness -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_parameter_edits_rebuild_the_volume():
    """In-place edits (same storage, next version) of an appearance plane, of basis_mat and of the light row each drop the
    volume; the render follows the new parameters and stays within the route bound of the render without a volume."""
    scene = _scene96()                                       # (a model of its own: the edits stay here)
    m = scene[0]
    before, _ = _render(scene, 1)
    for what, edit in (("app_plane", lambda: m.app_plane[1].mul_(1.3)), ("basis_mat", lambda: m.basis_mat.weight.mul_(0.8)),
                       ("light_line", lambda: m.light_line.weight.add_(0.05))):
        assert m.dense_app_state()["on"]                     # (the render without a volume has dropped it: built again here)
        vol0 = m._field_cache["dense"]["app"]["vol"]
        assert vol0 is not None
        with torch.no_grad():
            edit()
        on, _ = _render(scene, 1)
        assert m._field_cache["dense"]["app"]["vol"] is not vol0, what
        off, _ = _render(scene, 0)
        _check_route(on, off, what)
        assert not torch.equal(on["rgb_with_brdf_map"], before["rgb_with_brdf_map"]), what
        before = on


@pytest.mark.gpu
@torch.no_grad()
def test_graph_recaptures_and_needs_a_built_volume():
    from tensoir_amd import Renderer_TensoIR_train
    from tensoir_amd._lib import TensoirHipError
    from tensoir_amd.graph import GraphedRenderer
    m, rays, lidx, kw = _scene96()
    with P.policy(True):
        gr = GraphedRenderer(m, rays.shape[0], args=P.ARGS)
        a = gr(rays, lidx)["rgb_with_brdf_map"].clone()
        assert gr.captures == 1 and m.dense_app_state()["on"]
        assert torch.equal(gr(rays, lidx)["rgb_with_brdf_map"], a)                                   # two replays, same bits
        assert torch.equal(Renderer_TensoIR_train(rays, None, lidx, m, **kw)["rgb_with_brdf_map"], a)
        m.app_plane[0].mul_(1.2)
        b = gr(rays, lidx)["rgb_with_brdf_map"].clone()
        assert gr.captures == 2 and not torch.equal(a, b)
        assert torch.equal(Renderer_TensoIR_train(rays, None, lidx, m, **kw)["rgb_with_brdf_map"], b)
        with _switch(dense_app=0):
            c = gr(rays, lidx)["rgb_with_brdf_map"].clone()
            assert gr.captures == 3
            assert torch.equal(Renderer_TensoIR_train(rays, None, lidx, m, **kw)["rgb_with_brdf_map"], c)
        assert float((b - c).abs().max()) <= POLICY_TOL
        # a capture may not build the volume: its launch would become a node of the graph, its memory part of the graph's pool
        m._field_cache["dense"].pop("app")
        x = torch.zeros(8, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            x.add_(1.0)
            with pytest.raises(TensoirHipError, match="dense appearance volume"):
                m.packed_field_dense(app=True)
        assert m.dense_app_state()["on"]
