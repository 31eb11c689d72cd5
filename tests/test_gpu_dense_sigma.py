"""The dense density-feature volume (TirField::dense_sigma) and the secondary march that reads it.

Inside a grid cell the VM density feature is multilinear in (x, y, z), so the trilinear lookup of the volume
V[z][y][x] = feature(corner) equals it in real arithmetic; in fp32 the two differ by rounding.  Bounds used here:
  * feature level: the lookup may deviate from an fp64 evaluation (on the same fp32 taps) at most 2 x as much as ops.vm_density does;
  * route level: visibility, 1 - acc and indirect radiance agree with the VM route within a quarter of the project's parity
    tolerance (2.5e-5 on rel_err), the convention of the precision policy for a substituted kernel; record counts within 1e-4.
TENSOIR_DENSE_SIGMA_REPORT=<file.json>: the measured figures are merged into that file (profiles/*_dense_sigma_numerics.json)."""
import contextlib
import copy
import io
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.helpers import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUARTER_TOL = 2.5e-5


def _report(key, value):
    print(f"[dense_sigma] {key}: {json.dumps(value)}")
    path = os.environ.get("TENSOIR_DENSE_SIGMA_REPORT")
    if not path:
        return
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = value
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)


@contextlib.contextmanager
def _switch(dense_sigma=None, max_mb=None):
    from tensoir_amd import ops
    old = dict(ops.TUNE)
    if dense_sigma is not None:
        ops.TUNE["dense_sigma"] = dense_sigma
    if max_mb is not None:
        ops.TUNE["dense_sigma_max_mb"] = max_mb
    try:
        yield
    finally:
        ops.TUNE.clear()
        ops.TUNE.update(old)


def _model(grid, seed=20211202, mask=False, **kw):
    import tensoir_amd
    from tensoir_amd import synth
    ck = synth.make_checkpoint(grid=grid, seed=seed, **kw)
    m = tensoir_amd.model_from_checkpoint(ck, "cuda", envmap_h=8, envmap_w=16)
    if mask:
        with contextlib.redirect_stdout(io.StringIO()):
            m.updateAlphaMask((128, 128, 128))
    return ck, m


# ---- feature level ---------------------------------------------------------------------------------------------------------------
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


def _vm_feature_fp64(m, xyz):
    """sum_i sum_c bilinear(plane_i,c) * linear(line_i,c) in fp64 on the fp32 taps the kernels use."""
    xyz = xyz.cpu().float()
    grid = [int(g) for g in m.gridSize.tolist()]
    tp = [_taps32(xyz[:, a], grid[a]) for a in range(3)]
    out = torch.zeros(xyz.shape[0], dtype=torch.float64)
    for i, (m0, m1, vi) in enumerate(((0, 1, 2), (0, 2, 1), (1, 2, 0))):
        plane = m.density_plane[i].detach().cpu().double()[0]          # [C, grid[m1], grid[m0]]
        line = m.density_line[i].detach().cpu().double()[0, :, :, 0]   # [C, grid[vi]]
        x0, x1, wx0, wx1 = tp[m0]
        y0, y1, wy0, wy1 = tp[m1]
        l0, l1, wl0, wl1 = tp[vi]
        bil = (plane[:, y0, x0] * (wx0 * wy0) + plane[:, y0, x1] * (wx1 * wy0)
               + plane[:, y1, x0] * (wx0 * wy1) + plane[:, y1, x1] * (wx1 * wy1))
        lin = line[:, l0] * wl0 + line[:, l1] * wl1
        out += (bil * lin).sum(0)
    return out


def _feature_points(grid, gen, n=200_000):
    """Random points of the box + points on cell faces (one coordinate on a grid node) + points on the first / last row of
    each axis (coordinate exactly -1 / 1) + the eight box corners."""
    pts = [torch.rand(n, 3, generator=gen) * 2 - 1]
    for a in range(3):
        p = torch.rand(n // 10, 3, generator=gen) * 2 - 1
        node = torch.randint(0, grid[a], (n // 10,), generator=gen).float()
        p[:, a] = node / float(grid[a] - 1) * 2 - 1
        pts.append(p)
        for edge in (-1.0, 1.0):
            q = torch.rand(n // 20, 3, generator=gen) * 2 - 1
            q[:, a] = edge
            pts.append(q)
    pts.append(torch.tensor([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]))
    return torch.cat(pts).clamp(-1, 1).contiguous()


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("n_dcomp", [16, 4, 8, 32])
def test_dense_feature_deviates_no_more_than_twice_the_vm_gather(n_dcomp):
    from tensoir_amd import ops
    grid = (45, 52, 39)                                      # unequal axes: a swapped axis in the build kernel cannot pass
    _, m = _model(grid, seed=11 + n_dcomp, density_n_comp=(n_dcomp,) * 3)
    xyz = _feature_points(grid, torch.Generator().manual_seed(5))
    ref = _vm_feature_fp64(m, xyz)
    st = m.dense_sigma_state()
    assert st["on"], st
    fd = m.packed_field_dense()
    assert int(fd.dense_pitch) == grid[0] + 1 and int(fd.dense_sigma) != 0
    dense = ops.dense_sigma(fd, xyz.cuda())[0].cpu().double()
    vm = ops.vm_density(m.packed_field(), xyz.cuda())[0].cpu().double()
    dev_dense, dev_vm = float((dense - ref).abs().max()), float((vm - ref).abs().max())
    _report(f"feature/n_dcomp={n_dcomp}", {"points": int(xyz.shape[0]), "feature_peak": float(ref.abs().max()),
                                           "max_dev_dense": dev_dense, "max_dev_vm": dev_vm,
                                           "rms_dev_dense": float((dense - ref).pow(2).mean().sqrt()),
                                           "rms_dev_vm": float((vm - ref).pow(2).mean().sqrt())})
    assert float(ref.abs().max()) > 1e-2                    # a field with content
    assert dev_dense <= 2.0 * dev_vm, (dev_dense, dev_vm)
    # the activation is the march's own: the same softplus on the looked-up feature
    sig = ops.dense_sigma(fd, xyz.cuda(), want_feat=False, want_sigma=True)[1].cpu().double()
    want = torch.nn.functional.softplus(dense + float(m.density_shift))
    assert rel_err(sig, want) <= 1e-6


@pytest.mark.gpu
@torch.no_grad()
def test_points_outside_the_grid_take_zero_weight_corners():
    """make_tap_q's masking carried over: beyond the last corner and in front of the first one the out-of-range corner of a
    pair has weight 0 (zero padding), further out the feature is 0 -- as in the VM gather, whose every term carries the
    same masked weights."""
    from tensoir_amd import ops
    grid = (20, 24, 17)
    _, m = _model(grid, seed=3)
    gen = torch.Generator().manual_seed(9)
    xyz = (torch.rand(50_000, 3, generator=gen) * 2 - 1) * 1.3
    ref = _vm_feature_fp64(m, xyz)
    dense = ops.dense_sigma(m.packed_field_dense(), xyz.cuda())[0].cpu().double()
    vm = ops.vm_density(m.packed_field(), xyz.cuda())[0].cpu().double()
    outside = (xyz.abs() > 1).any(dim=1)
    assert int(outside.sum()) > 1000
    dev_dense, dev_vm = float((dense - ref).abs().max()), float((vm - ref).abs().max())
    _report("feature/outside_the_grid", {"max_dev_dense": dev_dense, "max_dev_vm": dev_vm})
    assert dev_dense <= 2.0 * dev_vm, (dev_dense, dev_vm)
    far = (xyz.abs() > 1 + 2.0 / (min(grid) - 1)).any(dim=1)
    assert int(far.sum()) > 100 and float(dense[far].abs().max()) == 0.0


# ---- route level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("grid", [300, 400])
def test_dense_route_agrees_with_the_vm_route(grid):
    """The scene of test_lds_staged_lines_march_is_bit_identical: compute_radiance / compute_transmittance with the volume
    on and off."""
    from tensoir_amd import relight
    _, m = _model((grid,) * 3, mask=True)
    gen = torch.Generator().manual_seed(17)
    P = 40_000 + 37
    pts = (torch.rand(P, 3, generator=gen) * 2 - 1).mul(1.1).cuda()
    dirs = torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1).cuda()
    li = torch.zeros(P, 1, dtype=torch.int32, device="cuda")
    res, recs = {}, {}
    for on in (1, 0):
        with _switch(dense_sigma=on):
            assert m.dense_sigma_state()["on"] == bool(on)
            m.__dict__.pop("_rec_cap_hints", None)
            v, nf, ind = relight.compute_radiance(m, pts, dirs, li, nSample=96, vis_near=0.05, vis_far=1.5)
            v2, nf2, ind2 = relight.compute_radiance(m, pts, dirs, li, nSample=96, vis_near=0.05, vis_far=1.5)   # hinted route
            v3, nf3, ind3 = relight.compute_radiance(m, pts, dirs, li, nSample=96, vis_near=0.05, vis_far=1.5)
            t, tn = relight.compute_transmittance(m, pts, dirs, nSample=57, vis_near=0.05, vis_far=1.5)
            tl, tnl = relight.compute_transmittance(m, pts, dirs, nSample=200, vis_near=0.05, vis_far=1.5)   # > 96: visibility only
            res[on] = dict(vis=v, one_minus_acc=nf, indirect=ind, vis_t57=t, one_minus_acc_t57=tn, vis_t200=tl,
                           one_minus_acc_t200=tnl)
            # call to call, bit for bit: the march's own outputs from the first call on, indirect radiance between calls that
            # decode alike.  The first call of a problem size sizes the record rows to the count it has just read back, a hinted
            # call to the learnt capacity, and ops.mlp picks the aux-table decoder from the row count (8 x aux rows <= rows:
            # here 320 k lies between the count and the capacity) -- on the VM route as on this one.
            assert torch.equal(v, v2) and torch.equal(nf, nf2)
            assert torch.equal(v2, v3) and torch.equal(nf2, nf3) and torch.equal(ind2, ind3)
            f = m.packed_field_dense()
            from tensoir_amd import ops
            z = relight._z_table(96, 0.05, 1.5, "cuda")
            _, _, rec = ops.march_secondary(f, pts, dirs, z, P, None, None, None, m.march_t_stop, True, 4_000_000, False, 0)
            recs[on] = int(rec["counter"][0])
    errs = {k: rel_err(res[1][k], res[0][k]) for k in res[1]}
    diff = abs(recs[1] - recs[0]) / max(recs[0], 1)
    _report(f"route/grid={grid}", {"rel_err": errs, "records_vm": recs[0], "records_dense": recs[1], "records_rel_diff": diff})
    assert float(res[0]["vis"].min()) < 0.01 and float(res[0]["vis"].max()) > 0.99 and float(res[0]["indirect"].abs().max()) > 0
    assert recs[0] > 10_000
    for k, e in errs.items():
        assert e <= QUARTER_TOL, (k, e)
    assert diff < 1e-4, (recs, diff)


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("n_dcomp", [4, 8, 32])
def test_dense_march_serves_every_component_count(n_dcomp):
    """The volume does not care about the component count: records (<= 96 samples) and visibility-only (up to 256) launches on
    fields the LDS-staged kernel does not serve, against the plain VM kernel; pair lists; a ray's result does not depend on the
    rays it shares a launch with (halves == whole, bit for bit)."""
    from tensoir_amd import ops, relight
    _, m = _model((64, 72, 56), seed=100 + n_dcomp, mask=True, density_n_comp=(n_dcomp,) * 3)
    gen = torch.Generator().manual_seed(n_dcomp)
    P = 9_000 + 13
    pts = (torch.rand(P, 3, generator=gen) * 2 - 1).mul(1.1).cuda()
    dirs = torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1).cuda()
    fv, fd = m.packed_field(), m.packed_field_dense()
    assert fd is not fv and int(fd.dense_sigma) != 0
    worst = {}
    for n_sample, rec in ((96, True), (33, True), (96, False), (256, False)):
        z = relight._z_table(n_sample, 0.05, 1.5, "cuda")
        out = {}
        for name, f in (("vm", fv), ("dense", fd)):
            out[name] = ops.march_secondary(f, pts, dirs, z, P, None, None, None, m.march_t_stop, rec, 2_000_000 if rec else 0, True, 0)
        worst[f"{n_sample}/{'rec' if rec else 'vis'}"] = max(rel_err(out["dense"][0], out["vm"][0]), rel_err(out["dense"][1], out["vm"][1]))
        if rec:
            a, b = int(out["vm"][2]["counter"][0]), int(out["dense"][2]["counter"][0])
            assert a > 1000 and abs(a - b) <= max(1, int(1e-4 * a)), (a, b)
            # per-ray record segments: same weights within the tolerance wherever the counts agree
            ca, cb = out["vm"][2]["cnt"], out["dense"][2]["cnt"]
            assert float((ca != cb).float().mean()) < 1e-3
        # halves == whole on the dense route, launches of the same kind (the record and the visibility-only instantiation
        # are two compilations of the body: each is compared with itself)
        h = P // 2 + 5
        cap = 2_000_000 if rec else 0
        va = ops.march_secondary(fd, pts[:h], dirs[:h], z, h, None, None, None, m.march_t_stop, rec, cap, True, 0)
        vb = ops.march_secondary(fd, pts[h:], dirs[h:], z, P - h, None, None, None, m.march_t_stop, rec, cap, True, 0)
        assert torch.equal(torch.cat([va[0], vb[0]]), out["dense"][0]) and torch.equal(torch.cat([va[1], vb[1]]), out["dense"][1])
        if rec:
            assert torch.equal(torch.cat([va[2]["cnt"], vb[2]["cnt"]]), out["dense"][2]["cnt"])
        # a shuffled pair list addresses the same rays
        ids = torch.randperm(P, generator=gen).to(torch.int32).cuda()
        n_ids = torch.full((1,), P, dtype=torch.int32, device="cuda")
        vl = ops.march_secondary(fd, pts, dirs, z, P, None, None, None, m.march_t_stop, rec, cap, True, 0, ray_ids=ids, n_ids_dev=n_ids)
        assert torch.equal(vl[0], out["dense"][0]) and torch.equal(vl[1], out["dense"][1])
        if rec:
            assert torch.equal(vl[2]["cnt"], out["dense"][2]["cnt"])
    _report(f"march/n_dcomp={n_dcomp}", worst)
    assert max(worst.values()) <= QUARTER_TOL, worst


# ---- cache and switches ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@torch.no_grad()
def test_parameter_change_rebuilds_the_volume():
    import tensoir_amd
    from tensoir_amd import relight
    ck, m = _model((64, 64, 64), seed=7)
    gen = torch.Generator().manual_seed(1)
    P = 6_000
    pts = (torch.rand(P, 3, generator=gen) * 2 - 1).mul(1.1).cuda()
    dirs = torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1).cuda()
    before = relight.compute_transmittance(m, pts, dirs, nSample=96, vis_near=0.05, vis_far=1.5)
    vol0 = m._field_cache["dense"]["vol"]
    assert vol0 is not None and m.packed_field_dense() is m.packed_field_dense()      # cached: one descriptor, one volume
    m.density_line[0].mul_(1.7)                            # in place (no_grad): same storage, new version
    m.density_plane[2].add_(0.01)
    after = relight.compute_transmittance(m, pts, dirs, nSample=96, vis_near=0.05, vis_far=1.5)
    assert m._field_cache["dense"]["vol"] is not vol0
    ck2 = copy.deepcopy(ck)
    ck2["state_dict"]["density_line.0"] = ck2["state_dict"]["density_line.0"] * 1.7
    ck2["state_dict"]["density_plane.2"] = ck2["state_dict"]["density_plane.2"] + 0.01
    fresh = tensoir_amd.model_from_checkpoint(ck2, "cuda", envmap_h=8, envmap_w=16)
    want = relight.compute_transmittance(fresh, pts, dirs, nSample=96, vis_near=0.05, vis_far=1.5)
    assert torch.equal(after[0], want[0]) and torch.equal(after[1], want[1])
    assert not torch.equal(after[0], before[0])


@pytest.mark.gpu
@torch.no_grad()
def test_switch_and_cap_fall_back_to_the_vm_kernels():
    from tensoir_amd import ops, relight
    _, m = _model((64, 64, 64), seed=7)
    gen = torch.Generator().manual_seed(2)
    P = 5_000
    pts = (torch.rand(P, 3, generator=gen) * 2 - 1).mul(1.1).cuda()
    dirs = torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1).cuda()
    z = relight._z_table(96, 0.05, 1.5, "cuda")
    vm = ops.march_secondary(m.packed_field(), pts, dirs, z, P, None, None, None, m.march_t_stop, False, 0, True, 0)
    st = m.dense_sigma_state()
    assert st["on"] and st["why"] is None and abs(st["mb"] - 4 * 65 * 64 * 64 / 2 ** 20) < 1e-9
    on = relight.compute_transmittance(m, pts, dirs, nSample=96, vis_near=0.05, vis_far=1.5)
    for kw, why in ((dict(dense_sigma=0), "switched off"), (dict(max_mb=0), "above the size cap")):
        with _switch(**kw):
            st = m.dense_sigma_state()
            assert not st["on"] and st["why"] == why, st
            assert m.packed_field_dense() is m.packed_field()
            off = relight.compute_transmittance(m, pts, dirs, nSample=96, vis_near=0.05, vis_far=1.5)
            assert torch.equal(off[0], vm[0]) and torch.equal(off[1], vm[1])          # the VM kernels, bit for bit
    assert m.dense_sigma_state()["on"]                     # the switches are read per call: back on
    again = relight.compute_transmittance(m, pts, dirs, nSample=96, vis_near=0.05, vis_far=1.5)
    assert torch.equal(again[0], on[0]) and torch.equal(again[1], on[1])
    # a zeroed volume member (what a C client that zeroes the struct passes) is the VM route as well
    g = type(m.packed_field()).from_buffer_copy(m.packed_field_dense())
    g.dense_sigma, g.dense_pitch = None, 0
    z_ = ops.march_secondary(g, pts, dirs, z, P, None, None, None, m.march_t_stop, False, 0, True, 0)
    assert torch.equal(z_[0], vm[0]) and torch.equal(z_[1], vm[1])


def test_environment_switches_reach_ops_tune():
    """TENSOIR_DENSE_SIGMA / TENSOIR_DENSE_SIGMA_MAX_MB are read once at import, like the other launch options."""
    code = "from tensoir_amd import ops; print(ops.TUNE['dense_sigma'], ops.TUNE['dense_sigma_max_mb'])"
    for env, want in (({}, "1 1024"), ({"TENSOIR_DENSE_SIGMA": "0"}, "0 1024"), ({"TENSOIR_DENSE_SIGMA_MAX_MB": "64"}, "1 64")):
        e = {k: v for k, v in os.environ.items() if not k.startswith("TENSOIR_DENSE_SIGMA")}
        e.update(env)
        out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, env=e).decode().split("\n")
        assert want in [ln.strip() for ln in out], (env, out)


def test_dense_entry_points_validate_on_the_host():
    """No volume -> UNSUPPORTED before any device work; a pitch without the spare element is an argument error."""
    import ctypes as C
    from tensoir_amd import _lib
    L = _lib.lib()
    keep = torch.zeros(64, dtype=torch.float32)
    ptr = keep.data_ptr()
    f = _lib.TirField()
    f.grid[:] = (8, 8, 8)
    f.n_dcomp, f.n_acomp, f.app_dim, f.n_lights = 16, 48, 27, 1
    for i in range(3):
        f.dplane[i] = f.dline[i] = ptr
    assert L.tir_dense_sigma_fwd(C.byref(f), ptr, ptr, None, 10, None) == -1002
    assert L.tir_dense_sigma_build(C.byref(f), ptr, 8, None) == -1001
    assert L.tir_dense_sigma_build(C.byref(f), None, 9, None) == -1001
    f.grid[:] = (8, 5000, 5000)                              # grid y * grid z beyond the 24-bit multiplier
    assert L.tir_dense_sigma_build(C.byref(f), ptr, 9, None) == -1002
