"""The march and compositing kernels on their own, through the ops wrappers, against the torch restatement (tests/march_reference.py)
in float64: tir_march_primary_fwd / _train_fwd / _fused_fwd, tir_exclusive_scan[_capped], tir_compact_primary,
tir_composite_primary[_fused], tir_composite_primary_bwd, tir_march_primary_bwd (its LDS-lines arm, its global-atomic arm, its
persistent loop), tir_march_secondary_fwd / _ids_fwd (the plain kernel, the LDS kernel with 512 and with 1024 threads).

Comparison rule (shade_reference.distance / bound, as in tests/test_gpu_shade_kernels.py): per output tensor and case, the device's
distance from the float64 restatement -- max abs difference over the float64 result's maximum -- is at most ten times the float32
restatement's own distance on the same fixture, and no less than ten half-ulps of 1.  Map rows and their cotangents are compared
per column group.  Where the float64 result is identically zero the device must be exactly zero.  Integer outputs (record counts,
rec_ray, rec_k) and the records' normalised positions are exact.  Nothing is excluded: tests/test_march_cpu.py asserts the margins
that keep every discrete decision the same in float32 and float64 on every fixture used here.  Every test prints
`device d (bound b)`.

Measured on an MI355X: see DESIGN 2, "The march and compositing kernels on their own"."""
import pytest
import torch

from tests import march_reference as M
from tests.pointwise_ref import DENSITY, check_params, scene64, zero_grads

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def dev(t):
    return None if t is None else t.contiguous().cuda()


def check(label, got, f32, f64):
    got = torch.as_tensor(got).detach().cpu()
    assert torch.isfinite(got).all(), label
    if not bool((torch.as_tensor(f64) != 0).any()):
        print(f"\n[march {label}] device exactly zero (float64 is)")
        assert bool((got == 0).all()), (label, "float64 is identically zero")
        return
    d, b = M.distance(got, f64), M.bound(f32, f64)
    print(f"\n[march {label}] device {d:.2e} (bound {b:.2e})")
    assert d <= b, (label, d, b)


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)


class World:
    """One model per scene of march_reference.SCENES, built on first use."""

    def __init__(self):
        import tensoir_amd
        from tensoir_amd import _lib
        assert torch.cuda.is_available() and _lib.lib().tir_device_check() == 0
        self.tensoir_amd, self.models = tensoir_amd, {}

    def model(self, name):
        if name not in self.models:
            s = M.scene(name)
            m = self.tensoir_amd.model_from_checkpoint(s.ck, "cuda", envmap_h=M.CS.ENVMAP_HW[0], envmap_w=M.CS.ENVMAP_HW[1])
            assert (m.alphaMask is not None) == (s.sc.alpha_volume is not None)
            self.models[name] = m
        return self.models[name]

    def field(self, name):
        return self.model(name).packed_field()


@pytest.fixture(scope="module")
def world():
    return World()


# ---- 1. primary march, forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.PRIMARY_FORWARD, ids=ident)
def test_march_primary_forward(world, case):
    """One wave per ray, four per block: B of 1, 3, 4, 5, 257; 64 samples per chunk: S of 1, 2, 63, 64, 65, 129, 200, without and with
    jitter; every density width and relu; the occupancy mask on and off; t_stop 0, 1e-6, 1e-2.  weight, sigma, acc, depth and t_end
    under the rule, app_count exact, weights after an early stop exactly zero; tir_march_primary_fwd gives the bits of the
    training entry."""
    from tensoir_amd import ops
    name, B, S, _j = case
    fx = M.primary_case(*case)
    f, rays, jit = world.field(name), dev(fx.rays), dev(fx.jitter)
    for t_stop in M.PRIMARY_T_STOPS:
        r64, r32 = M.primary_reference(fx, t_stop, F64), M.primary_reference(fx, t_stop, F32)
        weight, sigma, acc, depth, t_end, cnt = (t.cpu() for t in ops.march_primary_train(f, rays, jit, S, t_stop))
        label = f"primary_fwd {ident(case)} t_stop {t_stop:g}"
        for what, got in (("weight", weight), ("sigma", sigma), ("acc", acc), ("depth", depth), ("t_end", t_end)):
            check(f"{label} {what}", got, getattr(r32, what), getattr(r64, what))
        assert torch.equal(cnt, r64.cnt) and torch.equal(r32.cnt, r64.cnt), label
        assert bool((weight[~r64.live] == 0).all()) and bool((sigma[~r64.live] == 0).all()), label
        assert weight.shape == (B, S)
        plain = [t.cpu() for t in ops.march_primary(f, rays, jit, S, t_stop)]
        for a, b in zip(plain, (weight, acc, depth, t_end, cnt)):
            assert torch.equal(a, b), label
    stopped = ~M.primary_reference(fx, 1e-2, F64).live
    print(f"[march primary_fwd {ident(case)}] samples behind an early stop at 1e-2: {int(stopped.sum())}")
    if S > 128:
        assert bool(stopped.any())


def test_march_primary_fused_equals_plain(world):
    """tir_march_primary_fused_fwd: the march's outputs bit for bit, the view-direction table, the capped scan of its counts (cap
    above, inside and at 0) and the re-armed counter words."""
    from tensoir_amd import ops
    fx = M.primary_case("fine", 257, 65, False)
    f, rays = world.field("fine"), dev(fx.rays)
    w0, acc0, dep0, _t, cnt0 = ops.march_primary(f, rays, None, fx.S, 1e-6)
    total = int(cnt0.sum())
    want = torch.cat([torch.zeros(1, dtype=torch.int64), cnt0.cpu().long().cumsum(0)])
    for cap in (1 << 30, total // 2, 0):
        words = torch.full((8,), 0, dtype=torch.int32, device="cuda")
        words[1:3] = 9
        w, acc, dep, cnt, off, tot, vd = ops.march_primary_fused(f, rays, fx.S, 1e-6, cap, words)
        for a, b in ((w, w0), (acc, acc0), (dep, dep0), (cnt, cnt0), (vd, rays[:, 3:6])):
            assert torch.equal(a, b), cap
        assert torch.equal(off.cpu().long(), want.clamp(max=cap)) and int(tot) == total
        assert words.cpu().tolist() == [0, 0, 0, 0, 0, total, 0, 0]


# ---- 2. the scan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", M.SCAN_SIZES)
def test_exclusive_scan(n):
    """k_exclusive_scan (1024 threads, carry loop): n round the wave, the block and two blocks; counts in [0, 300] with runs of
    zeros; uncapped and capped above the total, at half of it and at 0: exact against cumsum, the total included."""
    from tensoir_amd import ops
    counts = M.scan_counts(n)
    want = torch.cat([torch.zeros(1, dtype=torch.int64), counts.long().cumsum(0)])
    total = int(want[-1])
    assert torch.equal(ops.exclusive_scan(dev(counts)).cpu().long(), want)
    for cap in (total + 5, total // 2, 0):
        off, tot = ops.exclusive_scan_capped(dev(counts), cap)
        assert torch.equal(off.cpu().long(), want.clamp(max=cap)) and int(tot) == total, (n, cap)


# ---- 3. compaction -------------------------------------------------------------------------------------------------------------------
def expected_records(r32):
    ray, k = torch.nonzero(r32.keep, as_tuple=True)
    return ray.int(), k.int(), r32.weight[r32.keep], r32.xyz32[r32.keep]


@pytest.mark.parametrize("case", M.PRIMARY_FORWARD, ids=ident)
def test_compact_primary(world, case):
    """The float32 restatement's weights in, offsets from their counts: records in (ray, sample) order, rec_w the weights' bits,
    rec_k, rec_ray and the normalised positions exact."""
    from tensoir_amd import ops
    fx = M.primary_case(*case)
    r32 = M.primary_reference(fx, 0.0, F32)
    want = expected_records(r32)
    off = torch.cat([torch.zeros(1, dtype=torch.int64), r32.cnt.long().cumsum(0)]).int()
    A = int(off[-1])
    got = ops.compact_primary(world.field(case[0]), dev(fx.rays), dev(fx.jitter), dev(r32.weight), dev(off), A)
    for name, a, b in zip(("rec_ray", "rec_k", "rec_w", "rec_xyz"), got, want):
        assert torch.equal(a.cpu(), b), (name, int((a.cpu() != b).sum()), A)
    print(f"\n[march compact {ident(case)}] {A} records, exact")


def test_compact_primary_capped(world):
    """Capped offsets (tir_exclusive_scan_capped's) that cut a ray's segment in the middle, fall on a segment boundary, and are all
    0: the slots below the cap are right, the sentinel at and past the cap is untouched."""
    from tensoir_amd import ops
    case = ("fine", 40, 129, True)
    fx = M.primary_case(*case)
    r32 = M.primary_reference(fx, 0.0, F32)
    want = expected_records(r32)
    full = torch.cat([torch.zeros(1, dtype=torch.int64), r32.cnt.long().cumsum(0)])
    A = int(full[-1])
    r = int(torch.nonzero(r32.cnt >= 3)[2])                      # a ray with at least three records, not the first such
    caps = {"inside": int(full[r]) + int(r32.cnt[r]) // 2, "boundary": int(full[r]), "zero": 0}
    assert full[r] < caps["inside"] < full[r + 1] and caps["boundary"] > 0
    for what, cap in caps.items():
        out = (torch.full((A + 64,), -7, dtype=torch.int32, device="cuda"), torch.full((A + 64,), -7, dtype=torch.int32, device="cuda"),
               torch.full((A + 64,), -7.0, device="cuda"), torch.full((A + 64, 3), -7.0, device="cuda"))
        got = ops.compact_primary(world.field(case[0]), dev(fx.rays), dev(fx.jitter), dev(r32.weight), dev(full.clamp(max=cap).int()), A, out=out)
        for name, a, b in zip(("rec_ray", "rec_k", "rec_w", "rec_xyz"), got, want):
            a = a.cpu()
            assert torch.equal(a[:cap], b[:cap]), (what, name)
            assert bool((a[cap:] == -7).all()), (what, name, "written at or past the cap")
    print(f"\n[march compact capped] caps {caps} of {A} records")


# ---- 4. compositing, forward ---------------------------------------------------------------------------------------------------------
DROPS = [()] + [(n,) for n in M.RECORD_INPUTS] + [M.RECORD_INPUTS]
COMPOSITE_CASES = [(B, wb, rl) for B in M.COMPOSITE_B for wb in (1, 0) for rl in (1, 0)]


@pytest.mark.parametrize("B,white_bg,is_relight", COMPOSITE_CASES)
def test_composite_primary_forward(B, white_bg, is_relight):
    """One wave per ray, lanes stride over its records: B of 1, 3, 4, 5, 257, rays with 0, 1, 63, 64, 65 and 130 records, all four
    (white_bg, is_relight), every per-record pointer None in turn and all of them None.  The 20 map columns under the rule per
    column group; without relight columns 4-19 are exactly 0 except acc; the fused entry's rows equal the plain entry's."""
    from tensoir_amd import ops
    fx = M.composite_case(B)
    for drop in DROPS:
        args = M.composite_inputs(fx, drop)
        got = ops.composite_primary(*[dev(a) for a in args], white_bg, is_relight, M.FIXED_FRESNEL).cpu()
        with torch.no_grad():
            m64, m32 = M.composite(*args, white_bg, is_relight, F64), M.composite(*args, white_bg, is_relight, F32)
        label = f"composite_fwd B {B} white_bg {white_bg} relight {is_relight} without {'+'.join(drop) or 'nothing'}"
        for group, cols in M.COLUMN_GROUPS.items():
            check(f"{label} {group}", got[:, cols], m32[:, cols], m64[:, cols])
        assert bool((got[:, 19] == 0).all()) and got.shape == (B, M.MAP_STRIDE)
        if not is_relight:
            assert bool((got[:, 4:14] == 0).all()) and bool((got[:, 15:] == 0).all()) and torch.equal(got[:, 14], fx.acc)
        words = torch.zeros(8, dtype=torch.int32, device="cuda")
        fused, _smooth = ops.composite_primary_fused(*[dev(a) for a in args], white_bg, is_relight, M.FIXED_FRESNEL, words)
        assert torch.equal(fused.cpu(), got), label
        if fx.rows and is_relight and not drop:
            e = got[fx.rows["empty"]]
            assert e[4:7].tolist() == ([0.0, 0.0, 1.0] if white_bg else [0.0, 0.0, 0.0]) and e[7:11].tolist() == [float(white_bg)] * 4
            assert e[11] == (1.0 if white_bg else torch.tensor(M.FIXED_FRESNEL)) and e[14] == 0
            assert got[fx.rows["acc_one"], 14] == 1.0
            assert bool((got[fx.rows["clipped"], 0:3] == got[fx.rows["clipped"], 0]).all()) and abs(float(got[fx.rows["clipped"], 0]) - 1) < 1e-6
    cnt = fx.offsets[1:] - fx.offsets[:-1]
    if B == 257:
        assert sorted(set(cnt.tolist())) == sorted(M.RECORD_COUNTS)


# ---- 5. compositing, backward --------------------------------------------------------------------------------------------------------
def poison(*tensors):
    """Fill and free device blocks of the outputs' sizes with NaN, so that an output the kernel leaves unwritten reads as NaN."""
    for t in tensors:
        if t is not None:
            torch.full(t.shape, float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,white_bg,is_relight", COMPOSITE_CASES)
def test_composite_primary_backward(B, white_bg, is_relight):
    """tir_composite_primary_bwd on the forward's cases with random cotangents on all 20 columns: g_rgb, g_brdf, g_brdf_jit, g_pred,
    g_der, g_weight [B, S] at (ray, rec_k), g_acc and g_depth against float64 autograd of the restatement; g_weight is zero off the
    records; an input that is None gets no gradient and leaves the others right; an input the branch does not use (everything but
    rgb without relight, the derived normal without the predicted one) gets a written zero."""
    from tensoir_amd import ops
    fx = M.composite_case(B)
    cot = M.composite_cotangent(B)
    ray, k = fx.rec_ray.long(), fx.rec_k.long()
    for drop in DROPS:
        args = M.composite_inputs(fx, drop)
        on_device = [dev(fx.rays), dev(fx.offsets), dev(fx.rec_k)] + [dev(a) for a in args[2:]]
        g_maps = dev(cot)
        poison(*args[3:8], fx.acc, fx.depth)
        out = ops.composite_primary_bwd(*on_device, fx.S, white_bg, is_relight, M.FIXED_FRESNEL, g_maps)
        got = dict(zip(M.RECORD_INPUTS + ("g_weight", "acc", "depth"), out))
        g64, g32 = (M.composite_gradients(fx, drop, white_bg, is_relight, cot, dt) for dt in (F64, F32))
        label = f"composite_bwd B {B} white_bg {white_bg} relight {is_relight} without {'+'.join(drop) or 'nothing'}"
        for name in M.RECORD_INPUTS:
            if name in drop:
                assert got[name] is None, (label, name)
            else:
                check(f"{label} g_{name}", got[name], g32[name], g64[name])
        check(f"{label} g_acc", got["acc"], g32["acc"], g64["acc"])
        check(f"{label} g_depth", got["depth"], g32["depth"], g64["depth"])
        gw = got["g_weight"].cpu()
        assert gw.shape == (B, fx.S)
        check(f"{label} g_weight", gw[ray, k], g32["rec_w"], g64["rec_w"])
        off_records = torch.ones(B, fx.S, dtype=torch.bool)
        off_records[ray, k] = False
        assert bool((gw[off_records] == 0).all()), label
        if fx.rows and is_relight and not drop:
            a = int(fx.offsets[fx.rows["clipped"]])
            assert bool((got["rgb"].cpu()[a] == 0).all())                      # the clip stops the colour's gradient


# ---- 6. primary march, backward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.PRIMARY_BACKWARD, ids=ident)
def test_march_primary_backward(world, case):
    """tir_march_primary_bwd with random cotangents on weight, acc and depth: d loss / d density feature per sample against float64
    autograd through the restatement, under the rule (S of 1, 63, 64, 65, 129; B of 1, 5, 257; ray 0 crosses the opaque middle of
    the blob on the small grids, where 1 - alpha + 1e-10 is 1e-10 and a suffix sum formed as total - prefix would be noise divided by it); the plane
    and line gradients against autograd into pointwise_ref.scene64's leaves through check_params, its tolerance set by the rule
    (check_params' default of 1e-5 was chosen for per-point gradients; through a whole march the float32 restatement itself is
    up to 1e-5 from float64 on the small scenes and 1e-4 on the long-axis one, whose field changes from texel to texel along x).  Every density width and relu on the
    LDS-lines arm, the long-axis scene on the global-atomic arm, 2053 rays at S = 33 on the persistent blocks' loop.

    The long-axis scene's g_feature is not compared with a march on shortened lines: the length of a line is the grid's size along
    that axis, so a shorter line is another step size, other sample positions and other interpolation cells -- another fixture.
    The feature gradient is formed before the arm-specific scatter and is held to float64 on both arms instead."""
    from tensoir_amd import ops, training
    name, B, S, _j = case
    fx = M.primary_case(*case)
    s = M.scene(name)
    arm = M.primary_bwd_arm(s.grid, s.n_dcomp)
    assert (arm == "global-atomic") == (name == "long_axis") and ((B + 3) // 4 > 512) == (B == 2053)
    m = world.model(name)
    f = m.packed_field()
    bufs = training._grad_buffers(m, f)
    cot = M.march_cotangent(B, S)
    rays, jit = dev(fx.rays), dev(fx.jitter)
    weight, sigma, _acc, _depth, _t, _c = ops.march_primary_train(f, rays, jit, S, 0.0)
    g_feature = ops.march_primary_bwd(f, bufs["desc"], rays, jit, sigma, weight, *[dev(c) for c in cot], want_g_feature=True).cpu()
    label = f"primary_bwd {ident(case)} {arm}"
    g64, g32 = M.march_gradients(fx, cot, F64), M.march_gradients(fx, cot, F32)
    check(f"{label} g_feature", g_feature, g32, g64)
    r64 = M.primary_reference(fx, 0.0, F64)
    assert bool((g_feature[~r64.valid] == 0).all()), label
    if s.grid != M.FINE_GRID:
        assert M.least_pass(s.sc, r64) < 1e-16, "ray 0 no longer crosses an opaque stretch"
    # planes and lines: float64 autograd into the model's own parameters (scene64), the yardstick from float32 leaves
    sc64, params = scene64(m)
    M.march_gradients(fx, cot, F64, field=sc64)
    fld32, params32 = M.density_leaves(s.sc, F32)
    M.march_gradients(fx, cot, F32, field=fld32)
    zero_grads(m)
    named = dict(m.named_parameters())
    short = {"density_plane": "dp", "density_line": "dl"}
    try:
        for nm in DENSITY:
            base, i = nm.split(".")
            assert torch.equal(params32[nm].detach().double(), params[nm].detach()), nm
            named[nm].grad = training._to_param_layout(bufs[f"{short[base]}{i}"]).clone()
            g64 = torch.zeros_like(params[nm]) if params[nm].grad is None else params[nm].grad
            g32 = torch.zeros_like(params32[nm]) if params32[nm].grad is None else params32[nm].grad
            if not bool((g64 != 0).any()):
                assert bool((named[nm].grad == 0).all()), nm
            d, b = M.distance(named[nm].grad, g64), M.bound(g32, g64)
            print(f"[march {label} {nm}] device {d:.2e} (bound {b:.2e})")
            check_params(m, params, [nm], tol=b)
    finally:
        zero_grads(m)


# ---- 7. secondary march --------------------------------------------------------------------------------------------------------------
class Route:
    """The field of a route with the launch option that selects it, restored on exit; asserts the launcher's arithmetic."""

    def __init__(self, world, route, n_sample):
        self.scene_name, self.lds = M.SECONDARY_ROUTES[route]
        s = M.scene(self.scene_name)
        arm = M.secondary_arm(s.grid, s.n_dcomp, n_sample, self.lds)
        assert arm == (route if route.startswith("lds") else "plain"), (route, n_sample, arm)
        self.f = world.field(self.scene_name)

    def __enter__(self):
        self.prev = self.f.tune_lds_lines
        self.f.tune_lds_lines = 1 if self.lds else 2
        return self.f

    def __exit__(self, *exc):
        self.f.tune_lds_lines = self.prev
        return False


FILL = -3.0


def run_secondary(f, fx, n_pairs, t_stop, records, rec_cap=None, pad=64, **addr):
    """One launch with every per-pair output pre-filled with FILL / -3 and sentinel-filled record buffers of rec_cap + pad slots."""
    from tensoir_amd import ops
    vis, oma = torch.full((n_pairs,), FILL, device="cuda"), torch.full((n_pairs,), FILL, device="cuda")
    rec = None
    if records:
        n = rec_cap + pad
        rec = {"counter": torch.zeros(2, dtype=torch.int32, device="cuda"), "ray": torch.full((n,), -7, dtype=torch.int32, device="cuda"),
               "w": torch.full((n,), -7.0, device="cuda"), "xyz": torch.full((n, 3), -7.0, device="cuda"),
               "off": torch.full((n_pairs,), -3, dtype=torch.int32, device="cuda"), "cnt": torch.full((n_pairs,), -3, dtype=torch.int32, device="cuda")}
    origins, dirs = addr.pop("origins"), addr.pop("dirs")
    n_rays = addr.pop("n_rays", n_pairs)
    addr = {k: (dev(v) if torch.is_tensor(v) else v) for k, v in addr.items()}
    ops.march_secondary(f, dev(origins), dev(dirs), dev(fx.z_vals), n_rays, t_stop=t_stop, want_records=records, rec_cap=rec_cap or 0, vis=vis,
                        oma=oma, rec=rec, **addr)
    return vis.cpu(), oma.cpu(), None if rec is None else {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in rec.items()}


def flat_records(r):
    """A reference run's records in ray order: (offset of each ray's first record [n + 1], weights, positions)."""
    return torch.cat([torch.zeros(1, dtype=torch.int64), r.cnt.long().cumsum(0)]), r.weight[r.keep], r.xyz32[r.keep]


def check_secondary(label, fx, t_stop, sel, out, zero=None, rec_cap=None):
    """sel [n_pairs]: the fixture ray each pair is (-1: the pair is not marched).  zero: pairs that are switched off (they read 0
    and have no records); the other pairs with sel < 0 keep what they were pre-filled with.  rec_cap None: every record fits."""
    vis, oma, rec = out
    r64, r32 = M.secondary_reference(fx, t_stop, F64), M.secondary_reference(fx, t_stop, F32)
    on = sel >= 0
    zero = torch.zeros_like(on) if zero is None else zero
    kept = ~on & ~zero
    if bool(on.any()):
        check(f"{label} vis", vis[on], r32.t_end[sel[on]], r64.t_end[sel[on]])
        check(f"{label} one_minus_acc", oma[on], r32.one_minus_acc[sel[on]], r64.one_minus_acc[sel[on]])
    assert bool((vis[zero] == 0).all()) and bool((oma[zero] == 0).all()), label
    assert bool((vis[kept] == FILL).all()) and bool((oma[kept] == FILL).all()), label
    if rec is None:
        return
    assert torch.equal(r32.keep, r64.keep)
    ref_off, ref_w32, ref_xyz = flat_records(r32)
    ref_w64 = r64.weight[r64.keep]
    want_cnt = torch.where(on, r64.cnt[sel.clamp(min=0)], torch.zeros_like(r64.cnt[sel.clamp(min=0)]))
    total = int(want_cnt.sum())
    counter, cnt, off = rec["counter"].tolist(), rec["cnt"], rec["off"]
    assert counter[0] == total, (label, counter, total)
    assert bool((cnt[kept] == -3).all()) and bool((cnt[zero] == 0).all()), label
    live_cnt = cnt[on | zero]
    if rec_cap is None:
        assert torch.equal(cnt[on], want_cnt[on]) and counter[1] == total, label
    else:
        dropped = on & (cnt == 0) & (want_cnt > 0)
        assert bool(((cnt == want_cnt) | dropped)[on].all()), label            # a ray keeps its whole segment or nothing
        assert int(live_cnt.sum()) <= rec_cap and counter[1] <= rec_cap, (label, int(live_cnt.sum()), counter)
        print(f"[march {label}] rec_cap {rec_cap} of {total}: kept {int(live_cnt.sum())} records, dropped {int(dropped.sum())} rays")
    have = on & (cnt > 0)
    pairs = torch.nonzero(have).reshape(-1)
    n = cnt[have].long()
    within = torch.arange(int(n.sum())) - torch.repeat_interleave(n.cumsum(0) - n, n)
    slot = torch.repeat_interleave(off[have].long(), n) + within                 # where the device put each record
    src = torch.repeat_interleave(ref_off[sel[have]], n) + within                # the reference record it must be
    assert slot.numel() == 0 or (int(slot.min()) >= 0 and int(slot.max()) < counter[1]), label
    assert torch.unique(slot).numel() == slot.numel(), (label, "segments overlap")
    assert torch.equal(rec["ray"][slot], torch.repeat_interleave(pairs, n).int()), label
    assert torch.equal(rec["xyz"][slot], ref_xyz[src]), (label, "rec_xyz")
    if slot.numel():
        check(f"{label} rec_w", rec["w"][slot], ref_w32[src], ref_w64[src])
    cap = total if rec_cap is None else rec_cap
    untouched = torch.ones(rec["ray"].numel(), dtype=torch.bool)
    untouched[slot] = False
    assert bool((rec["ray"][cap:] == -7).all()) and bool((rec["w"][cap:] == -7).all()) and bool((rec["xyz"][cap:] == -7).all()), (label, "written at or past rec_cap")
    assert bool((rec["ray"][untouched] == -7).all()) and bool((rec["w"][untouched] == -7).all()), (label, "written outside the kept segments")


def total_records(fx, t_stop, sel):
    r = M.secondary_reference(fx, t_stop, F64)
    return int(r.cnt[sel[sel >= 0]].sum())


@pytest.mark.parametrize("route,n_sample", M.SECONDARY_CASES, ids=ident)
def test_march_secondary_samples(world, route, n_sample):
    """32 samples per step: n_sample of 1, 2, 31, 32, 33, 64, 95, 96 on every route (97 and 256 on the plain kernel), 129 rays
    addressed directly, t_stop 0 and 1e-4, with and without records.  vis and 1 - acc under the rule; every ray's record segment
    through ray_rec_off / ray_rec_cnt: count, rec_ray and positions exact, weights under the rule; rec_counter = the total."""
    fx = M.secondary_case(M.SECONDARY_ROUTES[route][0], n_sample)
    n = 129
    sel = torch.arange(n)
    with Route(world, route, n_sample) as f:
        for t_stop in M.SECONDARY_T_STOPS:
            for records in (False, True):
                out = run_secondary(f, fx, n, t_stop, records, rec_cap=total_records(fx, t_stop, sel), origins=fx.origins[:n], dirs=fx.dirs[:n])
                check_secondary(f"secondary {route} n_sample {n_sample} t_stop {t_stop:g} records {int(records)}", fx, t_stop, sel, out)
    stopped = ~M.secondary_reference(fx, 1e-4, F64).live[:n]
    print(f"[march secondary {route} n_sample {n_sample}] rays stopped early at 1e-4: {int(stopped.any(1).sum())} of {n}")


KERNEL_ROUTES = ("plain-16", "lds-512", "lds-1024")


@pytest.mark.parametrize("route", KERNEL_ROUTES)
def test_march_secondary_ray_counts(world, route):
    """32 rays per block (plain) or 64 / 128 per batch (LDS), half a wave per ray: n_rays of 1, 31, 32, 33, 63, 64, 65, 129 at 33
    samples with records and t_stop 1e-4."""
    fx = M.secondary_case(M.SECONDARY_ROUTES[route][0], 33)
    with Route(world, route, 33) as f:
        for n in M.SECONDARY_RAYS:
            sel = torch.arange(n)
            out = run_secondary(f, fx, n, 1e-4, True, rec_cap=total_records(fx, 1e-4, sel), origins=fx.origins[:n], dirs=fx.dirs[:n])
            check_secondary(f"secondary {route} n_rays {n}", fx, 1e-4, sel, out)


@pytest.mark.parametrize("route", KERNEL_ROUTES)
def test_march_secondary_addressing(world, route):
    """org_map + dir_map into permuted tables with repeated rays; `active` with some, all and no rays switched off (they read
    exactly 0 and own no records); the n_dirs pair grid with n_dirs of 1, 3 and 24."""
    name = M.SECONDARY_ROUTES[route][0]
    fx = M.secondary_case(name, 33)
    gen = torch.Generator().manual_seed(9)
    N = fx.origins.shape[0]
    n = 203
    sel = torch.randint(0, N, (n,), generator=gen)
    sel[:7] = 5                                                                   # one ray seven times
    po, pd = torch.randperm(N, generator=gen), torch.randperm(N, generator=gen)
    inv_o, inv_d = torch.argsort(po), torch.argsort(pd)
    maps = dict(origins=fx.origins[po], dirs=fx.dirs[pd], org_map=inv_o[sel].int(), dir_map=inv_d[sel].int())
    with Route(world, route, 33) as f:
        for what, off in (("none off", torch.zeros(n, dtype=torch.bool)), ("some off", torch.rand(n, generator=gen) < 0.4),
                          ("all off", torch.ones(n, dtype=torch.bool))):
            s = torch.where(off, torch.full_like(sel, -1), sel)
            out = run_secondary(f, fx, n, 1e-4, True, rec_cap=max(total_records(fx, 1e-4, s), 1), active=(~off).to(torch.uint8), **maps)
            check_secondary(f"secondary {route} maps, {what}", fx, 1e-4, s, out, zero=off)
        grid = M.secondary_grid_case(name, 33)
        for n_dirs in (1, 3, 24):
            view = M.grid_subset(grid, n_dirs)
            n_pairs = view.origins.shape[0]
            sel_g = torch.arange(n_pairs)
            out = run_secondary(f, view, n_pairs, 0.0, True, rec_cap=max(total_records(view, 0.0, sel_g), 1), origins=grid.points,
                                dirs=grid.table[:n_dirs], n_dirs=n_dirs)
            check_secondary(f"secondary {route} pair grid n_dirs {n_dirs}", view, 0.0, sel_g, out)


@pytest.mark.parametrize("route", KERNEL_ROUTES)
def test_march_secondary_id_lists(world, route):
    """tir_march_secondary_ids_fwd: a list of pair ids in a shuffled order with *n_ids_dev equal to, below and above n_rays, and 0:
    the listed pairs are marched (outputs addressed by the pair id), the others keep what they were pre-filled with."""
    fx = M.secondary_case(M.SECONDARY_ROUTES[route][0], 33)
    gen = torch.Generator().manual_seed(19)
    n_pairs, n_list = 150, 97
    ids = torch.randperm(n_pairs, generator=gen)[:n_list].int()
    with Route(world, route, 33) as f:
        for what, n_dev, n_rays in (("equal", n_list, n_list), ("below", 41, n_list), ("above", n_list + 30, n_list), ("zero", 0, n_list)):
            listed = ids[:min(n_dev, n_rays)].long()
            sel = torch.full((n_pairs,), -1, dtype=torch.int64)
            sel[listed] = listed
            out = run_secondary(f, fx, n_pairs, 1e-4, True, rec_cap=max(total_records(fx, 1e-4, sel), 1), origins=fx.origins[:n_pairs],
                                dirs=fx.dirs[:n_pairs], n_rays=n_rays, ray_ids=ids, n_ids_dev=torch.tensor([n_dev], dtype=torch.int32))
            check_secondary(f"secondary {route} id list, n_ids_dev {what}", fx, 1e-4, sel, out)


@pytest.mark.parametrize("route", ("lds-512", "lds-1024"))
def test_march_secondary_persistent_loop(world, route):
    """More rays than the persistent grid takes in one round (512 blocks x 64 rays, 256 x 128): 32768 + 69 rays at 33 samples,
    the fixture's rays over and over through the maps."""
    fx = M.secondary_case(M.SECONDARY_ROUTES[route][0], 33)
    N = fx.origins.shape[0]
    n = 32768 + 69
    sel = (torch.arange(n) * 7) % N
    with Route(world, route, 33) as f:
        out = run_secondary(f, fx, n, 1e-4, True, rec_cap=total_records(fx, 1e-4, sel), origins=fx.origins, dirs=fx.dirs, org_map=sel.int(),
                            dir_map=sel.int())
        check_secondary(f"secondary {route} persistent loop", fx, 1e-4, sel, out)


@pytest.mark.parametrize("route", KERNEL_ROUTES)
def test_march_secondary_overflow(world, route):
    """rec_cap at 0, at half the total and one below it.  Whichever blocks fit: every ray has its whole reference segment inside
    [0, rec_counter[1]) or ray_rec_cnt = 0, the kept counts sum to at most rec_cap, rec_counter[0] is still the reference total, and
    nothing is written at or past rec_cap."""
    fx = M.secondary_case(M.SECONDARY_ROUTES[route][0], 33)
    n = 129
    sel = torch.arange(n)
    total = total_records(fx, 0.0, sel)
    with Route(world, route, 33) as f:
        for cap in (0, total // 2, total - 1):
            out = run_secondary(f, fx, n, 0.0, True, rec_cap=cap, pad=total + 64, origins=fx.origins[:n], dirs=fx.dirs[:n])
            check_secondary(f"secondary {route} rec_cap {cap}", fx, 0.0, sel, out, rec_cap=cap)
