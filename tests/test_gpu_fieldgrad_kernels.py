"""The field-gradient scatter and optimiser kernels on their own, through the ops wrappers, against the torch restatement
(tests/fieldgrad_reference.py) in float64: tir_vm_app_bwd (k_app_dy + k_vm_app_bwd: four widths, the radiance / intrinsic / both
kernels, the staged and the global line arm, staged and global light rows, idx_map, the persistent loops), tir_density_grad_bwd
(four widths, relu and softplus, the x > 20 shortcut, the normal's clamp arm, LDS lines and global atomics, its loop) and
tir_adam_step (float4 and scalar arm, tails, chunk lookup, several launches, empty tensors).

Comparison rule (shade_reference.distance / bound, as in tests/test_gpu_shade_kernels.py): per compared tensor and case, the device's
distance from the float64 restatement -- max abs difference over the float64 result's maximum -- is at most ten times the float32
restatement's own distance on the same fixture, and no less than ten half-ulps of 1.  Where the float64 result is identically zero
the device must be exactly zero.  Nothing is excluded: tests/test_fieldgrad_cpu.py asserts the margins that keep every discrete
decision the same in float32 and float64 on every fixture used here.  Every test prints `device d (bound b)`.

The gradients go through float atomics: a repeat need not have the same bits.  Instead a second call on the same, un-zeroed buffers
must give twice the reference under the rule (the kernels add), and every texel and line row that is no tap of a sample stays
exactly 0.  y_rad / y_int are overwritten and deterministic: a repeat has the same bits.

The basis gradient is compared twice: g^T y formed in float64 on the host from the device's y, under the rule; and through
ops.gemm_tn_small / ops.gemm_tn as tensoir_amd.training composes them.  Those products run on split-bf16 operands (x = hi + lo,
three products): hi keeps 8 significant bits, lo the next 8, so the dropped lo * lo product and the two residuals of lo are each
at most 2^-18 |a| |b| per product -- the composition is held to the rule's bound plus 3 * 2^-18 * max(|g|^T |y|) / max |g^T y|.

Measured on an MI355X: see DESIGN 2, "The field-gradient kernels on their own"."""
import gc

import pytest
import torch

from tests import fieldgrad_reference as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SPLIT_BF16 = 3 * 2.0 ** -18


def dev(t):
    return None if t is None else t.contiguous().cuda()


def check(label, got, f32, f64, extra=0.0):
    got = torch.as_tensor(got).detach().cpu()
    assert got.shape == f64.shape, (label, got.shape, f64.shape)
    assert torch.isfinite(got).all(), label
    if not bool((torch.as_tensor(f64) != 0).any()):
        print(f"\n[fieldgrad {label}] device exactly zero (float64 is)")
        assert bool((got == 0).all()), (label, "float64 is identically zero")
        return
    d, b = R.distance(got, f64), R.bound(f32, f64) + extra
    print(f"\n[fieldgrad {label}] device {d:.2e} (bound {b:.2e})")
    assert d <= b, (label, d, b)


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)


class World:
    """One model per scene of fieldgrad_reference.SCENES, built on first use."""

    def __init__(self):
        import tensoir_amd
        from tensoir_amd import _lib
        assert torch.cuda.is_available() and _lib.lib().tir_device_check() == 0
        self.tensoir_amd, self.models = tensoir_amd, {}

    def model(self, name):
        if name not in self.models:
            s = R.scene(name)
            m = self.tensoir_amd.model_from_checkpoint(s.ck, "cuda", envmap_h=R.CS.ENVMAP_HW[0], envmap_w=R.CS.ENVMAP_HW[1])
            assert float(m.density_shift) == float(s.sc.density_shift) and m.light_num == s.n_lights
            self.models[name] = m
        return self.models[name]


@pytest.fixture(scope="module")
def world():
    """The models of this file; on the way out their memory goes back to the driver, so that the caching allocator of the test
    session holds no blocks of this file's sizes (tests further on count what the allocator hands out)."""
    w = World()
    yield w
    w.models.clear()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def device_in_order():
    """Wait for the device after every test, so that an error belongs to the test that caused it; after a device error no
    further test of the session is started."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further GPU test is started: {e}", returncode=3)


def param_grads(bufs, short, names):
    """The gradient buffers in the parameters' [1, C, H, W] layout, on the host."""
    from tensoir_amd import training
    out = {}
    for nm in names:
        base, i = nm.split(".")
        out[nm] = training._to_param_layout(bufs[f"{short[base]}{i}"]).detach().cpu().clone()
    return out


def untouched_are_zero(label, grads, prefix, grid, xyz):
    """Every texel and line row that is no tap of a sample is exactly 0."""
    planes, lines = R.touched(grid, xyz)
    for i in range(3):
        p, l = grads[f"{prefix}_plane.{i}"], grads[f"{prefix}_line.{i}"]
        assert p.shape[2:] == planes[i].shape and l.shape[2] == lines[i].shape[0], (label, i)
        assert bool((p[0][:, ~planes[i]] == 0).all()), (label, "plane", i)
        assert bool((l[0, :, :, 0][:, ~lines[i]] == 0).all()), (label, "line", i)


# ---- 1. the appearance scatter -------------------------------------------------------------------------------------------------------
def app_scatter(world, case):
    from tensoir_amd import ops, training
    fx = R.app_case(*case)
    s = fx.scene
    label = f"app {ident(case)}"
    line_lds, lds_light, blocks, chunks, passes = R.app_bwd_launch(s.grid, s.n_acomp, s.n_lights, fx.n)
    label += f" {'lds' if line_lds else 'global'}-line {'lds' if lds_light else 'global'}-light chunks {chunks}"
    m = world.model(s.name)
    f = m.packed_field()
    assert f.n_acomp == s.n_acomp and f.n_lights == s.n_lights and list(f.grid) == s.grid
    light_mean = m._field_cache["lm"].detach().cpu()
    assert R.distance(light_mean, s.sc.light_line.double().mean(0)) <= 2.0 ** -22
    r64, r32 = R.app_reference(fx, F64, light_mean), R.app_reference(fx, F32, light_mean)
    bufs = training._grad_buffers(m, f)
    xyz, li, imap, g_rad, g_int = dev(fx.xyz), dev(fx.light_idx), dev(fx.idx_map), dev(fx.g_rad), dev(fx.g_int)

    def launch():
        return ops.vm_app_bwd(f, bufs["desc"], xyz, li if g_rad is not None else None, imap, g_rad, g_int)

    def collect():
        g = param_grads(bufs, {"app_plane": "ap", "app_line": "al"}, R.APP_LEAVES[:6])
        g["light_line"], g["light_mean"] = bufs["ll"].detach().cpu().clone(), bufs["lm"].detach().cpu().clone()
        return g
    y_rad, y_int = launch()
    once = collect()
    ys = {}
    for name, y, y32, y64 in (("y_rad", y_rad, r32.y_rad, r64.y_rad), ("y_int", y_int, r32.y_int, r64.y_int)):
        assert (y is None) == (y64 is None), (label, name)
        if y is None:
            continue
        ys[name] = y.cpu()
        check(f"{label} {name}", ys[name], y32, y64)
        zero_row = (y64 == 0).all(1)
        assert bool((ys[name][zero_row] == 0).all()), (label, name, "a sample beyond every tap has an all-zero row")
    for k in R.APP_LEAVES:
        check(f"{label} {k}", once[k], r32.grads[k], r64.grads[k])
    untouched_are_zero(label, once, "app", s.grid, fx.xyz)
    check(f"{label} basis (host float64 product of the device's y)", R.basis_gradient(fx, ys.get("y_rad"), ys.get("y_int")), r32.basis, r64.basis)
    if fx.stride == 32:                                       # the feature stride of the training step: its own composition
        nb = 3 * s.n_acomp
        assert ops.MLP_IMPL == "bf16x3"
        pairs = [(g, y) for g, y in ((g_rad, y_rad), (g_int, y_int)) if g is not None]
        d_basis = torch.zeros(R.APP_DIM, nb, device="cuda")
        if nb <= 160:
            ops.gemm_tn_small(pairs, R.APP_DIM, nb, d_basis)
        else:
            for ga, ya in pairs:
                ops.gemm_tn(ga, R.APP_DIM, ya, nb, d_basis)
        mass = torch.zeros(R.APP_DIM, nb, dtype=F64)
        for g, y in ((fx.g_rad, r64.y_rad), (fx.g_int, r64.y_int)):
            if g is not None:
                mass += g[:, :R.APP_DIM].double().abs().T @ y.abs()
        check(f"{label} basis ({'gemm_tn_small' if nb <= 160 else 'gemm_tn'})", d_basis, r32.basis, r64.basis,
              extra=SPLIT_BF16 * float(mass.max()) / float(r64.basis.abs().max()))
    # a second call on the same buffers: y has the same bits, the gradients are added to
    y_rad2, y_int2 = launch()
    twice = collect()
    for name, y in (("y_rad", y_rad2), ("y_int", y_int2)):
        assert y is None or torch.equal(y.cpu(), ys[name]), (label, name, "a repeat changes y")
    for k in R.APP_LEAVES:
        check(f"{label} {k} twice", twice[k], 2 * r32.grads[k], 2 * r64.grads[k])
    untouched_are_zero(label, twice, "app", s.grid, fx.xyz)


@pytest.mark.parametrize("case", R.APP_CASES, ids=ident)
def test_app_scatter(world, case):
    """tir_vm_app_bwd per case of fieldgrad_reference.APP_CASES: y_rad / y_int, the six plane and line gradients, light_line and
    light_mean each alone, the basis gradient twice; NaN in the cotangent rows' padding reaches nothing; with radiance only the
    gradient of light_mean is exactly 0, with intrinsic only that of light_line."""
    app_scatter(world, case)


def test_app_scatter_persistent_loops(world):
    """The thin 48-component field at the first point count at which a wave takes a second chunk (256-block cap, more than 80 KB of
    LDS) and k_app_dy a second pass (768-block cap)."""
    fx = R.app_case(*R.LARGE_APP)
    s = fx.scene
    assert R.app_bwd_launch(s.grid, s.n_acomp, s.n_lights, fx.n)[2:] == (256, 2, 2)
    app_scatter(world, R.LARGE_APP)


# ---- 2. the derived-normal backward --------------------------------------------------------------------------------------------------
def normal_backward(world, case):
    from tensoir_amd import ops, training
    fx = R.normal_case(*case)
    s = fx.scene
    lds_lines, blocks, loops = R.density_grad_launch(s.grid, s.n_dcomp, fx.n)
    label = f"normal {ident(case)} {'lds' if lds_lines else 'global'}-lines loops {loops}"
    m = world.model(s.name)
    f = m.packed_field()
    assert f.n_dcomp == s.n_dcomp and f.act == (1 if s.name.startswith("relu") else 0) and list(f.grid) == s.grid
    r64, r32 = R.normal_reference(fx, F64), R.normal_reference(fx, F32)
    bufs = training._grad_buffers(m, f)
    xyz, g_normal = dev(fx.xyz), dev(fx.g_normal)
    for times in (1, 2):
        ops.density_grad_bwd(f, bufs["desc"], xyz, g_normal)
        got = param_grads(bufs, {"density_plane": "dp", "density_line": "dl"}, R.NORMAL_LEAVES)
        for k in R.NORMAL_LEAVES:
            check(f"{label} {k}" + (" twice" if times == 2 else ""), got[k], times * r32[k], times * r64[k])
        untouched_are_zero(label, got, "density", s.grid, fx.xyz)
    for nm in ("ap0", "al1", "ll", "lm"):
        assert bool((bufs[nm] == 0).all()), (label, nm, "the appearance gradients are not this kernel's")


@pytest.mark.parametrize("case", R.NORMAL_CASES, ids=ident)
def test_density_normal_backward(world, case):
    """tir_density_grad_bwd per case of fieldgrad_reference.NORMAL_CASES: the six density gradients, per width, activation and arm,
    the clamp-arm scene included."""
    normal_backward(world, case)


def test_density_normal_backward_loop(world):
    """The first point count at which the 1024 blocks of k_density_grad_bwd walk a second stretch of lane groups."""
    fx = R.normal_case(*R.LARGE_NORMAL)
    assert R.density_grad_launch(fx.scene.grid, fx.scene.n_dcomp, fx.n)[1:] == (R.DENSITY_GRAD_CAP, 2)
    normal_backward(world, R.LARGE_NORMAL)


# ---- 3. Adam ---------------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def adam_entries(fx, roles):
    P, G, Mo, V = roles
    cut = lambda r, t: r[fx.offsets[t]:fx.offsets[t] + fx.counts[t]]
    return [(cut(P, t), cut(G, t), cut(Mo, t), cut(V, t), fx.lr[t], fx.bc1[t], fx.bc2[t]) for t in range(len(fx.counts))]


@pytest.mark.parametrize("name", list(R.ADAM_LISTS))
def test_adam_step(name):
    """tir_adam_step over a list of fieldgrad_reference.ADAM_LISTS in one call: p, m and v per tensor under the rule; every guard
    float between the tensors and every byte of g as before; the same list as one call per tensor gives the same bits (the update is
    elementwise, without atomics)."""
    from tensoir_amd import ops
    fx = R.adam_case(name)
    roles = [dev(r) for r in (fx.p, fx.g, fx.m, fx.v)]
    for r in roles:
        assert r.data_ptr() % 16 == 0
        for c, o in zip(fx.counts, fx.offsets):
            assert (r.data_ptr() + 4 * o) % 16 == (0 if fx.aligned else 4)
    ops.adam_step(adam_entries(fx, roles), R.BETAS[0], R.BETAS[1], R.EPS)
    torch.cuda.synchronize()
    ref64, ref32 = R.adam_reference(fx, F64), R.adam_reference(fx, F32)
    used = torch.zeros(fx.total, dtype=torch.bool)
    got = [r.cpu() for r in roles]
    for t, (c, o) in enumerate(zip(fx.counts, fx.offsets)):
        used[o:o + c] = True
        if c == 0:
            continue
        for what, i, role in (("p", 0, 0), ("m", 1, 2), ("v", 2, 3)):
            check(f"adam {name} tensor {t} ({c} elements, step {fx.step[t]}) {what}", got[role][o:o + c], ref32[t][i], ref64[t][i])
        assert float(got[0][o]) == float(fx.p[o]), (name, t, "g = m = v = 0 moves p")
    assert torch.equal(bits(got[1]), bits(fx.g)), (name, "g was written")
    for what, role, before in (("p", got[0], fx.p), ("m", got[2], fx.m), ("v", got[3], fx.v)):
        assert torch.equal(bits(role)[~used], bits(before)[~used]), (name, what, "a guard float was written")
    # one call per tensor
    single = [dev(r) for r in (fx.p, fx.g, fx.m, fx.v)]
    for e in adam_entries(fx, single):
        ops.adam_step([e], R.BETAS[0], R.BETAS[1], R.EPS)
    torch.cuda.synchronize()
    for what, a, b in zip("pgmv", roles, single):
        assert torch.equal(bits(a), bits(b)), (name, what, "one call per tensor gives other bits")
