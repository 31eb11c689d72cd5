"""CPU leg of the field-gradient suite (tests/test_gpu_fieldgrad_kernels.py): the fixtures' margins and redraw caps, the arm each
fixture reaches (from the launchers' own arithmetic), and the tie of the restatement (tests/fieldgrad_reference.py) to the pinned
oracle and to torch.optim.Adam.  Prints the float32 restatement's own distance from float64 per fixture -- a tenth of what the GPU
tests allow.

The ties use the suite's rule with the pinned code in the device's place: the oracle's float32 gradients (torch.optim.Adam's
float32 step) must come within ten times the float32 restatement's own distance from the float64 restatement -- a tolerance taken
from the float32 runs' distance to float64, not from each other."""
import pytest
import torch

from oracle import tensoir_oracle as O
from tests import fieldgrad_reference as R
from tests import march_reference as M

F32, F64 = torch.float32, torch.float64
APP_CASES = R.APP_CASES + [R.LARGE_APP]
NORMAL_CASES = R.NORMAL_CASES + [R.LARGE_NORMAL]


def ident(v):
    return "-".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)


def within_rule(label, got, f32, f64):
    if not bool((f64 != 0).any()):
        assert bool((got == 0).all()), label
        return
    d, b = R.distance(got, f64), R.bound(f32, f64)
    print(f"\n[fieldgrad cpu {label}] pinned float32 {d:.2e} (bound {b:.2e}; float32 restatement {R.distance(f32, f64):.2e})")
    assert d <= b, (label, d, b)


def leaf_scene(sc, names):
    """The float32 scene with leaf copies of the named parameter lists / tensors."""
    work = O.Scene(**sc.__dict__)
    for nm in names:
        v = getattr(sc, nm)
        setattr(work, nm, [t.detach().clone().requires_grad_(True) for t in v] if isinstance(v, list) else v.detach().clone().requires_grad_(True))
    return work


# ---- the appearance scatter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", APP_CASES, ids=ident)
def test_app_fixture(case):
    """What each fixture is for, and the tie: the float32 gradients of autograd through O.both_feature on the same leaves (the
    clamped, mapped light index handed in; light_line's gradient composed as ll + lm / n_lights) against the restatement."""
    fx = R.app_case(*case)
    s, n = fx.scene, fx.n
    name, kind, _n, mode, stride, map_kind = case
    assert fx.xyz.shape == (n, 3) and fx.xyz.dtype == F32 and fx.light_idx.dtype == torch.int32
    for g in (fx.g_rad, fx.g_int):
        assert g is None or (g.shape == (n, stride) and bool(torch.isfinite(g[:, :R.APP_DIM]).all()) and bool(torch.isnan(g[:, R.APP_DIM:]).all()))
    assert (fx.g_rad is None) == (mode == "int") and (fx.g_int is None) == (mode == "rad")
    li = effective_light(fx)
    raw = fx.light_idx.long()
    if n >= 4 * R.WAVE_CHUNK:
        assert int(raw.min()) == -1 and int(raw.max()) == s.n_lights and {0, s.n_lights - 1} <= set(li.tolist())
        chunks = li[:n // R.WAVE_CHUNK * R.WAVE_CHUNK].view(-1, R.WAVE_CHUNK)
        if map_kind != "perm":
            assert bool((chunks == chunks[:, :1]).all(1).any()), "no chunk with one light"
        assert bool((chunks.view(-1, R.RUN)[:, 1:] != chunks.view(-1, R.RUN)[:, :-1]).any(1).any()), "no run in which the light changes"
    if map_kind == "monotone":
        assert bool((fx.idx_map[1:] >= fx.idx_map[:-1]).all()) and fx.light_idx.numel() == int(fx.idx_map[-1]) + 1
    if map_kind == "perm":
        assert sorted(fx.idx_map.tolist()) == list(range(n)) and n > 1 and not bool((fx.idx_map[1:] >= fx.idx_map[:-1]).all())
    r64, r32 = R.app_reference(fx, F64), R.app_reference(fx, F32)
    if kind == "generic" and n >= 64:
        lo_face, inside = (fx.xyz.abs() == 1).any(1), (fx.xyz.abs() <= 1).all(1)
        y = r64.y_rad if r64.y_rad is not None else r64.y_int
        zero_row = (y == 0).all(1)
        assert bool(lo_face.any()) and bool((~inside).any()) and float(fx.xyz.abs().max()) <= 1 + R.OUTSIDE
        assert bool(zero_row.any()) and bool((~inside & ~zero_row).any()), "points outside the box: some beyond every tap, some within a texel"
        assert not bool(zero_row[inside].any())
        for a in range(3):                                   # points on grid lines of every axis: an exact node in float32
            ix = ((fx.xyz[:, a] + 1.0) * 0.5) * float(s.grid[a] - 1)
            assert int(((ix == torch.floor(ix)) & (fx.xyz[:, a].abs() < 1)).sum()) >= 3, a
    if kind == "rays" and n >= 64:
        cell = torch.stack(R.tap_cells(fx.xyz[:, 0], s.grid[0]) + R.tap_cells(fx.xyz[:, 1], s.grid[1]), 1)
        same = (cell[1:] == cell[:-1]).all(1)
        assert 0.3 < float(same.float().mean()) < 0.9, "consecutive samples neither stay in a cell nor leave it"
    if kind == "dups":
        assert bool((fx.xyz == fx.xyz[0]).all()) and n == 4096
    if kind == "alternate":
        for a in range(3):
            c = R.tap_cells(fx.xyz[:, a], s.grid[a])[0]
            assert bool((c[1:] != c[:-1]).all()), a
    # the tie to the oracle
    work = leaf_scene(s.sc, ("app_plane", "app_line", "light_line"))
    rad, intr = O.both_feature(work, fx.xyz, li, "explicit")
    loss = 0.0
    if fx.g_rad is not None:
        loss = loss + (rad * fx.g_rad[:, :R.APP_DIM]).sum()
    if fx.g_int is not None:
        loss = loss + (intr * fx.g_int[:, :R.APP_DIM]).sum()
    loss.backward()
    label = f"app {ident(case)}"
    for kind_, ts in (("plane", work.app_plane), ("line", work.app_line)):
        for i, t in enumerate(ts):
            within_rule(f"{label} app_{kind_}.{i}", t.grad, r32.grads[f"app_{kind_}.{i}"], r64.grads[f"app_{kind_}.{i}"])
    compose = lambda r: r.grads["light_line"] + r.grads["light_mean"][None] / s.n_lights
    within_rule(f"{label} light_line composed", work.light_line.grad, compose(r32), compose(r64))
    if mode == "rad":
        assert not bool((r64.grads["light_mean"] != 0).any())
    if mode == "int":
        assert not bool((r64.grads["light_line"] != 0).any())
    print(f"[fieldgrad cpu {label}] float32 restatement: y_rad {0 if r64.y_rad is None else R.distance(r32.y_rad, r64.y_rad):.1e} "
          f"y_int {0 if r64.y_int is None else R.distance(r32.y_int, r64.y_int):.1e} basis {R.distance(r32.basis, r64.basis):.1e} " +
          " ".join(f"{k} {R.distance(r32.grads[k], r64.grads[k]):.1e}" for k in R.APP_LEAVES))


def effective_light(fx):
    li = R.effective_light(fx)
    assert int(li.min()) >= 0 and int(li.max()) <= fx.scene.n_lights - 1
    return li


def test_app_cases_reach_their_arms():
    """Through launch_app_bwd's arithmetic: every width, the three kernels, the staged and the global line arm, the staged and the
    global light rows, every point count's unit, and the large case's second chunk per wave and second k_app_dy pass."""
    launch = lambda case: R.app_bwd_launch(R.scene(case[0]).grid, R.scene(case[0]).n_acomp, R.scene(case[0]).n_lights, R.app_case(*case).n)
    by_scene = {c[0]: launch(c) for c in R.APP_CASES}
    assert {R.scene(c[0]).n_acomp for c in R.APP_CASES} == {16, 24, 48, 96}
    assert {(c[0], c[3]) for c in R.APP_CASES} >= {(s, m) for s in R.APP_WIDTHS for m in ("rad", "int", "both")}
    assert {c[4] for c in R.APP_CASES} == set(R.APP_STRIDES) and {c[5] for c in R.APP_CASES} == {"none", "monotone", "perm"}
    assert {c[2] for c in R.APP_CASES if c[:2] == ("d16_a48", "rays") and c[3:] == ("both", 32, "none")} == set(R.APP_COUNTS)
    for name, (line_lds, lds_light, blocks, chunks, passes) in by_scene.items():
        assert line_lds == (name != "long_axis"), name                       # d16_a96 still stages its line
        assert lds_light == (name != "d16_a48_l17"), name
        assert chunks == 1 and passes == 1, name
    assert R.scene("long_axis").grid == [1520, 10, 12] and by_scene["d16_a96"][0]
    assert launch(("d16_a48", "rays", 513, "both", 32, "none"))[2] == 2      # more than one block
    s, n = R.scene("thin"), R.large_app_n()
    line_lds, lds_light, blocks, chunks, passes = R.app_bwd_launch(s.grid, s.n_acomp, s.n_lights, n)
    assert s.grid == [450, 10, 12] and s.n_acomp == 48 and line_lds and blocks == 256 and chunks == 2 and passes == 2
    assert R.app_bwd_launch(s.grid, s.n_acomp, s.n_lights, n - R.RUN - 1)[3] == 1 and n == 131081
    assert R.app_bwd_launch(R.scene("d16_a48").grid, 48, 3, n)[3] == 1       # under 80 KB of LDS the cap is 512 blocks: why the thin field


# ---- the derived-normal backward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NORMAL_CASES, ids=ident)
def test_normal_fixture(case):
    """Margins, redraw caps, the branches, and the tie: on the points whose taps all lie in the grid (where the oracle's zero
    padding and the clamped taps are the same function) the float32 gradients of autograd through O.density_grad(...)[2]."""
    fx = R.normal_case(*case)
    s, n = fx.scene, fx.n
    name, kind, _n = case
    assert fx.clean and fx.rounds <= M.REDRAW_ROUNDS and int(fx.redrawn.sum()) <= M.REDRAW_SHARE * n, (case, fx.rounds, int(fx.redrawn.sum()))
    assert not bool(R.normal_bad_points(s.sc, fx.xyz).any())
    s64, s32 = R.normal_states(s.sc, fx.xyz, F64), R.normal_states(s.sc, fx.xyz, F32)
    relu = O.density_act(s.sc) == "relu"
    assert relu == name.startswith("relu")
    if relu:
        assert float(s64.feat.abs().min()) > R.RELU_MARGIN and torch.equal(s64.feat > 0, s32.feat > 0)
        if n >= 100:
            assert bool((s64.feat > 0).any()) and bool((s64.feat < 0).any())
    else:
        assert torch.equal(s64.x > R.SOFTPLUS_LINEAR, s32.x > R.SOFTPLUS_LINEAR)
        if n >= 1000 and name != "clamp" and kind in ("generic", "rays"):      # the stock scenes (DENSITY_SCALE 30) reach it in the blob's core
            assert bool((s64.x > R.SOFTPLUS_LINEAR).any()) and bool((s64.x <= R.SOFTPLUS_LINEAR).any()), "the fixture needs pre-activations above 20"
    assert float((s64.g_norm / R.CLAMP - 1).abs().min()) > R.CLAMP_MARGIN and torch.equal(s64.g_norm > R.CLAMP, s32.g_norm > R.CLAMP)
    clamped = s64.g_norm <= R.CLAMP
    if name == "clamp" and n >= 100:
        assert float((clamped & (s64.g_norm > 0)).float().mean()) > 0.5, "most points take the clamp arm with a non-zero gradient"
    r64, r32 = R.normal_reference(fx, F64), R.normal_reference(fx, F32)
    if name == "clamp":
        assert all(bool((r64[k] != 0).any()) for k in R.NORMAL_LEAVES)
    label = f"normal {ident(case)}"
    print(f"\n[fieldgrad cpu {label}] redrawn {int(fx.redrawn.sum())} in {fx.rounds} rounds; x > 20 at {int((s64.x > 20).sum())}, clamp arm at "
          f"{int(clamped.sum())}; float32 restatement " + " ".join(f"{k} {R.distance(r32[k], r64[k]):.1e}" for k in R.NORMAL_LEAVES))
    if n == 1 or kind in ("dups", "alternate"):
        inside = torch.ones(n, dtype=torch.bool)
        assert bool((fx.xyz.abs() < 1).all())
    else:
        inside = (fx.xyz.abs() < 1).all(1)
    if not bool(inside.all()):                                # the restatement on the inside points alone
        sub = R.SimpleNamespace(scene=s, xyz=fx.xyz[inside].contiguous(), g_normal=fx.g_normal[inside].contiguous(), n=int(inside.sum()),
                                key=fx.key + ("inside",))
        r64, r32 = R.normal_reference(sub, F64), R.normal_reference(sub, F32)
    work = leaf_scene(s.sc, ("density_plane", "density_line"))
    (O.density_grad(work, fx.xyz[inside])[2] * fx.g_normal[inside]).sum().backward()
    for kind_, ts in (("plane", work.density_plane), ("line", work.density_line)):
        for i, t in enumerate(ts):
            got = torch.zeros_like(t) if t.grad is None else t.grad
            within_rule(f"{label} density_{kind_}.{i}", got, r32[f"density_{kind_}.{i}"], r64[f"density_{kind_}.{i}"])


def test_normal_cases_reach_their_arms():
    launch = lambda case: R.density_grad_launch(R.scene(case[0]).grid, R.scene(case[0]).n_dcomp, R.normal_case(*case).n)
    assert {R.scene(c[0]).n_dcomp for c in R.NORMAL_CASES} == {4, 8, 16, 32}
    assert {c[2] for c in R.NORMAL_CASES if c[:2] == ("d16_a48", "rays")} == set(R.NORMAL_COUNTS)
    for c in R.NORMAL_CASES:
        lds_lines, blocks, loops = launch(c)
        assert lds_lines == (c[0] != "long_axis") and loops == 1, c
    assert launch(("d16_a48", "rays", 129))[1] == 2 and launch(("d16_a48", "rays", 128))[1] == 1
    s, n = R.scene("d16_a48"), R.large_density_n()
    assert R.density_grad_launch(s.grid, s.n_dcomp, n) == (True, R.DENSITY_GRAD_CAP, 2)
    assert R.density_grad_launch(s.grid, s.n_dcomp, n - R.RUN - 1)[2] == 1
    assert float(R.scene("clamp").sc.density_shift) == R.CLAMP_SHIFT < float(s.sc.density_shift)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.ADAM_LISTS))
def test_adam_fixture(name):
    """The layout (guards, alignment, empties), the launches each list needs, the designed elements, and the tie: torch.optim.Adam's
    single float32 step from the same state (step - 1 steps taken) under the rule against the float64 restatement."""
    fx = R.adam_case(name)
    counts = fx.counts
    used = torch.zeros(fx.total, dtype=torch.bool)
    for c, o in zip(counts, fx.offsets):
        assert not bool(used[o - R.ADAM_GUARD:o + c + R.ADAM_GUARD].any()) or c == 0, "tensors closer than the guard"
        assert (o % 4 == 0) if fx.aligned else (o % 4 == 1)
        used[o:o + c] = True
    for role in (fx.p, fx.g, fx.m, fx.v):
        assert bool((role[~used] == R.GUARD_VALUE).all()) and bool(torch.isfinite(role).all())
    launches = R.adam_launches(counts)
    assert [t for l in launches for t, _f, _c in l] == [t for t, c in enumerate(counts) if c]
    assert all(l[0][1] == 0 and all(b[1] == a[1] + a[2] for a, b in zip(l, l[1:])) for l in launches)
    tensors = sum(1 for c in counts if c)
    if name.startswith("tensors_"):
        assert tensors == int(name.split("_")[1]) and counts[0] == 0 and counts[-1] == 0 and (tensors < 8 or 0 in counts[1:-1])
        assert len(launches) == {1: 1, 40: 1, 41: 2, 83: 3}[tensors]
    else:
        assert tuple(counts) == R.ADAM_SIZES and len(launches) == 1 and max(c for _t, _f, c in launches[0]) == 4
    assert len(counts) < 4 or set(fx.step) == set(R.ADAM_STEPS)
    ref64, ref32 = R.adam_reference(fx, F64), R.adam_reference(fx, F32)
    worst = {}
    for t, c in enumerate(counts):
        if c == 0:
            continue
        p0, g, m0, v0 = (R.adam_view(fx, r, t) for r in (fx.p, fx.g, fx.m, fx.v))
        assert float(g[0]) == 0 and float(m0[0]) == 0 and float(v0[0]) == 0 and float(ref32[t][0][0]) == float(p0[0]) == float(ref64[t][0][0])
        if c >= 1000:
            mag = g[g != 0].abs()
            assert float(mag.min()) < 1e-6 and float(mag.max()) > 1e2
        p = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([p], lr=fx.lr[t], betas=R.BETAS, eps=R.EPS)
        opt.state[p] = {"step": torch.tensor(float(fx.step[t] - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        p.grad = g.clone()
        opt.step()
        for what, got, i in (("p", p.detach(), 0), ("m", opt.state[p]["exp_avg"], 1), ("v", opt.state[p]["exp_avg_sq"], 2)):
            d, b = R.distance(got, ref64[t][i]), R.bound(ref32[t][i], ref64[t][i])
            assert d <= b, (name, t, what, d, b)
            worst[what] = max(worst.get(what, (0, 0)), (d, b))
    print(f"\n[fieldgrad cpu adam {name}] {tensors} tensors, {len(launches)} launch(es); torch.optim.Adam float32, worst (distance, bound): {worst}")
