"""torch restatement of the field-gradient scatter and optimiser kernels of tir_train.hip -- k_app_dy + k_vm_app_bwd (tir_vm_app_bwd),
k_density_grad_bwd (tir_density_grad_bwd), k_adam (tir_adam_step) -- as compositions of the oracle's dtype-agnostic functions
(oracle/tensoir_oracle.py) and of the border-clamped taps of tests/pointwise_ref.py, run in float32 or float64 on demand with
autograd on.  The float32 run's distance from the float64 run on the same fixture is the yardstick of
tests/test_gpu_fieldgrad_kernels.py (the device must come within ten times it: shade_reference.distance / bound);
tests/test_fieldgrad_cpu.py asserts the fixtures' margins and arms and ties the restatement to the pinned oracle.  Also the
fixtures both test files use, and the launchers' arithmetic (app_bwd_launch, density_grad_launch, adam_launches) the case sizes
are taken from.

Inputs are the float32 values the kernels get, widened.  Coordinates are normalised float32 and go to the kernels as they are.

Appearance scatter.  Leaves: app_plane[3], app_line[3], light_line and light_mean as a leaf of its own (the kernel keeps the two
light gradients apart; the model composes them as ll + lm / n_lights afterwards).  basis_mat is constant.  The loss is
sum(g_rad * rad_feat) + sum(g_int * intr_feat) over the first 27 columns of the cotangent rows, rad_feat from
light_line[clamp(light_idx[idx_map[i] or i], 0, n_lights - 1)] -- the clamp is the kernel's (include/tensoir_hip.h).  The taps are
grid_sample's (align_corners, zero padding: O.app_planeline), whose value is continuous across a cell border, so that the floor
needs no margin.  y_rad = (plane * line) * light row and y_int = (plane * line) * light_mean are restated too, and the basis
gradient is g_rad[:, :27]^T y_rad + g_int[:, :27]^T y_int formed in float64 from either run's y.

Derived-normal backward.  The loss is sum(g_normal * n), n = -g / max(|g|, 1e-6), g = act'(feat + shift) * grad feat over the
border-clamped taps with unclamped weights (pointwise_ref._clamped_feature / _ref_normals: the floor is taken in the kernel's
float32 arithmetic in both types); leaves density_plane[3], density_line[3].

Adam.  One step of m += (g - m)(1 - b1); v = v b2 + (1 - b2) g g; p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps) in the kernel's
operation order; the scalars are the float32 values the launcher forms (1 - b1, lr / bc1, 1 / sqrt(bc2)), widened.

Margins (asserted by tests/test_fieldgrad_cpu.py, so that the GPU tests exclude nothing).  On a relu fixture the float64 density
feature keeps RELU_MARGIN = 1e-6 from 0; on every derived-normal fixture |g| keeps CLAMP_MARGIN = 1e-3 relative from 1e-6; and
float32 and float64 take the same side of the relu sign, of x > 20 and of the normal's clamp.  The builders redraw offending
points (uniform in the box) from the fixture's seeded generator, in at most march_reference.REDRAW_ROUNDS = 8 rounds and for at
most REDRAW_SHARE = 5 % of a fixture's points; the seeds are chosen so that every fixture stays within that."""
from types import SimpleNamespace

import torch

from oracle import tensoir_oracle as O
from tests import config_scenes as CS
from tests import march_reference as M
from tests.helpers import scene_from_checkpoint
from tests.pointwise_ref import _clamped_feature, _ref_normals
from tests.shade_reference import bound, distance  # noqa: F401  (the comparison rule, re-exported)

F32, F64 = torch.float32, torch.float64
RELU_MARGIN, CLAMP, CLAMP_MARGIN, SOFTPLUS_LINEAR = M.RELU_MARGIN, 1e-6, 1e-3, 20.0
APP_DIM = 27
# the kernels' units (tir_train.hip)
RUN, WAVE_CHUNK, APP_THREADS, APP_MAX_L, APP_DY_CAP, DENSITY_GRAD_CAP = 8, 32, 1024, 16, 768, 1024
ADAM_MAX_T, ADAM_CHUNK = 40, 8192
CLAMP_SHIFT = -30.0                 # density_shift of the `clamp` scene: softplus' is about e^-30 off the blob

# name -> (matrix row, grid, density_shift or None).  `long_axis` ([1520, 10, 12]) has density lines of 98688 bytes > 96 KiB and
# an appearance line of 1520 x 48 floats, over the 160 KB budget: the global-atomic line arm of both kernels.  `thin` keeps the
# appearance planes small and its longest line (450 x 48 floats = 86400 bytes) staged, for more than 80 KB of LDS: the 256-block cap.
SCENES = {name: (name, CS.GRID, None) for name in ("d16_a48", "d4_a48", "d8_a48", "d32_a48", "d16_a16", "d16_a24", "d16_a96",
                                                   "relu_d16_a48", "d16_a48_l17")}
SCENES.update(long_axis=("d16_a48", [1520, 10, 12], None), thin=("d16_a48", [450, 10, 12], None), clamp=("d16_a48", CS.GRID, CLAMP_SHIFT))
_SHARED = {"d16_a48": "d16_a48_open", "d4_a48": "d4_a48", "d8_a48": "d8_a48", "d32_a48": "d32_a48", "relu_d16_a48": "relu_d16_a48",
           "long_axis": "long_axis"}          # the same unmasked scene of march_reference.SCENES, built once for both suites
_scenes = {}


def scene(name):
    """-> namespace(name, ck: reference-format checkpoint, sc: float32 oracle Scene, grid, n_dcomp, n_acomp, n_lights), built once."""
    if name not in _scenes:
        row_name, grid, shift = SCENES[name]
        row = CS.ROW[row_name]
        if name in _SHARED:
            assert M.SCENES[_SHARED[name]] == (row_name, False, grid)
            s = M.scene(_SHARED[name])
            ck, sc = s.ck, s.sc
        else:
            ck = CS.checkpoint(row, grid=grid)
            if shift is not None:
                ck = dict(ck, kwargs=dict(ck["kwargs"], density_shift=shift))
            sc = scene_from_checkpoint(ck, *CS.ENVMAP_HW)
        _scenes[name] = SimpleNamespace(name=name, ck=ck, sc=sc, grid=[int(g) for g in grid], n_dcomp=row.n_dcomp, n_acomp=row.n_acomp,
                                        n_lights=row.n_lights)
    return _scenes[name]


# ---- the launchers' arithmetic (tir_train.hip: launch_app_bwd, tir_density_grad_bwd, tir_adam_step) ------------------------------
def _ceil(a, b):
    return -(-a // b)


def app_bwd_launch(grid, n_acomp, n_lights, n):
    """-> (line_lds, lds_light, blocks, chunks per wave, k_app_dy passes) of tir_vm_app_bwd over n samples."""
    nl = min(n_lights, APP_MAX_L)
    base = 2 * (nl + 1) * 3 * n_acomp * 4
    line = max(grid) * n_acomp * 4
    line_lds = base + line <= 160 * 1024
    lds = base + (line if line_lds else 0)
    blocks = min(_ceil(2 * n, APP_THREADS), 256 * (2 if lds <= 80 * 1024 else 1))
    chunks_per_wave = _ceil(_ceil(n, WAVE_CHUNK), blocks * (APP_THREADS // 64))
    dy_blocks = min(_ceil(n, 128), APP_DY_CAP)
    return line_lds, n_lights <= APP_MAX_L, blocks, chunks_per_wave, _ceil(_ceil(n, 32), dy_blocks * 4)


def density_grad_launch(grid, n_dcomp, n):
    """-> (lds_lines, blocks, loop iterations) of tir_density_grad_bwd over n samples."""
    lps = min(n_dcomp, 16)
    blocks = min(_ceil(_ceil(n, RUN) * lps, 256), DENSITY_GRAD_CAP)
    lanes = _ceil(_ceil(n, RUN) * lps, 256) * 256
    return sum(grid) * n_dcomp * 4 <= 96 * 1024, blocks, _ceil(lanes, blocks * 256)


def adam_launches(counts):
    """-> one list per launch of (tensor, first chunk, chunks): empty tensors take no slot, a launch holds ADAM_MAX_T tensors."""
    launches, t = [], 0
    while t < len(counts):
        table, chunks = [], 0
        while t < len(counts) and len(table) < ADAM_MAX_T:
            if counts[t]:
                c = _ceil(counts[t], ADAM_CHUNK)
                table.append((t, chunks, c))
                chunks += c
            t += 1
        if table:
            launches.append(table)
    return launches


def first_looping_n(launch):
    """The first n at which launch(n) -> passes is 2, plus RUN: the second pass holds one full lane group and one single sample."""
    n = 1
    while launch(2 * n) < 2:
        n *= 2
    lo, hi = n, 2 * n                       # launch(lo) < 2 <= launch(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if launch(mid) >= 2 else (mid, hi)
    return hi + RUN


def large_app_n():
    s = scene("thin")
    return first_looping_n(lambda n: app_bwd_launch(s.grid, s.n_acomp, s.n_lights, n)[3])


def large_density_n():
    s = scene("d16_a48")
    return first_looping_n(lambda n: density_grad_launch(s.grid, s.n_dcomp, n)[2])


# ---- point sets --------------------------------------------------------------------------------------------------------------------
RAY_LENGTH = 21                      # samples per seeded ray: odd, so rays (and a per-ray light) end inside lane groups and chunks
OUTSIDE = 0.3


def box_points(gen, n):
    return torch.rand(n, 3, generator=gen) * 2 - 1


def generic_points(gen, n, grid):
    """Of every eight points: five in the box, one on a face, one on a grid line of an axis, one up to OUTSIDE outside along an
    axis (the axes in turn).  A single point is in the box."""
    x = box_points(gen, n)
    i = torch.arange(n)
    kind, axis = i % 8, (i // 8) % 3
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    size = torch.tensor(grid)[axis]
    node = (torch.rand(n, generator=gen) * size).long().clamp(max=size - 1)
    on_line = (2.0 * node.float() / (size - 1).float() - 1.0)
    out = sign * (1.0 + OUTSIDE * torch.rand(n, generator=gen).clamp(min=1e-3))
    col = x[i, axis]
    col = torch.where(kind == 4, sign, torch.where(kind == 5, on_line, torch.where(kind == 6, out, col)))
    x[i, axis] = col
    return x.contiguous(), i // RAY_LENGTH


def ray_points(gen, n, grid):
    """Consecutive samples half a voxel apart along seeded rays of RAY_LENGTH samples (they start in the middle 80 % of the box and
    may leave it): a lane group stays in a cell for 2-3 samples.  -> xyz [n, 3], ray id [n]."""
    n_rays = _ceil(n, RAY_LENGTH)
    start = box_points(gen, n_rays) * 0.8
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=gen), dim=-1)
    voxel = 2.0 / (torch.tensor(grid).float() - 1)
    k = torch.arange(RAY_LENGTH).float()
    pts = start[:, None, :] + 0.5 * k[None, :, None] * (d * voxel)[:, None, :]
    return pts.reshape(-1, 3)[:n].contiguous(), torch.arange(n_rays).repeat_interleave(RAY_LENGTH)[:n]


def dup_points(gen, n, grid):
    """n copies of one point: one run that is never flushed before the end; every atomic collides."""
    return (box_points(gen, 1) * 0.9).expand(n, 3).contiguous(), torch.arange(n) // RAY_LENGTH


def alternate_points(gen, n, grid):
    """Two points of different plane cells and line rows in turn: every step flushes."""
    a = box_points(gen, 1) * 0.4
    pair = torch.cat([a - 0.45, a + 0.45])
    return pair[torch.arange(n) % 2].contiguous(), torch.arange(n) // RAY_LENGTH


POINTS = {"generic": generic_points, "rays": ray_points, "dups": dup_points, "alternate": alternate_points}


def light_pattern(n, n_lights):
    """[n] int32: per 32 entries in turn one constant index, one that changes with every entry, one that changes every third entry;
    the values cycle through the first light, the last, the out-of-range -1 and n_lights, then the lights between."""
    vals = torch.tensor([0, n_lights - 1, -1, n_lights] + list(range(1, n_lights - 1)))
    i = torch.arange(n)
    chunk = i // WAVE_CHUNK
    pick = torch.where(chunk % 3 == 0, chunk // 3, torch.where(chunk % 3 == 1, i, i // 3))
    return vals[pick % len(vals)].int()


def tap_cells(x32, size):
    """The two (clamped) tap indices along one axis, from the kernels' float32 arithmetic (tir::unnorm, make_tap)."""
    i0 = torch.floor(((x32 + 1.0) * 0.5) * float(size - 1)).long()
    return i0.clamp(0, size - 1), (i0 + 1).clamp(0, size - 1)


def touched(grid, xyz32):
    """-> per VM group the [H, W] plane texels and the [R] line rows that are taps of a sample (bool): what a scatter may write."""
    planes, lines = [], []
    for i in range(3):
        m0, m1 = O.MAT_MODE[i]
        vi = O.VEC_MODE[i]
        W, H, R = grid[m0], grid[m1], grid[vi]
        xs, ys, ls = tap_cells(xyz32[:, m0], W), tap_cells(xyz32[:, m1], H), tap_cells(xyz32[:, vi], R)
        p = torch.zeros(H, W, dtype=torch.bool)
        for yy in ys:
            for xx in xs:
                p[yy, xx] = True
        l = torch.zeros(R, dtype=torch.bool)
        l[ls[0]] = True
        l[ls[1]] = True
        planes.append(p)
        lines.append(l)
    return planes, lines


# ---- the appearance scatter --------------------------------------------------------------------------------------------------------
APP_COUNTS = (1, 7, 8, 9, 31, 32, 33, 511, 512, 513, 1000)
APP_STRIDES = (27, 28, 32, 40)
APP_WIDTHS = ("d16_a16", "d16_a24", "d16_a48", "d16_a96")
LARGE_APP = ("thin", "rays", "large", "both", 32, "monotone")
# (scene, point set, n, rad / int / both, cotangent row stride, idx_map: none / monotone / perm)
APP_CASES = [("d16_a48", "rays", n, "both", 32, "none") for n in APP_COUNTS] + \
            [(s, "generic", 1000, "both", 32, "none") for s in APP_WIDTHS + ("d16_a48_l17", "long_axis")] + \
            [(s, "rays", 513, mode, 32, "none") for s in APP_WIDTHS + ("d16_a48_l17",) for mode in ("rad", "int")] + \
            [("d16_a48", "rays", 513, "both", st, "none") for st in APP_STRIDES if st != 32] + [("d16_a24", "generic", 33, "both", 27, "none")] + \
            [("d16_a48", "rays", 1000, "both", 32, mp) for mp in ("monotone", "perm")] + [("d16_a48_l17", "rays", 1000, "rad", 28, "perm")] + \
            [("d16_a48", "dups", 4096, "both", 32, "none"), ("long_axis", "dups", 4096, "both", 32, "none"),
             ("d16_a48", "alternate", 513, "both", 32, "none"), ("d16_a96", "alternate", 33, "both", 32, "monotone")]
_app = {}


def app_case(scene_name, kind, n, mode, stride, map_kind):
    """-> namespace(scene, xyz [n, 3], light_idx (int32: [n], or one per ray with the monotone map), idx_map ([n] int32 or None),
    g_rad, g_int ([n, stride], NaN in every padding column; None where the mode leaves one out), n, key), built once."""
    key = (scene_name, kind, n, mode, stride, map_kind)
    if key not in _app:
        s = scene(scene_name)
        if n == "large":
            n = large_app_n()
        gen = torch.Generator().manual_seed(7000 + 13 * n + stride + 101 * list(POINTS).index(kind) + len(scene_name))
        xyz, ray = POINTS[kind](gen, n, s.grid)
        if map_kind == "monotone":
            light, idx_map = light_pattern(int(ray[-1]) + 1, s.n_lights), ray.int()
        elif map_kind == "perm":
            light, idx_map = light_pattern(n, s.n_lights), torch.randperm(n, generator=gen).int()
        else:
            light, idx_map = light_pattern(n, s.n_lights), None

        def cotangent():
            g = torch.full((n, stride), float("nan"))
            g[:, :APP_DIM] = torch.randn(n, APP_DIM, generator=gen)
            return g
        _app[key] = SimpleNamespace(scene=s, xyz=xyz, light_idx=light, idx_map=idx_map, n=n, key=key, mode=mode, stride=stride,
                                    g_rad=cotangent() if mode != "int" else None, g_int=cotangent() if mode != "rad" else None)
    return _app[key]


def effective_light(fx):
    """The light row each sample multiplies: light_idx[idx_map[i] or i], clamped to [0, n_lights - 1] as the kernel does."""
    li = fx.light_idx.long()
    sel = fx.idx_map.long() if fx.idx_map is not None else torch.arange(fx.n)
    return li[sel].clamp(0, fx.scene.n_lights - 1)


APP_LEAVES = [f"app_{k}.{i}" for k in ("plane", "line") for i in range(3)] + ["light_line", "light_mean"]


def app_leaves(sc, dtype, light_mean=None):
    """sc in dtype with leaf copies of the appearance planes, lines and light rows; light_mean [3 Ca] (default: the float32 mean of
    the rows) a leaf of its own -> (field, light_mean leaf, name -> leaf)."""
    fld = sc.to(dtype)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    fld.app_plane, fld.app_line = [leaf(t) for t in fld.app_plane], [leaf(t) for t in fld.app_line]
    fld.light_line = leaf(fld.light_line)
    lm = leaf((sc.light_line.mean(0) if light_mean is None else torch.as_tensor(light_mean).detach().cpu().float()).to(dtype))
    params = {f"app_{kind}.{i}": t for kind, ts in (("plane", fld.app_plane), ("line", fld.app_line)) for i, t in enumerate(ts)}
    params.update(light_line=fld.light_line, light_mean=lm)
    return fld, lm, params


def basis_gradient(fx, y_rad, y_int):
    """g_rad[:, :27]^T y_rad + g_int[:, :27]^T y_int in float64."""
    out = torch.zeros(APP_DIM, 3 * fx.scene.n_acomp, dtype=F64)
    for g, y in ((fx.g_rad, y_rad), (fx.g_int, y_int)):
        if g is not None:
            out += g[:, :APP_DIM].double().T @ torch.as_tensor(y).detach().cpu().double()
    return out


APP_BLOCK = 16384
_app_ref = {}


def app_reference(fx, dtype, light_mean=None):
    """The restatement over a fixture in dtype -> namespace(y_rad, y_int [n, 3 Ca] or None, grads: name -> gradient of every leaf
    of APP_LEAVES, basis [27, 3 Ca] float64).  The samples go through autograd in blocks of APP_BLOCK (the gradients add up in the
    leaves).  light_mean: the row the kernel is given (the model's own float32 mean), default the float32 mean formed here."""
    key = (fx.key, dtype, None if light_mean is None else "given")
    if key in _app_ref:
        return _app_ref[key]
    sc = fx.scene.sc
    fld, lm, params = app_leaves(sc, dtype, light_mean)
    basis = fld.basis_mat.detach()
    li = effective_light(fx)
    ys = {"rad": torch.zeros(fx.n, basis.shape[1], dtype=dtype), "int": torch.zeros(fx.n, basis.shape[1], dtype=dtype)}
    for b in range(0, fx.n, APP_BLOCK):
        rows = slice(b, b + APP_BLOCK)
        pl = O.app_planeline(fld, fx.xyz[rows].to(dtype), "explicit").T
        loss = 0.0
        for name, g, row in (("rad", fx.g_rad, None), ("int", fx.g_int, lm)):
            if g is None:
                continue
            y = pl * (fld.light_line[li[rows]] if row is None else row[None])
            ys[name][rows] = y.detach()
            loss = loss + (g[rows, :APP_DIM].to(dtype) * torch.nn.functional.linear(y, basis)).sum()
        loss.backward()
    grads = {k: (torch.zeros_like(t) if t.grad is None else t.grad) for k, t in params.items()}
    y_rad, y_int = (ys["rad"] if fx.g_rad is not None else None), (ys["int"] if fx.g_int is not None else None)
    _app_ref[key] = SimpleNamespace(y_rad=y_rad, y_int=y_int, grads=grads, basis=basis_gradient(fx, y_rad, y_int))
    return _app_ref[key]


# ---- the derived-normal backward ---------------------------------------------------------------------------------------------------
NORMAL_COUNTS = (1, 7, 8, 9, 127, 128, 129, 1000)
NORMAL_WIDTHS = ("d4_a48", "d8_a48", "d16_a48", "d32_a48")
LARGE_NORMAL = ("d16_a48", "rays", "large")
# (scene, point set, n)
NORMAL_CASES = [("d16_a48", "rays", n) for n in NORMAL_COUNTS] + \
               [(s, "generic", 1000) for s in NORMAL_WIDTHS + ("relu_d16_a48", "long_axis", "clamp")] + \
               [(s, "rays", 129) for s in ("d4_a48", "d8_a48", "d32_a48", "relu_d16_a48", "clamp")] + \
               [("d16_a48", "dups", 4096), ("long_axis", "dups", 4096), ("d32_a48", "alternate", 513), ("d4_a48", "alternate", 33)]
_normal = {}


def normal_states(sc, xyz32, dtype):
    """What the branches of k_density_grad_bwd turn on, in dtype -> namespace(feat [n], x = feat + shift, g_norm = |act' grad feat|)."""
    fld = sc.to(dtype)
    x = xyz32.detach().clone().to(dtype).requires_grad_(True)
    feat = _clamped_feature(fld, xyz32, x)
    g = torch.autograd.grad(O.feature2density(fld, feat).sum(), x)[0]
    return SimpleNamespace(feat=feat.detach(), x=feat.detach() + sc.density_shift, g_norm=torch.linalg.vector_norm(g, dim=-1))


def normal_bad_points(sc, xyz32):
    """[n] bool: points that break a margin or on which float32 and float64 take a different side of a branch."""
    s64, s32 = normal_states(sc, xyz32, F64), normal_states(sc, xyz32, F32)
    if O.density_act(sc) == "relu":
        bad = (s64.feat.abs() <= RELU_MARGIN) | ((s64.feat > 0) != (s32.feat > 0))
    else:
        bad = (s64.x > SOFTPLUS_LINEAR) != (s32.x > SOFTPLUS_LINEAR)
    return bad | ((s64.g_norm / CLAMP - 1).abs() <= CLAMP_MARGIN) | ((s64.g_norm > CLAMP) != (s32.g_norm > CLAMP))


def normal_case(scene_name, kind, n):
    """-> namespace(scene, xyz [n, 3], g_normal [n, 3], n, key, redrawn, rounds, clean), built once."""
    key = (scene_name, kind, n)
    if key not in _normal:
        s = scene(scene_name)
        if n == "large":
            n = large_density_n()
        gen = torch.Generator().manual_seed(9000 + 17 * n + 101 * list(POINTS).index(kind) + len(scene_name))
        xyz, _ray = POINTS[kind](gen, n, s.grid)
        fx = SimpleNamespace(scene=s, xyz=xyz, g_normal=torch.randn(n, 3, generator=gen), n=n, key=key)

        def redraw(bad):
            fx.xyz[bad] = box_points(gen, int(bad.sum()))
            return bad
        fx.redrawn, fx.rounds, fx.clean = M._settle(n, lambda: normal_bad_points(s.sc, fx.xyz), redraw)
        _normal[key] = fx
    return _normal[key]


NORMAL_BLOCK = 32768
NORMAL_LEAVES = [f"density_{k}.{i}" for k in ("plane", "line") for i in range(3)]
_normal_ref = {}


def normal_reference(fx, dtype):
    """Autograd of sum(g_normal * n) through pointwise_ref._ref_normals in dtype -> name -> gradient of every leaf of NORMAL_LEAVES."""
    key = (fx.key, dtype)
    if key not in _normal_ref:
        fld, params = M.density_leaves(fx.scene.sc, dtype)
        for b in range(0, fx.n, NORMAL_BLOCK):
            x32 = fx.xyz[b:b + NORMAL_BLOCK]
            normal = _ref_normals(fld, x32, x32.detach().clone().to(dtype).requires_grad_(True))
            (normal * fx.g_normal[b:b + NORMAL_BLOCK].to(dtype)).sum().backward()
        _normal_ref[key] = {k: (torch.zeros_like(t) if t.grad is None else t.grad) for k, t in params.items()}
    return _normal_ref[key]


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------
# betas (0.9, 0.99) as tir_adam_step receives them: floats.  1 - beta in float32 is then exact; it is 1e-6 relative from 1 - 0.99
BETAS, EPS = (float(torch.tensor(0.9)), float(torch.tensor(0.99))), 1e-8
ADAM_SIZES = (1, 3, 4, 5, 255, 1023, 1024, 1025, 8191, 8192, 8193, 3 * 8192 + 5)
ADAM_GUARD, GUARD_VALUE = 8, -7.25
ADAM_LRS = (0.02, 0.001, 0.0005)
ADAM_STEPS = (1, 1000)
_MANY = (5, 1, 1025, 3, 255, 4, 8193, 1023)            # the sizes the long lists cycle through (8193: a tensor of two chunks)


def _with_empties(sizes):
    """An empty tensor first, last, and after every seventh tensor."""
    out = [0]
    for i, c in enumerate(sizes):
        out.append(c)
        if i % 7 == 6:
            out.append(0)
    return out + [0]


# name -> (element counts, every base 16-byte aligned).  The long lists hold 1 / 40 / 41 / 83 tensors that have elements -- the
# launcher's table of ADAM_MAX_T entries counts those -- and empty ones first, last and between.
ADAM_LISTS = {"sizes_aligned": (list(ADAM_SIZES), True), "sizes_offset": (list(ADAM_SIZES), False)}
ADAM_LISTS.update({f"tensors_{k}": (_with_empties([_MANY[i % len(_MANY)] for i in range(k)]), i_al) for k, i_al in
                   ((1, True), (40, False), (41, True), (83, False))})
_adam = {}


def adam_case(name):
    """-> namespace(counts, offsets (floats into the role's allocation), total, aligned, p, g, m, v: [total] float32 with
    GUARD_VALUE in the ADAM_GUARD floats between tensors, lr, bc1, bc2: per tensor), built once.  Gradients span 1e-8 to 1e4;
    every tensor starts with an element of g = m = v = 0 (denom = eps, p unchanged); tensors at step 1 have zero moments."""
    if name in _adam:
        return _adam[name]
    counts, aligned = ADAM_LISTS[name]
    gen = torch.Generator().manual_seed(400 + len(counts) + int(aligned))
    offsets, at = [], 0
    for c in counts:
        at = _ceil(at + ADAM_GUARD, 4) * 4 + (0 if aligned else 1)
        offsets.append(at)
        at += c
    total = at + ADAM_GUARD
    role = lambda: torch.full((total,), GUARD_VALUE)
    fx = SimpleNamespace(name=name, counts=counts, offsets=offsets, total=total, aligned=aligned, p=role(), g=role(), m=role(), v=role(),
                         lr=[], bc1=[], bc2=[], step=[])
    for t, (c, o) in enumerate(zip(counts, offsets)):
        step = ADAM_STEPS[t % 2]
        g = torch.randn(c, generator=gen) * 10.0 ** (torch.rand(c, generator=gen) * 12 - 8)
        m = torch.randn(c, generator=gen) * g.abs() if step > 1 else torch.zeros(c)
        v = (g * (0.5 + torch.rand(c, generator=gen))) ** 2 if step > 1 else torch.zeros(c)
        if c:
            g[0], m[0], v[0] = 0.0, 0.0, 0.0
        fx.p[o:o + c], fx.g[o:o + c], fx.m[o:o + c], fx.v[o:o + c] = 0.1 * torch.randn(c, generator=gen), g, m, v
        fx.lr.append(ADAM_LRS[t % 3])
        fx.step.append(step)
        fx.bc1.append(1 - BETAS[0] ** step)
        fx.bc2.append(1 - BETAS[1] ** step)
    _adam[name] = fx
    return fx


def adam_view(fx, role, t):
    return role[fx.offsets[t]:fx.offsets[t] + fx.counts[t]]


def _f32(x):
    return torch.tensor(x, dtype=F32)


def adam_step(p, g, m, v, lr, bc1, bc2, dtype, betas=BETAS, eps=EPS):
    """One step in dtype, in k_adam's operation order; the scalars are formed in float32 as tir_adam_step forms them (the host
    arrays are float), then widened -> (p, m, v)."""
    b1, b2, eps = _f32(betas[0]), _f32(betas[1]), _f32(eps)
    w1, w2 = 1.0 - b1, 1.0 - b2
    step_size, inv_bc2_sqrt = _f32(lr) / _f32(bc1), 1.0 / torch.sqrt(_f32(bc2))
    b2, eps, w1, w2, step_size, inv_bc2_sqrt = (x.to(dtype) for x in (b2, eps, w1, w2, step_size, inv_bc2_sqrt))
    p, g, m, v = (x.to(dtype) for x in (p, g, m, v))
    m = m + (g - m) * w1
    v = v * b2 + w2 * g * g
    denom = torch.sqrt(v) * inv_bc2_sqrt + eps
    return p - step_size * (m / denom), m, v


def adam_reference(fx, dtype):
    """-> per tensor (p, m, v) after the step, in dtype."""
    return [adam_step(adam_view(fx, fx.p, t), adam_view(fx, fx.g, t), adam_view(fx, fx.m, t), adam_view(fx, fx.v, t), fx.lr[t], fx.bc1[t],
                      fx.bc2[t], dtype) for t in range(len(fx.counts))]
