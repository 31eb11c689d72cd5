"""torch restatement of the march and compositing stage (tir_march.hip: k_march_primary, k_exclusive_scan, k_compact_primary,
k_composite_primary, k_march_secondary[_lds]; tir_train.hip: k_composite_primary_bwd, k_march_primary_bwd) as compositions of the
oracle's dtype-agnostic functions (oracle/tensoir_oracle.py), run in float32 or float64 on demand with autograd on.  The float32
run's distance from the float64 run on the same fixture is the yardstick of tests/test_gpu_march_kernels.py (the device must come
within ten times it: shade_reference.distance / bound); tests/test_march_cpu.py asserts the fixtures' margins and ties the
restatement to the pinned oracle.  Also the fixtures both test files use.

Sample positions.  The kernels form z, o + d z and the normalised coordinates with individually rounded float32 operations, which
is what torch's float32 tensor operations do: O.sample_ray / O.sample_ray_equally / O.normalize_coord in float32 give the kernels'
bits (rec_xyz is compared exactly).  The float64 run takes those float32 world positions and distances widened to float64 and
evaluates everything behind them (normalisation, taps, activation, raw2alpha, sums) in float64.  The bounding-box and occupancy
decisions are taken once, in float32, on the float32 positions.

Early stop.  The primary kernel tests the running transmittance after every 64-sample chunk, the secondary kernels after every
32-sample step: weights (and the stored sigma) are zero from the first chunk after the one whose end transmittance fell below
t_stop, and t_end / vis is the transmittance at the end of that chunk.

Margins (asserted by tests/test_march_cpu.py, so that the GPU tests exclude nothing).  On every fixture every float64 weight keeps
W_MARGIN = 1e-3 relative from weight_thres, every chunk-end transmittance T_MARGIN = 1e-3 relative from every t_stop > 0 the tests
use, the occupancy decision is the same in float32 and float64, a relu field's density feature keeps RELU_MARGIN = 1e-6 from 0, and
float32 and float64 agree on every one of these decisions.  The builders redraw offending rays from a seeded generator, in at
most REDRAW_ROUNDS = 8 rounds and for at most REDRAW_SHARE = 5 % of a fixture's rays.  The compositing fixtures keep
COMPOSITE_MARGIN = 1e-5 on the max(a, a_jit, 1e-6) ties, on view . normal, on the [0, 1] clamps, on the sRGB knee and on the
normal-length clamp; their designed rays sit on thresholds with exact values.

The occupancy mask of the masked scene is built by the oracle (O.update_alpha_mask) on the CPU and travels in the checkpoint, so
that the CPU file sees the very fixtures the GPU file runs; building a mask on the device is tested in tests/test_gpu_occupancy_kernels.py."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import tensoir_oracle as O
from tensoir_amd import synth
from tests import config_scenes as CS
from tests.helpers import scene_from_checkpoint
from tests.shade_reference import KNEE, MAP_STRIDE, bound, distance  # noqa: F401  (the comparison rule, re-exported)

F32, F64 = torch.float32, torch.float64
PRIMARY_CHUNK, SECONDARY_STEP = 64, 32
ALPHA_GRID = (16, 18, 20)
PRIMARY_T_STOPS = (0.0, 1e-6, 1e-2)
SECONDARY_T_STOPS = (0.0, 1e-4)
W_MARGIN, T_MARGIN, RELU_MARGIN, COMPOSITE_MARGIN = 1e-3, 1e-3, 1e-6, 1e-5
REDRAW_SHARE, REDRAW_ROUNDS = 0.05, 8
NEAR, FAR = CS.SECOND["second_near"], CS.SECOND["second_far"]
FIXED_FRESNEL = 0.04

# name -> (matrix row, occupancy mask, grid).  The two thin fields reach the large-grid arms for a few hundred kilobytes per
# plane: `long_axis` has density lines of (1520 + 10 + 12) x 16 floats = 98688 bytes > 96 KiB (the primary march backward's
# global-atomic arm), `lds_1024` lines of 922 x 16 floats, more than two 512-thread blocks hold (the secondary march's 1024 arm).
# On CS.GRID a march step is 0.064 and a ray has left the box after some 45 samples: whatever the sample count, the second
# 64-sample chunk would hold culled samples only.  The sweeps over S and B therefore run on the same field at four times the
# resolution (step 0.016), with rays aimed so that they turn opaque across sample 64 or 128 (boundary_rays): the transmittance
# carried from chunk to chunk, the early stop at a chunk's end and the last sample's zero distance then meet samples that count.
FINE_GRID = [80, 96, 112]
SCENES = {
    "d16_a48": ("d16_a48", True, CS.GRID), "d16_a48_open": ("d16_a48", False, CS.GRID), "d4_a48": ("d4_a48", False, CS.GRID),
    "d8_a48": ("d8_a48", False, CS.GRID), "d32_a48": ("d32_a48", False, CS.GRID), "relu_d16_a48": ("relu_d16_a48", False, CS.GRID),
    "long_axis": ("d16_a48", False, [1520, 10, 12]), "lds_1024": ("d16_a48", False, [900, 10, 12]),
    "fine": ("d16_a48", True, FINE_GRID), "fine_open": ("d16_a48", False, FINE_GRID),
}
_scenes = {}


def scene(name):
    """-> namespace(name, ck: reference-format checkpoint, sc: float32 oracle Scene, grid, n_dcomp), built once."""
    if name not in _scenes:
        row_name, mask, grid = SCENES[name]
        row = CS.ROW[row_name]
        ck = CS.checkpoint(row, grid=grid)
        sc = scene_from_checkpoint(ck, *CS.ENVMAP_HW)
        if mask:
            with torch.no_grad():
                O.update_alpha_mask(sc, ALPHA_GRID)
            vol = sc.alpha_volume.bool()
            ck = dict(ck)
            ck["alphaMask.shape"] = tuple(vol.shape)
            ck["alphaMask.mask"] = np.packbits(vol.numpy().reshape(-1))
            ck["alphaMask.aabb"] = sc.alpha_aabb.clone()
            sc = scene_from_checkpoint(ck, *CS.ENVMAP_HW)
        _scenes[name] = SimpleNamespace(name=name, ck=ck, sc=sc, grid=[int(g) for g in grid], n_dcomp=row.n_dcomp)
    return _scenes[name]


# ---- which kernel a scene selects: the arithmetic of the launchers (tir_train.hip: tir_march_primary_bwd; tir_march.hip:
# tir_march_secondary_ids_fwd), TIR_TAPREC = 9 floats per tap record ----------------------------------------------------------------
def primary_bwd_arm(grid, n_dcomp):
    return "lds-lines" if sum(grid) * n_dcomp * 4 <= 96 * 1024 else "global-atomic"


def secondary_arm(grid, n_dcomp, n_sample, lds_lines=True):
    line_floats = sum(grid) * n_dcomp
    fixed = (line_floats + ((n_sample + 3) & ~3)) * 4
    lds512, lds1024 = fixed + (8 * 64 * 9 + 3 * 64) * 4, fixed + (16 * 64 * 9 + 3 * 128) * 4
    if lds_lines and n_dcomp == 16 and n_sample <= 96 and max(grid) < 65536 and lds1024 + 8192 <= 158 * 1024:
        return "lds-512" if lds512 + 4096 <= 80 * 1024 else "lds-1024"
    return "plain"


def plane_index_ok(grid, n_dcomp):
    """tir_plane_index_ok (tir_common.hpp)."""
    return all(grid[i] * grid[j] * n_dcomp * 4 < 2 ** 32 and grid[i] * n_dcomp * 4 < 2 ** 24 and grid[j] * n_dcomp * 4 < 2 ** 24
               for i in range(3) for j in range(i + 1, 3))


# ---- the restatement: marches ---------------------------------------------------------------------------------------------------------
def occupancy(sc, pts32, inside, dtype):
    """[B, S] bool: in the box and, where the scene has a mask, occupied -- the trilinear sample evaluated in dtype."""
    valid = inside.clone()
    if sc.alpha_volume is not None and bool(inside.any()):
        with torch.no_grad():
            valid[inside] = O.sample_occupancy(sc.to(dtype), pts32[inside].to(dtype), "explicit") > 0
    return valid


def _march(sc, pts32, z32, inside, t_stop, chunk, dtype, field=None, feature_leaf=False):
    """Cull + density + raw2alpha + the early stop per `chunk` samples on float32 positions pts32 [B, S, 3] at distances z32
    [B, S].  field: a scene that carries the density planes, lines and activation in dtype (leaf copies for autograd); default
    sc in dtype.  feature_leaf: the density feature [B, S] becomes a leaf (for d loss / d feature)."""
    B, S = z32.shape
    valid = occupancy(sc, pts32, inside, F32)
    with torch.no_grad():
        xyz32 = O.normalize_coord(sc, pts32)
    geo = sc.to(dtype)
    fld = geo if field is None else field
    pts, z = pts32.to(dtype), z32.to(dtype)
    xyz = O.normalize_coord(geo, pts)
    feat = torch.zeros(B, S, dtype=dtype)
    if bool(valid.any()):
        feat = feat.index_put((valid,), O.density_feature(fld, xyz[valid], "explicit"))
    if feature_leaf:
        feat = feat.detach().requires_grad_(True)
    sigma = torch.where(valid, O.feature2density(fld, feat), torch.zeros_like(feat))
    dists = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), dim=-1) * sc.distance_scale
    alpha, weight, _ = O.raw2alpha(sigma, dists)
    T = torch.cumprod(1.0 - alpha + 1e-10, dim=-1)
    ends = torch.tensor([min(c + chunk, S) - 1 for c in range(0, S, chunk)])
    T_ends = T[:, ends]
    below = T_ends.detach() < t_stop
    stop = torch.where(below.any(1), below.int().argmax(1), torch.full((B,), len(ends) - 1))
    live = (torch.arange(S)[None] // chunk) <= stop[:, None]
    weight = torch.where(live, weight, torch.zeros_like(weight))
    sigma_out = torch.where(live, sigma, torch.zeros_like(sigma))
    keep = weight.detach() > sc.weight_thres
    return SimpleNamespace(weight=weight, sigma=sigma_out, acc=weight.sum(-1), depth=(weight * z).sum(-1),
                           t_end=T_ends.gather(1, stop[:, None])[:, 0], cnt=keep.sum(-1).int(), keep=keep, feat=feat, valid=valid,
                           inside=inside, live=live, z=z, z32=z32, pts32=pts32, xyz32=xyz32, T_ends=T_ends)


def march_primary(sc, rays, S, jitter, t_stop, dtype, **kw):
    """tir_march_primary_fwd / _train_fwd: rays [B, 6], jitter [B, 1] or None -> weight, sigma [B, S], acc, depth, t_end, cnt
    [B] (and what they were made from)."""
    rays = torch.as_tensor(rays).float()
    with torch.no_grad():
        pts32, z32, inside = O.sample_ray(sc, rays[:, :3], rays[:, 3:6], S, jitter)
    return _march(sc, pts32, z32.expand(rays.shape[0], S).contiguous(), inside, t_stop, PRIMARY_CHUNK, dtype, **kw)


def z_values(n_sample):
    """The float32 sample distances the caller hands to the secondary march."""
    t = torch.linspace(0.0, 1.0, n_sample)
    return NEAR * (1.0 - t) + FAR * t


def march_secondary(sc, origins, dirs, n_sample, t_stop, dtype):
    """tir_march_secondary_fwd per ray: origins, dirs [n, 3] -> t_end (vis), 1 - acc, weight, keep (the records, in sample order)."""
    with torch.no_grad():
        pts32, z32, inside = O.sample_ray_equally(sc, origins.float(), dirs.float(), n_sample, NEAR, FAR)
    assert torch.equal(z32[0], z_values(n_sample))
    out = _march(sc, pts32, z32.expand(origins.shape[0], n_sample).contiguous(), inside, t_stop, SECONDARY_STEP, dtype)
    out.one_minus_acc = 1 - out.acc
    return out


def march_bad_rays(sc, run, t_stops, chunk):
    """[B] bool: the rays of a fixture that break a margin or on which float32 and float64 take a different decision.
    run(dtype) -> the un-stopped march (t_stop 0) in dtype."""
    r64, r32 = run(F64), run(F32)
    thres = sc.weight_thres
    bad = ((r64.weight / thres - 1).abs() <= W_MARGIN).any(1) | (r64.keep != r32.keep).any(1)
    for t in t_stops:
        if t > 0:
            bad |= ((r64.T_ends / t - 1).abs() <= T_MARGIN).any(1) | ((r64.T_ends < t) != (r32.T_ends < t)).any(1)
    bad |= (occupancy(sc, r64.pts32, r64.inside, F64) != r64.valid).any(1)
    if O.density_act(sc) == "relu":
        bad |= (r64.valid & (r64.feat.abs() <= RELU_MARGIN)).any(1) | (r64.valid & ((r64.feat > 0) != (r32.feat > 0))).any(1)
    return bad


def _unit(gen, n):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)


# ---- fixtures: primary rays ------------------------------------------------------------------------------------------------------------
N_DESIGNED = 5


def designed_rays():
    """0 straight down the middle of the blob (two zero direction components: the 1e-6 substitution; an opaque stretch where
    1 - alpha + 1e-10 is 1e-10), 1 starts inside the box, 2 misses the box, 3 enters through the top and leaves through a side
    long before its last sample, 4 one zero direction component, off the middle."""
    d = lambda *v: torch.nn.functional.normalize(torch.tensor(v), dim=0)
    rows = [(torch.tensor([0.02, -0.03, 4.0]), torch.tensor([0.0, 0.0, -1.0])),
            (torch.tensor([0.3, -0.2, 1.0]), d(-0.2, 0.1, -1.0)),
            (torch.tensor([0.0, 0.0, 4.0]), d(0.9, 0.9, -1.0)),
            (torch.tensor([0.0, 0.0, 4.0]), d(0.5, 0.45, -1.0)),
            (torch.tensor([0.4, 0.1, 4.0]), d(0.0, -0.08, -1.0))]
    return torch.stack([torch.cat(r) for r in rows])


BOUNDARY_POOL = 64
_boundary = {}


def boundary_rays(s, chunk):
    """BOUNDARY_POOL rays of scene s on which the float64 transmittance at the end of 64-sample chunk `chunk` (0 or 1) lies in
    (0.05, 0.95): the blob's surface -- where a ray turns opaque within a few samples -- falls across sample 64 or 128, so the
    kernel's chunk-to-chunk carry multiplies weights that count.  Drawn from a seeded generator and selected by the reference
    alone: points round the surface, inward directions, the origin 6 units back (outside the box)."""
    key = (s.name, chunk)
    if key not in _boundary:
        gen = torch.Generator().manual_seed(600 + chunk)
        found = []
        half = (s.sc.aabb[1] - s.sc.aabb[0]) / 2
        for _ in range(20):
            p = _unit(gen, 4096) * half * 0.66 * (0.9 + 0.2 * torch.rand(4096, 1, generator=gen))
            d = _unit(gen, 4096)
            d = torch.where(((d * p).sum(-1, keepdim=True) > 0), -d, d)
            rays = torch.cat([p - 6.0 * d, d], -1)
            with torch.no_grad():
                T = march_primary(s.sc, rays, 64 * (chunk + 1), None, 0.0, F64).T_ends[:, chunk]
            found.append(rays[(T > 0.05) & (T < 0.95)])
            if sum(f.shape[0] for f in found) >= BOUNDARY_POOL:
                break
        _boundary[key] = torch.cat(found)[:BOUNDARY_POOL].contiguous()
        assert _boundary[key].shape[0] == BOUNDARY_POOL, "too few rays turn opaque across the chunk's end"
    return _boundary[key]


def base_rays(B, s=None):
    """The designed rays (a fan ray second), then a pin-hole fan at the blob in a seeded order; on the fine scenes every third
    and every third-plus-one of the first 3 * BOUNDARY_POOL fan places holds a ray of boundary_rays(s, 0) / (s, 1) instead."""
    n = 16
    while n * n + N_DESIGNED < B:
        n *= 2
    fan = synth.make_rays(n, n)
    fan = fan[torch.randperm(n * n, generator=torch.Generator().manual_seed(5))]
    if s is not None and s.grid == FINE_GRID:
        for chunk in (0, 1):
            fan[chunk:3 * BOUNDARY_POOL:3] = boundary_rays(s, chunk)
    order = [0, N_DESIGNED] + list(range(1, N_DESIGNED)) + list(range(N_DESIGNED + 1, N_DESIGNED + n * n))
    return torch.cat([designed_rays(), fan])[order][:B].contiguous()


def random_rays(n, gen):
    o = torch.tensor([0.0, 0.0, 4.0]) + (torch.rand(n, 3, generator=gen) - 0.5) * 0.6
    target = (torch.rand(n, 3, generator=gen) - 0.5) * 1.6
    return torch.cat([o, torch.nn.functional.normalize(target - o, dim=-1)], -1)


def _settle(n, bad_of, redraw):
    """Redraw offending rays (redraw(bad) -> the rays it drew again) until none is left or the rounds run out -> (redrawn [n]
    bool, rounds, clean)."""
    redrawn, rounds = torch.zeros(n, dtype=torch.bool), 0
    while True:
        bad = bad_of()
        if not bool(bad.any()):
            return redrawn, rounds, True
        if rounds == REDRAW_ROUNDS:
            return redrawn, rounds, False
        rounds += 1
        redrawn |= redraw(bad)


_primary = {}


def primary_case(scene_name, B, S, jitter=False):
    """-> namespace(scene, rays [B, 6], jitter [B, 1] or None, S, redrawn, rounds, clean), built once and left unchanged."""
    key = (scene_name, B, S, jitter)
    if key not in _primary:
        s = scene(scene_name)
        gen = torch.Generator().manual_seed(1000 * B + 10 * S + int(jitter))
        fx = SimpleNamespace(scene=s, rays=base_rays(B, s), jitter=torch.rand(B, 1, generator=gen) if jitter else None, S=S, B=B)

        def redraw(bad):
            fx.rays[bad] = random_rays(int(bad.sum()), gen)
            return bad
        fx.redrawn, fx.rounds, fx.clean = _settle(
            B, lambda: march_bad_rays(s.sc, lambda dt: march_primary(s.sc, fx.rays, S, fx.jitter, 0.0, dt), PRIMARY_T_STOPS, PRIMARY_CHUNK),
            redraw)
        _primary[key] = fx
    return _primary[key]


def primary_reference(fx, t_stop, dtype, **kw):
    return march_primary(fx.scene.sc, fx.rays, fx.S, fx.jitter, t_stop, dtype, **kw)


# (scene, B, S, jitter): one sweep per axis around (fine, 40, 65), then every density width, relu and the mask on and off
PRIMARY_FORWARD = [("fine", B, 65, False) for B in (1, 3, 4, 5, 257)] + \
                  [("fine", 40, S, j) for S in (1, 2, 63, 64, 65, 129, 200) for j in (False, True)] + \
                  [(name, 40, 65, True) for name in ("fine_open", "d16_a48", "d16_a48_open", "d4_a48", "d8_a48", "d32_a48", "relu_d16_a48")]
PRIMARY_BACKWARD = [("fine_open", 40, S, True) for S in (1, 63, 64, 65, 129)] + [("fine_open", B, 65, False) for B in (1, 5, 257)] + \
                   [(name, 40, 65, True) for name in ("d16_a48_open", "d4_a48", "d8_a48", "d32_a48", "relu_d16_a48", "long_axis")] + \
                   [("fine", 2053, 33, False)]


def march_gradients(fx, cot, dtype, field=None):
    """Autograd through the primary-march restatement (t_stop 0) of (weight g_weight).sum() + (acc g_acc).sum() + (depth
    g_depth).sum(), cot = (g_weight [B, S], g_acc [B], g_depth [B]): -> d / d density feature [B, S]; with `field` (leaf planes and
    lines) the loss is also sent back to them (their .grad)."""
    r = primary_reference(fx, 0.0, dtype, field=field, feature_leaf=field is None)
    gw, ga, gd = (c.to(dtype) for c in cot)
    loss = (r.weight * gw).sum() + (r.acc * ga).sum() + (r.depth * gd).sum()
    if field is None:
        return torch.autograd.grad(loss, r.feat)[0]
    feat = r.feat
    g = torch.autograd.grad(loss, feat, retain_graph=True)[0]
    loss.backward()
    return g


def density_leaves(sc, dtype):
    """sc in dtype with leaf copies of the density planes and lines (+ name -> leaf): the float32 counterpart of
    pointwise_ref.scene64 for the yardstick of the plane and line gradients."""
    fld = sc.to(dtype)
    fld.density_plane = [t.detach().clone().requires_grad_(True) for t in fld.density_plane]
    fld.density_line = [t.detach().clone().requires_grad_(True) for t in fld.density_line]
    params = {f"density_{kind}.{i}": t for kind, ts in (("plane", fld.density_plane), ("line", fld.density_line)) for i, t in enumerate(ts)}
    return fld, params


def least_pass(sc, r, ray=0):
    """The smallest 1 - alpha along a ray of a float64 run: 0 where a sample is opaque to the last bit (the kernel's factor is
    then the 1e-10 it adds), a few 1e-9 on the fine scenes' shorter steps."""
    dist = (r.z[ray, 1] - r.z[ray, 0]) * sc.distance_scale
    return float(torch.exp(-r.sigma[ray].detach() * dist).min())


def march_cotangent(B, S, seed=31):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, generator=gen), torch.randn(B, generator=gen), torch.randn(B, generator=gen)


# ---- fixtures: secondary rays ----------------------------------------------------------------------------------------------------------
LIST_RAYS = 160
GRID_POINTS, GRID_DIRS = 5, 24
_secondary = {}


def _shell(gen, n):
    """Points round the blob's surface (the density feature crosses its shift near radius 0.95): some inside it, some outside."""
    return _unit(gen, n) * (0.85 + 0.5 * torch.rand(n, 1, generator=gen))


def _secondary_settle(fx, gen, group):
    """Redraw the origins of offending rays; group > 1: rays come in blocks of `group` that share an origin (the pair grid)."""
    s, n = fx.scene, fx.origins.shape[0]

    def bad_of():
        return march_bad_rays(s.sc, lambda dt: march_secondary(s.sc, fx.origins, fx.dirs, fx.n_sample, 0.0, dt), SECONDARY_T_STOPS,
                              SECONDARY_STEP)

    def redraw(bad):
        pts = bad.view(-1, group).any(1)
        fx.origins.view(-1, group, 3)[pts] = _shell(gen, int(pts.sum()))[:, None, :]
        return pts[:, None].expand(-1, group).reshape(-1)         # every ray of a redrawn point counts as redrawn
    fx.redrawn, fx.rounds, fx.clean = _settle(n, bad_of, redraw)


def secondary_case(scene_name, n_sample):
    """LIST_RAYS independent secondary rays: origins round the blob's surface, unit directions; 0 starts at the middle of the blob
    along +z (zero direction components, opaque from the first sample), 1 starts outside the box and enters it along -x, 2 starts
    outside and never enters.  Every way the kernels address rays (direct, origin / direction maps, lists of ids) selects rays
    of this list.  -> namespace(scene, origins, dirs [n, 3], n_sample, z_vals, redrawn, rounds, clean), built once."""
    key = (scene_name, n_sample)
    if key not in _secondary:
        gen = torch.Generator().manual_seed(77 + n_sample)
        origins, dirs = _shell(gen, LIST_RAYS), _unit(gen, LIST_RAYS)
        origins[0], dirs[0] = torch.tensor([0.01, 0.02, -0.01]), torch.tensor([0.0, 0.0, 1.0])
        origins[1], dirs[1] = torch.tensor([1.7, 0.2, 0.3]), torch.tensor([-1.0, 0.0, 0.0])
        origins[2], dirs[2] = torch.tensor([1.7, 0.2, 0.3]), torch.tensor([1.0, 0.0, 0.0])
        fx = SimpleNamespace(scene=scene(scene_name), origins=origins, dirs=dirs, n_sample=n_sample, z_vals=z_values(n_sample))
        _secondary_settle(fx, gen, 1)
        fx.key = key
        _secondary[key] = fx
    return _secondary[key]


def secondary_grid_case(scene_name, n_sample=33):
    """The dense pair grid: GRID_POINTS origins x GRID_DIRS directions, pair p = point p / n_dirs, direction p % n_dirs.  origins
    and dirs hold the expanded pairs; points [P, 3] and table [D, 3] what the kernel is given.  A smaller n_dirs uses the first
    directions of the table: grid_subset()."""
    key = (scene_name, n_sample, "grid")
    if key not in _secondary:
        gen = torch.Generator().manual_seed(501 + n_sample)
        table = _unit(gen, GRID_DIRS)
        origins = _shell(gen, GRID_POINTS)[:, None, :].expand(-1, GRID_DIRS, 3).reshape(-1, 3).contiguous()
        fx = SimpleNamespace(scene=scene(scene_name), origins=origins, dirs=table[None].expand(GRID_POINTS, -1, 3).reshape(-1, 3).contiguous(),
                             table=table, n_sample=n_sample, z_vals=z_values(n_sample))
        _secondary_settle(fx, gen, GRID_DIRS)
        fx.points = fx.origins.view(GRID_POINTS, GRID_DIRS, 3)[:, 0].contiguous()
        fx.key = key
        _secondary[key] = fx
    return _secondary[key]


def grid_subset(grid, n_dirs):
    """The pair grid with the first n_dirs directions as a fixture of its own: its rays are pairs of the full grid."""
    sub = (torch.arange(GRID_POINTS)[:, None] * GRID_DIRS + torch.arange(n_dirs)[None]).reshape(-1)
    return SimpleNamespace(**{**grid.__dict__, "origins": grid.origins[sub], "dirs": grid.dirs[sub], "key": grid.key + (n_dirs,)})


_secondary_ref = {}


def secondary_reference(fx, t_stop, dtype):
    """march_secondary over the fixture's rays, once per (fixture, t_stop, dtype)."""
    key = (fx.key, t_stop, dtype)
    if key not in _secondary_ref:
        with torch.no_grad():
            _secondary_ref[key] = march_secondary(fx.scene.sc, fx.origins, fx.dirs, fx.n_sample, t_stop, dtype)
    return _secondary_ref[key]


# route -> (scene, density lines staged in LDS); the launcher's arithmetic (secondary_arm) says which kernel that selects
SECONDARY_ROUTES = {"plain-8": ("d8_a48", True), "plain-16": ("d16_a48", False), "lds-512": ("d16_a48", True), "lds-1024": ("lds_1024", True)}
SECONDARY_SAMPLES = (1, 2, 31, 32, 33, 64, 95, 96)
SECONDARY_SAMPLES_PLAIN = (97, 256)
SECONDARY_RAYS = (1, 31, 32, 33, 63, 64, 65, 129)
SECONDARY_CASES = [(route, n) for route in SECONDARY_ROUTES for n in SECONDARY_SAMPLES + (SECONDARY_SAMPLES_PLAIN if route == "plain-16" else ())]


# ---- the restatement: compositing ------------------------------------------------------------------------------------------------------
def composite(rays, offsets, rec_w, rgb, brdf, brdf_jit, pred, der, acc, depth, white_bg, is_relight, dtype, fixed_fresnel=FIXED_FRESNEL,
              aux=None):
    """tir_composite_primary (models/tensorBase_rotated_lights.py:973-1031): per-record tensors (any of them None: taken as 0)
    summed per ray through offsets [B + 1] -> map rows [B, 20]: rgb 0-2, depth 3, normal 4-6, albedo 7-9, roughness 10, fresnel
    11-13, acc 14, normals_diff 15, normals_orientation 16, albedo / roughness smoothness cost 17 / 18, 19 zero.  Differentiable.
    aux (a dict) receives the sums before the clamps."""
    c = lambda t: None if t is None else (t if t.dtype == dtype else t.to(dtype))
    rays, rec_w, rgb, brdf, brdf_jit, pred, der, acc, depth = (c(t) for t in (rays, rec_w, rgb, brdf, brdf_jit, pred, der, acc, depth))
    B = rays.shape[0]
    cnt = (offsets[1:] - offsets[:-1]).long()
    ray = torch.repeat_interleave(torch.arange(B), cnt)
    seg = lambda v: torch.zeros(B, v.shape[1], dtype=dtype).index_add(0, ray, v)
    zeros = lambda n: torch.zeros(B, n, dtype=dtype)
    w = rec_w[:, None]
    bg = (1.0 - acc)[:, None]
    rgb_map = seg(w * rgb) if rgb is not None else zeros(3)
    depth = depth[:, None]
    if white_bg:
        depth = depth + bg * rays[:, 5:6]
        rgb_map = rgb_map + bg
    if not is_relight:
        return torch.cat([rgb_map, depth, zeros(10), acc[:, None], zeros(5)], -1)
    albedo, rough, alb_cost, rgh_cost = zeros(3), zeros(1), zeros(1), zeros(1)
    if brdf is not None:
        va, vr = brdf[:, :3], brdf[:, 3:4] * 0.9 + 0.09
        albedo, rough = seg(w * va), seg(w * vr)
        if brdf_jit is not None:
            alb_cost = seg(w * O.relative_smoothness(va, brdf_jit[:, :3]))
            rgh_cost = seg(w * O.relative_smoothness(vr, brdf_jit[:, 3:4] * 0.9 + 0.09))
    normal, ndiff, norient = zeros(3), zeros(1), zeros(1)
    if pred is not None:
        normal = seg(w * pred)
        if der is not None:
            ndiff = seg(w * torch.sum((pred - der) ** 2, dim=-1, keepdim=True))
        norient = seg(w * torch.sum(rays[ray, 3:6] * pred, dim=-1, keepdim=True).clamp(min=0))
    fresnel = torch.full((B, 1), fixed_fresnel, dtype=dtype)
    if white_bg:
        normal = normal + bg * torch.tensor([0.0, 0.0, 1.0], dtype=dtype)
        albedo, rough, fresnel = albedo + bg, rough + bg, fresnel + bg
    if aux is not None:
        aux.update(rgb=rgb_map.detach(), albedo=albedo.detach(), rough=rough.detach(), fresnel=fresnel.detach(),
                   normal_length=torch.linalg.norm(normal.detach(), dim=-1, keepdim=True))
    return torch.cat([O.linear2srgb(rgb_map.clamp(0, 1)), depth, O.safe_l2_normalize(normal), albedo.clamp(0, 1), rough.clamp(0, 1),
                      fresnel.clamp(0, 1).expand(B, 3), acc[:, None], ndiff, norient, alb_cost, rgh_cost, zeros(1)], -1)


RECORD_COUNTS = (130, 0, 65, 1, 64, 63)
COMPOSITE_S = 200
COMPOSITE_B = (1, 3, 4, 5, 257)
RECORD_INPUTS = ("rgb", "brdf", "brdf_jit", "pred", "der")
# the designed rays (where B has them): 1 has no records and acc 0 (white_bg 1: normal (0, 0, 1) and albedo 1 exactly; white_bg
# 0: a normal sum of length 0 inside the 1e-6 clamp), 2 has acc 1 exactly, 3 one record whose colour sum 0.75 x 2 clips at 1
COMPOSITE_DESIGNED = {"empty": 1, "acc_one": 2, "clipped": 3}
COLUMN_GROUPS = {"rgb": slice(0, 3), "depth": slice(3, 4), "normal": slice(4, 7), "albedo": slice(7, 10), "roughness": slice(10, 11),
                 "fresnel": slice(11, 14), "acc": slice(14, 15), "normals_diff": slice(15, 16), "normals_orientation": slice(16, 17),
                 "albedo_cost": slice(17, 18), "roughness_cost": slice(18, 19)}
_composite = {}


def _draw_records(gen, n, view):
    """n records of one ray with view direction `view`: weights that sum to less than 1, decoder outputs away from their ties."""
    u = lambda *shape: torch.rand(*shape, generator=gen)
    w = 0.2 + 0.8 * u(n)
    w = w / w.sum() * (0.3 + 0.65 * u(1)) if n else w
    brdf = 0.05 + 0.9 * u(n, 4)
    jit = (brdf + 0.05 * torch.randn(n, 4, generator=gen)).clamp(0.02, 0.98)
    pred = _unit(gen, n) * (0.5 + u(n, 1))
    return w, u(n, 3), brdf, jit, pred, _unit(gen, n)


def composite_case(B):
    """-> namespace(rays [B, 6], offsets [B + 1] int32, rec_k, rec_ray [A] int32, rec_w [A], rgb [A, 3], brdf, brdf_jit [A, 4], pred,
    der [A, 3], acc, depth [B], S, rows: the designed rays that fit, redrawn, rounds, clean).  Records per ray: 130, 0, 65, 1, 64,
    63 in turn (the lane-stride loop's edges)."""
    if B in _composite:
        return _composite[B]
    gen = torch.Generator().manual_seed(300 + B)
    cnt = torch.tensor([RECORD_COUNTS[i % len(RECORD_COUNTS)] for i in range(B)])
    if B == 1:
        cnt[0] = 65
    off = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])
    A = int(off[-1])
    rays = torch.cat([torch.randn(B, 3, generator=gen), _unit(gen, B)], -1)
    fx = SimpleNamespace(rays=rays, offsets=off.int(), S=COMPOSITE_S, B=B, rec_ray=torch.repeat_interleave(torch.arange(B), cnt).int(),
                         rec_k=torch.zeros(A, dtype=torch.int32), rec_w=torch.zeros(A), rgb=torch.zeros(A, 3), brdf=torch.zeros(A, 4),
                         brdf_jit=torch.zeros(A, 4), pred=torch.zeros(A, 3), der=torch.zeros(A, 3), acc=torch.zeros(B),
                         depth=2.0 + 4.0 * torch.rand(B, generator=gen))
    fx.rows = {k: i for k, i in COMPOSITE_DESIGNED.items() if i < B and B >= 4}

    def fill(r):
        a, e = int(off[r]), int(off[r + 1])
        fx.rec_k[a:e] = torch.sort(torch.randperm(COMPOSITE_S, generator=gen)[:e - a]).values.int()
        fx.rec_w[a:e], fx.rgb[a:e], fx.brdf[a:e], fx.brdf_jit[a:e], fx.pred[a:e], fx.der[a:e] = _draw_records(gen, e - a, rays[r, 3:6])
        fx.acc[r] = float(fx.rec_w[a:e].sum()) + 0.04 * float(torch.rand(1, generator=gen))
    for r in range(B):
        fill(r)
    if fx.rows:
        fx.acc[fx.rows["empty"]] = 0.0
        fx.acc[fx.rows["acc_one"]] = 1.0
        a = int(off[fx.rows["clipped"]])
        fx.rec_w[a], fx.rgb[a], fx.acc[fx.rows["clipped"]] = 0.75, 2.0, 0.8125
    designed = torch.zeros(B, dtype=torch.bool)
    designed[list(fx.rows.values())] = True

    def redraw(bad):
        for r in torch.nonzero(bad).reshape(-1).tolist():
            fill(r)
        return bad
    fx.redrawn, fx.rounds, fx.clean = _settle(B, lambda: composite_bad_rays(fx) & ~designed, redraw)
    fx.designed = designed
    _composite[B] = fx
    return fx


def composite_inputs(fx, drop=()):
    """The argument list of composite() / ops.composite_primary up to `depth`, the per-record tensors named in `drop` as None."""
    rec = [None if name in drop else getattr(fx, name) for name in RECORD_INPUTS]
    return [fx.rays, fx.offsets, fx.rec_w] + rec + [fx.acc, fx.depth]


def composite_states(fx, dtype):
    """The side every clamp, the knee and the normal-length test take, per ray, for both backgrounds -> dict of int tensors."""
    out = {}
    for wb in (0, 1):
        aux = {}
        with torch.no_grad():
            composite(*composite_inputs(fx), wb, 1, dtype, aux=aux)
        for k in ("rgb", "albedo", "rough", "fresnel"):
            out[f"{k}/{wb}"] = (aux[k] >= 0).int() + (aux[k] > 1).int()
        out[f"knee/{wb}"] = (aux["rgb"].clamp(0, 1) <= KNEE).int()
        out[f"length/{wb}"] = (aux["normal_length"] > 1e-6).int()
    return out


def composite_bad_rays(fx):
    """[B] bool: rays that break COMPOSITE_MARGIN somewhere or on which float32 and float64 take a different side."""
    m = COMPOSITE_MARGIN
    B = fx.B
    ray = fx.rec_ray.long()
    per_ray = lambda rec_bad: torch.zeros(B).index_add(0, ray, rec_bad.float()) > 0
    a, j = fx.brdf.double().clone(), fx.brdf_jit.double().clone()
    a[:, 3], j[:, 3] = a[:, 3] * 0.9 + 0.09, j[:, 3] * 0.9 + 0.09
    bad = per_ray((((a - j).abs() <= m) | ((torch.maximum(a, j) - 1e-6).abs() <= m)).any(1))
    dot = (fx.rays[ray, 3:6].double() * fx.pred.double()).sum(-1)
    bad |= per_ray(dot.abs() <= m)
    s64, s32 = composite_states(fx, F64), composite_states(fx, F32)
    for wb in (0, 1):
        aux = {}
        with torch.no_grad():
            composite(*composite_inputs(fx), wb, 1, F64, aux=aux)
        near = lambda x, t: (x != t) & ((x - t).abs() <= m)          # a sum that is exactly 0 or 1 (no records) is so in both types
        for k in ("rgb", "albedo", "rough", "fresnel"):
            bad |= (near(aux[k], 0.0) | near(aux[k], 1.0)).any(1)
        bad |= near(aux["rgb"], KNEE).any(1) | ((aux["normal_length"] != 0) & near(aux["normal_length"], 1e-6)).any(1)
    for k in s64:
        bad |= (s64[k] != s32[k]).any(1)
    return bad


def composite_gradients(fx, drop, white_bg, is_relight, cot, dtype):
    """Autograd of (maps cot).sum() through composite(): -> dict name -> gradient for rec_w, the per-record inputs that are given
    (zero where the branch does not use them), acc and depth."""
    names = ["rec_w"] + [n for n in RECORD_INPUTS if n not in drop] + ["acc", "depth"]
    leaves = {n: getattr(fx, n).detach().clone().to(dtype).requires_grad_(True) for n in names}
    rec = [leaves.get(n) for n in RECORD_INPUTS]
    maps = composite(fx.rays, fx.offsets, leaves["rec_w"], *rec, leaves["acc"], leaves["depth"], white_bg, is_relight, dtype)
    grads = torch.autograd.grad((maps * cot.to(dtype)).sum(), list(leaves.values()), allow_unused=True)
    return {n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(names, grads)}


def composite_cotangent(B, seed=41):
    return torch.randn(B, MAP_STRIDE, generator=torch.Generator().manual_seed(seed))


# ---- the scan --------------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)


def scan_counts(n, seed=3):
    """Counts in [0, 300] with runs of zeros."""
    gen = torch.Generator().manual_seed(seed + n)
    c = torch.randint(0, 301, (n,), generator=gen)
    runs = torch.rand(n, generator=gen) < 0.3
    for i in range(1, n):                                   # stretch the zeros into runs
        if runs[i - 1] and torch.rand(1, generator=gen) < 0.7:
            runs[i] = True
    return torch.where(runs, torch.zeros_like(c), c).int()
