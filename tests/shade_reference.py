"""torch restatement of the shading stage (tir_shade.hip: k_ggx, k_shade_setup, k_shade_integrate, k_relight_importance[_cells],
k_env_sg, k_env_lookup; tir_train.hip: k_shade_integrate_bwd, k_env_sg_bwd; tir_march.hip: k_accumulate_records) as thin
compositions of the oracle's dtype-agnostic functions (oracle/tensoir_oracle.py), run in float32 or float64 on demand with
autograd on.  The float32 run's distance from the float64 run on the same fixture is the yardstick of the GPU tests
(tests/test_gpu_shade_kernels.py: the device must come within ten times it, DESIGN 4.8's rule); tests/test_shade_cpu.py prints
it per fixture and ties the restatement to the pinned oracle.  Also the fixtures both test files use.

Fixture invariant (as in the pipeline, where the secondary march fills only the pairs that pass the cosine mask): `vis` and
`indirect` are zero wherever the cosine is <= 1e-6.  The kernel's backward passes the cosine's gradient where cos_raw > 0 and
autograd's clamp(min=0) where cos_raw >= 0; both multiply it by a light of zero there, so the tests never feed the kernel a state
the pipeline cannot produce.

Margins (asserted by tests/test_shade_cpu.py, so that the GPU tests exclude nothing): on every row that is not a designed one a
dot product of unit vectors is at least DOT_MARGIN = 1e-5 (about 80 float32 ulps of 1) from each of its thresholds, the raw GGX
denominator at least NOM_MARGIN = 1e-2 relative from its lower clamp (nom0 = 1 - NoH^2 (1 - alpha^2) cancels: an error of 2^-23 in
NoH^2 is 4e-4 relative at the smallest nom0 that reaches the clamp at roughness 0.02, twice that in nom0^2), and a row total at
least TOTAL_MARGIN = 1e-3 relative from 0.0031308 and from 1 (the float32 total is within 2e-4 of the float64 one at roughness
0.02).  The builders redraw offending random rows until this holds; the designed rows sit on their thresholds with exact values
(axis-aligned vectors, exact products), and every predicate of every row takes the same value in float32 and float64."""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tensoir_oracle as O

MAP_STRIDE = 20                 # TIR_MAP_STRIDE: depth 3, normal 4-6, albedo 7-9, roughness 10, fresnel 11-13, acc 14
ACC_THRES = 0.5
COS_THRESHOLD = 1e-6
KNEE = 0.0031308
DOT_MARGIN, NOM_MARGIN, TOTAL_MARGIN = 1e-5, 1e-2, 1e-3
GROUPS = {"normal": slice(4, 7), "albedo": slice(7, 10), "roughness": slice(10, 11), "fresnel": slice(11, 14)}


def _c(x, dtype):
    x = torch.as_tensor(x)
    return x.to(dtype) if x.is_floating_point() else x


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def shade_integrate(maps, rays, dirs, light_idx, vis, indirect, env, weight_d, equal_area, use_srgb, acc_thres, dtype, aux=None):
    """render_with_BRDF's shading (models/relight_utils.py:452-480) on [M, 20] map rows -> [M, 3]; background rows (acc <=
    acc_thres) are white, light_idx is clamped to [0, n_lights - 1] as the kernel does.  aux (a dict) receives the row totals
    before the clip."""
    maps, rays, dirs, vis, env = (_c(x, dtype) for x in (maps, rays, dirs, vis, env))
    M, D = maps.shape[0], dirs.shape[0]
    normal, albedo, rough, fresnel, acc = maps[:, 4:7], maps[:, 7:10], maps[:, 10:11], maps[:, 11:14], maps[:, 14]
    surf2l = dirs.reshape(1, D, 3).expand(M, D, 3)
    surf2c = O.safe_l2_normalize(-rays[:, 3:6])
    cosine = torch.einsum("ijk,ik->ij", surf2l, normal).clamp(min=0.0)
    spec = O.ggx_specular(normal, surf2c, surf2l, rough.repeat(1, 3), fresnel)
    brdf = albedo.unsqueeze(1).expand(-1, D, -1) / np.pi + spec
    li = torch.as_tensor(light_idx).reshape(-1).long().clamp(0, env.shape[0] - 1)
    light = vis.reshape(M, D, 1) * torch.index_select(env, 0, li)
    if indirect is not None:
        light = light + _c(indirect, dtype).reshape(M, D, 3)
    if equal_area:
        total = torch.mean(4 * torch.pi * brdf * light * cosine[:, :, None], dim=1)
    else:
        total = torch.sum(brdf * light * cosine[:, :, None] * _c(weight_d, dtype)[None, :, None], dim=1)
    if aux is not None:
        aux["total"] = total.detach()
    rgb = total.clamp(0.0, 1.0)
    if use_srgb:
        rgb = O.linear2srgb(rgb)
    return torch.where((acc > acc_thres)[:, None], rgb, torch.ones_like(rgb))


def shade_setup(maps, rays, dirs, acc_thres, dtype):
    """-> surf [M, 3] = o + depth * d (the product and the sum rounded separately: two tensor operations), active [M, D] bool."""
    maps, rays, dirs = (_c(x, dtype) for x in (maps, rays, dirs))
    prod = maps[:, 3:4] * rays[:, 3:6]
    surf = rays[:, 0:3] + prod
    cosine = torch.einsum("jk,ik->ij", dirs, maps[:, 4:7]).clamp(min=0.0)
    return surf, (cosine > COS_THRESHOLD) & (maps[:, 14] > acc_thres)[:, None]


def surf_fused(maps, rays):
    """float32 o + depth * d rounded once (what a fused multiply-add gives): the float32 product is exact in float64."""
    maps, rays = torch.as_tensor(maps), torch.as_tensor(rays)
    return (rays[:, 0:3].double() + maps[:, 3:4].double() * rays[:, 3:6].double()).float()


def env_sg(sgs, rot, dirs, dtype):
    """get_light_rgbs for spherical Gaussians: dirs [D, 3] @ rot [L, 3, 3], then the lobes -> [L, D, 3]."""
    sgs, rot, dirs = (_c(x, dtype) for x in (sgs, rot, dirs))
    L = rot.reshape(-1, 3, 3).shape[0]
    remapped = torch.matmul(dirs.reshape(1, -1, 3), rot.reshape(-1, 3, 3)).reshape(-1, 3)
    return O.sg_radiance(sgs, remapped).reshape(L, -1, 3)


def relight_importance(normal, albedo, rough, fresnel, rays_d, light_dir, light_rgb, light_pdf, vis, dtype, aux=None):
    """scripts/relight_importance.py:154-170 given the samples and their visibility: normal, albedo, fresnel, rays_d [M, 3], rough
    [M], light_dir / light_rgb [M, Ns, 3], light_pdf / vis [M, Ns] -> [M, 3]."""
    normal, albedo, rough, fresnel, rays_d, light_dir, light_rgb, light_pdf, vis = \
        (_c(x, dtype) for x in (normal, albedo, rough, fresnel, rays_d, light_dir, light_rgb, light_pdf, vis))
    M, Ns = light_dir.shape[:2]
    surf2c = O.safe_l2_normalize(-rays_d)
    cosine = torch.einsum("ijk,ik->ij", light_dir, normal)
    spec = O.ggx_specular(normal, surf2c, light_dir, rough.reshape(M, 1), fresnel)
    brdf = albedo.unsqueeze(1).expand(-1, Ns, -1) / np.pi + spec
    contrib = brdf * (vis.reshape(M, Ns, 1) * light_rgb) * cosine[:, :, None] / light_pdf.reshape(M, Ns, 1)
    total = torch.mean(contrib, dim=1)
    if aux is not None:
        aux["total"] = total.detach()
    return O.linear2srgb(total.clamp(0.0, 1.0))


def records_sum(off, cnt, rec_w, rec_rgb, dtype=torch.float64):
    """[n] offsets and counts into rec_w [R], rec_rgb [R, 3] -> [n, 3]: each ray's records added one by one in sample order."""
    off, cnt = np.asarray(off).reshape(-1), np.asarray(cnt).reshape(-1)
    w, c = _c(rec_w, dtype), _c(rec_rgb, dtype)
    out = torch.zeros((len(off), 3), dtype=dtype)
    for k in range(int(cnt.max()) if len(cnt) else 0):
        live = torch.from_numpy(cnt > k)
        i = torch.from_numpy(np.where(cnt > k, off + k, 0).astype(np.int64))
        out = torch.where(live[:, None], out + w[i][:, None] * c[i], out)
    return out


def distance(got, ref):
    """max |got - ref| / max |ref| (0 when they are equal), in float64."""
    a = torch.as_tensor(got).detach().cpu().double().numpy()
    b = torch.as_tensor(ref).detach().cpu().double().numpy()
    if a.size == 0:
        return 0.0
    d = np.abs(a - b).max()
    return 0.0 if d == 0 else float(d / np.abs(b).max())


def bound(f32, f64):
    """The device's allowance: ten times the float32 restatement's own distance, and no less than ten half-ulps of 1."""
    return 10 * max(distance(f32, f64), 2.0 ** -24)


# ---- branch predicates --------------------------------------------------------------------------------------------------------------
def _state(x, lo, hi):
    """0 below lo, 1 in [lo, hi] (where clamp passes its gradient), 2 above hi."""
    return (x >= lo).to(torch.int8) + (x > hi).to(torch.int8)


def geometry(normal, rays_d, L, rough, dtype):
    """The raw quantities every branch of GGX_specular and of the cosine turns on, in dtype: normal, rays_d [M, 3], L [D, 3] or
    [M, D, 3] (used raw in the cosine, normalised in the BRDF), rough [M] or [M, 3] -> dict of [M, D(, 3)] / [M] tensors."""
    normal, rays_d, L, rough = (_c(x, dtype) for x in (normal, rays_d, L, rough))
    M = normal.shape[0]
    if L.dim() == 2:
        L = L.reshape(1, -1, 3).expand(M, -1, 3)
    rough = rough.reshape(M, -1)
    cos = torch.einsum("ijk,ik->ij", L, normal)
    Ln = F.normalize(L, dim=-1)
    V = F.normalize(O.safe_l2_normalize(-rays_d), dim=-1)
    H = F.normalize((Ln + V[:, None, :]) / 2.0, dim=-1)
    N = F.normalize(normal, dim=-1)
    nov0 = torch.sum(V * N, dim=-1, keepdim=True)
    N = N * nov0.sign()
    nol, noh, voh = (torch.sum(a * b, dim=-1) for a, b in ((N[:, None, :], Ln), (N[:, None, :], H), (V[:, None, :], H)))
    nov = torch.sum(N * V, dim=-1)
    alpha = rough * rough
    alpha2, k = (alpha * alpha)[:, None, :], ((alpha + 2 * rough + 1.0) / 8.0)[:, None, :]
    cl = lambda x: x.clamp(1e-6, 1)[..., None]
    nom0 = cl(noh) * cl(noh) * (alpha2 - 1) + 1
    nom = 4 * np.pi * nom0 * nom0 * (cl(nov)[:, None] * (1 - k) + k) * (cl(nol) * (1 - k) + k)
    return {"cos": cos, "nol": nol, "noh": noh, "voh": voh, "nov": nov, "nov0": nov0[:, 0], "nom": nom}


def geometry_predicates(q):
    """geometry()'s output -> the value of every branch predicate (integer tensors)."""
    return {"cos_mask": (q["cos"].clamp(min=0.0) > COS_THRESHOLD).to(torch.int8), "cos_positive": (q["cos"] > 0).to(torch.int8),
            "nol": _state(q["nol"], 1e-6, 1), "noh": _state(q["noh"], 1e-6, 1), "voh": _state(q["voh"], 1e-6, 1),
            "nov": _state(q["nov"], 1e-6, 1), "sign": q["nov0"].sign().to(torch.int8), "nom": _state(q["nom"], 1e-6, 4 * np.pi)}


def total_predicates(total):
    """Row totals before the clip -> the clip's state and the sRGB knee's side."""
    return {"clip": _state(total, 0.0, 1.0), "knee": (total.clamp(0.0, 1.0) <= KNEE).to(torch.int8)}


def geometry_margins_ok(q):
    """[M] bool, from the float64 geometry(): every dot product of the row keeps DOT_MARGIN from 1e-6 and from 1 (the cosine:
    from 1e-6, which covers 0), the raw denominator NOM_MARGIN relative from 1e-6."""
    far = lambda x, t: (x - t).abs() >= DOT_MARGIN
    pair = far(q["cos"], COS_THRESHOLD)
    for name in ("nol", "noh", "voh"):
        pair = pair & far(q[name], 1e-6) & far(q[name], 1.0)
    pair = pair & ((q["nom"] / 1e-6 - 1).abs() >= NOM_MARGIN).all(-1)
    return pair.all(1) & far(q["nov"], 1e-6) & far(q["nov"], 1.0) & (q["nov0"].abs() >= DOT_MARGIN)


def total_margins_ok(total):
    """[M] bool: every channel of the row total is exactly 0 or keeps TOTAL_MARGIN relative from the knee and from 1."""
    t = total.double()
    return ((t == 0) | (((t / KNEE - 1).abs() >= TOTAL_MARGIN) & ((t - 1).abs() >= TOTAL_MARGIN) & (t > 0))).all(1)


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and sorted(a) == sorted(b)


# ---- fixtures: surface rows ---------------------------------------------------------------------------------------------------------
DESIGNED = {"acc_at_threshold": 1, "flip": 2, "nov_zero": 3, "normal_half": 4, "normal_double": 5, "normal_zero": 6, "ray_long": 7,
            "ray_zero": 8, "mirror_002": 9, "mirror_03": 10, "mirror_1": 11, "bright": 12, "below_horizon": 13, "srgb_linear": 14,
            "acc_above_threshold": 15, "nom_top": 16}
MIRROR_VIEW = (0.6, 0.0, 0.8)                   # the mirror rows: N = (0, 0, 1), rays_d = -MIRROR_VIEW, dirs[0] = (-0.6, 0, 0.8)
# Which clamp edges a gradient can see at all: NoL, NoV or NoH equal to 1 means L, V or H equal to N, and the gradient that such a
# dot product sends to the normal is along N -- the normalisation's Jacobian removes it, so the pass-through at 1 cannot show.
# The denominator's upper edge can: at roughness 1 with N = V = L (row nom_top with dirs[1] = (0, 0, 1)) the raw value is 4 pi
# exactly in both types and on the device, and what passes reaches the roughness.
VARIANTS = [(ea, ind) for ea in (False, True) for ind in (False, True)]             # (equal_area, indirect given)


def _unit(rng, n):
    x = rng.normal(size=(n, 3))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _draw_rows(rng, n, rough):
    """n random rows: maps [n, 20] (every column filled: the kernels must ignore 0-2 and 15-19) and rays [n, 6]."""
    maps = rng.uniform(-1.0, 1.0, (n, MAP_STRIDE))
    maps[:, 3] = rng.uniform(2.0, 6.0, n)
    maps[:, 4:7] = _unit(rng, n)
    maps[:, 7:10] = rng.uniform(0.05, 1.0, (n, 3))
    maps[:, 10] = rough
    maps[:, 11:14] = rng.uniform(0.02, 0.1, (n, 3))
    maps[:, 14] = rng.uniform(0.6, 1.0, n)
    rays = np.concatenate([rng.uniform(-1.5, 1.5, (n, 3)), _unit(rng, n) * rng.uniform(0.5, 4.0, (n, 1))], 1)
    return maps, rays


def _design(maps, rays, M):
    """Overwrite the designed rows that fit into M rows; -> name -> row."""
    rows = {k: i for k, i in DESIGNED.items() if i < M}
    z = np.float64([0.0, 0.0, 1.0])

    def put(name, normal=None, ray=None, **cols):
        i = rows.get(name)
        if i is None:
            return
        if normal is not None:
            maps[i, 4:7] = normal
        if ray is not None:
            rays[i, 3:6] = ray
        for c, v in cols.items():
            maps[i, int(c[1:])] = v

    put("acc_at_threshold", c14=0.5)                                                  # background: the test is a strict >
    if "flip" in rows:                                                                # N.V < 0, clear of 0
        i = rows["flip"]
        rays[i, 3:6] = 1.7 * (maps[i, 4:7] + 0.4 * np.roll(maps[i, 4:7], 1))
    put("nov_zero", normal=z, ray=(-2.0, 0.0, 0.0))                                   # N.V = 0 exactly: sign 0, N becomes 0
    if "normal_half" in rows:
        maps[rows["normal_half"], 4:7] *= 0.5                                         # raw in the cosine, normalised in the BRDF
    if "normal_double" in rows:
        maps[rows["normal_double"], 4:7] *= 2.0
    put("normal_zero", normal=(0.0, 0.0, 0.0))                                        # F.normalize's 1e-12 path
    if "ray_long" in rows:
        i = rows["ray_long"]
        rays[i, 3:6] *= 3.0 / np.linalg.norm(rays[i, 3:6])
    put("ray_zero", ray=(0.0, 0.0, 0.0))                                              # safe_l2_normalize's 1e-6 path
    for name, r in (("mirror_002", 0.02), ("mirror_03", 0.3), ("mirror_1", 1.0)):       # NoH = 1 with dirs[0]
        put(name, normal=z, ray=tuple(-v for v in MIRROR_VIEW), c10=r)
    tilt = lambda x, y: np.float64([x, y, 1.0]) / math.sqrt(x * x + y * y + 1.0)      # faces dirs[0], whatever else was drawn
    put("bright", normal=tilt(-0.2, 0.3), c7=200.0, c8=200.0, c9=200.0)               # total > 1: the clip stops the gradient
    put("srgb_linear", normal=tilt(0.3, 0.2))                                         # total in (0, 0.0031308]: surface_rows scales its light
    put("below_horizon", normal=-z, ray=(0.3, -0.2, 1.0))                             # every direction has z > 0: total exactly 0
    put("nom_top", normal=z, ray=(0.0, 0.0, -1.0), c10=1.0)                           # raw denominator = 4 pi exactly, with dirs[1]
    put("acc_above_threshold", c14=float(np.nextafter(np.float32(0.5), np.float32(1.0))))
    for i in range(20, M, 7):                                                         # background rows among the random ones
        maps[i, 14] = 0.45 * maps[i, 14]
    return rows


def _tensors(maps, rays, dirs, vis, ind, env, weight_d, light_idx):
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return SimpleNamespace(maps=f(maps), rays=f(rays), dirs=f(dirs), vis=f(vis), indirect=f(ind), env=f(env), weight_d=f(weight_d),
                           light_idx=torch.from_numpy(np.ascontiguousarray(light_idx, np.int32)), acc_thres=ACC_THRES)


def fixture_predicates(fx, dtype, totals=None):
    """Every predicate of a surface_rows fixture in dtype: the geometry's, the acc threshold's, and per variant of VARIANTS the
    clip's and the knee's.  totals (a dict) receives the row totals per variant."""
    p = geometry_predicates(geometry(fx.maps[:, 4:7], fx.rays[:, 3:6], fx.dirs, fx.maps[:, 10], dtype))
    p["fg"] = (fx.maps[:, 14].to(dtype) > fx.acc_thres).to(torch.int8)
    for ea, ind in VARIANTS:
        aux = {}
        with torch.no_grad():
            shade_integrate(fx.maps, fx.rays, fx.dirs, fx.light_idx, fx.vis, fx.indirect if ind else None, fx.env, fx.weight_d, ea, True,
                            fx.acc_thres, dtype, aux)
        for k, v in total_predicates(aux["total"]).items():
            p[f"{k}/{int(ea)}{int(ind)}"] = v
        if totals is not None:
            totals[(ea, ind)] = aux["total"]
    return p


def _rows_that_differ(a, b):
    bad = torch.zeros(a["fg"].shape[0], dtype=torch.bool)
    for k in a:
        d = a[k] != b[k]
        bad |= d.reshape(d.shape[0], -1).any(1)
    return bad


def surface_rows(M, D, rough=0.5, n_lights=3, seed=0):
    """-> namespace(maps [M, 20], rays [M, 6], dirs [D, 3], light_idx [M] int32, vis [M, D], indirect [M, D, 3], env [L, D, 3],
    weight_d [D], acc_thres, rows: name -> index of the designed rows that fit, random [M] bool: the others), float32, seeded.
    Unit directions with z > 0.05 (dirs[0] the mirror rows' direction, dirs[1] = (0, 0, 1) for row nom_top), normals and views in every relative orientation, random
    light_idx with -1 in row 0 and n_lights in the last row, the module's invariant and margins."""
    for attempt in range(20):
        rng = np.random.default_rng([seed, attempt, M, D, n_lights, int(round(rough * 1000))])
        dirs = _unit(rng, D)
        dirs[:, 2] = np.abs(dirs[:, 2])
        dirs[dirs[:, 2] < 0.05] = (0.0, 0.6, 0.8)
        dirs[0] = (-MIRROR_VIEW[0], 0.0, MIRROR_VIEW[2])
        if D > 1:
            dirs[1] = (0.0, 0.0, 1.0)
        weight_d = rng.uniform(0.5, 1.5, D) * 4 * math.pi / D
        env = 0.6 * np.exp(rng.normal(0.0, 0.7, (n_lights, D, 3)))
        light_idx = rng.integers(0, n_lights, M)
        light_idx[0], light_idx[M - 1] = -1, (n_lights if M > 1 else -1)
        maps, rays = _draw_rows(rng, M, rough)
        rows = _design(maps, rays, M)
        random = np.ones(M, bool)
        random[list(rows.values())] = False
        vis_raw = rng.uniform(0.0, 1.0, (M, D)) * (rng.uniform(size=(M, D)) > 0.1)            # exact zeros among the lit pairs
        ind_raw = rng.uniform(0.0, 0.3, (M, D, 3))
        for name in ("bright", "srgb_linear"):
            if name in rows:
                vis_raw[rows[name], 0] = 0.75
        if "nom_top" in rows and D > 1:
            vis_raw[rows["nom_top"], 1] = 0.75
        for _ in range(60):
            fx = _tensors(maps, rays, dirs, vis_raw, ind_raw, env, weight_d, light_idx)
            on = shade_setup(fx.maps, fx.rays, fx.dirs, -1e30, torch.float64)[1].numpy()
            vis, ind = vis_raw * on, ind_raw * on[:, :, None]
            if "srgb_linear" in rows:                          # the light of this row scaled until its largest total is 0.0015
                i = rows["srgb_linear"]
                one = _tensors(maps[i:i + 1], rays[i:i + 1], dirs, vis[i:i + 1], ind[i:i + 1], env, weight_d, light_idx[i:i + 1])
                tot = {}
                fixture_predicates(one, torch.float64, tot)
                s = 0.0015 / max(float(t.max()) for t in tot.values())
                vis[i], ind[i] = vis[i] * s, ind[i] * s
            fx = _tensors(maps, rays, dirs, vis, ind, env, weight_d, light_idx)
            tot = {}
            p64, p32 = fixture_predicates(fx, torch.float64, tot), fixture_predicates(fx, torch.float32)
            q = geometry(fx.maps[:, 4:7], fx.rays[:, 3:6], fx.dirs, fx.maps[:, 10], torch.float64)
            ok = geometry_margins_ok(q)
            for t in tot.values():
                ok &= total_margins_ok(t)
            bad = (_rows_that_differ(p64, p32) | (~ok & torch.from_numpy(random))).numpy()
            if not bad.any():
                fx.rows, fx.random = rows, torch.from_numpy(random)
                return fx
            if (bad & ~random).any():
                break                                           # a designed row against this draw of dirs: draw everything again
            n = int(bad.sum())
            m2, r2 = _draw_rows(rng, n, rough)
            m2[:, 14] = maps[bad, 14]                           # a redrawn row stays background or foreground
            maps[bad], rays[bad] = m2, r2
            vis_raw[bad] = rng.uniform(0.0, 1.0, (n, D)) * (rng.uniform(size=(n, D)) > 0.1)
    raise RuntimeError(f"no admissible fixture for M {M} D {D} roughness {rough}")


def horizon_case():
    """One row, N = (0, 0, 1), V = N, four directions (1, 0, z), un-normalised, z in {0, 2^-20, 2^-19, -2^-19}: n.l = z exactly, and
    2^-20 < 1e-6 < 2^-19, so only the third passes the mask.  Roughness 0 makes alpha2, hence the specular term, exactly 0: what
    is left is ((albedo / pi * (vis * env)) * cosine) * weight added to 0, which no fused multiply-add can change -- without the
    sRGB curve the device must give the float32 restatement's bits."""
    maps = np.zeros((1, MAP_STRIDE))
    maps[0, 3], maps[0, 4:7], maps[0, 7:10], maps[0, 10], maps[0, 11:14], maps[0, 14] = 3.0, (0, 0, 1), (0.7, 0.5, 0.3), 0.0, 0.04, 1.0
    rays = np.float64([[0.1, 0.2, 4.0, 0.0, 0.0, -1.0]])
    dirs = np.float64([(1, 0, z) for z in (0.0, 2.0 ** -20, 2.0 ** -19, -(2.0 ** -19))])
    vis = np.float64([[0.0, 0.0, 0.625, 0.0]])
    env = np.float64([[(3.0 + d, 5.0 + d, 7.0 + d) for d in range(4)]]) * 1e4
    fx = _tensors(maps, rays, dirs, vis, np.zeros((1, 4, 3)), env, np.float64([0.37, 1.37, 2.37, 3.37]), np.int32([0]))
    fx.rows, fx.random = {}, torch.zeros(1, dtype=torch.bool)
    return fx


def clamp_case(top=False):
    """One row and one direction: the mirror geometry at roughness 0.02, so the only pair sits inside the denominator's lower clamp
    (raw value 2.2e-13 against 1e-6).  The denominator passes no gradient: the normal's gradient is the cosine's alone and the
    roughness gradient is d(frac)/d(roughness) / 1e-6 (clamp_gradients()).  top: N = V = L = (0, 0, 1) at roughness 1 instead -- the
    raw denominator equals the upper clamp value 4 pi exactly, where clamp passes its gradient (inclusively)."""
    maps = np.zeros((1, MAP_STRIDE))
    maps[0, 3], maps[0, 4:7], maps[0, 7:10], maps[0, 10], maps[0, 11:14], maps[0, 14] = 3.0, (0, 0, 1), (0.7, 0.5, 0.3), 0.02, (0.04, 0.06, 0.08), 1.0
    rays = np.float64([[0.1, 0.2, 4.0] + [-v for v in MIRROR_VIEW]])
    dirs = np.float64([(-MIRROR_VIEW[0], 0.0, MIRROR_VIEW[2])])
    if top:
        maps[0, 10], rays[0, 3:6], dirs[0] = 1.0, (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)
    fx = _tensors(maps, rays, dirs, np.float64([[0.75]]), np.full((1, 1, 3), 0.125), np.float64([[(0.5, 0.75, 1.0)]]), np.float64([1.25]),
                  np.int32([0]))
    fx.rows, fx.random = {}, torch.zeros(1, dtype=torch.bool)
    return fx


def clamp_gradients(fx, cot, nom=1e-6):
    """float64, by hand, for clamp_case() without the equal-area weight and without sRGB: (roughness gradient, normal gradient)
    with the denominator held at nom."""
    m, l = fx.maps[0].double(), fx.dirs[0].double()
    V = -fx.rays[0, 3:6].double()
    V, Ln = V / V.norm(), l / l.norm()
    H = (Ln + V) / 2
    voh = (V * (H / H.norm())).sum().clamp(1e-6, 1)
    p2 = torch.pow(torch.tensor(2.0, dtype=torch.float64), ((-5.55473) * voh - 6.98316) * voh)
    r, F0 = m[10], m[11:14]
    frac0 = F0 + (1 - F0) * p2
    light = fx.vis[0, 0].double() * fx.env[0, 0].double() + fx.indirect[0, 0].double()
    cos, wd = (l * m[4:7]).sum(), fx.weight_d[0].double()
    brdf = m[7:10] / np.pi + frac0 * r ** 4 / nom
    g = cot.double().reshape(3)
    return (g * light * cos * wd * frac0 * 4 * r ** 3 / nom).sum(), (g * brdf * light * wd).sum() * l


def shade_gradients(fx, indirect, equal_area, use_srgb, cot, dtype):
    """Autograd through shade_integrate: -> (out, d/d maps [M, 20], d/d env [L, D, 3]) of (out * cot).sum()."""
    maps, env = (x.detach().clone().to(dtype).requires_grad_(True) for x in (fx.maps, fx.env))
    out = shade_integrate(maps, fx.rays, fx.dirs, fx.light_idx, fx.vis, fx.indirect if indirect else None, env, fx.weight_d, equal_area,
                          use_srgb, fx.acc_thres, dtype)
    (out * cot.to(dtype)).sum().backward()
    return out.detach(), maps.grad, env.grad


def cotangent(M, seed=13):
    return torch.randn(M, 3, generator=torch.Generator().manual_seed(seed))


# the cases of the GPU tests: (M, D, n_lights, roughness), one sweep per axis around the base case
BASE = (65, 33, 3, 0.5)
FORWARD_SHAPES = [(M, 33, 3, 0.5) for M in (1, 3, 4, 5, 65, 257)] + [(65, D, 3, 0.5) for D in (1, 24, 63, 64, 65, 130)] + \
                 [(65, 33, 1, 0.5), (65, 33, 3, 0.02), (65, 33, 3, 1.0)]
ARM_SHAPES = {"lds-largest": (9, 127, 43, 0.5), "global-atomic": (9, 128, 43, 0.5), "persistent-loop": (2053, 24, 1, 0.5)}
BACKWARD_SHAPES = [BASE, (65, 33, 3, 0.02)] + list(ARM_SHAPES.values())
SETUP_SHAPES = [(1, 1), (33, 31), (32, 32), (41, 25), (3079, 1), (7, 441)]         # M * D: 1, 1023, 1024, 1025, 3 * 1024 + 7 (twice)
_cache = {}


def case(M, D, n_lights=3, rough=0.5):
    """surface_rows, built once per process and left unchanged by the tests."""
    key = (M, D, n_lights, rough)
    if key not in _cache:
        _cache[key] = surface_rows(M, D, rough, n_lights)
    return _cache[key]


# ---- fixtures: records, GGX, spherical Gaussians, importance samples, map lookups ------------------------------------------------------
def records_case(fx, seed=5):
    """Secondary records for a surface_rows fixture: per pair 0, 1, 2, 5 or 96 records (none at a masked pair), offsets in a
    shuffled pair order -> (off [M * D], cnt [M * D] int32, rec_w [R], rec_rgb [R, 3] float32)."""
    rng = np.random.default_rng(seed)
    M, D = fx.vis.shape
    on = shade_setup(fx.maps, fx.rays, fx.dirs, -1e30, torch.float64)[1].numpy().reshape(-1)
    cnt = rng.choice([0, 1, 2, 5, 96], M * D, p=[0.2, 0.3, 0.3, 0.15, 0.05]) * on
    if on.any():
        cnt[np.nonzero(on)[0][0]] = 96
    order = rng.permutation(M * D)
    off = np.zeros(M * D, np.int64)
    off[order] = np.cumsum(cnt[order]) - cnt[order]
    R = int(cnt.sum())
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    i = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32))
    return i(off), i(cnt), f(rng.uniform(0.0, 0.02, R)), f(rng.uniform(0.0, 1.0, (R, 3)))


GGX_SHAPES = [(1, 1), (5, 51), (37, 65)]                     # M * D: 1, 255, above 256


def ggx_case(M, D, seed=0):
    """normal, view [M, 3] (any length), l [M, D, 3], rough, fresnel [M, 3] distinct per channel; rows 1 and 2: N.V = 0 and the
    exact mirror pair.  Random rows are redrawn until geometry_margins_ok holds and float32 and float64 agree on every predicate."""
    for attempt in range(100):
        rng = np.random.default_rng([seed, attempt, M, D])
        n, v = _unit(rng, M) * rng.uniform(0.5, 2.0, (M, 1)), _unit(rng, M) * rng.uniform(0.5, 4.0, (M, 1))
        l = _unit(rng, M * D).reshape(M, D, 3) * rng.uniform(0.5, 2.0, (M, D, 1))
        rough, fres = rng.uniform(0.02, 1.0, (M, 3)), rng.uniform(0.02, 0.9, (M, 3))
        designed = np.zeros(M, bool)
        if M > 2:
            n[1], v[1] = (0, 0, 1), (2, 0, 0)
            n[2], v[2], l[2, 0] = (0, 0, 1), MIRROR_VIEW, (-MIRROR_VIEW[0], 0, MIRROR_VIEW[2])
            designed[1:3] = True
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
        t = SimpleNamespace(normal=f(n), view=f(v), l=f(l), rough=f(rough), fresnel=f(fres))
        q = geometry(t.normal, -t.view, t.l, t.rough, torch.float64)
        p32 = geometry_predicates(geometry(t.normal, -t.view, t.l, t.rough, torch.float32))
        if same(geometry_predicates(q), p32) and geometry_margins_ok(q)[torch.from_numpy(~designed)].all():
            return t
    raise RuntimeError("no admissible GGX fixture")


SG_LOBES = (1, 63, 128, 129, 200)
SG_PAIRS = [(1, 1), (3, 85), (2, 128), (1, 257), (3, 300)]               # L * D: 1, 255, 256, 257, 900
SG_CASES = [(n, 3, 85) for n in SG_LOBES] + [(128, L, D) for L, D in SG_PAIRS if (L, D) != (3, 85)]


def sg_case(n_sg, L, D, seed=0):
    """sgs [n_sg, 7] (axis, lambda, mu), rot [L, 3, 3] rotations about z, dirs [D, 3] unit.  Designed lobes, where n_sg is long
    enough: 0 negative lambda and a negative mu, 1 a zero mu, 2 lambda = 0, 3 an axis of length 0.1, 4 of length 10, 5 lambda =
    200 (the exponential underflows to 0 away from the axis)."""
    rng = np.random.default_rng([seed, n_sg, L, D])
    sgs = np.concatenate([_unit(rng, n_sg) * rng.uniform(0.5, 2.0, (n_sg, 1)), rng.uniform(1.0, 30.0, (n_sg, 1)),
                          rng.uniform(0.05, 1.0, (n_sg, 3)) * 8.0 / n_sg], 1)
    sgs[0, 3], sgs[0, 5] = -sgs[0, 3], -sgs[0, 5]
    if n_sg > 5:
        sgs[1, 4] = 0.0
        sgs[2, 3] = 0.0
        sgs[3, 0:3] *= 0.1 / np.linalg.norm(sgs[3, 0:3])
        sgs[4, 0:3] *= 10.0 / np.linalg.norm(sgs[4, 0:3])
        sgs[5, 3] = 200.0
    a = rng.uniform(0.0, 2 * math.pi, L)
    rot = np.zeros((L, 3, 3))
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1.0
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return SimpleNamespace(sgs=f(sgs), rot=f(rot), dirs=f(_unit(rng, D)), cot=f(rng.normal(size=(L, D, 3))))


def sg_gradients(c, dtype):
    sgs = c.sgs.detach().clone().to(dtype).requires_grad_(True)
    out = env_sg(sgs, c.rot, c.dirs, dtype)
    (out * c.cot.to(dtype)).sum().backward()
    return out.detach(), sgs.grad


IMPORTANCE_CASES = [(M, 64) for M in (1, 4, 5)] + [(5, Ns) for Ns in (1, 63, 65, 100)]


def importance_case(M, Ns, cells=40, seed=0):
    """Cell tables env_dir [C, 3] (unit, the whole sphere), env_rgb [C, 3], env_pdf [C], samples cell [M, Ns] int32, surface rows and
    vis [M, Ns]: 0 wherever the cosine is <= 1e-6 (about half of the samples: the cosine is not clamped, scripts/relight_importance
    .py:125) and at a few lit samples.  Redrawn until the margins hold and float32 and float64 agree on every predicate."""
    for attempt in range(200):
        rng = np.random.default_rng([seed, attempt, M, Ns])
        env_dir, env_rgb, env_pdf = _unit(rng, cells), np.exp(rng.normal(0.0, 1.0, (cells, 3))), rng.uniform(0.05, 2.0, cells)
        cell = rng.integers(0, cells, (M, Ns))
        n, d = _unit(rng, M), _unit(rng, M) * rng.uniform(0.5, 4.0, (M, 1))
        if M > 1:
            n[1], d[1] = -n[1], 1.5 * (n[1] + 0.3 * np.roll(n[1], 1))               # one flipped row
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
        t = SimpleNamespace(normal=f(n), albedo=f(rng.uniform(0.05, 1.0, (M, 3))), rough=f(rng.uniform(0.05, 1.0, M)),
                            fresnel=f(rng.uniform(0.02, 0.1, (M, 3))), rays_d=f(d), env_dir=f(env_dir), env_rgb=f(env_rgb), env_pdf=f(env_pdf),
                            cell=torch.from_numpy(cell.astype(np.int32)))
        ci = t.cell.long()
        t.light_dir, t.light_rgb, t.light_pdf = t.env_dir[ci], t.env_rgb[ci], t.env_pdf[ci]
        q = geometry(t.normal, t.rays_d, t.light_dir, t.rough, torch.float64)
        t.vis = f(rng.uniform(0.0, 1.0, (M, Ns)) * (rng.uniform(size=(M, Ns)) > 0.1)) * (q["cos"] > COS_THRESHOLD).float()
        if same(importance_predicates(t, torch.float64), importance_predicates(t, torch.float32)) and geometry_margins_ok(q).all() and \
                total_margins_ok(importance_predicates(t, torch.float64, True)).all():
            return t
    raise RuntimeError("no admissible importance fixture")


def importance_predicates(t, dtype, total=False):
    aux = {}
    with torch.no_grad():
        relight_importance(t.normal, t.albedo, t.rough, t.fresnel, t.rays_d, t.light_dir, t.light_rgb, t.light_pdf, t.vis, dtype, aux)
    if total:
        return aux["total"]
    p = geometry_predicates(geometry(t.normal, t.rays_d, t.light_dir, t.rough, dtype))
    p.update(total_predicates(aux["total"]))
    return p


def lookup_case(seed=0):
    """A 6 x 12 map and directions: 0-1 the poles, 2-3 the +-pi seam (dy = +-0), 4-5 dz = +-(1 + 2^-23) (outside acos's domain by
    one ulp), 6-7 the poles again, 8.. random unit directions.  -> (hdr [6, 12, 3], dirs [n, 3]) float32."""
    rng = np.random.default_rng(seed)
    hdr = np.exp(rng.normal(0.0, 1.0, (6, 12, 3))).astype(np.float32)
    over = 1.0 + 2.0 ** -23
    dirs = np.concatenate([np.float64([(0, 0, 1), (0, 0, -1), (-1, 0.0, 0), (-1, -0.0, 0), (0, 0, over), (0, 0, -over), (0, 0, 1), (0, 0, -1)]),
                           _unit(rng, 56)]).astype(np.float32)
    return torch.from_numpy(hdr), torch.from_numpy(dirs)
