"""The per-point bake (tensoir_amd/bake.py) restated with the oracle's functions only -- the yardstick of
tests/test_gpu_bake.py.  It shares no code with the product: dense [N, S] marches, boolean-mask indexing and torch reductions,
in the precision of `dtype` (fp64 for the reference values, fp32 to qualify a point set: tests/test_bake_cpu.py).

Per point p with unit outward direction n, s = the scene's march step:
  1. o = p + n_outside * s * n, d = -n; sample_ray_equally(near = 0, far = (S - 1) * s) + cull + density + raw2alpha
     (compute_radiance up to the line that decodes radiance)
  2. at the samples with w > weight_thres: intrin_feature -> render_brdf -> albedo, roughness = 0.9 raw + 0.09; the normal that
     forward_primary composites for the scene's normals_kind
  3. over those samples only (the march's records): coverage = sum w; albedo, roughness = clamp(sum w x / max(coverage, 1e-6),
     0, 1); normal = safe_l2_normalize(sum w normal), n where coverage <= 0.5 or the sum is shorter than 1e-6;
     surface = o + d * sum w z / max(coverage, 1e-6)
  4. over the scene's fixed light directions with cos = dot(dir, normal) > 1e-6, for coverage > 0.5:
     vis = compute_transmittance(surface, dir)[0]; ao = sum vis cos w / sum cos w (1 for an empty sum);
     irradiance = sum vis env[light] cos w.  Elsewhere ao = 1, irradiance = 0."""
import torch

from oracle import tensoir_oracle as O


def shading_normals(sc, xyz, intr):
    kind = getattr(sc, "normals_kind", "derived_plus_predicted")
    if kind in ("purely_predicted", "derived_plus_predicted"):
        return O.render_normal(sc, xyz, intr)
    if kind == "purely_derived":
        return O.density_grad(sc, xyz)[2]
    if kind == "residue_prediction":
        return O.render_normal_residue(sc, xyz, O.density_grad(sc, xyz)[2], intr)
    raise ValueError(f"normals_kind {kind!r}")


@torch.no_grad()
def bake(scene, points, outward, light_idx=0, n_sample=96, n_outside=16, lighting=True, vis_n_sample=96, vis_near=0.05,
         vis_far=1.5, dtype=torch.float64, pair_chunk=4096):
    """-> dict of `dtype` tensors: albedo [N, 3], roughness [N], normal [N, 3], coverage [N], surface [N, 3], records [N] (the
    number of decoded samples per point), margin_w / margin_coverage (the smallest |w / weight_thres - 1| over all samples and
    the smallest |coverage - 0.5| over all points: how close the set comes to the two discontinuities of steps 2 and 3), and with lighting ao [N], irradiance [N, 3], pairs (the number of marched pairs)."""
    sc = scene.to(dtype)
    p, n = points.to(dtype), outward.to(dtype)
    N = p.shape[0]
    step = O.step_geometry(sc.aabb, sc.grid, sc.step_ratio).step
    o, d = p + n_outside * step * n, -n
    pts, z, valid = O.sample_ray_equally(sc, o, d, n_sample, 0.0, float(step) * (n_sample - 1))
    z = z.expand(N, n_sample)
    dists = torch.cat((z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])), dim=-1)
    sigma, valid, xyz = O.march_sigma(sc, pts, valid)
    _, weight, _ = O.raw2alpha(sigma, dists * sc.distance_scale)
    mask = weight > sc.weight_thres
    margin_w = float((weight / sc.weight_thres - 1).abs().min())       # how close a sample comes to the record threshold (relative)
    weight = torch.where(mask, weight, torch.zeros_like(weight))       # only the decoded samples (the march's records) are composited
    albedo = torch.zeros(N, n_sample, 3, dtype=dtype)
    rough = torch.zeros(N, n_sample, dtype=dtype)
    normal = torch.zeros(N, n_sample, 3, dtype=dtype)
    if mask.any():
        xa = xyz[mask]
        intr = O.intrin_feature(sc, xa)
        brdf = O.render_brdf(sc, xa, intr)
        albedo[mask] = brdf[:, :3]
        rough[mask] = brdf[:, 3] * 0.9 + 0.09
        normal[mask] = shading_normals(sc, xa, intr)
    acc = weight.sum(-1)
    den = acc.clamp(min=1e-6)
    nv = (weight[..., None] * normal).sum(-2)
    use_n = (acc <= 0.5) | (torch.linalg.norm(nv, dim=-1) <= 1e-6)
    out = {"albedo": ((weight[..., None] * albedo).sum(-2) / den[:, None]).clamp(0, 1),
           "roughness": ((weight * rough).sum(-1) / den).clamp(0, 1),
           "normal": torch.where(use_n[:, None], n, O.safe_l2_normalize(nv)),
           "coverage": acc,
           "surface": o + d * ((weight * z).sum(-1) / den)[:, None],
           "records": mask.sum(-1), "margin_w": margin_w, "margin_coverage": float((acc - 0.5).abs().min())}
    if not lighting:
        return out
    area, dirs = O.envmap_dirs(sc.envmap_h, sc.envmap_w)
    area, dirs = area.to(dtype), dirs.to(dtype)
    li = (light_idx if torch.is_tensor(light_idx) else torch.full((N,), int(light_idx))).reshape(-1).long()
    env = O.light_rgbs(sc, dirs)[li]                                        # [N, D, 3]
    cos = torch.einsum("dk,nk->nd", dirs, out["normal"])
    active = (cos > 1e-6) & (acc > 0.5)[:, None]
    vis = torch.zeros_like(cos)
    pi, di = torch.nonzero(active, as_tuple=True)
    for a in range(0, pi.numel(), pair_chunk):
        sl = slice(a, a + pair_chunk)
        vis[pi[sl], di[sl]] = O.compute_transmittance(sc, out["surface"][pi[sl]], dirs[di[sl]], vis_n_sample, vis_near, vis_far)[0]
    cw = torch.where(active, cos * area[None], torch.zeros_like(cos))
    dsum = cw.sum(-1)
    out["ao"] = torch.where(dsum > 0, (vis * cw).sum(-1) / dsum.clamp(min=1e-30), torch.ones_like(dsum))
    out["irradiance"] = ((vis * cw)[..., None] * env).sum(-2)
    out["pairs"] = int(active.sum())
    return out
