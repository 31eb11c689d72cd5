"""Shared test helpers: golden fixture -> checkpoint / oracle Scene, error metrics."""
import io

import numpy as np
import torch

from oracle import tensoir_oracle as O


def golden_checkpoint(g):
    """Rebuild the reference-format checkpoint stored in tests/golden/small_scene.npz."""
    sd = {k[3:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith("sd/")}
    rot = [int(r) for r in g["scene/light_rotation"]]
    kwargs = {
        "aabb": torch.from_numpy(np.array(g["scene/aabb"])), "gridSize": [int(x) for x in g["scene/grid"]],
        "density_n_comp": [16, 16, 16], "appearance_n_comp": [48, 48, 48], "app_dim": 27,
        "density_shift": -10, "alphaMask_thres": 0.001, "distance_scale": 25,
        "rayMarch_weight_thres": 0.0001, "fea2denseAct": "softplus", "near_far": [2.0, 6.0],
        "step_ratio": 0.5, "shadingMode": "MLP_Fea", "pos_pe": 2, "view_pe": 2, "fea_pe": 2,
        "featureC": 128, "normals_kind": "derived_plus_predicted", "light_num": len(rot),
        "light_kind": "sg", "numLgtSGs": 128, "light_rotation": rot,
    }
    vol = torch.from_numpy(np.array(g["scene/alpha_volume"]))
    ckpt = {"kwargs": kwargs, "state_dict": sd,
            "alphaMask.shape": tuple(vol.shape),
            "alphaMask.mask": np.packbits(vol.bool().numpy().reshape(-1)),
            "alphaMask.aabb": torch.from_numpy(np.array(g["scene/alpha_aabb"]))}
    return ckpt


def scene_from_checkpoint(ckpt, envmap_h, envmap_w):
    vol = aabb = None
    if "alphaMask.aabb" in ckpt:
        n = int(np.prod(ckpt["alphaMask.shape"]))
        vol = torch.from_numpy(np.unpackbits(ckpt["alphaMask.mask"])[:n].reshape(ckpt["alphaMask.shape"])).float()
        aabb = ckpt["alphaMask.aabb"]
    return O.scene_from_state_dict(ckpt["state_dict"], ckpt["kwargs"], vol, aabb, envmap_h, envmap_w)


def golden_scene(g):
    h, w = [int(x) for x in g["scene/envmap_hw"]]
    return scene_from_checkpoint(golden_checkpoint(g), h, w)


def T(g, key):
    return torch.from_numpy(np.array(g[key]))


def max_err(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) if a.numel() else 0.0


def rel_err(a, b, floor=1.0):
    """max |a-b| / max(|b|, floor): the parity metric (north_star: 1e-4 relative)."""
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    if a.numel() == 0:
        return 0.0
    return float(((a - b).abs() / b.abs().clamp(min=floor)).max())


def scene_from_model(ckpt, model, envmap_h, envmap_w):
    """Oracle Scene of a synthetic checkpoint whose occupancy mask was built on the device
    (model.updateAlphaMask): same parameters, same 0/1 volume, same mask aabb."""
    ck = dict(ckpt)
    if model.alphaMask is not None:
        vol = model.alphaMask.alpha_volume[0, 0].bool().cpu()
        ck["alphaMask.shape"] = tuple(vol.shape)
        ck["alphaMask.mask"] = np.packbits(vol.numpy().reshape(-1))
        ck["alphaMask.aabb"] = model.alphaMask.aabb.cpu()
    return scene_from_checkpoint(ck, envmap_h, envmap_w)


def parity_metrics(a, b, min_norm=1e-2):
    """The three error figures reported for a rendered map (hip a vs reference b):
    max_abs, max |d| / max(|ref|, 1) (the test metric; maps live in [0,1] / unit normals / depth ~4) and the
    true per-pixel relative error ||d|| / ||ref|| over pixels with ||ref|| > min_norm (vector maps: L2 over channels)."""
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    if a.numel() == 0:
        return {"max_abs": 0.0, "max_rel_floor1": 0.0, "max_rel_pixel": 0.0}
    d = (a - b).abs()
    a2, b2, d2 = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1), (a - b).reshape(a.shape[0], -1)
    nb = b2.norm(dim=-1)
    sel = nb > min_norm
    relpix = float((d2.norm(dim=-1)[sel] / nb[sel]).max()) if bool(sel.any()) else 0.0
    return {"max_abs": float(d.max()), "max_rel_floor1": float((d / b.abs().clamp(min=1.0)).max()),
            "max_rel_pixel": relpix}


def ggx_flip_rays(ref_normal_map, rays, eps=1e-5):
    """Rays on which the reference's physically-based colour is DISCONTINUOUS in its inputs: GGX_specular flips the normal by
    sign(N.V) (models/relight_utils.py:30-31: ``N = N * NoV.sign()``), so a ray whose composited normal is perpendicular to the
    view direction within fp32 noise (|N.V| < eps; the maps themselves agree to ~1e-5) takes either branch -- the specular
    term, hence rgb_with_brdf_map, jumps by percents (measured: one ray of the 4096-ray bench batch, oracle N.V = +1.0e-6, split-bf16
    decoders -8e-8, exact fp32 decoders +1.0e-6: profiles/r05_outlier_diag.json).  Such rays are reported, not compared."""
    n = torch.as_tensor(ref_normal_map).detach().double().cpu()
    d = torch.as_tensor(rays).detach().double().cpu()[:, 3:6]
    n = n / n.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    v = -d / d.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    return (n * v).sum(-1).abs() < eps


def depth_discontinuity_rays(O, sc, ref, rays, light_idx, candidates, n_sample, tol=1e-5, limit=16):
    """Rays on which the reference's physically-based colour is DISCONTINUOUS in the ray's own depth: the secondary rays start at
    rays_o + depth * rays_d (models/relight_utils.py:433), and a secondary sample that sits on an occupancy-cell or bounding-box
    boundary within the last bits is culled or not (:683-695, :803-815) -- the visibility of that light direction, hence
    rgb_with_brdf_map, jumps.  The criterion involves the ORACLE only: its own render_with_brdf on its own maps, with its own depth
    moved by -2 ... +2 ulps, varies by more than `tol` (measured on the headline batch: two rays of 4096 jump by 2.1e-4 and 1.3e-4 for
    ONE ulp of depth, their neighbours by 1e-7 per ulp; profiles/r06_depth_discontinuity_rays.txt).  Only `candidates` (ray indices into
    the oracle's rows, at most `limit`) are examined.  -> {ray: the oracle's own spread}."""
    import numpy as np
    out = {}
    rays = torch.as_tensor(rays).detach().cpu().float()
    light_idx = torch.as_tensor(light_idx).detach().cpu()
    for i in [int(c) for c in candidates][:limit]:
        g = lambda k: ref[k][i:i + 1]
        d0 = g("depth_map").reshape(1).float().numpy()
        vals = []
        for u in (-2, -1, 0, 1, 2):
            d = d0.copy()
            for _ in range(abs(u)):
                d = np.nextafter(d, np.float32(np.inf if u > 0 else -np.inf))
            with torch.no_grad():
                o = O.render_with_brdf(sc, torch.from_numpy(d), g("normal_map"), g("albedo_map"), g("roughness_map").reshape(1, -1).expand(1, 3),
                                       g("fresnel_map"), rays[i:i + 1], light_idx[i:i + 1], n_sample=n_sample)
            vals.append(o.reshape(-1))
        v = torch.stack(vals)
        spread = float((v.max(0).values - v.min(0).values).max())
        if spread > tol:
            out[i] = spread
    return out


# ---- recorded host-side results of the reference (tests/golden/host_reference.npz, oracle/make_golden_host.py) -------------
def digest(t):
    """sha256 over a tensor's shape and values (floats widened to float64, integers to int64): equal digests <=> torch.equal."""
    import hashlib
    x = t.detach().cpu().contiguous()
    x = x.to(torch.float64) if x.is_floating_point() else x.to(torch.int64)
    return hashlib.sha256(repr(tuple(x.shape)).encode() + x.numpy().tobytes()).hexdigest()


def tv_loss(x):
    """Total variation of a [N, C, H, W] plane as TensoRF-style models regularise it (weight 1): twice the mean squared forward
    difference along H plus that along W (means over C x (H-1) x W and C x H x (W-1)), divided by N."""
    n, c, h, w = x.shape
    dh = (x[:, :, 1:, :] - x[:, :, :h - 1, :]).pow(2).sum()
    dw = (x[:, :, :, 1:] - x[:, :, :, :w - 1]).pow(2).sum()
    return 2 * (dh / (c * (h - 1) * w) + dw / (c * h * (w - 1))) / n


def field_trace(m):
    """What the upsample / shrink comparison pins of a model: every plane and line, the box and the step geometry."""
    out = {}
    for name in ("density_plane", "density_line", "app_plane", "app_line"):
        for i, t in enumerate(getattr(m, name)):
            out[f"{name}.{i}"] = digest(t)
    for name in ("aabb", "gridSize", "units", "invaabbSize"):
        out[name] = digest(getattr(m, name))
    out["stepSize"] = repr(float(m.stepSize))
    out["nSamples"] = repr(int(m.nSamples))
    return out


def upsample_shrink_trace(m):
    """field_trace after loading, after upsample_volume_grid(gridSize + 5) and after shrink to a box inside the aabb; plus
    whether the shrink took the branch for a mask grid that differs from the field's."""
    import contextlib
    trace = {"load": field_trace(m)}
    target = [int(g) + 5 for g in m.gridSize]
    with contextlib.redirect_stdout(io.StringIO()):
        m.upsample_volume_grid(target)
    trace["upsample"] = field_trace(m)
    lo, hi = m.aabb[0], m.aabb[1]
    new_aabb = torch.stack([lo + 0.21 * (hi - lo), hi - 0.17 * (hi - lo)])
    trace["mask_grid_differs"] = repr(bool(not torch.all(m.alphaMask.gridSize == m.gridSize)))
    with contextlib.redirect_stdout(io.StringIO()):
        m.shrink(new_aabb.clone())
    trace["shrink"] = field_trace(m)
    return trace


def regulariser_trace(m, tv):
    """density_L1, vector_comp_diffs, TV_loss_density / _app (with the TV callable `tv`), the learning rates and parameter counts
    of the optimizer groups."""
    vals = {name: float(getattr(m, name)(*args).detach()) for name, args in
            (("density_L1", ()), ("vector_comp_diffs", ()), ("TV_loss_density", (tv,)), ("TV_loss_app", (tv,)))}
    lrs = [g["lr"] for g in m.get_optparam_groups(0.02, 0.001)]
    counts = [sum(p.numel() for p in (g["params"] if not isinstance(g["params"], torch.Tensor) else [g["params"]]))
              for g in m.get_optparam_groups()]
    return {"values": vals, "lrs": lrs, "counts": counts}


SEEDED_CASES = [("sg", "derived_plus_predicted"), ("pixel", "derived_plus_predicted"), ("sg", "residue_prediction")]


def seeded_construction_trace(ctor, light_kind, normals_kind):
    """A model built under torch seed 77 (`ctor(aabb, grid, device, **kw)`) and its stratified light directions under seeds
    5 and 6: digests of every state_dict entry, the light tables and the drawn directions."""
    import contextlib
    aabb = torch.tensor([[-1.5, -1.4, -1.3], [1.5, 1.4, 1.3]])
    kw = dict(density_n_comp=[16, 16, 16], appearance_n_comp=[48, 48, 48], app_dim=27, shadingMode="MLP_Fea", step_ratio=0.5,
              normals_kind=normals_kind, light_rotation=["000", "120"], envmap_w=8, envmap_h=4,
              light_kind=light_kind, numLgtSGs=128)
    torch.manual_seed(77)
    with contextlib.redirect_stdout(io.StringIO()):
        m = ctor(aabb.clone(), [12, 14, 16], "cpu", **kw)
    out = {"sd/" + k: digest(v) for k, v in m.state_dict().items()}
    for name in ("light_area_weight", "fixed_viewdirs", "light_rotation_matrix"):
        out[name] = digest(getattr(m, name))
    torch.manual_seed(5)
    out["dirs/stratified_sampling"] = digest(m.gen_light_incident_dirs(method="stratified_sampling"))
    torch.manual_seed(6)
    out["dirs/stratifed_sample_equal_areas"] = digest(m.gen_light_incident_dirs(method="stratifed_sample_equal_areas"))
    return out
