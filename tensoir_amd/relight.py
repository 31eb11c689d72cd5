"""Host-side mirror of ``models/relight_utils.py`` (live functions only): same names, argument
meaning and return shapes; per-sample work runs in libtensoir_hip.so."""
from __future__ import annotations

import functools
import os

import numpy as np
import torch

from . import capacity, indirect, ops
from .field_model import safe_l2_normalize  # noqa: F401  (re-exported, as the reference module does)

MAP_STRIDE = ops.MAP_STRIDE


_CONST_CACHE = {}


def _z_table(n_sample, near, far, device):
    """sample_ray_equally's distances (models/relight_utils.py:716-717), computed by the same torch ops
    on the same device as the reference would; cached per (n, near, far, device)."""
    key = ("z", int(n_sample), float(near), float(far), str(device))
    z = _CONST_CACHE.get(key)
    if z is None:
        t = torch.linspace(0.0, 1.0, n_sample, device=device)
        z = (near * (1.0 - t) + far * t).contiguous()
        _CONST_CACHE[key] = z
    return z


def _on_device(tensoIR, name, src, device):
    """Device-resident copy of a small host-side table of the model (direction grid, solid angles ...)."""
    cache = tensoIR.__dict__.setdefault("_dev_tables", {})
    key = (name, str(device), src.data_ptr(), src._version)
    t = cache.get(name)
    if t is None or t[0] != key:
        t = (key, src.to(device, torch.float32).contiguous())
        cache[name] = t
    return t[1]


def _rec_capacity(n_rays):
    return int(min(max(1 << 20, 16 * n_rays), 1 << 28))


def _gather_then_decode(tensoIR, f, fh, rec_xyz, light_idx, rec_ray, light_div, dirs, dir_map, n_dirs, n_dev, full=False):
    """Appearance gather, then the radiance decoder, as two launches (features through HBM).  full: the primary-stage kernels
    (fp32 taps, split-bf16 x3 decoder) whatever the precision policy says."""
    if fh is not None and not full:   # indirect-light precision policy: fp16 shadow taps, fp16 matrix operands
        feat = ops.vm_app_h16(f, fh, rec_xyz, light_idx, rec_ray, light_div, n_dev)
    else:
        feat = ops.vm_app(f, rec_xyz, light_idx, rec_ray, True, False, None, light_div, n_dev)[0]
    # view direction of a record = that of its ray (ray id -> direction via aux_mod on the dense [point][direction] grid)
    return ops.mlp(tensoIR.renderModule.packed(), feat, dirs, rec_ray if dir_map is None else
                   dir_map[rec_ray.long().clamp_(0, dir_map.numel() - 1)].contiguous(), None if full else ops.secondary_mlp_impl(),
                   n_dirs if dir_map is None else 0, n_dev)


def _fusable(f, dirs, dir_map, n_dirs, n_rows):
    """Whether the one-launch kernels (ops.indirect_fused, ops.indirect_fused_hp) take this pass's records."""
    return dir_map is None and n_dirs > 0 and dirs.shape[0] * 8 <= max(n_rows, 1) and int(f.app_dim) == 27 and int(f.n_acomp) == 48


def _decode_records(tensoIR, f, fh, kind, rec_xyz, rec_ray, n_dev, light_idx, light_div, dirs, dir_map, n_dirs):
    """Radiance rows of secondary-ray records from the kernels of one tier.  kind: "f16" (fp16 shadow `fh` + fp16 decoder), "hp"
    (fp32 taps, fp16 + fp8-residue weights) or "full" (the primary-stage kernels).  light index / view direction of a record =
    those of its ray (ray id -> point via light_div, ray id -> direction via n_dirs on the dense [point][direction] grid)."""
    if _fusable(f, dirs, dir_map, n_dirs, rec_xyz.shape[0]):
        if kind == "f16" and fh is not None and ops.fused_indirect() and int(f.n_lights) <= 16:
            # gather -> basis contraction -> radiance decoder in ONE launch, the feature rows never reach HBM
            return ops.indirect_fused(f, fh, tensoIR.renderModule.packed(), rec_xyz, light_idx, rec_ray, light_div, dirs, n_dirs, n_dev)
        if kind == "hp" and ops.AUX_TABLE and ops.MLP_IMPL == "bf16x3" and int(f.n_lights) <= 8:
            return ops.indirect_fused_hp(f, tensoIR.renderModule.packed(), rec_xyz, light_idx, rec_ray, light_div, dirs, n_dirs, n_dev)
    return _gather_then_decode(tensoIR, f, fh, rec_xyz, light_idx, rec_ray, light_div, dirs, dir_map, n_dirs, n_dev, full=kind != "f16")


def _range_failed(tensoIR, rng):
    """The range guard (tir_pack_half_checked's contract) on the maxima of THIS version's fp16 shadow; waits for them if they have
    not arrived.  True: an fp16 product could overflow -> the verdict is `full`, the caller decodes with the primary-stage kernels."""
    if rng is None or rng.ok():
        return False
    indirect.set_verdict(tensoIR, "full", "range", {"bound": rng.bound, "maxima": rng.maxima})
    return True


def _map_measure(probe_map, vis, packed, full_rows, count, n_rays, map_limit):
    """indirect.establish's `measure` where the caller renders rgb_with_brdf_map from BOTH decodes of ALL records of this pass
    (probe_map): the quantity the tolerance is stated on, measured -- not estimated."""
    def measure(cand):
        n_valid, ref = count(), full_rows()
        d = (cand[:n_valid] - ref[:n_valid]).double()
        delta = probe_map(vis, packed(cand), packed(ref))
        v = (torch.stack([d.mean(0).abs().max(), d.pow(2).mean().sqrt(), d.abs().max()]).tolist() if n_valid else [0.0, 0.0, 0.0])
        return delta <= map_limit, {"kind": "map", "map_max_abs": delta, "records": n_valid, "rays": n_rays, "bias": v[0], "rms": v[1],
                                    "max": v[2], "limit": map_limit}                   # (NaN fails)
    return measure


def _decode_pass(tensoIR, f, vis, rec, n_rows, n_dev, count, lookup, n_rays, force_full, keep_records, training, probe_map):
    """The record-decoding middle of one march attempt of _secondary: pick the tier (`full` when force_full, else the precision
    policy's), run the range guard where its maxima are at hand, decode the first n_rows records -- through indirect.establish
    when the policy has no verdict yet; count() = the valid rows, asked for after the f16 decode has been queued -- and pack or
    accumulate them per ray -> (indirect_rgb, rng); rng = a range check still pending (judged at the end-of-pass check)."""
    capturing = tensoIR.__dict__.get("_capture") is not None
    mode = "full" if force_full else indirect.mode(tensoIR, training)
    if mode == "probe" and capturing:
        raise ops._lib.TensoirHipError("graph capture needs an established indirect-light precision verdict (run the pass eagerly first)")
    if n_rows <= 0:
        return torch.zeros((n_rays, 3), dtype=torch.float32, device=vis.device), None
    rec_ray, rec_w, rec_xyz = rec["ray"][:n_rows], rec["w"][:n_rows], rec["xyz"][:n_rows]
    fh = tensoIR.packed_field_half(_fresh=True) if (mode != "full" and ops.secondary_app_impl() == "h16") else None
    rng = tensoIR.half_range(_fresh=True) if (fh is not None and ops.INDIRECT_GUARD) else None
    if rng is not None and (mode == "probe" or rng.ready()):   # a pass that waits anyway, or maxima that have arrived: now
        if _range_failed(tensoIR, rng):
            mode, fh = "full", None
        rng = None
    if capturing and rng is not None and not rng.ready():
        raise ops._lib.TensoirHipError("graph capture needs a finished range check of the fp16 field shadow (run the pass eagerly first)")

    def decode(kind):
        return _decode_records(tensoIR, f, fh, kind, rec_xyz, rec_ray, n_dev, *lookup)

    def packed(rgb):
        if keep_records:       # the caller's integration kernel sums the records itself (tir_shade_integrate_records)
            return {"off": rec["off"], "cnt": rec["cnt"], "w": rec_w, "rgb": rgb}
        return ops.accumulate_records(rec["off"], rec["cnt"], rec_w, rgb, n_rays)

    if mode != "probe":        # (probe: auto policy, no verdict for these parameters yet -> self-check on this pass's own records)
        return packed(decode(mode)), rng
    if probe_map is not None:
        decode = functools.lru_cache(maxsize=None)(decode)       # the full rows: measured against, and the last tier
        # a TRAINING pass renders the map as a no_grad constant of the loss (models/relight_utils.py:344): there the
        # policy accepts up to the contract's own tolerance; inference / export use the strict limit
        measure = _map_measure(probe_map, vis, packed, lambda: decode("full"), lambda: min(count(), n_rows), n_rays,
                               ops.INDIRECT_PROBE["train_map_limit" if training else "map_limit"])
        try_hp = ops.INDIRECT_HP
    else:
        def measure(rows):
            return indirect.record_estimate(rows, min(count(), n_rows), lambda sel: _decode_records(
                tensoIR, f, None, "full", rec_xyz[sel].contiguous(), rec_ray[sel].contiguous(), None, *lookup))
        try_hp = ops.INDIRECT_HP and _fusable(f, *lookup[2:], n_rows) and ops.AUX_TABLE and ops.MLP_IMPL == "bf16x3"
    return packed(indirect.establish(tensoIR, decode, measure, try_hp, train_limit=training and probe_map is not None)[1]), rng


def _secondary(tensoIR, origins, dirs, n_rays, z, org_map, dir_map, active, light_idx, light_div,
               want_indirect, want_nerfactor=False, n_dirs=0, keep_records=False, ids=None, defer=False, training=False,
               probe_map=None):
    """Shared driver of compute_transmittance / compute_radiance / render_with_BRDF: march (+ record the w > thres samples) ->
    _decode_pass, repeated until the records fit and the range guard holds, under the record-capacity protocol of capacity.py.
    An inference pass marches through the dense density volume (packed_field_dense) and, where it decodes records, reads their
    f16-tier appearance features from the dense appearance volume; a training pass keeps the VM kernels."""
    f = tensoIR.packed_field() if training else tensoIR.packed_field_dense(app=bool(want_indirect))
    if not want_indirect:
        vis, oma, _ = ops.march_secondary(f, origins, dirs, z, n_rays, org_map, dir_map, active,
                                          tensoIR.march_t_stop, False, 0, want_nerfactor, n_dirs)
        return vis, oma, None
    rc = capacity.PassCapacity(tensoIR.__dict__.setdefault("_rec_cap_hints", {}), n_rays, 1.5, max_entries=32,
                               capture=tensoIR.__dict__.get("_capture"), check_key=("secondary", n_rays))
    first = rc.hinted() is None
    cap = _rec_capacity(n_rays) if first else rc.hinted()
    extra = {} if ids is None else dict(ray_ids=ids["pair_ids"], n_ids_dev=ids["n_active"], vis=ids["vis"], rec_cnt=ids["rec_cnt"])
    # a record counter the primary march of this pass has already zeroed on the device (no fill launch); first attempt only
    armed = tensoIR.__dict__.pop("_rec_counter_armed", None)
    if armed is not None and armed.device == origins.device:
        extra["counter"] = armed
    lookup, force_full = (light_idx, light_div, dirs, dir_map, n_dirs), False
    while True:
        vis, oma, rec = ops.march_secondary(f, origins, dirs, z, n_rays, org_map, dir_map, active,
                                            tensoIR.march_t_stop, True, cap, want_nerfactor, n_dirs, **extra)
        extra.pop("counter", None)
        n_total, n_dev = rec["counter"][0:1], rec["counter"][1:2]      # all records / the written prefix consumers may read
        if first:                                      # no history yet: learn the count before sizing buffers
            total = int(n_total.item())
            if total > cap:
                cap = rc.regrow(total)
                continue
        else:
            rc.watch(n_total, cap)                     # (capturing: registers the counter with the graph's owner instead)
        out, rng = _decode_pass(tensoIR, f, vis, rec, total if first else cap, n_dev, lambda: total if first else rc.count.get(), lookup,
                                n_rays, force_full, keep_records, training, probe_map)
        if not first and (defer or rc.capture is not None):
            break                                      # settled later: by the caller, after ITS launches are queued too / by the graph's owner
        total = total if first else rc.count.get()     # waits for the march only, not for what was queued behind it
        if total <= cap and _range_failed(tensoIR, rng):
            force_full = True                          # re-run, decoding with the primary-stage kernels
        elif rc.settle(total):
            return vis, oma, out
        else:
            cap = rc.regrow(total)                     # overflow: some rays were dropped -> redo with room
    if rc.capture is None:                             # (a failed range guard too makes the caller re-run: then with the primary-stage kernels)
        tensoIR.__dict__.setdefault("_pending_checks", []).append(lambda: rc.settle() and not _range_failed(tensoIR, rng))
    elif _range_failed(tensoIR, rng):
        raise ops._lib.TensoirHipError("graph capture: the fp16 field shadow fails the range guard")
    return vis, oma, out


@torch.no_grad()
def compute_transmittance(tensoIR, surf_pts, light_in_dir, nSample=128, vis_near=0.1, vis_far=2, device="cuda"):
    """models/relight_utils.py:657-705 -> (nerv_vis [N], nerfactor_vis [N]).
    nSample <= 256 (the secondary-march kernels' limit; the reference's configs use 96): larger values raise TensoirHipError."""
    surf_pts = surf_pts.to(torch.float32).contiguous()
    light_in_dir = light_in_dir.to(torch.float32).contiguous()
    z = _z_table(nSample, vis_near, vis_far, surf_pts.device)
    vis, oma, _ = _secondary(tensoIR, surf_pts, light_in_dir, surf_pts.shape[0], z, None, None, None,
                             None, 0, False, True)
    return vis, oma


@torch.no_grad()
def compute_radiance(tensoIR, surf_pts, light_in_dir, light_idx, nSample=128, vis_near=0.05, vis_far=1.5,
                     device=None):
    """models/relight_utils.py:777-834 -> (nerv_vis [N], nerfactor_vis [N], indirect [N,3]).  nSample <= 256 (see compute_transmittance)."""
    surf_pts = surf_pts.to(torch.float32).contiguous()
    light_in_dir = light_in_dir.to(torch.float32).contiguous()
    li = light_idx.reshape(-1).to(surf_pts.device, torch.int32).contiguous()
    z = _z_table(nSample, vis_near, vis_far, surf_pts.device)
    return _secondary(tensoIR, surf_pts, light_in_dir, surf_pts.shape[0], z, None, None, None, li, 0,
                      True, True)


@torch.no_grad()
def compute_secondary_shading_effects(tensoIR, surface_pts, surf2light, light_idx, nSample=96, vis_near=0.05,
                                      vis_far=1.5, chunk_size=15000, device="cuda"):
    """models/relight_utils.py:344-399 -> (visibility [N,1], indirect [N,3]).  chunk_size only bounded
    the reference's intermediates; the fused march needs no chunking."""
    vis, _, ind = compute_radiance(tensoIR, surface_pts, surf2light, light_idx, nSample, vis_near, vis_far)
    return vis.reshape(-1, 1), ind.reshape(-1, 3)


def GGX_specular(normal, pts2c, pts2l, roughness, fresnel):
    """models/relight_utils.py:17-50 -> tir_ggx_specular."""
    return ops.ggx_specular(normal, pts2c, pts2l, roughness, fresnel)


brdf_specular = GGX_specular


def linear2srgb_torch(tensor_0to1):
    """models/relight_utils.py:489-515 (elementwise glue for callers outside the fused kernels)."""
    if isinstance(tensor_0to1, np.ndarray):
        x = np.clip(tensor_0to1, 0, 1)
        return np.where(x <= 0.0031308, x * 12.92, 1.055 * np.power(x + 1e-6, 1 / 2.4) - (1.055 - 1))
    x = tensor_0to1.clamp(0, 1)
    return torch.where(x <= 0.0031308, x * 12.92, 1.055 * torch.pow(x + 1e-6, 1 / 2.4) - (1.055 - 1))


def _maps_from_parts(depth_map, normal_map, albedo_map, roughness_map, fresnel_map):
    M = depth_map.shape[0]
    maps = torch.zeros((M, MAP_STRIDE), dtype=torch.float32, device=depth_map.device)
    maps[:, 3] = depth_map.reshape(-1)
    maps[:, 4:7] = normal_map
    maps[:, 7:10] = albedo_map
    maps[:, 10] = roughness_map.reshape(M, -1)[:, 0]
    maps[:, 11:14] = fresnel_map
    return maps


def finish_pending(tensoIR):
    """Run the deferred record-capacity checks of the shading stage; False = something overflowed (re-run the pass)."""
    ok = True
    for check in tensoIR.__dict__.pop("_pending_checks", []):
        ok = check() and ok
    return ok


def shade_from_maps(tensoIR, maps, rays, light_idx, sample_method="fixed_envirmap", args=None,
                    use_linear2srgb=True, acc_thres=-1e30, return_aux=False, _defer_check=False):
    """The body of render_with_BRDF (models/relight_utils.py:417-480) on packed [M,20] map rows.
    Rows with acc <= acc_thres are background: no secondary rays, white output (renderer.py:86-106).
    Material edits need no argument here -- a caller edits the rows first:
        out, maps = model(rays, light_idx, _return_maps=True)
        materials.apply_to_maps(maps, rays, edits, acc_thres=0.5)
        rgb = shade_from_maps(model, maps, rays, light_idx, "fixed_envirmap", args, acc_thres=0.5)"""
    dev = maps.device
    M = maps.shape[0]
    rays = ops.to_device(rays, dev, torch.float32).contiguous()
    li = ops.to_device(light_idx.reshape(-1), dev, torch.int32).contiguous()
    if sample_method == "fixed_envirmap":
        dirs = _on_device(tensoIR, "fixed_viewdirs", tensoIR.fixed_viewdirs, dev)
    else:
        dirs = ops.to_device(tensoIR.gen_light_incident_dirs(method=sample_method), dev, torch.float32).contiguous()
    D = dirs.shape[0]
    area = _on_device(tensoIR, "light_area_weight", tensoIR.light_area_weight, dev)
    z = _z_table(int(args.second_nSample), args.second_near, args.second_far, dev)
    if M == 0:
        out = torch.zeros((0, 3), dtype=torch.float32, device=dev)
        return (out, None) if return_aux else out
    train = torch.is_grad_enabled() and (maps.requires_grad or any(t.requires_grad for t in tensoIR.light_parameters()))
    fuse = not train and not return_aux
    with torch.no_grad():      # compute_secondary_shading_effects is @torch.no_grad (models/relight_utils.py:344)
        # only the pairs that pass the cosine / acc masks get a secondary ray: compacted id list (the reference's
        # boolean-mask indexing, :440-441); the pair counter is re-armed by the integration kernel at the end
        n_active = tensoIR.__dict__.get("_pair_counter")
        if n_active is None or n_active.device != dev:
            n_active = tensoIR.__dict__["_pair_counter"] = torch.zeros((1,), dtype=torch.int32, device=dev)
        surf, active, pair_ids, vis0, cnt0 = ops.shade_setup_compact(maps.detach(), rays, dirs, acc_thres, n_active)
        ids = {"pair_ids": pair_ids, "n_active": n_active, "vis": vis0, "rec_cnt": cnt0}
        equal_area = sample_method == "stratifed_sample_equal_areas"
        w_d = None if equal_area else area

        def probe_map(vis_p, ind_a, ind_b):
            """max |d rgb_with_brdf_map| over this pass's rays between two decodes of the secondary records (auto policy):
            the integration kernel run on both (no_grad; the pair counter is left alone).  One host synchronisation."""
            env_p = tensoIR.get_light_rgbs(dirs, device=dev).detach()
            outs = []
            for ind in (ind_a, ind_b):
                if isinstance(ind, dict):
                    outs.append(ops.shade_integrate_records(maps.detach(), rays, dirs, li, vis_p.view(M, D), ind["off"], ind["cnt"], ind["w"],
                                                            ind["rgb"], env_p, w_d, equal_area, use_linear2srgb, acc_thres, reset_counter=None))
                else:
                    outs.append(ops.shade_integrate(maps.detach(), rays, dirs, li, vis_p.view(M, D), ind.view(M, D, 3), env_p, w_d, equal_area,
                                                    use_linear2srgb, acc_thres))
            return float((outs[0] - outs[1]).abs().max())

        try:
            vis, _, ind = _secondary(tensoIR, surf, dirs, M * D, z, None, None, None, li, D, True, False, D,
                                     keep_records=fuse, ids=ids, defer=_defer_check, training=train, probe_map=probe_map)
        except BaseException:
            # the pair counter is re-armed by the integration kernel at the end of the pass; if the pass is abandoned
            # in between (capacity error under capture, OOM ...) it must not stay non-zero for the next call
            if tensoIR.__dict__.get("_capture") is None:
                n_active.zero_()
            else:
                tensoIR.__dict__.pop("_pair_counter", None)
            raise
    env = tensoIR.get_light_rgbs(dirs, device=dev)
    if not isinstance(ind, dict):
        ids["n_active"].zero_()            # the fused integration kernel (which re-arms the pair counter) is not on this route
    if train:
        from . import training
        rgb = training.ShadeFn.apply(maps, env, rays, dirs, li, vis.view(M, D), ind.view(M, D, 3), w_d, equal_area,
                                     use_linear2srgb, acc_thres)
    elif isinstance(ind, dict):
        rgb = ops.shade_integrate_records(maps, rays, dirs, li, vis.view(M, D), ind["off"], ind["cnt"], ind["w"],
                                          ind["rgb"], env, w_d, equal_area, use_linear2srgb, acc_thres,
                                          reset_counter=ids["n_active"])
    else:
        rgb = ops.shade_integrate(maps, rays, dirs, li, vis.view(M, D), ind.view(M, D, 3), env, w_d, equal_area,
                                  use_linear2srgb, acc_thres)
    if return_aux:
        return rgb, {"vis": vis.view(M, D), "indirect": ind.view(M, D, 3), "env": env, "surf": surf,
                     "active": active}
    return rgb


def render_with_BRDF(depth_map, normal_map, albedo_map, roughness_map, fresnel_map, rays, tensoIR, light_idx,
                     sample_method="fixed_envirmap", chunk_size=15000, device="cuda", use_linear2srgb=True,
                     args=None):
    """models/relight_utils.py:403-483 (same positional arguments; roughness_map is [M,3] or [M,1])."""
    maps = _maps_from_parts(depth_map.to(torch.float32), normal_map, albedo_map, roughness_map, fresnel_map)
    return shade_from_maps(tensoIR, maps, rays, light_idx, sample_method, args, use_linear2srgb)


class MisConfig:
    """Multiple importance sampling of the environment map and the BRDF lobes for the relighting entry points.
    brdf_fraction: the share of a point's samples drawn from the BRDF mixture, n_b = round(brdf_fraction * num_samples), the other
    n_l = num_samples - n_b from the map's own distribution (0: the jittered light-only estimator, 1: BRDF only).  lobe_select:
    the probability with which a BRDF sample comes from the cosine lobe and not the GGX half-vector lobe.  linear: the raw linear
    mean instead of the clamped, sRGB-encoded colour."""

    __slots__ = ("brdf_fraction", "lobe_select", "linear")

    def __init__(self, brdf_fraction=0.5, lobe_select=0.5, linear=False):
        for name, v in (("brdf_fraction", brdf_fraction), ("lobe_select", lobe_select)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) <= 1.0:      # (a NaN fails the comparison)
                raise ValueError(f"MisConfig: {name} lies in [0, 1], got {v!r}")
        self.brdf_fraction, self.lobe_select, self.linear = float(brdf_fraction), float(lobe_select), bool(linear)

    def split(self, num_samples):
        """-> (n_l, n_b) for `num_samples` samples per point."""
        num_samples = int(num_samples)
        if num_samples < 1:
            raise ValueError(f"MisConfig: num_samples >= 1, got {num_samples}")
        n_b = min(max(int(round(self.brdf_fraction * num_samples)), 0), num_samples)
        return num_samples - n_b, n_b

    def __repr__(self):
        return f"MisConfig(brdf_fraction={self.brdf_fraction}, lobe_select={self.lobe_select}, linear={self.linear})"


class Environment_Light:
    """models/relight_utils.py:110-205 with the HDR maps handed in as arrays (the reference reads
    ``*.hdr`` files with OpenCV, which is I/O outside the hot path)."""

    def __init__(self, hdr_path=None, device="cuda", hdr_maps=None):
        self.hdr_rgbs, self.hdr_pdf_sample, self.hdr_pdf_return, self.hdr_dir = {}, {}, {}, {}
        self.hdr_row_cdf, self.hdr_col_cdf, self.hdr_cdf_guide, self._cell_records = {}, {}, {}, {}
        self.hdr_row_sin = {}
        self._draws = 0
        maps = dict(hdr_maps or {})
        if torch.device(device).type == "cuda" and not torch.cuda.is_available():
            raise ops._lib.TensoirHipError("Environment_Light: no GPU is visible; tensoir_amd has no CPU path")
        if hdr_path is not None and str(hdr_path).startswith("synthetic"):       # no *.hdr files offline: seeded maps
            from . import synth
            from .synth_dataset import parse_spec
            spec = {"h": 32, "w": 64, **{k: v for k, v in parse_spec(hdr_path).items() if k in ("h", "w")}}
            maps.update(synth.make_hdr_maps(synth.HDR_NAMES, int(spec["h"]), int(spec["w"])))
        elif hdr_path is not None:
            for file in os.listdir(hdr_path):
                if file.endswith(".hdr"):
                    maps[file.split(".")[0]] = torch.from_numpy(read_hdr(os.path.join(hdr_path, file)))
        for name, rgbs in maps.items():
            rgbs = torch.as_tensor(rgbs, dtype=torch.float32).cpu()
            H, W, _ = rgbs.shape
            inten = torch.sum(rgbs, dim=2, keepdim=True)
            sin_theta = torch.sin(torch.linspace(0 + 0.5 / H, np.pi - 0.5 / H, H))
            pdf = inten * sin_theta.view(-1, 1, 1)
            pdf = pdf / torch.sum(pdf)
            pdf_ret = pdf * H * W / (2 * np.pi * np.pi * sin_theta.view(-1, 1, 1))
            lat, lng = np.pi / H, 2 * np.pi / W
            phi, theta = torch.meshgrid([torch.linspace(np.pi / 2 - 0.5 * lat, -np.pi / 2 + 0.5 * lat, H),
                                         torch.linspace(np.pi - 0.5 * lng, -np.pi + 0.5 * lng, W)], indexing="ij")
            dirs = torch.stack([torch.cos(theta) * torch.cos(phi), torch.sin(theta) * torch.cos(phi),
                                torch.sin(phi)], dim=-1).view(H, W, 3)
            self.hdr_rgbs[name] = rgbs.to(device)
            self.hdr_pdf_sample[name] = pdf.to(device)
            self.hdr_pdf_return[name] = pdf_ret.to(device)
            self.hdr_dir[name] = dirs.to(device)
            # the sin(theta) table hdr_pdf_return was divided by: pdf_return * row_sin = P_cell H W / (2 pi^2) (tir_env_mis_setup)
            self.hdr_row_sin[name] = sin_theta.float().to(device).contiguous()
            # inverse-CDF tables of the device sampler (tir_env_sample_setup): row marginal + row-conditional columns,
            # accumulated in fp64 so that the fp32 tables are the correctly rounded prefix sums
            p2 = pdf.view(H, W).double()
            rows = p2.sum(dim=1)
            row_cdf = torch.cumsum(rows, 0) / rows.sum()
            col_cdf = torch.cumsum(p2, 1) / rows.clamp(min=1e-300).unsqueeze(1)
            row_cdf[-1] = 1.0
            col_cdf[:, -1] = 1.0
            self.hdr_row_cdf[name] = row_cdf.float().to(device).contiguous()
            self.hdr_col_cdf[name] = col_cdf.float().to(device).contiguous()
            # guide tables of that search (ops.cdf_guide_tables): ~4 dependent loads per draw instead of log2(H) + log2(W)
            self.hdr_cdf_guide[name] = (ops.cdf_guide_tables(self.hdr_row_cdf[name], self.hdr_col_cdf[name])
                                        if os.environ.get("TENSOIR_CDF_GUIDE", "1") != "0" else None)
            # :144-146, the tables of sample_type="uniform" (solid-angle-uniform cells; like the reference they belong to the
            # size of the LAST map read)
            updf = torch.ones(H, W, 1) * sin_theta.view(-1, 1, 1) / (H * W)
            updf = updf / torch.sum(updf)
            self.envir_map_uniform_pdf = updf.to(device)
            self.envir_map_uniform_pdf_return = (updf * H * W / (2 * np.pi * np.pi * sin_theta.view(-1, 1, 1))).to(device)

    @torch.no_grad()
    def sample_light(self, light_name, bs, num_samples, sample_type="importance"):
        """:150-188.  The reference draws torch.multinomial over an expanded [bs, H*W] pdf; sampling bs*num
        indices from the 1-D pdf is the same distribution without materialising bs copies."""
        if sample_type == "importance":
            pdf, pdf_ret = self.hdr_pdf_sample[light_name].view(-1), self.hdr_pdf_return[light_name].view(-1)
        elif sample_type == "uniform":                   # :174-188 (no caller in the reference's scripts)
            pdf, pdf_ret = self.envir_map_uniform_pdf.view(-1), self.envir_map_uniform_pdf_return.view(-1)
            if pdf.numel() != self.hdr_dir[light_name].shape[0] * self.hdr_dir[light_name].shape[1]:
                raise ValueError(f"sample_light(uniform): map {light_name!r} has another size than the uniform tables (built for the last map read)")
        else:
            raise ValueError(f"sample_light: unknown sample_type {sample_type!r}")
        idx = torch.multinomial(pdf, bs * num_samples, replacement=True).view(bs, num_samples)
        d = self.hdr_dir[light_name].view(-1, 3)[idx]
        rgb = self.hdr_rgbs[light_name].view(-1, 3)[idx]
        p = pdf_ret[idx].unsqueeze(-1)
        return d, rgb, p

    @torch.no_grad()
    def sample_cells(self, light_name, normal, num_samples):
        """Device-side sample_light + cosine mask (tir_env_sample_setup): per surface point `num_samples` cells of the map
        drawn from hdr_pdf_sample by inverse-CDF search with Philox uniforms keyed by the framework's CUDA seed.  Returns
        (cell [M, Ns] int32, active [M, Ns] uint8): direction / radiance / pdf are hdr_dir / hdr_rgbs / hdr_pdf_return
        at the cell -- the [M, Ns, 3] tensors of the reference are never materialised."""
        self._draws += 1
        return ops.env_sample_setup(self.hdr_row_cdf[light_name], self.hdr_col_cdf[light_name],
                                    self.hdr_dir[light_name].view(-1, 3), normal, num_samples,
                                    torch.cuda.initial_seed(), self._draws)

    @torch.no_grad()
    def sample_cells_listed(self, light_name, normal, num_samples, bins=(1, 1), block_pairs=256, m_dev=None):
        """sample_cells with the same draws (same Philox counters) + the compacted list of the unmasked pairs, optionally
        direction-binned inside blocks of `block_pairs` pairs (tir_env_sample_setup_list).  Returns (cell [M, Ns],
        vis [M, Ns] with the masked pairs' zeros, pair_ids [M * Ns], n_active [1] on the device)."""
        self._draws += 1
        rec = self.cell_records(light_name)               # the direction comes from the records the integration reads later
        return ops.env_sample_setup_list(self.hdr_row_cdf[light_name], self.hdr_col_cdf[light_name],
                                           self.hdr_dir[light_name].view(-1, 3) if rec is None else rec, normal, num_samples,
                                           torch.cuda.initial_seed(), self._draws, bins, block_pairs,
                                           self.hdr_cdf_guide.get(light_name), m_dev)

    @torch.no_grad()
    def sample_mis(self, light_name, normal, rays_d, rough, num_samples, cfg, m_dev=None, block_pairs=512):
        """Per surface point cfg.split(num_samples) = (n_l, n_b) directions from the map's distribution (jittered inside their cells)
        and from the BRDF mixture, with their cells and the balance heuristic's mixture density (tir_env_mis_setup; needs the packed
        cell records).  One draw counter, like sample_cells / sample_cells_listed.  Returns (dirs [M, N, 3], cell [M, N], pdf_mix
        [M, N], vis [M, N] with the inactive pairs' zeros, pair_ids [M * N], n_active [1] on the device)."""
        if not isinstance(cfg, MisConfig):
            raise TypeError(f"sample_mis: cfg is a MisConfig, got {type(cfg).__name__}")
        rec = self.cell_records(light_name)
        if rec is None:
            raise ops._lib.TensoirHipError("multiple importance sampling needs the packed cell records (TENSOIR_ENV_RECORDS != 0)")
        n_l, n_b = cfg.split(num_samples)
        self._draws += 1
        return ops.env_mis_setup(self.hdr_row_cdf[light_name], self.hdr_col_cdf[light_name], rec, self.hdr_row_sin[light_name], normal,
                                 rays_d, rough, n_l, n_b, cfg.lobe_select, torch.cuda.initial_seed(), self._draws, block_pairs,
                                 self.hdr_cdf_guide.get(light_name), m_dev)

    def cell_records(self, light_name):
        """[H*W, 8] records {direction, pdf_return, radiance, 0} of a map (ops.pack_env_cells), built on first use: the
        integration kernel reads one 32-byte record per sample instead of three tables.  TENSOIR_ENV_RECORDS=0: None."""
        if os.environ.get("TENSOIR_ENV_RECORDS", "1") == "0":
            return None
        rec = self._cell_records.get(light_name)
        if rec is None:
            rec = ops.pack_env_cells(self.hdr_dir[light_name], self.hdr_rgbs[light_name], self.hdr_pdf_return[light_name])
            self._cell_records[light_name] = rec
        return rec

    def get_light(self, light_name, incident_dir):
        """:191-205 (background lookup, bilinear, align_corners=True) -> tir_env_lookup."""
        return ops.env_lookup(self.hdr_rgbs[light_name], incident_dir.reshape(-1, 3))


def read_hdr(path):
    """OpenCV's reader where there is one; tensoir_amd.hdr's where the import fails or the launcher's stand-in (shims.py) raises."""
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        with open(path, "rb") as h:
            buf = np.frombuffer(h.read(), np.uint8)
        try:
            return cv2.cvtColor(cv2.imdecode(buf, cv2.IMREAD_UNCHANGED), cv2.COLOR_BGR2RGB)
        except RuntimeError:
            if not getattr(cv2, "__tensoir_shim__", False):
                raise
    from . import hdr
    return hdr.read_hdr(path)


def _org_map(M, Ns, dev):
    """pair id -> surface point of the dense [M, Ns] pair grid, cached under the key the relighting entry points share."""
    key = ("orgmap", M, Ns, str(dev))
    org_map = _CONST_CACHE.get(key)
    if org_map is None:
        pair = torch.arange(M * Ns, dtype=torch.int32, device=dev)
        org_map = torch.div(pair, Ns, rounding_mode="floor").to(torch.int32)
        if len(_CONST_CACHE) > 64:
            _CONST_CACHE.clear()
        _CONST_CACHE[key] = org_map
    return org_map


@torch.no_grad()
def relight_with_envmap(tensoIR, surface_xyz, normal, albedo, roughness, fresnel, rays_d, light_dir,
                        light_rgb, light_pdf, nSample=96, vis_near=0.05, vis_far=1.5):
    """Loop body of scripts/relight_importance.py:119-170 for one environment map, given the samples
    drawn by Environment_Light.sample_light: cosine mask -> visibility march -> BRDF*L*cos/pdf mean -> sRGB."""
    dev = surface_xyz.device
    M, Ns = light_dir.shape[:2]
    light_dir = light_dir.to(torch.float32).contiguous()
    normal = normal.to(torch.float32).contiguous()
    cosine = torch.einsum("ijk,ik->ij", light_dir, normal)
    active = (cosine > 1e-6).to(torch.uint8).contiguous()
    z = _z_table(nSample, vis_near, vis_far, dev)
    vis, _, _ = ops.march_secondary(tensoIR.packed_field_dense(), surface_xyz.to(torch.float32).contiguous(),
                                    light_dir.view(-1, 3), z, M * Ns, _org_map(M, Ns, dev), None, active.view(-1),
                                    tensoIR.march_t_stop, False, 0, False)
    return ops.relight_importance(normal, albedo, roughness, fresnel, rays_d, light_dir, light_rgb,
                                  light_pdf, vis.view(M, Ns))


@torch.no_grad()
def relight_importance_sampled(tensoIR, env, light_name, surface_xyz, normal, albedo, roughness, fresnel, rays_d,
                               num_samples=512, nSample=96, vis_near=0.05, vis_far=1.5, m_dev=None, mis=None):
    """The loop body of scripts/relight_importance.py:119-170 for one environment map, entirely on the device:
    importance sampling + cosine mask (tir_env_sample_setup) -> visibility march of the unmasked (point, cell) pairs with
    the map's direction table as `dirs` and the cell index as `dir_map` -> BRDF x radiance x cosine / pdf mean -> sRGB
    (tir_relight_importance_cells).  Per sample 5 bytes of bookkeeping instead of the reference's 28 + masks.
    m_dev (int32 device scalar): the arrays have capacity M rows of which only the first m_dev are surface points
    (ops.surface_compact); rows beyond are neither sampled nor marched, their output rows are left unwritten.
    mis (a MisConfig; None = everything above, launch for launch): map and BRDF sampling combined under the balance heuristic
     -- tir_env_mis_setup -> the same march on the pairs' explicit directions -> tir_relight_mis; 28 bytes of
    bookkeeping per sample.  Needs the packed cell records."""
    dev = surface_xyz.device
    normal = normal.to(torch.float32).contiguous()
    M = normal.shape[0]
    if m_dev is not None and (not torch.is_tensor(m_dev) or m_dev.numel() != 1 or m_dev.dtype != torch.int32 or m_dev.device != dev):
        raise ValueError("m_dev: expected one int32 element on the points' device")
    if mis is not None and not isinstance(mis, MisConfig):
        raise TypeError(f"mis: None or a MisConfig, got {type(mis).__name__}")
    if mis is not None and env.cell_records(light_name) is None:
        raise ops._lib.TensoirHipError("multiple importance sampling needs the packed cell records (TENSOIR_ENV_RECORDS != 0)")
    if mis is not None and M > 0:
        dirs, cell, pdf_mix, vis0, pair_ids, n_active = env.sample_mis(light_name, normal, rays_d, roughness, num_samples, mis, m_dev)
        vis, _, _ = ops.march_secondary(tensoIR.packed_field_dense(), surface_xyz.to(torch.float32).contiguous(), dirs.view(-1, 3),
                                        _z_table(nSample, vis_near, vis_far, dev), M * num_samples, _org_map(M, num_samples, dev), None,
                                        None, tensoIR.march_t_stop, False, 0, False, ray_ids=pair_ids, n_ids_dev=n_active,
                                        vis=vis0.view(-1))
        return ops.relight_mis(normal, albedo, roughness, fresnel, rays_d, dirs, cell, pdf_mix, env.cell_records(light_name),
                               vis.view(M, num_samples), linear=mis.linear, m_dev=m_dev)
    if M == 0:
        # A call consumes one draw counter whatever M is (since round 5: the device-compacted chunk call, relight_chunk, cannot know
        # that a chunk is all background, and both routes must draw the same sequence).  Images rendered by rounds <= 4 with the
        # host-masked loop are therefore not reproduced bit for bit on views that contain all-background chunks (HISTORY, round 5).
        env._draws += 1
        return torch.zeros((0, 3), dtype=torch.float32, device=dev)
    order, bins, block_pairs = ops.c5_pair_order()
    if m_dev is not None and (order == "mask" or env.cell_records(light_name) is None):
        raise ops._lib.TensoirHipError("a device-side surface-point count needs the pair-list sampler and the packed cell records "
                                       "(TENSOIR_C5_PAIRS != mask, TENSOIR_ENV_RECORDS != 0)")
    if order == "mask":
        cell, active = env.sample_cells(light_name, normal, num_samples)
        listed = {}
    else:
        # :127-131 query visibility for the unmasked pairs only: so does the march, from a compacted list
        cell, vis0, pair_ids, n_active = env.sample_cells_listed(light_name, normal, num_samples, bins, block_pairs, m_dev)
        active = None
        listed = dict(ray_ids=pair_ids, n_ids_dev=n_active, vis=vis0.view(-1))
    z = _z_table(nSample, vis_near, vis_far, dev)
    env_dir = env.hdr_dir[light_name].view(-1, 3)
    vis, _, _ = ops.march_secondary(tensoIR.packed_field_dense(), surface_xyz.to(torch.float32).contiguous(), env_dir, z,
                                    M * num_samples, _org_map(M, num_samples, dev), cell.view(-1), None if active is None else active.view(-1),
                                    tensoIR.march_t_stop, False, 0, False, **listed)
    return ops.relight_importance_cells(normal, albedo, roughness, fresnel, rays_d, cell, env_dir,
                                        env.hdr_rgbs[light_name].view(-1, 3), env.hdr_pdf_return[light_name].view(-1),
                                        vis.view(M, num_samples), env_cell=env.cell_records(light_name), m_dev=m_dev)


@torch.no_grad()
def relight_chunk(tensoIR, env, light_names, rays, light_idx, num_samples=512, nSample=96, vis_near=0.05, vis_far=1.5,
                  N_samples=-1, out=None, mis=None, edits=None):
    """One chunk of scripts/relight_importance.py:93-185 for ALL environment maps without a host round trip: primary pass ->
    the acc > 0.5 rows compacted ON THE DEVICE (the script's boolean-mask indexing, :99-113, is a synchronisation per chunk
    plus ~12 indexing launches) -> per map: importance sampling, visibility march and BRDF integration bounded by the
    device-side point count -> relit colour where a ray hit, background lookup elsewhere (:166-171), written side by side into
    ONE [B, 3 * n_maps] buffer.  Same Philox counters per (point, sample) as the host-compacted sequence: identical colours.
    Returns (out [B, 3 n_maps], primary-pass tuple, compacted surface dict).
    What the caller still applies, as the script does AFTER its loop body (scripts/relight_importance.py:166-176): hit rows hold the
    relit colour already clamped and sRGB-encoded by the integration kernel; BACKGROUND rows hold the raw environment lookup
    (Environment_Light.get_light) -- the script's clamp, tone mapping of the background and its `acc > 0.9` blend of the two
    (`:172-176`) are the caller's (prim[6] is acc_map).
    mis: relight_importance_sampled's (a MisConfig: map and BRDF sampling under the balance heuristic; None: as above).
    edits (a materials.EditList or a list of MaterialEdit; None: no kernel is added and every result keeps its bits):
    materials.apply_to_maps runs once on the chunk's map rows before they are compacted, so the relit colours, the compacted
    arrays and the albedo, roughness and Fresnel maps handed back in `prim` (views of the edited rows, made so explicitly) are the
    edited ones.  What the primary pass composited from the unedited materials -- rgb_map, rgb_with_brdf_map -- is NOT
    re-rendered."""
    from . import materials
    edits = materials.as_edit_list(edits)                  # refused before the chunk is rendered
    dev = rays.device
    rays = rays.to(torch.float32).contiguous()
    B = rays.shape[0]
    names = list(light_names)
    prim, maps = tensoIR(rays, light_idx, N_samples=N_samples, _return_maps=True)
    if edits is not None and len(edits) > 0:
        materials.apply_to_maps(maps, rays, edits, 0.5)
        # unpack_maps hands out column views of `maps`; a forward that returned copies would still show the unedited materials
        prim = tuple(prim[:3]) + (maps[:, 7:10], maps[:, 10:11], maps[:, 11:14]) + tuple(prim[6:])
    c = ops.surface_compact(maps, rays, 0.5)
    if out is None:
        out = torch.empty((B, 3 * max(len(names), 1)), dtype=torch.float32, device=dev)
    for i, name in enumerate(names):
        rgb = relight_importance_sampled(tensoIR, env, name, c["surf"], c["normal"], c["albedo"], c["rough"], c["fresnel"], c["rays_d"],
                                         num_samples, nSample, vis_near, vis_far, m_dev=c["n_hit"], mis=mis)
        ops.env_compose(env.hdr_rgbs[name], rays, c["slot"], rgb, out, 3 * i)
    return out, prim, c


# columns of a [B, 20] map row that tir_denoise_guide reads, as positions in TensorVMSplit.unpack_maps' tuple -> (column, width)
_GUIDE_COLUMNS = {1: (3, 1), 2: (4, 3), 3: (7, 3), 4: (10, 1), 6: (14, 1)}


def _map_rows(prim, B):
    """[B, 20] map rows for tir_denoise_guide from the primary-pass tuple relight_chunk hands back.  unpack_maps returns column
    views of one contiguous [B, 20] tensor: where depth, normal, albedo, roughness and acc still lie at their columns of one such
    block (strides and addresses checked), that block is read in place; otherwise (a forward that returns copies) the rows are
    assembled from those columns, the others zero -- the kernel reads no other column."""
    cols = {i: prim[i] for i in _GUIDE_COLUMNS}
    base = cols[1].data_ptr() - 4 * _GUIDE_COLUMNS[1][0]
    in_place = B > 0 and all(t.dtype == torch.float32 and t.stride(0) == MAP_STRIDE and (t.dim() == 1 or t.stride(1) == 1)
                             and t.data_ptr() == base + 4 * c for t, (c, _) in ((cols[i], _GUIDE_COLUMNS[i]) for i in cols))
    first = cols[1].storage_offset() - _GUIDE_COLUMNS[1][0]            # element of the storage at which row 0 would begin
    if in_place and first >= 0 and cols[1].untyped_storage().nbytes() >= 4 * (first + B * MAP_STRIDE):
        return torch.as_strided(cols[1], (B, MAP_STRIDE), (MAP_STRIDE, 1), first)
    maps = torch.zeros((B, MAP_STRIDE), dtype=torch.float32, device=cols[1].device)
    for i, (c, w) in _GUIDE_COLUMNS.items():
        maps[:, c:c + w] = cols[i].reshape(B, w)
    return maps


@torch.no_grad()
def relight_view(tensoIR, env, light_names, rays, H, W, light_idx=None, num_samples=512, chunk=4096, nSample=96, vis_near=0.05,
                 vis_far=1.5, denoise=None, mis=None, edits=None):
    """A whole H x W view relit under every map of `light_names`: relight_chunk over chunks of `chunk` rays (rays [H * W, 6],
    row-major; light_idx [H * W] or [H * W, 1], default zeros) into one [H * W, 3 n_maps] buffer, the denoiser's guide rows packed
    next to it (tir_denoise_guide, one launch per chunk), and with denoise = a tensoir_amd.denoise.AtrousConfig the guided
    a-trous filter over all maps together (cfg.levels launches).  The loop adds no host synchronisation to relight_chunk's.
    -> {"rgb": [n_maps, H, W, 3], "raw": the image before the filter (the same tensor when denoise is None), "guide": [H, W, 12],
    "acc": [H, W]}.  Rows mean what relight_chunk documents: hit rows hold the clamped sRGB relit colour, background rows
    (acc <= 0.5: not valid in the guide) the raw environment lookup, which the filter neither changes nor reads.
    num_samples: importance samples per surface point and map -- with the filter, 16 to 64 instead of 512.
    mis: relight_importance_sampled's (a MisConfig: map and BRDF sampling under the balance heuristic; None: map only).
    edits: relight_chunk's (material edits; None: nothing is added).  The guide rows are built from the EDITED maps
    -- a guide of unedited albedo would let the filter blur across an edit's border; nothing the primary pass composited is
    re-rendered.
    Single process: the multi-rank gather of the benchmark keeps its own loop."""
    from . import denoise as dn
    H, W, chunk = int(H), int(W), int(chunk)
    names = list(light_names)
    if H < 1 or W < 1 or chunk < 1 or rays.dim() != 2 or tuple(rays.shape) != (H * W, 6):
        raise ValueError(f"relight_view: rays is [H * W, 6] = [{H * W}, 6] and chunk >= 1, got {tuple(rays.shape)} and chunk {chunk}")
    if not 1 <= len(names) <= ops.ATROUS_MAX_K // 3:
        raise ValueError(f"relight_view: 1 to {ops.ATROUS_MAX_K // 3} environment maps, got {len(names)}")
    if mis is not None and not isinstance(mis, MisConfig):
        raise TypeError(f"relight_view: mis is None or a MisConfig, got {type(mis).__name__}")
    if denoise is not None and not isinstance(denoise, dn.AtrousConfig):
        raise TypeError(f"relight_view: denoise is None or an AtrousConfig, got {type(denoise).__name__}")
    from . import materials
    edits = materials.as_edit_list(edits)
    if not rays.is_cuda:
        raise ops._lib.TensoirHipError("relight_view: rays must live on the GPU; tensoir_amd has no CPU path")
    dev, n = rays.device, H * W
    inv = None if denoise is None else denoise.inverses(tensoIR.aabb)        # refused before the view is rendered
    rays = rays.to(torch.float32).contiguous()
    lidx = (torch.zeros((n, 1), dtype=torch.int32, device=dev) if light_idx is None
            else ops.to_device(light_idx.reshape(n, 1), dev, torch.int32).contiguous())
    rows = torch.empty((n, 3 * len(names)), dtype=torch.float32, device=dev)
    guide = torch.empty((n, ops.DENOISE_GUIDE), dtype=torch.float32, device=dev)
    acc = torch.empty((n,), dtype=torch.float32, device=dev)
    for r0 in range(0, n, chunk):
        r1 = min(r0 + chunk, n)
        _, prim, _ = relight_chunk(tensoIR, env, names, rays[r0:r1], lidx[r0:r1], num_samples, nSample, vis_near, vis_far, out=rows[r0:r1],
                                   mis=mis, edits=edits)
        ops.denoise_guide(_map_rows(prim, r1 - r0), rays[r0:r1], guide, r0, 0.5)      # valid = relight_chunk's own acc > 0.5
        acc[r0:r1] = prim[6]
    image = lambda t: t.view(H, W, len(names), 3).permute(2, 0, 1, 3).contiguous()
    raw = image(rows)
    rgb = raw if denoise is None else image(dn.filter_rows(rows, guide, H, W, denoise.levels, inv))
    return {"rgb": rgb, "raw": raw, "guide": guide.view(H, W, ops.DENOISE_GUIDE), "acc": acc.view(H, W)}
