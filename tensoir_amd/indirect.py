"""Precision policy for INDIRECT light: which tier decodes the secondary-ray records of a pass.

The radiance of the SECONDARY-ray records (models/relight_utils.py:818-832) is averaged over a ray's records and over the light
directions before it reaches rgb_with_brdf_map; its gather and decoder may run at another precision than the launches whose
outputs are composited into the maps directly.  The knobs live in ops.py (bench.py reads and assigns them):
  TENSOIR_INDIRECT_PRECISION = f16: appearance taps from an fp16 shadow of the planes / lines (tir_vm_app_fwd_h16)
                                 and the single-product fp16 decoder (tir_mlp_fwd_auxtab_f16), fp32 accumulation everywhere;
                                 measured on rgb_with_brdf_map: profiles/r04_precision_policy.json
                             = full: the same kernels as the primary stage (fp32 taps, split-bf16 x3 decoder)
                             = auto (default, round 5): the f16 kernels, but only for field / decoder versions that pass (i) the
                                 RANGE guard -- max|plane_i| max|line_i| max|light row| and max|basis_mat| from the pack launch
                                 bound every fp16 product below 6e4, checked for every new parameter version without an extra
                                 host synchronisation (ops.HalfRange; relight._range_failed) -- and (ii) the SELF-CHECK probe
                                 (`establish`); re-probed whenever parameter storage changes (load, upsample, shrink) and every
                                 INDIRECT_PROBE["interval"] parameter versions otherwise (optimizer steps).  Anything else falls
                                 back to `full` for that version (`mode`; the verdict is kept with the model and written into
                                 checkpoints).
                             = hp (round 6): the high-precision fused kernel unconditionally (tir_indirect_fused_hp_fwd: fp32 taps,
                                 decoder weights as fp16 + fp8 residue).  Under `auto` it is the FIRST fallback: a version whose
                                 self-check rejects the f16 kernels is checked the same way with the hp kernel (both against the
                                 full kernels) and only goes to `full` when that fails too -- a field trained to 300^3 takes
                                 this route (profiles/r06_precision_trained_300.json).  TENSOIR_INDIRECT_HP=0 removes the tier.
Applies only while ops.MLP_IMPL is the split-bf16 default (the exact / cross-check decoder modes stay exact end to end).

The self-check.  Through render_with_BRDF / Renderer_TensoIR_train (relight.shade_from_maps) it is a MEASUREMENT of the
quantity the tolerance is stated on: all secondary-ray records of the pass are decoded by both paths, the integration kernel
renders rgb_with_brdf_map from both, and the f16 kernels are kept while
    max over the pass's rays of |rgb_with_brdf_map(f16) - rgb_with_brdf_map(full)|  <=  map_limit  (2.5e-5)
-- a quarter of the 1e-4 budget; other batches of the same parameters can be worse than the probed one, measured up to 2x
(profiles/r05_precision_trained.json), which leaves the policy's contribution under half of the budget.
The bare compute_radiance / compute_secondary_shading_effects entry points have no map to measure: there (`record_estimate`) an
evenly strided subset of up to INDIRECT_PROBE["records"] records is decoded by both paths and the map error is ESTIMATED from
the signed mean ("bias", max over the colour channels), the rms and the max of the difference:
    max(w_bias * bias + w_rms * rms, w_max * max) <= limit
calibrated on the scaling sweep and the trained checkpoint of tests/precision_cases.py, where the measured map error was
0.45 bias + 0.2 rms within 15 % on the smooth scenes and 0.2 max on the trained one (profiles/r05_precision_sweep.json: 3.3e-6 as
initialised, 3.0e-5 with the radiance decoder's weights doubled, 2.0e-4 with x4 -- unguarded fp16 leaves the budget there).
range: the largest |product| the range guard accepts (largest finite fp16 = 65504).
TENSOIR_INDIRECT_MAP_LIMIT overrides map_limit (a trained analytic scene measured 2.0e-5 ... 3.1e-5 on its own training rays:
around the default, so such a checkpoint may run either way; both are within the budget).
train_map_limit: what a TRAINING forward accepts (is_train renders feed the loss only, and the secondary stage is a no_grad
constant there, models/relight_utils.py:344): the contract's tolerance itself.  A verdict taken with it never serves an
inference pass (`mode` re-probes with the strict limit)."""
from __future__ import annotations

import torch

from . import ops

_ATTR = "_indirect_state"


def state(model):
    return model.__dict__.setdefault(_ATTR, {"verdict": None, "key": None, "storage": None, "age": 0, "why": None,
                                             "stats": None, "probes": 0, "fallbacks": 0})


def reset(model):
    """Forget the verdict (new parameters in the old storage: it must be re-established)."""
    model.__dict__.pop(_ATTR, None)


def verdict(model):
    """The stored verdict or None; creates no state."""
    return (model.__dict__.get(_ATTR) or {}).get("verdict")


def key(model):
    """(parameter versions, parameter storage) of everything the indirect-light kernels read: appearance field + radiance decoder."""
    if model._field_key is None:            # (callers inside a pass have just refreshed it: the key walk over ~35 parameters
        model.packed_field()                #  costs ~70 us of host time, and the training loop is host-bound)
    model.renderModule.packed()
    fk = model._field_key[0]
    k = (fk, model.renderModule._key)
    storage = (tuple((a, c) for a, _, c in fk), tuple(a for a, _ in model.renderModule._key))
    return k, storage


def mode(model, training=False):
    """Which kernels decode this pass's secondary-ray records: "full" (primary-stage kernels), "f16" (the precision policy's fast
    kernels), "hp" (the high-precision fused kernel, ops.indirect_fused_hp) or "probe" (auto policy, no valid verdict for the
    current parameters: `establish` one on this pass's own records).

    auto (ops.INDIRECT_GUARD): a verdict belongs to one parameter version.  Inference passes always use a verdict of exactly
    the current version (so the same parameters render the same image whatever was rendered before).  TRAINING passes
    (`training`: the forward of an optimizer step, where indirect light is a no_grad constant of the loss) carry it over to later
    versions of the SAME storage -- an optimizer step moves a parameter by at most the learning rate -- for
    ops.INDIRECT_PROBE["interval"] versions, then re-establish it; new storage (load, upsample, shrink) re-establishes it at
    once.  The range guard is evaluated for EVERY version (HalfRange, no extra synchronisation) by the caller."""
    if ops.secondary_app_impl() != "h16" and ops.secondary_mlp_impl() in (None, "hp"):
        return "hp" if ops.secondary_mlp_impl() == "hp" else "full"
    if not ops.INDIRECT_GUARD:
        return "f16"
    st = state(model)
    k, storage = key(model)
    # `key` is the version a probe MEASURED; `carried_key` the latest version a training pass carried that verdict over to.
    # Only a training pass may ride on a carried verdict: an inference pass at a version that was never probed probes.
    if st["verdict"] is not None and st["key"] == k and (training or not st.get("train_limit")):
        return st["verdict"]         # (an inference pass never rides on a verdict taken with the training limit)
    if training and st["verdict"] is not None and st["storage"] == storage:
        if st.get("carried_key") == k:
            return st["verdict"]     # (another pass at a version already counted)
        if st["age"] < ops.INDIRECT_PROBE["interval"]:
            st["age"] += 1
            st["carried_key"] = k
            return st["verdict"]
    return "probe"


def set_verdict(model, verdict, why, stats=None, train_limit=False):
    st = state(model)
    k, storage = key(model)
    if verdict != "f16" and st["verdict"] != verdict:       # (a version that left the fast kernels: to hp, or all the way to full)
        st["fallbacks"] += 1
    st.update(verdict=verdict, key=k, carried_key=None, storage=storage, age=0, why=why, train_limit=bool(train_limit))
    if stats is not None:
        st["stats"] = stats


def report(model):
    """What the policy decided for this model so far: {"policy": auto|f16|hp|full, "mode": f16|hp|full|None, "why": ...,
    "probe": {...}, "probes_run": ..., "fallbacks": ...} -- also written into checkpoints."""
    st = model.__dict__.get(_ATTR) or {}
    if ops.secondary_app_impl() is None and ops.secondary_mlp_impl() in (None, "hp"):
        pol = "hp" if ops.secondary_mlp_impl() == "hp" else "full"
    else:
        pol = "auto" if ops.INDIRECT_GUARD else "f16"
    return {"policy": pol, "mode": st.get("verdict") if pol == "auto" else pol, "why": st.get("why"), "probe": st.get("stats"),
            "probes_run": st.get("probes", 0), "fallbacks": st.get("fallbacks", 0)}


def record_estimate(cand_rows, n_valid, decode_full_subset):
    """The self-check where there is no map to measure: an evenly strided subset `sel` of the first n_valid records, decoded by
    the primary-stage kernels (decode_full_subset(sel) -> rows) and compared with the candidate tier's rows -> (ok, stats).
    One host synchronisation (only in passes that establish a verdict)."""
    lim = ops.INDIRECT_PROBE
    n_valid = min(int(n_valid), cand_rows.shape[0])
    if n_valid <= 0:
        return True, {"records": 0}
    step = max(1, n_valid // lim["records"])
    sel = torch.arange(0, n_valid, step, device=cand_rows.device)[:lim["records"]]
    ref = decode_full_subset(sel)
    d = (cand_rows[sel] - ref).double()
    v = torch.stack([d.mean(0).abs().max(), d.pow(2).mean().sqrt(), d.abs().max(), ref.double().pow(2).mean().sqrt()]).tolist()
    est = max(lim["w_bias"] * v[0] + lim["w_rms"] * v[1], lim["w_max"] * v[2])     # estimated max error on rgb_with_brdf_map
    stats = {"kind": "records", "records": int(sel.numel()), "of": n_valid, "bias": v[0], "rms": v[1], "max": v[2], "radiance_rms": v[3],
             "estimate": est}
    return bool(est <= lim["limit"]), stats                    # (NaN fails)


def establish(model, decode, measure, try_hp, train_limit):
    """The self-check ladder of the auto policy on one pass's own records: f16, else (try_hp) hp, else full, each candidate
    judged against the full kernels.  decode(kind) -> the rows of a tier; measure(rows) -> (ok, stats), where a comparison with
    NaN must come out as not ok.  Stores the verdict for the current parameter version -> (verdict, rows of that tier)."""
    state(model)["probes"] += 1          # passes that ran the self-check
    tier, rows = "f16", decode("f16")
    ok, stats = measure(rows)
    if not ok:
        tier = "full"
        if try_hp:                       # first fallback: the high-precision fused kernel, checked the same way
            rows_hp = decode("hp")
            ok, stats_hp = measure(rows_hp)
            stats = {**stats_hp, "f16": stats}
            if ok:
                tier, rows = "hp", rows_hp
        if tier == "full":
            rows = decode("full")
    set_verdict(model, tier, "probe", stats, train_limit=train_limit)
    return tier, rows
