"""tests/indirect_reference.py pinned without a GPU: the restatement against the oracle in float64, the conditions every fixture of
tests/test_gpu_indirect_kernels.py has to meet, the yardsticks (the distance of each arithmetic-class emulation from float64, printed;
DESIGN 2, "The indirect-light kernels on their own" holds them beside the device's), and the sensitivity of the comparison rule: each
mistake one of these kernels could make, applied to the restatement or to the emulation, lands beyond the loosest bound the GPU test
applies to that tensor on that fixture."""
import pytest
import torch

from oracle import tensoir_oracle as O
from tests import decoder_reference as D
from tests import indirect_reference as R

F32, F64 = R.F32, R.F64


def _scene(fld):
    return O.scene_from_state_dict(fld.ck["state_dict"], fld.ck["kwargs"]).to(F64)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_taps_are_the_kernels_own():
    """taps32 is _taps32 of tests/test_gpu_dense_app.py (make_tap_q on the host) on every point class; taps64 agrees with it wherever the
    two pick the same cell, to the rounding of the fp32 steps."""
    from tests.test_gpu_dense_app import _taps32
    for name in ("l1", "l17"):
        fld = R.field(name)
        xyz, ids = R.points(fld, torch.Generator().manual_seed(1))
        assert sorted(set(ids.tolist())) == list(range(6))
        for a in range(3):
            mine, theirs = R.taps32(xyz[:, a], fld.grid[a]), _taps32(xyz[:, a], fld.grid[a])
            for u, v in zip(mine, theirs):
                assert torch.equal(u.double(), v.double())
            i0, i1, w0, w1 = R.taps64(xyz[:, a], fld.grid[a])
            same = i0 == mine[0]
            assert float(same.double().mean()) > 0.9
            assert float((w0[same] - mine[2][same].double()).abs().max()) < 4e-6 and float((w1[same] - mine[3][same].double()).abs().max()) < 4e-6


@pytest.mark.parametrize("name", list(R.FIELDS))
def test_restatement_equals_the_oracle(name):
    """In float64, on float64 taps: features = oracle app_feature, output = oracle mlp3 on the oracle's input row, to 1e-12 of the scale,
    under every addressing (the +-65504 clamp of the fused entries is the only step the oracle does not have)."""
    fld = R.field(name)
    sc = _scene(fld)
    for addr in R.ADDRESSINGS:
        rec = R.population(name, addr)
        li = R.light_rows(fld, rec)
        want = O.app_feature(sc, rec.xyz.double(), li)
        got = R.features(fld, rec, F64, taps=R.taps64)
        scale = max(1.0, float(want.abs().max()))
        assert float((got - want).abs().max()) <= 1e-12 * scale, (name, addr)
        for dec in (("sig3", "tanh3") if addr == "d3" else ("sig4",)):
            od, act, _ = D.DECODERS[dec]
            w = {k: v.double() for k, v in R.weights(name, dec).items()}
            z = O.mlp3(w, O.mlp_input(want.clamp(-R.H_MAX, R.H_MAX), rec.dirs.double()[R.aux_rows(rec)], 2, 2))
            out = R.forward(fld, rec, dec, F64, taps=R.taps64, w=R.weights(name, dec))[1]
            # (huge regime: float64's own rounding of a feature of size 6e4 is 7e-12 in the phase of its positional encoding)
            tol = 1e-10 if fld.regime == "huge" else 1e-12
            assert float((out - (torch.tanh(z) if act == 1 else torch.sigmoid(z))).abs().max()) <= tol, (name, addr, dec)


def test_addressing_rule():
    fld = R.field("l8")
    rec = R.population("l8", "div5mod7")
    p = rec.rec_map.long()
    assert torch.equal(R.aux_rows(rec), p % 7)
    assert torch.equal(R.light_rows(fld, rec), rec.light_idx.long()[p // 5].clamp(0, 7))
    one = R.population("l1", "d3")
    assert bool((R.light_rows(R.field("l1"), one) == 0).all())                    # one light: row 0 whatever the index
    plain = R.population("l8", "nomap")
    assert torch.equal(R.aux_rows(plain), torch.arange(plain.n)) and plain.dirs.shape[0] == plain.n
    assert torch.equal(R.light_rows(fld, plain), plain.light_idx.long().clamp(0, 7))
    h = R.head(rec, 17)
    assert h.n == 17 and torch.equal(h.rec_map, rec.rec_map[:17]) and h.light_idx is rec.light_idx and h.dirs is rec.dirs


# ---- fixture conditions --------------------------------------------------------------------------------------------------------------
def test_fixture_conditions():
    """Feature peak above 1e-2; every output column spreads (standard deviation >= 0.1 over the rows); every population holds every
    point class, uses the first and the last ray and direction and the light indices -1 and n_lights + 3; the small regime reaches
    fp16's subnormals; the large regime passes the range guard with its largest product above 3e4; the huge regime has raw features
    beyond 448 and beyond 65504 with basis_mat inside fp16; the saturating weight sets have their maxima in [8, 16)."""
    print()
    for name, (lights, regime, grid) in R.FIELDS.items():
        fld = R.field(name)
        assert len(set(grid)) == 3 and all(g <= m for g, m in zip(sorted(grid), (20, 24, 28))) and fld.n_lights == lights
        assert fld.ck["kwargs"]["light_rotation"] == [(i * 360) // lights for i in range(lights)]
        for addr in R.ADDRESSINGS:
            rec = R.population(name, addr)
            li = R.light_rows(fld, rec)
            want = set(range(7 if fld.planted is not None else 6))
            assert set(rec.ids.tolist()) == want and int((rec.ids == 5).sum()) == 8, (name, addr)
            assert int((rec.xyz.abs() > 1).any(1).sum()) > 20
            if lights > 1:
                assert set(li.tolist()) == set(range(lights)), (name, addr)
                used = rec.light_idx.long()[R.pair_ids(rec) // max(rec.idx_div, 1)]
                assert -1 in used.tolist() and lights + 3 in used.tolist(), (name, addr)
            ai = R.aux_rows(rec)
            assert int(ai.min()) == 0 and int(ai.max()) == rec.dirs.shape[0] - 1
            if rec.rec_map is not None:
                assert int(rec.rec_map.max()) // rec.idx_div == rec.light_idx.numel() - 1 and int(rec.rec_map.min()) == 0
            for dec in R.DECODERS:
                r = R.refs(name, addr, dec)
                assert float(r.feat64.abs().max()) > 1e-2
                assert float(r.out64.std(0).min()) >= 0.1, (name, addr, dec, r.out64.std(0))
                assert bool(torch.isfinite(r.out64).all())
        prod = R.products(fld, rec.xyz, R.light_rows(fld, rec), F64).abs()
        ok, b = R.half_range_bound(fld)
        print(f"[indirect fixture] {name}: {regime}, lights {lights}, grid {grid}, largest product {float(prod.max()):.3g}, range bound {b:.3g} "
              f"({'ok' if ok else 'refused'}), feature peak {float(R.refs(name).feat64_raw.abs().max()):.3g}")
        if regime == "small":
            tiny = 2.0 ** -14                                               # smallest normal fp16
            assert float(prod.max()) < tiny and float((prod[prod > 0]).median()) > 2.0 ** -24
            assert float(max(p.abs().max() for p in fld.planes)) > tiny        # the tables themselves are normal numbers
        if regime == "large":
            assert ok and b < R.HALF_RANGE and float(prod.max()) > 3e4
            assert int(prod.argmax() % R.NCH) == fld.planted_channel
        if regime in ("unit", "small"):
            assert ok
        if regime == "huge":
            raw = R.refs(name).feat64_raw.abs()
            assert int((raw > R.F8_MAX).sum()) > 100 and int((raw > R.H_MAX).sum()) > 100 and float(fld.basis.abs().max()) < R.H_MAX
    for dec in R.DECODERS:
        w = R.saturating_decoder(dec)
        assert 8 <= float(w["w0"].abs().max()) < 16 and 8 <= float(w["w1"].abs().max()) < 16
        res = (w["w0"] - w["w0"].half().float()) * R.F8_SCALE
        assert float(res.abs().max()) > R.F8_MAX                              # the residue does saturate
        for name in ("l2", "l8"):
            assert float(R.refs(name, "d3", dec, wkind="saturating").out64.std(0).min()) >= 0.1


# ---- yardsticks ----------------------------------------------------------------------------------------------------------------------
def test_yardsticks_order_as_the_header_claims():
    """Distance from float64 of every class on every fixture, printed.  hp is nearer float64 than the f16 fused class, on the shadow taps
    and on the dense volume, on every fixture of the unit regime.  In the small and large regimes it need not be and the header does not
    claim it: a lo part below 2^-14 is an fp16 subnormal and one below 2^-25 is nothing, so where the products (small) or basis_mat
    (large: scaled down to keep the features at unit size) are that small hp's contraction is that of single fp16 operands
    (include/tensoir_hip.h, tir_indirect_fused_hp_fwd).  Those figures are printed."""
    print()
    worst = {}
    for name in R.FIELDS:
        fld = R.field(name)
        for addr in R.ADDRESSINGS:
            for dec in R.DECODERS:
                r = R.refs(name, addr, dec)
                d = {k: R.distance(getattr(r, k), r.out64 if k.startswith("out") else r.feat64_raw if k == "feat_h16" else r.feat64)
                     for k in ("feat32", "feat_h16", "feat_dense", "feat_hp", "out32", "out_h16", "out_dense", "out_hp") if hasattr(r, k)}
                print(f"[indirect yardstick] {name} {addr} {dec}: " + " ".join(f"{k} {v:.2e}" for k, v in d.items()))
                for k, v in d.items():
                    worst[(fld.regime, k)] = max(worst.get((fld.regime, k), 0.0), v)
                if "out_hp" in d and "out_h16" in d and fld.regime == "unit":
                    assert d["out_hp"] < d["out_h16"], (name, addr, dec, d)
                    assert d["feat_hp"] < d["feat_h16"], (name, addr, dec, d)
                if "out_hp" in d and "out_dense" in d and fld.regime == "unit":
                    assert d["out_hp"] < d["out_dense"], (name, addr, dec, d)
                assert fld.regime == "huge" or d["out32"] < d.get("out_hp", 1.0)     # (huge: float32 rounds the phase itself)
    for (regime, k), v in sorted(worst.items()):
        print(f"[indirect yardstick] worst {regime:6s} {k:10s} {v:.2e}")


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------------
def _beyond(label, wrong, f64, bounds, stat=R.distance):
    d = stat(wrong, f64)
    worst = max(bounds.values())
    print(f"[indirect sensitivity] {label}: mistake {d:.2e}, bounds " + ", ".join(f"{k} {v:.2e}" for k, v in bounds.items()) + f", margin x{d / worst:.1f}")
    assert d > worst, (label, d, bounds)


def _bounds(r, kind):
    ref = r.out64 if kind == "out" else r.feat64
    return {c: R.bound(getattr(r, f"{kind}_{c}"), ref) for c in ("h16", "dense", "hp") if hasattr(r, f"{kind}_{c}")}


@pytest.mark.parametrize("name", ["l2", "l8", "l16", "l17", "l1"])
def test_restatement_mistakes_land_beyond_the_bounds(name):
    """Feature ownership split at 13, sin and cos swapped, the light row from p % idx_div, aux_mod before the map, the out-of-range light
    index wrapped, two plane axes swapped in one VM group: each against the loosest bound of the tensors it reaches (the features are
    an output of tir_vm_app_fwd_h16 only, so only the mistakes of the gather are held against their bounds)."""
    print()
    fld = R.field(name)
    for addr in R.ADDRESSINGS[1:]:
        rec = R.population(name, addr)
        for dec in (("sig3", "tanh3") if addr == "d3" else ("sig4",) if addr == "d16" else ("sig1",)):
            r = R.refs(name, addr, dec)
            for mistake, light_only, gather in (("own13", False, False), ("pe_swap", False, False), ("light_mod", True, True),
                                                ("mod_before_map", False, False), ("light_wrap", True, True), ("plane_axes", False, True)):
                if light_only and fld.n_lights == 1:
                    continue                                   # (one light: no index is read)
                feat, out = R.forward(fld, rec, dec, F64, mistake=mistake)
                _beyond(f"{rec.name} {dec} {mistake} out", out, r.out64, _bounds(r, "out"))
                if gather:
                    _beyond(f"{rec.name} {mistake} features", feat, r.feat64, _bounds(r, "feat"))


def test_hp_mistakes_land_beyond_the_bounds():
    """One of the three hp products dropped: beyond the bound of `out` on the huge fixture, where a feature error of 2^-12 of a product
    turns the phase of the positional encoding (on the unit fixtures the fp16 rounding of the activations hides it under a max-norm
    rule: printed).  The residue dropped and the residue scale off by a factor of two: beyond the BIAS bound on the bias fixture (the
    max-norm figures are printed next to them)."""
    print()
    r = R.refs("l2x", "d3", "sig3")
    fld, rec = R.field("l2x"), r.rec
    wrong = R.hp_decode(rec, "sig3", R.hp_features(fld, rec, "hp_drop_product"), r.w)
    _beyond("l2x-d3 sig3 one hp product dropped out", wrong, r.out64, {"hp": R.bound(r.out_hp, r.out64)})
    u = R.refs("l2", "d3", "sig3")
    wrong = R.hp_decode(u.rec, "sig3", R.hp_features(R.field("l2"), u.rec, "hp_drop_product"))
    print(f"[indirect sensitivity] l2-d3 sig3 one hp product dropped out: mistake {R.distance(wrong, u.out64):.2e} against bound "
          f"{R.bound(u.out_hp, u.out64):.2e} (hidden under the activations' rounding)")
    for dec in R.BIAS_DECODERS:
        b = R.refs(*R.BIAS_FIXTURE, dec, R.BIAS_ROWS)
        assert b.rec.n >= 4096
        bb = {"hp": R.bias_bound(b.out_hp, b.out64)}
        for mistake in ("hp_no_residue", "hp_scale_x2"):
            wrong = R.hp_decode(b.rec, dec, b.feat_hp, mistake=mistake)
            print(f"[indirect sensitivity] {b.rec.name} {dec} {mistake} max-norm: mistake {R.distance(wrong, b.out64):.2e} against bound "
                  f"{R.bound(b.out_hp, b.out64):.2e}")
            _beyond(f"{b.rec.name} {dec} {mistake} bias", wrong, b.out64, bb, stat=R.bias_distance)
        print(f"[indirect sensitivity] {b.rec.name} {dec} bias: hp yardstick {R.bias_distance(b.out_hp, b.out64):.2e}, f16 fused yardstick "
              f"{R.bias_distance(b.out_h16, b.out64):.2e}")

