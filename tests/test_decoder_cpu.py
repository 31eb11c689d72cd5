"""tests/decoder_reference.py pinned without a GPU: the restatement against the oracle and against autograd in float64, the conditions
every fixture of tests/test_gpu_decoder_kernels.py has to meet, the yardsticks (the distance of the float32 restatement and of each
arithmetic-class emulation from float64, printed; DESIGN 2, "The decoder kernels on their own" holds them beside the device's), and
the sensitivity of the comparison rule: each mistake a decoder kernel could make, applied to the restatement, lands beyond the bound
the GPU test applies to that tensor on that fixture."""
import pytest
import torch

from oracle import tensoir_oracle as O
from tests import decoder_reference as R

F32, F64 = R.F32, R.F64


def gpu_fixtures():
    """Every fixture tests/test_gpu_decoder_kernels.py runs a forward or a backward on (the edge fixtures apart)."""
    out = []
    for dec in R.DECODERS:
        out += [R.make_fixture(dec, n) for n in R.ROWS]
        out += [R.make_fixture(dec, 700, kind, rows) for kind, rows in R.ADDRESSINGS]
        out.append(R.make_fixture(dec, 257, group="large"))
        out.append(R.large_fixture(dec, 16385))
    out.append(R.large_fixture("sig4", 65537))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec", list(R.DECODERS))
def test_restatement_equals_the_oracle(dec):
    for kind, rows in R.ADDRESSINGS:
        fx = R.make_fixture(dec, 257, kind, rows)
        r = R.forward(fx, F64)
        w = {k: v.double() for k, v in fx.w.items()}
        ai = R.aux_rows(fx.n, fx.aux_map, fx.aux_mod)
        x = O.mlp_input(fx.feat.double(), fx.aux.double()[ai], 2, 2)
        z = O.mlp3(w, x)
        want = torch.tanh(z) if fx.act == 1 else torch.sigmoid(z)
        assert x.shape == (257, R.IN) and float((r.x - x).abs().max()) <= 1e-12
        assert float((r.out - want).abs().max()) <= 1e-12 and float((r.z3 - z).abs().max()) <= 1e-12
        x160 = R.inputs160(fx, F64)
        assert x160.shape == (257, R.XPAD) and torch.equal(x160[:, :R.IN], x) and bool((x160[:, R.IN:] == 0).all())
        t = R.forward(fx, F64, table=True)
        for name in ("out", "h1", "h2", "z1", "z2", "z3"):
            assert float((getattr(t, name) - getattr(r, name)).abs().max()) <= 1e-12, name


def test_addressing_rule():
    m = torch.tensor([7, 0, 12, 5, 3], dtype=torch.int32)
    assert R.aux_rows(5, None, 0).tolist() == [0, 1, 2, 3, 4]
    assert R.aux_rows(5, None, 3).tolist() == [0, 1, 2, 0, 1]
    assert R.aux_rows(5, m, 0).tolist() == [7, 0, 12, 5, 3]
    assert R.aux_rows(5, m, 5).tolist() == [2, 0, 2, 0, 3]
    assert len(R.AUX_COLS) == 15 and len(R.FEAT_COLS) == 135
    # every entry is held to the yardstick of its own class ("bf16" holds "f16" as a substring: the lookup must not go by that)
    assert all(R.fwd_class(e) == c for e, c in R.FORWARD_ENTRIES.items())
    assert R.fwd_class("tir_mlp_train_fwd") == "exact" and R.fwd_class("tir_mlp_train_fwd_multi_bf16x3") == "split"
    assert R.fwd_class("tir_mlp_train_fwd_auxtab_bf16x3") == "split_table"


@pytest.mark.parametrize("dec", list(R.DECODERS))
def test_backward_equals_autograd(dec):
    fx = R.make_fixture(dec, 257)
    w = {k: v.double() for k, v in fx.w.items()}
    feat = fx.feat.double().requires_grad_(True)
    x = O.mlp_input(feat, fx.aux.double(), 2, 2)
    z1 = x @ w["w0"].T + w["b0"]
    z1.retain_grad()
    h1 = torch.relu(z1)
    z2 = h1 @ w["w1"].T + w["b1"]
    z2.retain_grad()
    h2 = torch.relu(z2)
    z3 = h2 @ w["w2"].T + w["b2"]
    z3.retain_grad()
    y = torch.tanh(z3) if fx.act == 1 else torch.sigmoid(z3)
    (y * fx.g_out.double()).sum().backward()
    b = R.backward(fx, y.detach(), h1.detach(), h2.detach(), F64)
    assert float((b.g_feat[:, :27] - feat.grad).abs().max()) <= 1e-10
    assert float((b.dz1 - z1.grad).abs().max()) <= 1e-10 and float((b.dz2 - z2.grad).abs().max()) <= 1e-10
    assert float((b.dz3[:, :fx.out_dim] - z3.grad).abs().max()) <= 1e-10
    assert bool((b.g_feat[:, 27:] == 0).all()) and bool((b.dz3[:, fx.out_dim:] == 0).all())


# ---- fixture conditions --------------------------------------------------------------------------------------------------------------
def test_fixture_conditions():
    """Output columns spread (standard deviation >= 0.1 over the rows; the ROWS fixtures are prefixes of one 700-row population, so a
    prefix too short to have a deviation -- fewer than 31 rows -- is covered by its population), 20 % .. 80 % of the hidden units active in
    each layer, every aux_map fixture uses row 0 and the last row, every aux_mod fixture wraps."""
    for fx in gpu_fixtures():
        r = R.forward_refs(fx)["f64"]
        if fx.n >= 31:
            assert float(r.out.std(0).min()) >= 0.1, (fx.name, r.out.std(0))
        if fx.n >= 31:
            for h in (r.h1, r.h2):
                frac = float((h > 0).double().mean())
                assert 0.2 <= frac <= 0.8, (fx.name, frac)
        if fx.aux_map is not None:
            ai = R.aux_rows(fx.n, fx.aux_map, fx.aux_mod)
            assert int(ai.min()) == 0 and int(ai.max()) == fx.aux.shape[0] - 1, fx.name
            assert len(set(ai.tolist())) < fx.n                                       # repeats
        if fx.aux_mod > 0:
            raw = fx.aux_map.long() if fx.aux_map is not None else torch.arange(fx.n)
            assert int(raw.max()) >= fx.aux_mod, fx.name
        if fx.kind == "map_mod":
            assert int(fx.aux_map.max()) == 10 * fx.aux_mod - 1
        assert bool(torch.isfinite(r.out).all())
    assert float(R.decoder("sig4")["b0"].abs().max()) > 1.5
    for dec in ("sig3", "tanh3", "sig4"):
        e = R.edge_fixture(dec)
        assert bool((e.h2[0] == 0).all()) and bool((e.h1[1] > 0).all()) and bool((e.h2[1] > 0).all())
        assert bool((e.h1[2, 0::3] == 0).all()) and bool(torch.signbit(e.h2[3, 1::3]).all()) and 0 < float(e.h1[4, 0]) < 2e-30
        assert bool((e.g_out[:, 1] == 0).all()) and float(e.feat.abs().max()) > 90


# ---- yardsticks ----------------------------------------------------------------------------------------------------------------------
def test_yardsticks_are_printed():
    """Distance from float64 of the float32 restatement and of each emulation, worst over the fixtures, per tensor."""
    worst = {}
    print()
    for fx in gpu_fixtures() + [R.edge_fixture(d) for d in ("sig3", "tanh3", "sig4")]:
        line = []
        refs = [] if fx.name.endswith("edge") else [("forward", R.forward_refs(fx), ("exact", "split", "split_table", "bf16", "f16"), R.FWD_TENSORS)]
        refs.append(("backward", R.backward_refs(fx), ("exact", "split"), R.BWD_TENSORS))
        for what, r, classes, tensors in refs:
            for cls in classes:
                ds = [R.distance(getattr(r[cls], t), getattr(r["f64"], t)) for t in tensors]
                line.append(f"{what[0]}.{cls} " + "/".join(f"{d:.1e}" for d in ds))
                for t, d in zip(tensors, ds):
                    worst[(what, cls, t)] = max(worst.get((what, cls, t), 0.0), d)
        print(f"[decoder yardstick] {fx.name} (out/h1/h2, g_feat/dz1/dz2/dz3): " + "; ".join(line))
    for (what, cls, t), d in sorted(worst.items()):
        print(f"[decoder yardstick] {what:8s} {cls:11s} {t:6s} {d:.2e}")
    assert worst[("forward", "exact", "out")] < 1e-5 and worst[("forward", "split", "out")] < 1e-4
    assert worst[("forward", "split", "out")] < worst[("forward", "f16", "out")] < worst[("forward", "bf16", "out")]


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------------
def _beyond(label, wrong, f64, bounds):
    d = R.distance(wrong, f64)
    worst = max(bounds.values())
    print(f"[decoder sensitivity] {label}: mistake {d:.2e}, bounds " + ", ".join(f"{k} {v:.2e}" for k, v in bounds.items()))
    assert d > worst, (label, d, bounds)


def _fwd_bounds(fx, t, classes):
    f = R.forward_refs(fx)
    return {c: R.bound(getattr(f[c], t), getattr(f["f64"], t)) for c in classes}


def _bwd_bounds(fx, t, classes=("exact", "split")):
    b = R.backward_refs(fx)
    return {c: R.bound(getattr(b[c], t), getattr(b["f64"], t)) for c in classes}


ALL = ("exact", "split", "split_table", "bf16", "f16")


@pytest.mark.parametrize("dec", list(R.DECODERS))
def test_forward_mistakes_land_beyond_the_bounds(dec):
    print()
    fx = R.make_fixture(dec, 700, "map_mod", 16)
    f64 = R.forward_refs(fx)["f64"]
    for cls, table in (("split", False), ("split_table", True)):
        wrong = R.forward(fx, F32, "split", table=table, mistake="drop_product")
        for t in R.FWD_TENSORS:
            _beyond(f"{fx.name} one split product dropped, {cls} {t}", getattr(wrong, t), getattr(f64, t), _fwd_bounds(fx, t, (cls,)))
    for mistake, kinds in (("pe_swap", ("rows",)), ("w1_swap", ("rows",)), ("aux_off_by_one", ("rows", "map", "map_mod", "mod")),
                           ("mod_before_map", ("map_mod",))):
        for kind in kinds:
            for rows in ((0,) if kind == "rows" else (16, 100)):
                fx = R.make_fixture(dec, 700, kind, rows)
                f64 = R.forward_refs(fx)["f64"]
                wrong = R.forward(fx, F64, mistake=mistake)
                for t in (("out", "h2") if mistake == "w1_swap" else R.FWD_TENSORS):
                    _beyond(f"{fx.name} {mistake} {t}", getattr(wrong, t), getattr(f64, t), _fwd_bounds(fx, t, ALL))


@pytest.mark.parametrize("dec", list(R.DECODERS))
def test_backward_mistakes_land_beyond_the_bounds(dec):
    print()
    fx = R.make_fixture(dec, 257)
    s, f64 = R.saved(fx), R.backward_refs(fx)["f64"]
    wrong = R.backward(fx, *s, F32, "split", mistake="drop_product")
    for t in ("g_feat", "dz1", "dz2"):
        _beyond(f"{fx.name} one split product dropped {t}", getattr(wrong, t), getattr(f64, t), _bwd_bounds(fx, t, ("split",)))
    for mistake, tensors in (("other_act", R.BWD_TENSORS), ("w1_swap", ("g_feat", "dz1"))):
        wrong = R.backward(fx, *s, F64, mistake=mistake)
        for t in tensors:
            _beyond(f"{fx.name} {mistake} {t}", getattr(wrong, t), getattr(f64, t), _bwd_bounds(fx, t))
    if fx.out_dim < 4:                    # float64 is identically zero there: the rule asks for exact zeros
        wrong = R.backward(fx, *s, F64, mistake="dz3_unzeroed")
        assert bool((f64.dz3[:, fx.out_dim:] == 0).all()) and bool((wrong.dz3[:, fx.out_dim] != 0).any())


@pytest.mark.parametrize("dec", ["sig3", "tanh3", "sig4"])
def test_mask_mistake_on_exact_zeros(dec):
    print()
    fx = R.edge_fixture(dec)
    f64 = R.backward_refs(fx)["f64"]
    wrong = R.backward(fx, *R.saved(fx), F64, mistake="mask_ge")
    for t in ("g_feat", "dz1", "dz2"):
        _beyond(f"{fx.name} mask h >= 0 {t}", getattr(wrong, t), getattr(f64, t), _bwd_bounds(fx, t))
    assert bool((f64.dz2[0] == 0).all()) and bool((f64.dz1[0] == 0).all()) and bool((f64.g_feat[0] == 0).all())
    assert bool((f64.dz3[5:7] == 0).all()) and bool((f64.dz3[:, 1] == 0).all())
