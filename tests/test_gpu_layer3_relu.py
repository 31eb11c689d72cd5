"""Layer 3 of the decoder kernels (tir_mlp.hip, layer3_relu_mfma: ReLU of the 64 layer-2 accumulators of a lane on the integer pipe, in
place, then the 4x4x1 matrix instructions) through ops.mlp (split-bf16), ops.mlp_multi and the fused indirect entry (the shadow-tap
kernel and the dense-volume kernel on the 20 x 24 x 28 one-light field).

The decoders are decoder_reference's with layer 2 re-drawn so that EVERY row has units whose pre-activation is exactly zero (w1 row
zero, b1 = 0), exactly +1 and exactly -1 (w1 row zero, b1 = +-1) next to the mixed ones: the sign test of the ReLU sees 0, clearly
positive and clearly negative values in every lane.  Compared with the float64 evaluation of tests/decoder_reference.py /
tests/indirect_reference.py under those tests' own rule (ten times the yardstick's distance, floor ten half-ulps).

One more case: a hidden unit with b1 = -inf.  Its ReLU is 0 (as torch.relu's), the outputs are finite and meet the same rule; the
earlier form of layer 3 (x + |x|) gave NaN there."""
import types

import pytest
import torch

from tests import decoder_reference as D
from tests import indirect_reference as IR

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 33, 257)
DECS = ("sig1", "sig3", "sig4")               # out_dim 1, 3, 4


def layer2_pattern(w, neg_inf=False):
    """Units u % 8 == 0 / 1 / 2: w1 row zero and b1 = 0 / +1 / -1; with neg_inf unit 5 gets b1 = -inf."""
    w = {k: v.clone() for k, v in w.items()}
    u = torch.arange(D.HID)
    for r, b in ((0, 0.0), (1, 1.0), (2, -1.0)):
        w["w1"][u % 8 == r] = 0.0
        w["b1"][u % 8 == r] = b
    if neg_inf:
        w["b1"][5] = float("-inf")
    return w


def check(label, got, yard, f64):
    got = torch.as_tensor(got).detach().cpu()
    assert torch.isfinite(got).all(), label
    d, b = D.distance(got, f64), D.bound(yard, f64)
    print(f"\n[layer3 {label}] device {d:.2e} (bound {b:.2e})")
    assert d <= b, (label, d, b)


class World:
    def __init__(self):
        from tensoir_amd import _lib, ops
        assert torch.cuda.is_available() and _lib.lib().tir_device_check() == 0
        self.ops, self._pm, self._field, self._fx = ops, {}, None, {}

    def pm(self, dec, neg_inf=False):
        if (dec, neg_inf) not in self._pm:
            w, (od, act, _) = layer2_pattern(D.decoder(dec), neg_inf), D.DECODERS[dec]
            seq = torch.nn.Sequential(torch.nn.Linear(D.IN, D.HID), torch.nn.ReLU(), torch.nn.Linear(D.HID, D.HID), torch.nn.ReLU(),
                                      torch.nn.Linear(D.HID, od))
            with torch.no_grad():
                for i, k in ((0, "0"), (2, "1"), (4, "2")):
                    seq[i].weight.copy_(w["w" + k])
                    seq[i].bias.copy_(w["b" + k])
            self._pm[(dec, neg_inf)] = (self.ops.PackedMlp(seq.cuda(), D.FEAT, D.PE, act), w)
        return self._pm[(dec, neg_inf)]

    def fixture(self, dec, n, neg_inf=False):
        """decoder_reference's 257-row fixture of the decoder (its first n rows) with the patterned layer 2, and its references, once."""
        if (dec, n, neg_inf) not in self._fx:
            # a copy of the shared fixture WITHOUT the references another test may have cached on it (they belong to its weights)
            fx = types.SimpleNamespace(**{k: v for k, v in D.make_fixture(dec, n).__dict__.items() if not k.startswith("_")})
            fx.w, fx.name = self.pm(dec, neg_inf)[1], f"{fx.name}-l2pattern{'-inf' if neg_inf else ''}"
            z2 = D.forward(fx, D.F64).z2
            for r, v in ((0, 0.0), (1, 1.0), (2, -1.0)):            # the fixture condition: exact 0, +1, -1 in every row
                assert bool((z2[:, torch.arange(D.HID) % 8 == r] == v).all()), (fx.name, r)
            self._fx[(dec, n, neg_inf)] = fx
        return self._fx[(dec, n, neg_inf)]

    def field(self):
        """The device model of indirect_reference's one-light 20 x 24 x 28 field -> (plain descriptor, fp16 shadow, dense descriptor)."""
        if self._field is None:
            import tensoir_amd
            fld = IR.field("l1")
            m = tensoir_amd.model_from_checkpoint(fld.ck, "cuda", envmap_h=8, envmap_w=16)
            plain, fh, dense = m.packed_field(), m.packed_field_half(), m.packed_field_dense(app=True)
            assert fh is not None and int(plain.dense_app or 0) == 0 and int(dense.dense_app or 0) != 0
            self._field = (m, plain, fh, dense)
        return self._field[1:]


@pytest.fixture(scope="module")
def world():
    return World()


def feat_rows(fx):
    rows = torch.zeros((fx.n, 32), dtype=D.F32)
    rows[:, :D.FEAT] = fx.feat
    return rows.cuda()


def run_mlp(world, fx, neg_inf=False):
    return world.ops.mlp(world.pm(fx.dec, neg_inf)[0], feat_rows(fx), fx.aux.cuda(), impl="bf16x3")


def run_multi(world, fxs, neg_inf=False):
    return world.ops.mlp_multi([(world.pm(fx.dec, neg_inf)[0], feat_rows(fx), fx.aux.cuda(), None) for fx in fxs])


def fused(world, rec, dec, kind, neg_inf=False):
    """ops.indirect_fused on the plain descriptor (kind "f16": k_indirect_fused) or the dense one ("dense": k_indirect_fused_dense)."""
    plain, fh, dense = world.field()
    pm = world.pm(dec, neg_inf)[0]
    return world.ops.indirect_fused(dense if kind == "dense" else plain, fh, pm, rec.xyz.cuda(), rec.light_idx.cuda(), rec.rec_map.cuda(),
                                    rec.idx_div, rec.dirs.cuda(), rec.aux_mod)


def fused_refs(world, rec, dec, neg_inf=False):
    fld, w = IR.field("l1"), world.pm(dec, neg_inf)[1]
    out64 = IR.forward(fld, rec, dec, D.F64, w=w)[1]
    return out64, {"f16": IR.f16_decode(rec, dec, IR.h16_features(fld, rec), w), "dense": IR.f16_decode(rec, dec, IR.dense_features(fld, rec), w)}


@pytest.mark.parametrize("dec", DECS)
@pytest.mark.parametrize("n", ROWS)
def test_mlp(world, dec, n):
    """ops.mlp (tir_mlp_fwd_bf16x3) and ops.mlp_multi (one job, and the decoder next to a four-output one) on the patterned decoder."""
    fx = world.fixture(dec, n)
    refs = D.forward_refs(fx)
    check(f"mlp {fx.name}", run_mlp(world, fx), refs["split"].out, refs["f64"].out)
    other = world.fixture("sig4" if dec != "sig4" else "sig1", n)
    single, pair = run_multi(world, [fx]), run_multi(world, [fx, other])
    check(f"mlp_multi 1 {fx.name}", single[0], refs["split"].out, refs["f64"].out)
    check(f"mlp_multi 2 {fx.name}", pair[0], refs["split"].out, refs["f64"].out)
    orefs = D.forward_refs(other)
    check(f"mlp_multi 2 {other.name}", pair[1], orefs["split"].out, orefs["f64"].out)


@pytest.mark.parametrize("dec", DECS)
@pytest.mark.parametrize("n", ROWS)
def test_fused(world, dec, n):
    """The fused indirect entry on the 20 x 24 x 28 one-light field: shadow-tap kernel and dense-volume kernel."""
    rec = IR.head(IR.population("l1", "d3"), n)
    out64, yard = fused_refs(world, rec, dec)
    for kind in ("f16", "dense"):
        check(f"fused {kind} {rec.name} {dec}", fused(world, rec, dec, kind), yard[kind], out64)


def test_neg_inf_unit(world):
    """b1 = -inf on one hidden unit: ReLU gives 0, every output is finite and within the rule of the float64 evaluation (torch.relu)."""
    n, dec = 257, "sig3"
    fx = world.fixture(dec, n, neg_inf=True)
    refs = D.forward_refs(fx)
    assert torch.isfinite(refs["f64"].out).all() and bool((refs["f64"].z2[:, 5] == float("-inf")).all())
    check(f"mlp {fx.name}", run_mlp(world, fx, True), refs["split"].out, refs["f64"].out)
    check(f"mlp_multi {fx.name}", run_multi(world, [fx], True)[0], refs["split"].out, refs["f64"].out)
    rec = IR.head(IR.population("l1", "d3"), n)
    out64, yard = fused_refs(world, rec, dec, True)
    assert torch.isfinite(out64).all()
    for kind in ("f16", "dense"):
        check(f"fused {kind} {rec.name} {dec} -inf", fused(world, rec, dec, kind, True), yard[kind], out64)
