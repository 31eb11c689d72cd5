"""The indirect-light kernels (k_vm_app_h16, k_vm_app_dense, k_pack_half of tensoir_amd/csrc/tir_field.hip; k_indirect_fused,
k_indirect_fused_dense, k_indirect_fused_hp of tir_mlp.hip) on their own against the torch restatement (tests/indirect_reference.py) in
float64, through ops._call on buffers of the test's own (sentinels and a guard region behind them) and through the ops wrappers.

Comparison rule (tests/indirect_reference.py; as in tests/test_gpu_decoder_kernels.py): per output tensor and case, distance = max |device
- float64| / max |float64| is at most ten times the distance of the YARDSTICK of the entry's arithmetic class from float64 on the same
fixture, floor ten half-ulps.  Nothing is excluded, every result is finite, every test prints `device d (bound b)`.  No device result
is compared with another kernel's; two launches of the SAME entry are compared bit for bit (row counts, *n_dev, tune_grid, repeats).
tests/test_indirect_cpu.py asserts the fixture conditions and that each mistake such a kernel could make lands beyond these bounds.

Which test covers which entry of include/tensoir_hip.h:
  tir_vm_app_fwd_h16 (plain and dense descriptor)      test_gather (fields, regimes, point classes, idx_map / idx_div, columns >= 27),
                                                       test_launch_invariants
  tir_indirect_fused_fwd (1, 2, 16, 17 lights, dense)  test_fused (rows, addressings, regimes), test_fused_decoders, test_launch_invariants
  tir_indirect_fused_hp_fwd (1, 2, 8 lights)           test_fused_hp (rows, addressings, regimes), test_fused_decoders, test_hp_saturating_weights,
                                                       test_hp_oversized_features, test_hp_bias, test_launch_invariants
  tir_indirect_fused_hp_fwd (9 lights)                 test_hp_refuses_nine_lights
  tir_pack_half, tir_pack_half_checked                 test_pack_half

Bit equality of a launch of n rows with the first n rows of the 1000-row launch holds without exception: a record's sums run inside
one lane pair in an order that does not depend on the tile or the row count.

Measured on an MI355X: see DESIGN 2, "The indirect-light kernels on their own"."""
import ctypes as C

import pytest
import torch

from tests import indirect_reference as R

pytestmark = pytest.mark.gpu

F32 = R.F32
SENTINEL = -12345.678
GUARD = 64
UNSUPPORTED = -1002


def check(label, got, yard, f64, stat=R.distance, bnd=R.bound):
    got = torch.as_tensor(got).detach().cpu()
    assert torch.isfinite(got).all(), label
    d, b = stat(got, f64), bnd(yard, f64)
    print(f"\n[indirect {label}] device {d:.2e} (bound {b:.2e})")
    assert d <= b, (label, d, b)
    return d / b


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Buf:
    """`count` floats of sentinel followed by a guard region, in an allocation of its own (16-byte aligned)."""

    def __init__(self, *shape):
        self.shape, self.count = shape, int(torch.Size(shape).numel())
        self.raw = torch.full((self.count + GUARD,), SENTINEL, dtype=F32, device="cuda")
        assert self.raw.data_ptr() % 16 == 0

    def ptr(self):
        return C.c_void_p(self.raw.data_ptr())

    def get(self, label=""):
        assert bool((bits(self.raw[self.count:]) == bits(torch.tensor([SENTINEL]))).all()), (label, "guard region written")
        return self.raw[:self.count].view(self.shape)


def untouched(t):
    return bool((bits(t) == bits(torch.tensor([SENTINEL]))).all())


class World:
    def __init__(self):
        from tensoir_amd import _lib, ops
        assert torch.cuda.is_available() and _lib.lib().tir_device_check() == 0
        self.ops, self.lib, self._field, self._pm, self._dev, self._table = ops, _lib.lib(), {}, {}, {}, {}

    def field(self, name):
        """The device model of fixture field `name`, loaded from its checkpoint -> (plain descriptor, fp16 shadow, dense descriptor | None)."""
        if name not in self._field:
            import tensoir_amd
            fld = R.field(name)
            m = tensoir_amd.model_from_checkpoint(fld.ck, "cuda", envmap_h=8, envmap_w=16)
            plain, fh = m.packed_field(), m.packed_field_half()
            assert fh is not None and int(plain.n_lights) == fld.n_lights and [int(g) for g in plain.grid] == list(fld.grid)
            assert int(plain.dense_app or 0) == 0
            dense = None
            if fld.n_lights == 1:
                dense = m.packed_field_dense(app=True)
                assert int(dense.dense_app or 0) != 0 and int(dense.dense_app_pitch) == fld.grid[0] + 1, m.dense_app_state()
            if fld.regime != "huge":
                assert m.half_range().ok() == R.half_range_bound(fld)[0] is True, name          # the device's own range guard agrees
            self._field[name] = (m, plain, fh, dense)
        return self._field[name][1:]

    def pm(self, fname, dec, wkind=None):
        key = (R.FIELDS[fname][1] == "huge", dec, wkind)
        if key not in self._pm:
            w, (od, act, _) = R.weights(fname, dec, wkind), R.D.DECODERS[dec]
            seq = torch.nn.Sequential(torch.nn.Linear(R.D.IN, R.D.HID), torch.nn.ReLU(), torch.nn.Linear(R.D.HID, R.D.HID), torch.nn.ReLU(),
                                      torch.nn.Linear(R.D.HID, od))
            with torch.no_grad():
                for i, k in ((0, "0"), (2, "1"), (4, "2")):
                    seq[i].weight.copy_(w["w" + k])
                    seq[i].bias.copy_(w["b" + k])
            self._pm[key] = self.ops.PackedMlp(seq.cuda(), R.D.FEAT, R.D.PE, act)
        return self._pm[key]

    def dev(self, rec):
        """The population's device tensors, once: xyz, rec_map, light_idx, dirs (a head of the population reads prefixes of them)."""
        key = rec.name.split("[")[0]
        if key not in self._dev:
            pop = R.population(rec.field, rec.addr, int(key.rsplit("-", 1)[1]))
            self._dev[key] = (pop.xyz.cuda(), None if pop.rec_map is None else pop.rec_map.cuda(), pop.light_idx.cuda(), pop.dirs.cuda())
        return self._dev[key]

    def table(self, pm, rec):
        key = (id(pm), rec.name.split("[")[0])
        if key not in self._table:
            self._table[key] = self.ops.mlp_aux_table(pm, self.dev(rec)[3])
        return self._table[key]


@pytest.fixture(scope="module")
def world():
    return World()


def run_gather(world, rec, dense=False, mapped=True, n_dev=None):
    """tir_vm_app_fwd_h16 through ops._call on a sentinel-filled [n, 32] buffer."""
    ops = world.ops
    plain, fh, dn = world.field(rec.field)
    xyz, rmap, lidx, _ = world.dev(rec)
    out = Buf(rec.n, 32)
    ops._call("tir_vm_app_fwd_h16", C.byref(dn if dense else plain), C.byref(fh), ops._ptr(xyz), ops._ptr(lidx), ops._ptr(rmap if mapped else None),
              out.ptr(), 32, rec.idx_div, rec.n, ops._ptr(n_dev), ops._stream())
    return out


def run_fused(world, rec, dec, kind, wkind=None, n_dev=None, desc=None):
    """tir_indirect_fused_fwd (kind "f16": plain descriptor, "dense": the dense one) or tir_indirect_fused_hp_fwd (kind "hp") through the
    raw entry on a sentinel-filled [n, out_dim] buffer -> (return code, Buf)."""
    ops = world.ops
    plain, fh, dn = world.field(rec.field)
    pm = world.pm(rec.field, dec, wkind)
    xyz, rmap, lidx, _ = world.dev(rec)
    table = world.table(pm, rec)
    out = Buf(rec.n, pm.out_dim)
    md = C.byref(desc if desc is not None else pm.desc)
    tail = (ops._ptr(xyz), ops._ptr(lidx), ops._ptr(rmap), rec.idx_div, rec.aux_mod, ops._ptr(table), out.ptr(), rec.n, ops._ptr(n_dev), ops._stream())
    if kind == "hp":
        rc = world.lib.tir_indirect_fused_hp_fwd(C.byref(plain), md, *tail)
    else:
        rc = world.lib.tir_indirect_fused_fwd(C.byref(dn if kind == "dense" else plain), C.byref(fh), md, *tail)
    return rc, out


def fused_out(world, rec, dec, kind, **kw):
    rc, out = run_fused(world, rec, dec, kind, **kw)
    assert rc == 0, (rec.name, dec, kind, rc)
    return out.get(rec.name)


YARD = {"f16": "out_h16", "dense": "out_dense", "hp": "out_hp"}


def kinds_of(fname, hp=False):
    if hp:
        return ("hp",)
    return ("f16", "dense") if R.FIELDS[fname][0] == 1 else ("f16",)


# ---- 1. the fp16 gather ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", R.F16_FIELDS)
def test_gather(world, fname):
    """tir_vm_app_fwd_h16 on the plain descriptor (and the dense one of a one-light field): the 1000-record population with every point
    class, whole and per class of at least 8 points; columns >= 27 exactly zero; light indices through idx_map / idx_div."""
    for dense in ((False, True) if R.FIELDS[fname][0] == 1 else (False,)):
        what = f"tir_vm_app_fwd_h16 {'dense' if dense else 'plain'}"
        for addr in ("nomap", "d3", "div5mod7"):
            r = R.refs(fname, addr)
            rec = r.rec
            got = run_gather(world, rec, dense).get(rec.name).cpu()
            assert bool((got[:, R.FEAT:] == 0).all()), (what, rec.name, "columns >= 27")
            yard, f64 = (r.feat_dense if dense else r.feat_h16), r.feat64_raw
            check(f"{what} {rec.name}", got[:, :R.FEAT], yard, f64)
            if addr != "nomap":
                continue
            for c, cname in enumerate(R.POINT_CLASSES):
                sel = rec.ids == c
                if int(sel.sum()) >= 8:
                    check(f"{what} {rec.name} {cname}", got[sel, :R.FEAT], yard[sel], f64[sel])


# ---- 2. the fused kernels --------------------------------------------------------------------------------------------------------------
def fused_cases(world, fname, kinds, rows):
    """Every addressing at 1000 rows, every row count on "d3" and "nomap" (bit-equal to the first rows of the 1000-row launch)."""
    for kind in kinds:
        what = "tir_indirect_fused_hp_fwd" if kind == "hp" else f"tir_indirect_fused_fwd {kind}"
        for addr in R.ADDRESSINGS:
            r = R.refs(fname, addr)
            full = fused_out(world, r.rec, "sig3", kind)
            check(f"{what} {r.rec.name} sig3", full, getattr(r, YARD[kind]), r.out64)
            if addr not in ("d3", "nomap"):
                continue
            for n in rows[:-1]:
                part = fused_out(world, R.head(r.rec, n), "sig3", kind)
                check(f"{what} {r.rec.name} sig3 n{n}", part, getattr(r, YARD[kind])[:n], r.out64[:n])
                assert torch.equal(bits(part), bits(full[:n])), (what, r.rec.name, n, "differs from the first rows of the 1000-row launch")


@pytest.mark.parametrize("fname", R.F16_FIELDS)
def test_fused(world, fname):
    """tir_indirect_fused_fwd: one light (no index read; shadow taps and dense volume), 2 and 16 lights (rows staged in LDS), 17 lights
    (rows from global memory), the small and the large regime; all row counts and addressings."""
    fused_cases(world, fname, kinds_of(fname), R.ROWS_F16)


@pytest.mark.parametrize("fname", [f for f in R.HP_FIELDS if R.FIELDS[f][1] != "huge"])
def test_fused_hp(world, fname):
    """tir_indirect_fused_hp_fwd with 1, 2 and 8 lights, the small and the large regime; all row counts and addressings."""
    fused_cases(world, fname, ("hp",), R.ROWS_HP)


@pytest.mark.parametrize("dec", R.DECODERS[1:])
def test_fused_decoders(world, dec):
    """out_dim 1 and 4 and the tanh decoder on every kernel and light arm."""
    for fname in ("l1", "l2", "l8", "l16", "l17"):
        r = R.refs(fname, "d3", dec)
        for kind in kinds_of(fname) + (("hp",) if fname in R.HP_FIELDS else ()):
            check(f"fused {kind} {r.rec.name} {dec}", fused_out(world, r.rec, dec, kind), getattr(r, YARD[kind]), r.out64)


def test_hp_refuses_nine_lights(world):
    """More than 8 lights: TIR_ERR_UNSUPPORTED, and the output buffer keeps every sentinel."""
    for addr in ("nomap", "d3"):
        rc, out = run_fused(world, R.population("l9", addr), "sig3", "hp")
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED, rc
        assert untouched(out.get("l9"))


@pytest.mark.parametrize("dec", ["sig3", "sig4"])
def test_hp_saturating_weights(world, dec):
    """Decoder weights with max |W0| and max |W1| in [8, 16): the e4m3 residue saturates at 448."""
    for fname in ("l2", "l8"):
        r = R.refs(fname, "d3", dec, wkind="saturating")
        check(f"tir_indirect_fused_hp_fwd {r.rec.name} {dec} saturating weights", fused_out(world, r.rec, dec, "hp", wkind="saturating"), r.out_hp, r.out64)


def test_hp_oversized_features(world):
    """Raw features beyond 448 (the residue operand's clamp) and beyond 65504 (the feature clamp of the fused entries)."""
    for addr, dec in (("d3", "sig3"), ("nomap", "sig4"), ("d16", "tanh3")):
        r = R.refs("l2x", addr, dec)
        check(f"tir_indirect_fused_hp_fwd {r.rec.name} {dec}", fused_out(world, r.rec, dec, "hp"), r.out_hp, r.out64)


@pytest.mark.parametrize("dec", R.BIAS_DECODERS)
def test_hp_bias(world, dec):
    """The mean signed deviation from float64 per output channel over 4096 records sharing a decoder: at most ten times the hp yardstick's
    own (tests/test_indirect_cpu.py: the emulation without the weight residue, or with its scale doubled, lands beyond this bound)."""
    r = R.refs(*R.BIAS_FIXTURE, dec, R.BIAS_ROWS)
    got = fused_out(world, r.rec, dec, "hp")
    check(f"tir_indirect_fused_hp_fwd {r.rec.name} {dec}", got, r.out_hp, r.out64)
    check(f"tir_indirect_fused_hp_fwd {r.rec.name} {dec} bias", got, r.out_hp, r.out64, stat=R.bias_distance, bnd=R.bias_bound)


# ---- 3. what must not depend on the launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gather", "gather dense", "f16", "dense", "hp"])
def test_launch_invariants(world, kind):
    """Two launches give equal bits; *n_dev of n - 3, 0 and above n: rows below min(n, *n_dev) carry the bits of the full call, every later
    row and the guard region keep their bits; tune_grid 1 and 2 on a copied TirMlp descriptor (one workgroup runs three or four tiles
    of the 1000 rows) give the bits of the default launch."""
    fname = "l1" if kind in ("gather dense", "dense") else "l8"
    for addr in ("d3", "nomap"):
        pop = R.population(fname, addr)
        if kind.startswith("gather"):
            run = lambda rec, **kw: run_gather(world, rec, dense=kind.endswith("dense"), **kw).get(rec.name)
        else:
            run = lambda rec, **kw: fused_out(world, rec, "sig4", kind, **kw)
        full = run(pop)
        assert torch.equal(bits(run(pop)), bits(full)), (kind, addr, "two launches differ")
        for n in (257, 385):
            rec = R.head(pop, n)
            for v in (n - 3, 0, n + 5):
                n_dev = torch.tensor([v], dtype=torch.int32, device="cuda")
                part = run(rec, n_dev=n_dev)
                k = min(n, v)
                assert torch.equal(bits(part[:k]), bits(full[:k])), (kind, addr, n, v)
                assert untouched(part[k:]), (kind, addr, n, v, "rows past *n_dev written")
        if not kind.startswith("gather"):
            pm = world.pm(fname, "sig4")
            for grid in (1, 2):
                desc = type(pm.desc).from_buffer_copy(pm.desc)
                desc.tune_grid = grid
                assert torch.equal(bits(run(pop, desc=desc)), bits(full)), (kind, addr, "tune_grid", grid)
        print(f"\n[indirect {kind} {pop.name}] repeat, *n_dev and tune_grid launches bit-equal, later rows untouched")


# ---- 4. the fp16 shadow ----------------------------------------------------------------------------------------------------------------
def _half_tables():
    gen = torch.Generator().manual_seed(R._seed("pack_half"))
    edge = torch.tensor([0.0, -0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                         2.0 ** -25 * 1.0001, -2.0 ** -14, 2.0 ** -14 - 2.0 ** -26, 5.9e-8, 65504.0, -65504.0, 65504.0 + 0.01, 65519.9, 65520.0, -65520.0,
                         7e4, -3e38, float("inf"), float("-inf"), 1e-30, -1e-40], dtype=F32)
    lens = (25, 1, 7, 8, 9, 2047, 8193, 20000)                 # none but one a multiple of the 8-element vector; one past a workgroup's 8192
    tabs = []
    for i, n in enumerate(lens):
        t = torch.randn(n, generator=gen) * (10.0 ** (i - 4))
        k = min(n, edge.numel())
        t[:k] = edge[:k]
        tabs.append(t)
    return tabs


def test_pack_half(world):
    """tir_pack_half / tir_pack_half_checked bit-exact against torch.clamp(x, -65504, 65504).half(): ties, subnormals, +-65504 + eps, +-inf;
    table lengths that are no multiple of the vector width; eight tables in one launch; a scan-only table; a NaN reported as NaN in
    absmax (its copy is not specified: every other element of that table still matches)."""
    ops = world.ops
    tabs = [t.cuda() for t in _half_tables()]
    assert len(tabs) == 8                                       # TIR_HALF_MAX_JOBS
    want = [torch.clamp(t, -65504.0, 65504.0).half() for t in tabs]
    copies, absmax = ops.pack_half(tabs)
    for i, (c, w, t) in enumerate(zip(copies, want, tabs)):
        assert torch.equal(c.view(torch.int16), w.view(torch.int16)), ("tir_pack_half_checked", i)
        assert float(absmax[i]) == float(t.abs().max()), (i, float(absmax[i]))
    k = len(tabs)
    outs = [torch.full((t.numel() + 8,), 7.0, dtype=torch.float16, device="cuda") for t in tabs]
    srcs = (C.c_void_p * k)(*[t.data_ptr() for t in tabs])
    dsts = (C.c_void_p * k)(*[o.data_ptr() for o in outs])
    cnts = (C.c_int64 * k)(*[t.numel() for t in tabs])
    ops._call("tir_pack_half", srcs, dsts, cnts, k, ops._stream())
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o[:w.numel()].view(torch.int16), w.view(torch.int16)) and bool((o[w.numel():] == 7.0).all()), ("tir_pack_half", i)
    # a scan-only table and a NaN
    nan_tab = tabs[5].clone()
    nan_tab[1234] = float("nan")
    copies, absmax = ops.pack_half([tabs[2], nan_tab], scan=(tabs[6], tabs[3]))
    assert len(copies) == 2 and float(absmax[0]) == float(tabs[2].abs().max()) and bool(torch.isnan(absmax[1]))
    assert float(absmax[2]) == float(tabs[6].abs().max()) and float(absmax[3]) == float(tabs[3].abs().max())
    keep = ~torch.isnan(nan_tab)
    assert torch.equal(copies[1][keep].view(torch.int16), want[5][keep].view(torch.int16))
    print(f"\n[indirect tir_pack_half] 8 tables of {[t.numel() for t in tabs]} elements bit-exact; NaN element copied as {float(copies[1][1234])}")
