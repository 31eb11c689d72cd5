"""The decoder kernels (tensoir_amd/csrc/tir_mlp.hip) on their own against the torch restatement (tests/decoder_reference.py) in
float64, forward and backward, through the ops wrappers -- and through ops._call wherever a test needs its own output buffers
(sentinels, guard regions, a copied descriptor) or an arm no wrapper reaches.

Comparison rule (tests/decoder_reference.py; as in tests/test_gpu_march_kernels.py): per output tensor and case, distance = max |device
- float64| / max |float64| is at most ten times the distance of the entry's YARDSTICK from float64 on the same fixture, floor ten
half-ulps: the float32 restatement for the fp32-operand entries, the split-bf16 / single-bf16 / single-fp16 emulation for the others.
Where float64 is identically zero the device is exactly zero.  Nothing is excluded.  Every test prints `device d (bound b)`.
tests/test_decoder_cpu.py asserts the fixture conditions and that each mistake a kernel could make lands beyond these bounds.
Feature columns >= 27 hold NaN in every layout that has them (tests 1, 3, 6, 8): no entry here reads a pad column into a product.

Which test covers which entry of include/tensoir_hip.h:
  tir_mlp_fwd, _valu, _bf16x3, _bf16, _auxtab_bf16x3, _auxtab_f16    test_forward (rows, layouts, addressings), test_n_dev, test_tune_grid
  tir_mlp_aux_table                                                  test_aux_table
  tir_mlp_train_fwd, _bf16x3, _auxtab_bf16x3, _multi_bf16x3          test_training_forward, test_n_dev
  tir_mlp_fwd_multi_bf16x3, _multi_auxtab_bf16x3                     test_multi_forward, test_persistent_loop_multi
  tir_mlp_inputs                                                     test_inputs
  tir_mlp_bwd, tir_mlp_bwd_bf16x3                                    test_backward_alone, test_backward_edges, test_persistent_loop
  tir_mlp_bwd_multi_bf16x3                                           test_multi_backward, test_persistent_loop_multi
  the persistent loop of tir_mlp_fwd, tir_mlp_train_fwd              test_persistent_loop (65,537 rows: 257 tiles on 256 workgroups)
  ops.mlp's choice between the direct and the table launch           test_wrapper_routes

Measured on an MI355X: see DESIGN 2, "The decoder kernels on their own"."""
import ctypes as C

import pytest
import torch

from tests import decoder_reference as R

pytestmark = pytest.mark.gpu

F32, F64 = R.F32, R.F64
SENTINEL = -12345.678
GUARD = 64


def check(label, got, yard, f64):
    got = torch.as_tensor(got).detach().cpu()
    assert torch.isfinite(got).all(), label
    if not bool((torch.as_tensor(f64) != 0).any()):
        print(f"\n[decoder {label}] device exactly zero (float64 is)")
        assert bool((got == 0).all()), (label, "float64 is identically zero")
        return
    d, b = R.distance(got, f64), R.bound(yard, f64)
    print(f"\n[decoder {label}] device {d:.2e} (bound {b:.2e})")
    assert d <= b, (label, d, b)


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


def layout(feat, name):
    """feat [n, 27] -> device rows in the layout, NaN in every column >= 27 -> (tensor [n, stride], stride)."""
    n = feat.shape[0]
    stride = int(name[1:3])
    rows = torch.full((n, stride), float("nan"), dtype=F32)
    rows[:, :R.FEAT] = feat
    if name.endswith("+1"):
        hold = torch.empty(n * stride + 1, dtype=F32, device="cuda")
        hold[1:] = rows.reshape(-1).cuda()
        d = hold[1:].view(n, stride)
        assert d.data_ptr() % 16 == 4
    else:
        d = rows.cuda()
        assert d.data_ptr() % 16 == 0
    return d, stride


class World:
    def __init__(self):
        from tensoir_amd import _lib, ops
        assert torch.cuda.is_available() and _lib.lib().tir_device_check() == 0
        self.ops, self._pm, self._pb, self._dev = ops, {}, {}, {}

    def pm(self, dec, group="unit"):
        if (dec, group) not in self._pm:
            w, (od, act, _) = R.decoder(dec, group), R.DECODERS[dec]
            seq = torch.nn.Sequential(torch.nn.Linear(R.IN, R.HID), torch.nn.ReLU(), torch.nn.Linear(R.HID, R.HID), torch.nn.ReLU(),
                                      torch.nn.Linear(R.HID, od))
            with torch.no_grad():
                for i, k in ((0, "0"), (2, "1"), (4, "2")):
                    seq[i].weight.copy_(w["w" + k])
                    seq[i].bias.copy_(w["b" + k])
            self._pm[(dec, group)] = self.ops.PackedMlp(seq.cuda(), R.FEAT, R.PE, act)
        return self._pm[(dec, group)]

    def pb(self, dec, group="unit"):
        if (dec, group) not in self._pb:
            w = R.decoder(dec, group)
            self._pb[(dec, group)] = self.ops.pack_mlp_bwd(w["w0"].cuda(), w["w1"].cuda(), w["w2"].cuda(), R.FEAT, R.PE)
        return self._pb[(dec, group)]

    def dev(self, fx, group="unit"):
        """aux, aux_map and the aux table of a fixture on the device, once."""
        if fx.name not in self._dev:
            aux = fx.aux.cuda()
            self._dev[fx.name] = (aux, None if fx.aux_map is None else fx.aux_map.cuda(), self.ops.mlp_aux_table(self.pm(fx.dec, group), aux))
        return self._dev[fx.name]


@pytest.fixture(scope="module")
def world():
    return World()


def group_of(fx):
    return "large" if fx.name.endswith("large") else "unit"


def run_forward(world, entry, fx, lay="s32", n_dev=None, save=False, desc=None, feat=None):
    """One single-decoder forward entry through ops._call on sentinel-filled buffers -> (out, h1, h2) Bufs."""
    ops = world.ops
    pm = world.pm(fx.dec, group_of(fx))
    aux, amap, table = world.dev(fx, group_of(fx))
    fd, stride = feat if feat is not None else layout(fx.feat, lay)
    out = Buf(fx.n, fx.out_dim)
    h1, h2 = (Buf(fx.n, R.HID), Buf(fx.n, R.HID)) if save else (None, None)
    args = [C.byref(desc if desc is not None else pm.desc), ops._ptr(fd), stride, ops._ptr(table if "auxtab" in entry else aux),
            ops._ptr(amap), fx.aux_mod, out.ptr()]
    if save:
        args += [h1.ptr(), h2.ptr()]
    ops._call(entry, *args, fx.n, ops._ptr(n_dev), ops._stream())
    return out, h1, h2


def forward_cases(dec):
    """(label, fixture, layout): ROWS at stride 32, the |feat| ~ 100 group, the five layouts at 257 rows, the addressings at 700."""
    cases = [(f"n{n}", R.make_fixture(dec, n), "s32") for n in R.ROWS]
    cases.append(("large", R.make_fixture(dec, 257, group="large"), "s32"))
    cases += [(lay, R.make_fixture(dec, 257), lay) for lay in R.LAYOUTS[1:]]
    cases += [(f"{kind}{rows}", R.make_fixture(dec, 700, kind, rows), "s32") for kind, rows in R.ADDRESSINGS[1:]]
    return cases


# ---- 1. forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec", list(R.DECODERS))
@pytest.mark.parametrize("entry", list(R.FORWARD_ENTRIES))
def test_forward(world, entry, dec):
    """Every forward entry x every decoder: ROWS at stride 32, the five row layouts at 257 rows, the aux addressings at 700 rows (the
    table entries with one table row per decoder row where the addressing is "rows"); the output buffer holds exactly n * out_dim floats
    of sentinel and a guard region behind them."""
    cls = R.fwd_class(entry)
    for label, fx, lay in forward_cases(dec):
        refs = R.forward_refs(fx)
        out, _, _ = run_forward(world, entry, fx, lay)
        check(f"{entry} {dec} {label} out", out.get(label), refs[cls].out, refs["f64"].out)


@pytest.mark.parametrize("dec", list(R.DECODERS))
def test_aux_table(world, dec):
    for kind, rows in (("rows", 0), ("map", 16), ("map", 100)):
        for n in ((1, 33, 700) if kind == "rows" else (700,)):
            fx = R.make_fixture(dec, n, kind, rows)
            got = world.ops.mlp_aux_table(world.pm(dec), fx.aux.cuda())
            check(f"tir_mlp_aux_table {fx.name}", got, R.aux_table(fx.w, fx.aux, F32), R.aux_table(fx.w, fx.aux, F64))


def test_wrapper_routes(world):
    """ops.mlp takes the table launch when aux.shape[0] * 8 <= n and the direct launch otherwise: both are reached and held to float64."""
    ops = world.ops
    assert ops.AUX_TABLE
    for kind, rows in R.ADDRESSINGS[1:]:
        fx = R.make_fixture("sig3", 700, kind, rows)
        refs = R.forward_refs(fx)
        aux, amap, _ = world.dev(fx)
        fd, _ = layout(fx.feat, "s32")
        tabled = rows * 8 <= fx.n
        for impl, cls in (("mfma", "exact"), ("valu", "exact"), ("bf16", "bf16"), ("bf16x3", "split_table" if tabled else "split"),
                          ("f16", "f16" if tabled else "split")):
            got = ops.mlp(world.pm("sig3"), fd, aux, amap, impl, fx.aux_mod)
            check(f"ops.mlp {impl} {fx.name} ({'table' if tabled else 'direct'})", got, refs[cls].out, refs["f64"].out)


# ---- 2. the device-side row count ----------------------------------------------------------------------------------------------------
N_DEV_ENTRIES = list(R.FORWARD_ENTRIES) + ["tir_mlp_train_fwd", "tir_mlp_train_fwd_bf16x3", "tir_mlp_train_fwd_auxtab_bf16x3"]


@pytest.mark.parametrize("entry", N_DEV_ENTRIES)
def test_n_dev(world, entry):
    """*n_dev of n - 3, 0 and above n: rows below min(n, *n_dev) carry the bits of the full call, every later row of out, h1 and h2 keeps
    its sentinel bits."""
    save = "train" in entry
    for fx in (R.make_fixture("sig4", 257), R.make_fixture("tanh2", 700, "map_mod", 16)):
        feat = layout(fx.feat, "s32")
        full = [b.get() for b in run_forward(world, entry, fx, save=save, feat=feat) if b is not None]
        for v in (fx.n - 3, 0, fx.n + 5):
            n_dev = torch.tensor([v], dtype=torch.int32, device="cuda")
            part = [b.get() for b in run_forward(world, entry, fx, n_dev=n_dev, save=save, feat=feat) if b is not None]
            k = min(fx.n, v)
            for a, b in zip(part, full):
                assert torch.equal(bits(a[:k]), bits(b[:k])), (entry, fx.name, v)
                assert untouched(a[k:]), (entry, fx.name, v, "rows past *n_dev written")
            print(f"\n[decoder {entry} {fx.name} n_dev {v}] {k} rows bit-equal, {fx.n - k} rows untouched")


# ---- 3. training forwards ------------------------------------------------------------------------------------------------------------
def check_hidden(label, got, yard, ref64, z64):
    """h under the rule; exactly 0 wherever the float64 pre-activation is below minus the margin, > 0 wherever it is above it."""
    check(label, got, yard, ref64)
    got = got.detach().cpu()
    margin = R.bound(yard, ref64) * float(z64.abs().max())
    assert bool((got[z64 < -margin] == 0).all()), (label, "a unit below the margin is not exactly zero")
    assert bool((got[z64 > margin] > 0).all()), (label, "a unit above the margin is not positive")
    assert bool((got >= 0).all()), label


def run_multi(world, entry, fxs, save=False, tables=None, n_dev=None):
    """A multi-decoder forward launch through ops._call (jobs on the "rows" or "map" addressing, stride 32) -> [(out, h1, h2) Bufs]."""
    ops = world.ops
    k, n = len(fxs), fxs[0].n
    feats = [layout(fx.feat, "s32")[0] for fx in fxs]
    devs = [world.dev(fx) for fx in fxs]
    outs = [Buf(n, fx.out_dim) for fx in fxs]
    h1s, h2s = [Buf(n, R.HID) for _ in fxs], [Buf(n, R.HID) for _ in fxs]
    arr = lambda ps: (C.c_void_p * k)(*ps)
    descs = (C.POINTER(ops.TirMlp) * k)(*[C.pointer(world.pm(fx.dec).desc) for fx in fxs])
    args = [descs, arr([t.data_ptr() for t in feats]), 32, arr([d[0].data_ptr() for d in devs]),
            arr([None if d[1] is None else d[1].data_ptr() for d in devs])]
    if tables is not None:
        args.append(arr([d[2].data_ptr() if t else None for d, t in zip(devs, tables)]))
    args.append(arr([o.raw.data_ptr() for o in outs]))
    if save:
        args += [arr([h.raw.data_ptr() for h in h1s]), arr([h.raw.data_ptr() for h in h2s])]
    ops._call(entry, *args, k, n, ops._ptr(n_dev), ops._stream())
    torch.cuda.synchronize()
    return [(o, h1 if save else None, h2 if save else None) for o, h1, h2 in zip(outs, h1s, h2s)]


@pytest.mark.parametrize("dec", list(R.DECODERS))
def test_training_forward(world, dec):
    """tir_mlp_train_fwd, _bf16x3, _auxtab_bf16x3 (mapped, and one table row per decoder row) and the multi entry with one job: out, h1,
    h2 under the rule, the ReLU decisions by the margin, out with the bits of the entry that does not save."""
    plain = {"tir_mlp_train_fwd": "tir_mlp_fwd", "tir_mlp_train_fwd_bf16x3": "tir_mlp_fwd_bf16x3",
             "tir_mlp_train_fwd_auxtab_bf16x3": "tir_mlp_fwd_auxtab_bf16x3", "tir_mlp_train_fwd_multi_bf16x3": "tir_mlp_fwd_bf16x3"}
    for fx, lay in ((R.make_fixture(dec, 33), "s32"), (R.make_fixture(dec, 257), "s29"), (R.make_fixture(dec, 700), "s32"),
                    (R.make_fixture(dec, 700, "map", 16), "s32"), (R.make_fixture(dec, 257, group="large"), "s32")):
        refs = R.forward_refs(fx)
        f64 = refs["f64"]
        for entry in plain:
            multi = "multi" in entry
            if multi and (lay != "s32" or group_of(fx) != "unit"):
                continue
            yard = refs[R.fwd_class(entry)]
            feat = layout(fx.feat, lay)
            out, h1, h2 = run_multi(world, entry, [fx], save=True)[0] if multi else run_forward(world, entry, fx, save=True, feat=feat)
            label = f"{entry} {fx.name} {lay}"
            check(f"{label} out", out.get(label), yard.out, f64.out)
            check_hidden(f"{label} h1", h1.get(label), yard.h1, f64.h1, f64.z1)
            check_hidden(f"{label} h2", h2.get(label), yard.h2, f64.h2, f64.z2)
            ref_out, _, _ = run_forward(world, plain[entry], fx, feat=feat)
            assert torch.equal(bits(out.get()), bits(ref_out.get())), (label, "out differs from the entry that does not save")


# ---- 4. the persistent tile loop -----------------------------------------------------------------------------------------------------
TUNED = ["tir_mlp_fwd_bf16x3", "tir_mlp_fwd_bf16", "tir_mlp_fwd_auxtab_bf16x3", "tir_mlp_fwd_auxtab_f16", "tir_mlp_train_fwd_bf16x3",
         "tir_mlp_train_fwd_auxtab_bf16x3"]


@pytest.mark.parametrize("entry", TUNED)
def test_tune_grid(world, entry):
    """The entries that read TirMlp.tune_grid: 1 and 2 persistent workgroups over the three tiles of 700 rows give the bits of the default
    launch (a copy of the descriptor carries the option)."""
    save = "train" in entry
    for fx in (R.make_fixture("sig4", 700), R.make_fixture("tanh3", 700, "map_mod", 16)):
        feat = layout(fx.feat, "s32")
        base = [b.get() for b in run_forward(world, entry, fx, save=save, feat=feat) if b is not None]
        for grid in (1, 2):
            desc = type(world.pm(fx.dec).desc).from_buffer_copy(world.pm(fx.dec).desc)
            desc.tune_grid = grid
            got = [b.get() for b in run_forward(world, entry, fx, save=save, feat=feat, desc=desc) if b is not None]
            for a, b in zip(got, base):
                assert torch.equal(bits(a), bits(b)), (entry, fx.name, grid)
        print(f"\n[decoder {entry} {fx.name}] tune_grid 1 and 2 bit-equal to the default launch")


def test_persistent_loop(world):
    """The entries that never read tune_grid, at 65,537 rows: 257 tiles on 256 workgroups, so one workgroup takes two tiles and the last
    tile holds one row."""
    ops = world.ops
    fx = R.large_fixture("sig4", 65537)
    refs, pm = R.forward_refs(fx), world.pm("sig4")
    f64 = refs["f64"]
    fd, _ = layout(fx.feat, "s32")
    aux = fx.aux.cuda()
    check("tir_mlp_fwd 65537 out", ops.mlp(pm, fd, aux, None, "mfma"), refs["exact"].out, f64.out)
    out, h1, h2 = ops.mlp_train(pm, fd, aux, impl="mfma")
    check("tir_mlp_train_fwd 65537 out", out, refs["exact"].out, f64.out)
    check_hidden("tir_mlp_train_fwd 65537 h1", h1, refs["exact"].h1, f64.h1, f64.z1)
    check_hidden("tir_mlp_train_fwd 65537 h2", h2, refs["exact"].h2, f64.h2, f64.z2)
    b = R.backward_refs(fx)
    s = [t.cuda() for t in R.saved(fx)]
    for impl, cls, entry in (("mfma", "exact", "tir_mlp_bwd"), ("bf16x3", "split", "tir_mlp_bwd_bf16x3")):
        got = ops.mlp_bwd(pm, world.pb("sig4"), fd, s[0], fx.g_out.cuda(), s[1], s[2], impl=impl)
        for name, t in zip(R.BWD_TENSORS, got):
            check(f"{entry} 65537 {name}", t, getattr(b[cls], name), getattr(b["f64"], name))


def test_persistent_loop_multi(world):
    """Multi launches with four jobs at 16,385 rows: 65 tiles against 64 workgroups per job."""
    ops = world.ops
    decs = ("sig1", "sig4", "tanh3", "tanh2")
    fxs = [R.large_fixture(d, 16385) for d in decs]
    feats = [layout(fx.feat, "s32")[0] for fx in fxs]
    jobs = [(world.pm(fx.dec), fd, fx.aux.cuda(), None) for fx, fd in zip(fxs, feats)]
    plain = ops.mlp_multi(jobs)
    train = ops.mlp_multi(jobs, save_hidden=True)
    bjobs = []
    for fx, fd, o, (to, h1, h2) in zip(fxs, feats, plain, train):
        refs = R.forward_refs(fx)
        check(f"tir_mlp_fwd_multi_bf16x3 16385 {fx.dec} out", o, refs["split"].out, refs["f64"].out)
        check(f"tir_mlp_train_fwd_multi_bf16x3 16385 {fx.dec} out", to, refs["split"].out, refs["f64"].out)
        check_hidden(f"tir_mlp_train_fwd_multi_bf16x3 16385 {fx.dec} h1", h1, refs["split"].h1, refs["f64"].h1, refs["f64"].z1)
        check_hidden(f"tir_mlp_train_fwd_multi_bf16x3 16385 {fx.dec} h2", h2, refs["split"].h2, refs["f64"].h2, refs["f64"].z2)
        s = [t.cuda() for t in R.saved(fx)]
        bjobs.append((world.pm(fx.dec), world.pb(fx.dec), fd, s[0], fx.g_out.cuda(), s[1], s[2]))
    for fx, got in zip(fxs, ops.mlp_bwd_multi(bjobs)):
        b = R.backward_refs(fx)
        for name, t in zip(R.BWD_TENSORS, got):
            check(f"tir_mlp_bwd_multi_bf16x3 16385 {fx.dec} {name}", t, getattr(b["split"], name), getattr(b["f64"], name))


# ---- 5. multi launches ---------------------------------------------------------------------------------------------------------------
MULTI_DECS = ("sig1", "sig4", "tanh3", "tanh2")


@pytest.mark.parametrize("n_jobs", [1, 2, 3, 4])
def test_multi_forward(world, n_jobs):
    """tir_mlp_fwd_multi_bf16x3 and tir_mlp_fwd_multi_auxtab_bf16x3 (the table on job 0 only, on every job, on none) with 1 to 4 jobs over
    different decoders, out_dim 1 and 4 in one launch; job 0 reads its aux rows through a map.  Each job under the rule and bit-equal to
    its single-job call."""
    fxs = [R.make_fixture(d, 700, "map" if i == 0 else "rows", 16 if i == 0 else 0) for i, d in enumerate(MULTI_DECS[:n_jobs])]
    runs = [("tir_mlp_fwd_multi_bf16x3", None), ("tir_mlp_fwd_multi_auxtab_bf16x3", [True] + [False] * (n_jobs - 1)),
            ("tir_mlp_fwd_multi_auxtab_bf16x3", [True] * n_jobs), ("tir_mlp_fwd_multi_auxtab_bf16x3", [False] * n_jobs)]
    for entry, tables in runs:
        got = run_multi(world, entry, fxs, tables=tables)
        for i, (fx, (out, _, _)) in enumerate(zip(fxs, got)):
            tabled = bool(tables and tables[i])
            refs = R.forward_refs(fx)
            label = f"{entry} jobs {n_jobs} tables {tables} job {i} {fx.name}"
            check(label, out.get(label), refs["split_table" if tabled else "split"].out, refs["f64"].out)
            single, _, _ = run_forward(world, "tir_mlp_fwd_auxtab_bf16x3" if tabled else "tir_mlp_fwd_bf16x3", fx)
            assert torch.equal(bits(out.get()), bits(single.get())), (label, "differs from the single-job call")


def run_backward(world, entry, fx, lay="s32"):
    """tir_mlp_bwd / tir_mlp_bwd_bf16x3 through ops._call, fed the float64 forward's out, h1, h2 rounded to float32 -> four Bufs."""
    ops = world.ops
    g = group_of(fx) if not fx.name.endswith("edge") else "large"
    pm, pb = world.pm(fx.dec, g), world.pb(fx.dec, g)
    fd, stride = layout(fx.feat, lay)
    out, h1, h2 = (t.contiguous().cuda() for t in R.saved(fx))
    g_out = fx.g_out.cuda()
    bufs = [Buf(fx.n, 32), Buf(fx.n, R.HID), Buf(fx.n, R.HID), Buf(fx.n, 4)]
    ops._call(entry, C.byref(pm.desc), ops._ptr(pb), ops._ptr(fd), stride, ops._ptr(out), ops._ptr(g_out), ops._ptr(h1), ops._ptr(h2), fx.n,
              *[b.ptr() for b in bufs], ops._stream())
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("n_jobs", [1, 2, 3, 4])
def test_multi_backward(world, n_jobs):
    """tir_mlp_bwd_multi_bf16x3 with 1 to 4 jobs over different decoders: each job under the rule and bit-equal to tir_mlp_bwd_bf16x3."""
    ops = world.ops
    fxs = [R.make_fixture(d, 700) for d in MULTI_DECS[:n_jobs]]
    jobs = []
    for fx in fxs:
        s = [t.cuda() for t in R.saved(fx)]
        jobs.append((world.pm(fx.dec), world.pb(fx.dec), layout(fx.feat, "s32")[0], s[0], fx.g_out.cuda(), s[1], s[2]))
    for fx, got in zip(fxs, ops.mlp_bwd_multi(jobs)):
        b = R.backward_refs(fx)
        single = run_backward(world, "tir_mlp_bwd_bf16x3", fx)
        for name, t, one in zip(R.BWD_TENSORS, got, single):
            check(f"tir_mlp_bwd_multi_bf16x3 jobs {n_jobs} {fx.name} {name}", t, getattr(b["split"], name), getattr(b["f64"], name))
            assert torch.equal(bits(t), bits(one.get())), (fx.name, name, "differs from the single-job call")


# ---- 6. backward-data alone ----------------------------------------------------------------------------------------------------------
def check_backward(label, bufs, fx, cls):
    b = R.backward_refs(fx)
    yard, f64 = b[cls], b["f64"]
    got = {name: buf.get(label).cpu() for name, buf in zip(R.BWD_TENSORS, bufs)}
    assert bool((got["g_feat"][:, R.FEAT:] == 0).all()), (label, "g_feat columns >= 27")
    assert bool((got["dz3"][:, fx.out_dim:] == 0).all()), (label, "dz3 columns >= out_dim")
    check(f"{label} g_feat", got["g_feat"][:, :R.FEAT], yard.g_feat[:, :R.FEAT], f64.g_feat[:, :R.FEAT])
    for name in ("dz1", "dz2"):
        check(f"{label} {name}", got[name], getattr(yard, name), getattr(f64, name))
    check(f"{label} dz3", got["dz3"][:, :fx.out_dim], yard.dz3[:, :fx.out_dim], f64.dz3[:, :fx.out_dim])
    if fx.n < R.COLUMN_ROWS:
        return got
    worst = 0.0
    for c, bc in enumerate(R.column_bounds(yard.g_feat[:, :R.FEAT], f64.g_feat[:, :R.FEAT])):
        if bc is None:
            assert bool((got["g_feat"][:, c] == 0).all()), (label, c)
            continue
        d = R.distance(got["g_feat"][:, c], f64.g_feat[:, c])
        worst = max(worst, d / bc)
        assert d <= bc, (label, "g_feat column", c, d, bc)
    print(f"[decoder {label} g_feat per column] worst device / bound {worst:.2f}")
    return got


@pytest.mark.parametrize("dec", list(R.DECODERS))
@pytest.mark.parametrize("entry,cls", [("tir_mlp_bwd", "exact"), ("tir_mlp_bwd_bf16x3", "split")])
def test_backward_alone(world, entry, cls, dec):
    """Both backward-data entries on saved activations the float64 forward made (every ReLU decision is the reference's): ROWS at stride
    32, the |feat| ~ 100 group, the five layouts at 257 rows; g_feat[:, :27] (also per column), dz1, dz2, dz3 under the rule, the padding
    columns exactly zero, guard regions intact.  Per column from decoder_reference.COLUMN_ROWS rows on (see there)."""
    cases = [(f"n{n}", R.make_fixture(dec, n), "s32") for n in R.ROWS] + [("large", R.make_fixture(dec, 257, group="large"), "s32")]
    cases += [(lay, R.make_fixture(dec, 257), lay) for lay in R.LAYOUTS[1:]]
    for label, fx, lay in cases:
        check_backward(f"{entry} {dec} {label}", run_backward(world, entry, fx, lay), fx, cls)


# ---- 7. backward edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec", ["sig3", "tanh3", "sig4"])
@pytest.mark.parametrize("entry,cls", [("tir_mlp_bwd", "exact"), ("tir_mlp_bwd_bf16x3", "split")])
def test_backward_edges(world, entry, cls, dec):
    """64 rows by hand (decoder_reference.edge_fixture): a row with no active layer-2 unit, a row with every unit active, h entries of
    +0.0, -0.0 and 1e-30, saturated outputs, a zero g_out column, features of size 100 in the positional encoding's chain rule."""
    fx = R.edge_fixture(dec)
    got = check_backward(f"{entry} {fx.name}", run_backward(world, entry, fx), fx, cls)
    for name in ("g_feat", "dz1", "dz2"):
        assert bool((got[name][0] == 0).all()), (name, "row 0 has no active layer-2 unit")
    assert bool((got["dz3"][5:7] == 0).all()), "saturated outputs"
    assert bool((got["dz3"][:, 1] == 0).all()), "zero g_out column"
    for r in (2, 3):
        assert bool((got["dz1"][r, 0::3] == 0).all()) and bool((got["dz2"][r, 1::3] == 0).all()), "+0.0 and -0.0 are inactive"
    f64 = R.backward_refs(fx)["f64"]
    live = f64.dz2[4, 1::3] != 0
    assert bool(live.any()) and bool((got["dz2"][4, 1::3][live] != 0).all()), "1e-30 is active"


# ---- 8. the input rows ---------------------------------------------------------------------------------------------------------------
def test_inputs(world):
    """tir_mlp_inputs over ROWS, the layouts and the addressings: the raw columns are bit-exact, the positional-encoding columns within the
    float32 restatement's own distance plus the 4e-7 absolute the kernel documents for its sincos, columns 150..159 exactly zero."""
    ops = world.ops
    dec = "sig3"
    for label, fx, lay in forward_cases(dec):
        aux, amap, _ = world.dev(fx, group_of(fx))
        fd, _ = layout(fx.feat, lay)
        got = ops.mlp_inputs(world.pm(dec, group_of(fx)), fd, aux, amap, fx.aux_mod).cpu()
        x32, x64 = R.inputs160(fx, F32), R.inputs160(fx, F64)
        assert got.shape == (fx.n, R.XPAD) and bool((got[:, R.IN:] == 0).all()), label
        assert torch.equal(bits(got[:, :30]), bits(x32[:, :30])), (label, "raw columns")
        allowed = R.distance(x32[:, 30:R.IN], x64[:, 30:R.IN]) * float(x64[:, 30:R.IN].abs().max()) + R.SINCOS_ABS
        d = float((got[:, 30:R.IN].double() - x64[:, 30:R.IN]).abs().max())
        print(f"\n[decoder tir_mlp_inputs {label} PE columns] device {d:.2e} (bound {allowed:.2e})")
        assert d <= allowed, (label, d, allowed)
