"""The three-layer decoders (tensoir_amd/csrc/tir_mlp.hip) restated in plain torch, parametrised by dtype, with the fixtures and
the comparison rule of tests/test_gpu_decoder_kernels.py.  tests/test_decoder_cpu.py pins everything here without a GPU.

Restatement (models/tensorBase_rotated_lights.py:12-17, :122-146, :182-208, as include/tensoir_hip.h states it):
  input row    [feat 27, aux 3, sin PE(feat) 54, cos PE(feat) 54, sin PE(aux) 6, cos PE(aux) 6] = 150 columns, PE(x) = x * (1, 2) per
               value; tir_mlp_inputs writes 160 columns, 150..159 zero
  forward      z1 = W0 x + b0, h1 = relu z1, z2 = W1 h1 + b1, h2 = relu z2, z3 = W2 h2 + b2, out = sigmoid z3 (act 0) or tanh z3 (act 1)
  aux table    T[a] = b0 + W0[:, AUX_COLS] x_aux(aux_a)   (tir_mlp_aux_table); the table-start forward is z1 = T[row] + W0[:, FEAT_COLS] x_feat
  backward     from (feat, out, g_out, h1, h2) alone, as the kernel defines it: dz3 [n, 4] = g_out * (y (1 - y) or 1 - y^2), zero in
               columns >= out_dim; dz2 = (h2 > 0) * (dz3 W2); dz1 = (h1 > 0) * (dz2 W1); g_feat [n, 32] = dz1 W0 through the positional
               encoding, columns >= 27 zero
  addressing   aux row of decoder row s = (aux_map ? aux_map[s] : s), then % aux_mod when aux_mod > 0

Arithmetic classes (`cls`), each taken from the header's text, float32 only.  They are yardsticks: the distance of an emulation from
float64 says how far a kernel of that class may sit from float64; nothing is ever compared with an emulation bit for bit.
  "exact"   the products in the dtype itself
  "split"   the bf16x3 entries: every operand of every matrix product is hi + lo in bf16, hi*hi + hi*lo + lo*hi summed in float32;
            layer 1's bias rides as the weight of a constant-1 input (with a table start the table is exact and carries the bias)
  "bf16"    tir_mlp_fwd_bf16: every operand rounded to bf16 once, layer 1's bias among them
  "f16"     tir_mlp_fwd_auxtab_f16: operands rounded to fp16, float32 accumulation, exact table, exact layer 3

Comparison rule: shade_reference.distance (max |got - float64| / max |float64|) against shade_reference.bound of the yardstick that
belongs to the entry's class (ten times the yardstick's own distance, floor ten half-ulps)."""
import functools
import types
import zlib

import torch

from tests.shade_reference import bound, distance  # noqa: F401  (re-exported: the rule)

F32, F64 = torch.float32, torch.float64
FEAT, PE, HID, IN, XPAD, NPF = 27, 2, 128, 150, 160, 54
AUX_COLS = [27, 28, 29] + list(range(30 + 2 * NPF, IN))
FEAT_COLS = [c for c in range(IN) if c not in AUX_COLS]
ROWS = (1, 31, 32, 33, 255, 256, 257, 700)
LAYOUTS = ("s32", "s28", "s27", "s29", "s32+1")          # stride; "+1": the base pointer one float into its allocation
LAYOUT_VEC = {"s32": True, "s28": True, "s27": False, "s29": False, "s32+1": False}      # which take the 16-byte row loads
# (kind, aux rows): 16 rows * 8 <= 700 takes the table launch of ops.mlp, 100 rows the direct one
ADDRESSINGS = (("rows", 0), ("map", 16), ("map", 100), ("map_mod", 16), ("map_mod", 100), ("mod", 16), ("mod", 100))
# name -> (out_dim, act, largest |b0|)
DECODERS = {"sig3": (3, 0, 0.08), "sig4": (4, 0, 1.6), "tanh3": (3, 1, 0.08), "tanh4": (4, 1, 0.08), "sig1": (1, 0, 0.08),
            "tanh2": (2, 1, 0.08)}
FORWARD_ENTRIES = {"tir_mlp_fwd": "exact", "tir_mlp_fwd_valu": "exact", "tir_mlp_fwd_bf16x3": "split", "tir_mlp_fwd_bf16": "bf16",
                   "tir_mlp_fwd_auxtab_bf16x3": "split_table", "tir_mlp_fwd_auxtab_f16": "f16"}
SINCOS_ABS = 4e-7                                        # fast_sincos, as the kernel's comment documents it


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _c(t, dtype):
    return t.to(dtype)


def bf(t):
    return t.to(torch.bfloat16).to(F32)


def h16(t):
    return t.to(torch.float16).to(F32)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def pe_blocks(x):
    """sin and cos blocks of the positional encoding of x [n, k] -> two [n, 2 k], column 2 d + f = fn(x_d * 2^f)."""
    y = (x[..., None] * torch.tensor([1.0, 2.0], dtype=x.dtype)).reshape(x.shape[0], -1)
    return torch.sin(y), torch.cos(y)


def input_row(feat, aux_g, mistake=None):
    """[n, 150]: feat [n, 27] and the gathered aux rows [n, 3], in their own dtype."""
    fs, fc = pe_blocks(feat)
    if mistake == "pe_swap":
        fs, fc = fc, fs
    as_, ac = pe_blocks(aux_g)
    return torch.cat([feat, aux_g, fs, fc, as_, ac], dim=-1)


def aux_rows(n, aux_map, aux_mod, mistake=None):
    """The addressing rule -> int64 [n]."""
    s = torch.arange(n)
    if mistake == "mod_before_map" and aux_map is not None and aux_mod > 0:
        return aux_map.long()[s % aux_mod] % aux_mod          # (wrapped again only to stay inside the table)
    ai = aux_map.long() if aux_map is not None else s
    if aux_mod > 0:
        ai = ai % aux_mod
    return ai


def _split(t):
    hi = bf(t)
    return hi, bf(t - hi)


def mm(a, bt, cls, drop=None):
    """a [n, k] @ bt [m, k]^T in the arithmetic class."""
    if cls == "exact":
        return a @ bt.T
    assert a.dtype == F32
    if cls == "bf16":
        return bf(a) @ bf(bt).T
    if cls == "f16":
        return h16(a) @ h16(bt).T
    ah, al = _split(a)
    bh, bl = _split(bt)
    r = ah @ bh.T
    if drop != "hi_lo":
        r = r + ah @ bl.T
    return r + al @ bh.T


def aux_table(w, aux, dtype):
    """tir_mlp_aux_table: [n_aux, 128]."""
    aux = _c(aux, dtype)
    s, c = pe_blocks(aux)
    return _c(w["b0"], dtype) + torch.cat([aux, s, c], dim=-1) @ _c(w["w0"], dtype)[:, AUX_COLS].T


def forward(fx, dtype, cls="exact", table=False, mistake=None):
    """out [n, out_dim], h1, h2, z1, z2, z3 of fixture fx.  table: layer 1 starts from the aux table's row (exact in every class)."""
    w = {k: _c(v, dtype) for k, v in fx.w.items()}
    if mistake == "w1_swap":
        w["w1"] = w["w1"][:, fx.unit_perm]
    feat = _c(fx.feat, dtype)
    ai = aux_rows(fx.n, fx.aux_map, fx.aux_mod, mistake)
    if mistake == "aux_off_by_one":
        ai = (ai + 1) % fx.aux.shape[0]
    x = input_row(feat, _c(fx.aux, dtype)[ai], mistake)
    drop = "hi_lo" if mistake == "drop_product" else None
    if table:
        z1 = aux_table(fx.w, fx.aux, dtype)[ai] + mm(x[:, FEAT_COLS], w["w0"][:, FEAT_COLS], cls, drop)
    elif cls in ("split", "bf16"):                      # the bias is the weight of a constant-1 input
        one = torch.ones((fx.n, 1), dtype=dtype)
        z1 = mm(torch.cat([x, one], -1), torch.cat([w["w0"], w["b0"][:, None]], -1), cls, drop)
    else:
        z1 = mm(x, w["w0"], cls) + w["b0"]
    h1 = torch.relu(z1)
    z2 = mm(h1, w["w1"], cls, drop) + w["b1"]
    h2 = torch.relu(z2)
    z3 = mm(h2, w["w2"], "exact" if cls == "f16" else cls, drop) + w["b2"]
    out = torch.tanh(z3) if fx.act == 1 else torch.sigmoid(z3)
    return types.SimpleNamespace(out=out, h1=h1, h2=h2, z1=z1, z2=z2, z3=z3, x=x)


def inputs160(fx, dtype):
    x = input_row(_c(fx.feat, dtype), _c(fx.aux, dtype)[aux_rows(fx.n, fx.aux_map, fx.aux_mod)])
    return torch.cat([x, torch.zeros((fx.n, XPAD - IN), dtype=dtype)], -1)


def backward(fx, out, h1, h2, dtype, cls="exact", mistake=None):
    """Backward-data as the kernel defines it: g_feat [n, 32], dz1, dz2 [n, 128], dz3 [n, 4] from the SAVED out, h1, h2."""
    w = {k: _c(v, dtype) for k, v in fx.w.items()}
    if mistake == "w1_swap":
        w["w1"] = w["w1"][:, fx.unit_perm]
    od, act = fx.out_dim, fx.act
    if mistake == "other_act":
        act = 1 - act
    feat, y, g = _c(fx.feat, dtype), _c(out, dtype), _c(fx.g_out, dtype)
    h1, h2 = _c(h1, dtype), _c(h2, dtype)
    drop = "hi_lo" if mistake == "drop_product" else None
    active = (lambda h: h >= 0) if mistake == "mask_ge" else (lambda h: h > 0)
    dz3 = torch.zeros((fx.n, 4), dtype=dtype)
    dz3[:, :od] = g * ((1 - y * y) if act == 1 else y * (1 - y))
    if mistake == "dz3_unzeroed" and od < 4:
        dz3[:, od] = dz3[:, 0]
    dz2 = active(h2) * mm(dz3[:, :od], w["w2"].T, cls, drop)
    dz1 = active(h1) * mm(dz2, w["w1"].T, cls, drop)
    gx = mm(dz1, w["w0"].T, cls, drop)
    s1, c1 = torch.sin(feat), torch.cos(feat)
    s2, c2 = torch.sin(2 * feat), torch.cos(2 * feat)
    gs, gc = gx[:, 30:30 + NPF].reshape(-1, FEAT, 2), gx[:, 30 + NPF:30 + 2 * NPF].reshape(-1, FEAT, 2)
    g_feat = torch.zeros((fx.n, 32), dtype=dtype)
    g_feat[:, :FEAT] = gx[:, :FEAT] + c1 * gs[..., 0] + 2 * c2 * gs[..., 1] - s1 * gc[..., 0] - 2 * s2 * gc[..., 1]
    return types.SimpleNamespace(g_feat=g_feat, dz1=dz1, dz2=dz2, dz3=dz3)


# ---- decoders and fixtures ---------------------------------------------------------------------------------------------------------
def _uniform(gen, shape, a):
    return (torch.rand(shape, generator=gen) * 2 - 1) * a


def _features(gen, n, group):
    if group == "large":
        return _uniform(gen, (n, FEAT), 100.0)
    return torch.randn(n, FEAT, generator=gen) * 0.8


@functools.lru_cache(maxsize=None)
def decoder(name, group="unit"):
    """Seeded weights (nn.Linear's init ranges) with w2 and b2 set from the float64 pre-activations of a 700-row calibration set of the
    feature group, so that every output column spreads: z3 has standard deviation 1.5 (sigmoid) or 0.8 (tanh) around a small offset."""
    od, act, b0max = DECODERS[name]
    gen = torch.Generator().manual_seed(_seed("decoder", name))
    w = {"w0": _uniform(gen, (HID, IN), IN ** -0.5), "b0": _uniform(gen, (HID,), b0max),
         "w1": _uniform(gen, (HID, HID), HID ** -0.5), "b1": _uniform(gen, (HID,), HID ** -0.5),
         "w2": _uniform(gen, (od, HID), HID ** -0.5), "b2": torch.zeros(od)}
    if group == "large":
        w["w0"][:, :FEAT] *= 0.02                        # raw features of size 100 weigh like unit ones: the hidden layers stay mixed
    feat, aux = _features(gen, 700, group), torch.randn(700, 3, generator=gen)
    x = input_row(feat.double(), aux.double())
    h2 = torch.relu(torch.relu(x @ w["w0"].double().T + w["b0"].double()) @ w["w1"].double().T + w["b1"].double())
    z3 = h2 @ w["w2"].double().T
    scale = (0.8 if act == 1 else 1.5) / z3.std(0)
    w["w2"] = (w["w2"].double() * scale[:, None]).float()
    w["b2"] = (0.2 * torch.arange(1, od + 1) / od - z3.mean(0) * scale).float()
    return w


def make_fixture(dec, n, kind="rows", R=0, group="unit", parent=700):
    """Rows [:n] of the seeded `parent`-row population of (decoder, addressing, group).  feat [n, 27], aux [R or n, 3], aux_map int32 [n]
    or None, aux_mod, g_out [n, out_dim]."""
    return _fixture(dec, n, kind, R, group, max(parent, n))


@functools.lru_cache(maxsize=None)
def _population(dec, kind, R, group, parent):
    od, act, _ = DECODERS[dec]
    gen = torch.Generator().manual_seed(_seed("rows", dec, kind, R, group, parent))
    feat = _features(gen, parent, group)
    g_out = torch.randn(parent, od, generator=gen)
    aux = torch.randn(parent if kind == "rows" else R, 3, generator=gen)
    aux_map, aux_mod = None, 0
    if kind == "map":                                    # repeats, row 0 and the last row among them
        aux_map = torch.randint(0, R, (parent,), generator=gen)
        aux_map[5], aux_map[17], aux_map[18] = 0, R - 1, R - 1
    elif kind == "map_mod":                              # pair ids up to 10 D, direction = id mod D
        aux_map, aux_mod = torch.randint(0, 10 * R, (parent,), generator=gen), R
        aux_map[5], aux_map[17] = 3 * R, 10 * R - 1
    elif kind == "mod":
        aux_mod = R
    return feat, g_out, aux, None if aux_map is None else aux_map.int(), aux_mod


@functools.lru_cache(maxsize=None)
def _fixture(dec, n, kind, R, group, parent):
    od, act, _ = DECODERS[dec]
    feat, g_out, aux, aux_map, aux_mod = _population(dec, kind, R, group, parent)
    gen = torch.Generator().manual_seed(_seed("perm", dec))
    j = int(torch.randint(0, HID - 1, (1,), generator=gen))
    perm = list(range(HID))
    perm[j], perm[j + 1] = perm[j + 1], perm[j]
    return types.SimpleNamespace(name=f"{dec}-{n}-{kind}{R or ''}-{group}", dec=dec, n=n, out_dim=od, act=act, w=decoder(dec, group),
                                 feat=feat[:n].contiguous(), g_out=g_out[:n].contiguous(), aux=aux[:n].contiguous() if kind == "rows" else aux,
                                 aux_map=None if aux_map is None else aux_map[:n].contiguous(), aux_mod=aux_mod, kind=kind, unit_perm=perm)


def edge_fixture(dec):
    """64 rows by hand for the backward's edges (the saved activations are arguments, so they need not come from a forward): row 0 with
    every layer-2 unit inactive, row 1 with every unit active, rows 2..4 with +0.0, -0.0 (inactive) and 1e-30 (active) entries, rows 5 and 6
    with saturated outputs (0 and 1 under sigmoid, -1 and +1 under tanh), g_out column 1 zero, features of
    the |feat| ~ 100 group."""
    od, act, _ = DECODERS[dec]
    n = 64
    gen = torch.Generator().manual_seed(_seed("edge", dec))
    fx = types.SimpleNamespace(name=f"{dec}-edge", dec=dec, n=n, out_dim=od, act=act, w=decoder(dec, "large"), kind="rows", aux=None,
                               aux_map=None, aux_mod=0, unit_perm=_fixture(dec, 1, "rows", 0, "unit", 700).unit_perm)
    fx.feat = _features(gen, n, "large")
    fx.g_out = torch.randn(n, od, generator=gen)
    fx.g_out[:, 1] = 0.0
    h1 = torch.relu(torch.randn(n, HID, generator=gen))
    h2 = torch.relu(torch.randn(n, HID, generator=gen))
    h2[0] = 0.0
    h1[1], h2[1] = h1[1].abs() + 0.1, torch.randn(HID, generator=gen).abs() + 0.1
    for r, v in ((2, 0.0), (3, -0.0), (4, 1e-30)):
        h1[r, 0::3], h2[r, 1::3] = v, v
    u = torch.rand(n, od, generator=gen) * 0.9 + 0.05
    out = 2 * u - 1 if act == 1 else u
    out[5], out[6] = (-1.0 if act == 1 else 0.0), 1.0
    fx.out, fx.h1, fx.h2 = out, h1, h2
    return fx


# ---- yardsticks and bounds ---------------------------------------------------------------------------------------------------------
FWD_TENSORS = ("out", "h1", "h2")
BWD_TENSORS = ("g_feat", "dz1", "dz2", "dz3")


def forward_refs(fx):
    """float64 and the emulations of the forward, once per fixture object."""
    if not hasattr(fx, "_fwd"):
        fx._fwd = {"f64": forward(fx, F64), "exact": forward(fx, F32), "split": forward(fx, F32, "split"), "bf16": forward(fx, F32, "bf16"),
                   "split_table": forward(fx, F32, "split", table=True), "f16": forward(fx, F32, "f16", table=True)}
    return fx._fwd


def saved(fx):
    """The float64 forward's out, h1, h2 rounded to float32: what the backward-data kernels are fed."""
    if hasattr(fx, "out"):
        return fx.out, fx.h1, fx.h2
    r = forward_refs(fx)["f64"]
    return r.out.float(), r.h1.float(), r.h2.float()


def backward_refs(fx):
    if not hasattr(fx, "_bwd"):
        s = saved(fx)
        fx._bwd = {"f64": backward(fx, *s, F64), "exact": backward(fx, *s, F32), "split": backward(fx, *s, F32, "split")}
    return fx._bwd


def fwd_class(entry, table=False):
    """Key into forward_refs of the yardstick an entry is held to."""
    if entry.endswith("_f16"):
        return "f16"
    if "bf16x3" in entry:
        return "split_table" if (table or "auxtab" in entry) else "split"
    return "bf16" if entry.endswith("_bf16") else "exact"


# The rule compares two maxima of rounding errors, the device's and the yardstick's, and its factor of ten covers the ratio of two
# such maxima when each is taken over enough values.  A column of a one-row fixture is ONE value: the ratio of two single rounding
# errors has no bound to speak of (a yardstick that happens to round exactly gives the floor).  So a tensor is compared per column only
# when a column holds at least as many values as the smallest whole tensor the rule is applied to anywhere (27 + 4: the 31-row fixture).
COLUMN_ROWS = 31


def column_bounds(yard, f64):
    """bound per column of a [n, k] tensor (None where the float64 column is identically zero)."""
    return [bound(yard[:, c], f64[:, c]) if bool((f64[:, c] != 0).any()) else None for c in range(f64.shape[1])]


def large_fixture(dec, n):
    return make_fixture(dec, n, parent=n)
