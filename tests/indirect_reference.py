"""The indirect-light stage (tir_vm_app_fwd_h16, tir_indirect_fused_fwd, tir_indirect_fused_hp_fwd; tensoir_amd/csrc/tir_field.hip,
tir_mlp.hip) restated in plain torch, parametrised by dtype, with the yardsticks of its arithmetic classes, the fixtures and the
comparison rule of tests/test_gpu_indirect_kernels.py.  tests/test_indirect_cpu.py pins everything here without a GPU.

Restatement (models/relight_utils.py:818-829 = compute_appfeature -> renderModule, as include/tensoir_hip.h states it).  For record s:
  pair id      p = rec_map ? rec_map[s] : s
  light row    light_idx[p // idx_div] (idx_div <= 1: p itself) clamped to [0, n_lights - 1]; a field with one light uses row 0
  aux row      p % aux_mod when aux_mod > 0, p otherwise
  features     basis_mat . (bilinear(plane_k) * linear(line_k) * light row) over the three VM groups, clamped to +-65504 where they
               feed a decoder (the fused entries)
  output       the table-start decoder of tests/decoder_reference.py on those features
The tap indices and weights are make_tap_q's, taken in the kernels' own fp32 steps (taps32: indices clamped, out-of-range weights
zero), so a point on a lattice line picks the same cell on both sides and nothing has to be excluded; everything after the taps runs
in the dtype.  taps64 is the same rule with float64 steps (the oracle's own: tests/test_indirect_cpu.py compares through it).

Arithmetic classes, float32 only, each written from the header's text and the kernel comments.  They are yardsticks (the distance of an
emulation from float64 says how far a kernel of that class may sit from float64), never compared with a device bit for bit.
  "h16"    tables, light rows and basis_mat rounded to fp16 (saturating), interpolation weights rounded to fp16, the bilinear and
           linear chains and (plane * line) * light rounded to fp16 after every packed step, contraction with fp32 accumulation
  "dense"  corner features accumulated in fp32 from the fp32 parameters, rounded once to fp16; the 8-corner weighted sum with fp16
           weights on the packed fp16 pipe (both lookups ship the packed form: tir_common.hpp, TIR_DENSE_APP_F32 = 0)
  "f16 fused"  h16 or dense features into decoder_reference's "f16" class (exact table, exact layer 3)
  "hp"     fp32 taps and interpolation; products and basis_mat split hi + lo in fp16, three products summed in fp32; decoder activations
           in fp16, weights fp16 + e4m3 residue of (W - fp16(W)) 2^17 clamped to +-448, the residue's activations in e4m3 (raw feature
           clamped to +-448 first, hidden activations cut at 448), layer 3 exact

Comparison rule: shade_reference.distance against shade_reference.bound of the class's yardstick on the same fixture; bias_distance /
bias_bound are the same rule on the per-channel mean signed deviation (the statistic that shows a dropped weight residue)."""
import functools
import types
import zlib

import torch

from tensoir_amd import synth
from tests import decoder_reference as D
from tests.shade_reference import bound, distance  # noqa: F401  (re-exported: the rule)

F32, F64 = torch.float32, torch.float64
CA, NCH, FEAT, NF0 = 48, 144, 27, 14
MAT_MODE, VEC_MODE = ((0, 1), (0, 2), (1, 2)), (2, 1, 0)
H_MAX, F8_MAX = 65504.0, 448.0
F8_SCALE = 2.0 ** 17
HALF_RANGE = 6.0e4                        # ops.INDIRECT_PROBE["range"]
# name -> (lights, regime, grid): three unequal axes, none above (20, 24, 28).  1 / 2..16 / 17 lights are the three light-row arms of
# k_indirect_fused, 8 and 9 the limit of k_indirect_fused_hp and its refusal.  "huge" (hp only): raw features beyond 448 and 65504.
FIELDS = {"l1": (1, "unit", (20, 24, 28)), "l1s": (1, "small", (20, 24, 28)), "l1g": (1, "large", (20, 24, 28)),
          "l2": (2, "unit", (13, 9, 17)), "l2s": (2, "small", (13, 9, 17)), "l2g": (2, "large", (13, 9, 17)),
          "l8": (8, "unit", (20, 24, 28)), "l9": (9, "unit", (9, 13, 11)), "l16": (16, "unit", (20, 24, 28)),
          "l17": (17, "unit", (11, 20, 7)), "l2x": (2, "huge", (13, 9, 17))}
F16_FIELDS = [k for k, v in FIELDS.items() if v[1] != "huge"]
HP_FIELDS = [k for k, v in FIELDS.items() if v[0] <= 8]
ROWS = (1, 15, 16, 17, 31, 32, 33, 1000)
ROWS_HP = ROWS[:-1] + (255, 256, 257, 1000)
ROWS_F16 = ROWS[:-1] + (383, 384, 385, 1000)
POP = 1000                                # rows of a record population: three or four tiles of every kernel
ADDRESSINGS = ("nomap", "d3", "d16", "div5mod7")
DECODERS = ("sig3", "sig1", "sig4", "tanh3")
POINT_CLASSES = ("interior", "nodes", "faces", "last_cell", "outside", "corners", "planted")
BIAS_ROWS = 4096
BIAS_FIXTURE, BIAS_DECODERS = ("l2", "d16"), ("sig3", "sig4")     # chosen on the CPU: tests/test_indirect_cpu.py shows the separation


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def sat16(t):
    return t.clamp(-H_MAX, H_MAX).to(torch.float16).to(F32)


def e4m3(t):
    """fp32 -> e4m3 -> fp32; clamped first (torch turns 500 into NaN)."""
    return t.clamp(-F8_MAX, F8_MAX).to(torch.float8_e4m3fn).to(F32)


# ---- taps ----------------------------------------------------------------------------------------------------------------------------
def taps32(x, size):
    """make_tap_q on the host: every fp32 step rounded on its own, indices clamped, out-of-range weights zero -> i0, i1, w0, w1 (fp32)."""
    x = x.to(F32)
    ix = ((x + 1.0) * 0.5) * torch.tensor(float(size - 1), dtype=F32)
    f0 = torch.floor(ix)
    t = ix - f0
    i0 = f0.long()
    i1 = i0 + 1
    w0 = torch.where((i0 >= 0) & (i0 < size), 1.0 - t, torch.zeros_like(t))
    w1 = torch.where((i1 >= 0) & (i1 < size), t, torch.zeros_like(t))
    return i0.clamp(0, size - 1), i1.clamp(0, size - 1), w0, w1


def taps64(x, size):
    """The same rule in float64 steps (grid_sample's unnormalisation, align_corners, zero padding)."""
    x = x.to(F64)
    ix = ((x + 1) / 2) * (size - 1)
    f0 = torch.floor(ix)
    t = ix - f0
    i0 = f0.long()
    i1 = i0 + 1
    w0 = torch.where((i0 >= 0) & (i0 < size), 1.0 - t, torch.zeros_like(t))
    w1 = torch.where((i1 >= 0) & (i1 < size), t, torch.zeros_like(t))
    return i0.clamp(0, size - 1), i1.clamp(0, size - 1), w0, w1


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def pair_ids(rec):
    return rec.rec_map.long() if rec.rec_map is not None else torch.arange(rec.n)


def light_rows(fld, rec, mistake=None):
    """The light row of every record -> int64 [n]."""
    if fld.n_lights == 1:
        return torch.zeros(rec.n, dtype=torch.long)
    p = pair_ids(rec)
    div = max(rec.idx_div, 1)
    ray = p % div if mistake == "light_mod" else p // div
    li = rec.light_idx.long()[ray]
    if mistake == "light_wrap":
        return li % fld.n_lights
    return li.clamp(0, fld.n_lights - 1)


def aux_rows(rec, mistake=None):
    return D.aux_rows(rec.n, rec.rec_map, rec.aux_mod, mistake)


def products(fld, xyz, li, dtype, taps=taps32, mistake=None):
    """(bilinear(plane_k) * linear(line_k)) * light row for the 144 channels, in dtype on the given taps -> [n, 144]."""
    light = fld.light.to(dtype)[li]
    out = []
    for k in range(3):
        m0, m1 = MAT_MODE[k]
        cx, cy = (m1, m0) if (mistake == "plane_axes" and k == 1) else (m0, m1)      # (the coordinates swap, the sizes stay: in bounds)
        x0, x1, wx0, wx1 = taps(xyz[:, cx], fld.grid[m0])
        y0, y1, wy0, wy1 = taps(xyz[:, cy], fld.grid[m1])
        l0, l1, wl0, wl1 = taps(xyz[:, VEC_MODE[k]], fld.grid[VEC_MODE[k]])
        wx0, wx1, wy0, wy1, wl0, wl1 = (w.to(dtype) for w in (wx0, wx1, wy0, wy1, wl0, wl1))
        pl, ln = fld.planes[k].to(dtype), fld.lines[k].to(dtype)
        bil = pl[:, y0, x0] * (wx0 * wy0) + pl[:, y0, x1] * (wx1 * wy0) + pl[:, y1, x0] * (wx0 * wy1) + pl[:, y1, x1] * (wx1 * wy1)
        lin = ln[:, l0] * wl0 + ln[:, l1] * wl1
        out.append(((bil * lin).T) * light[:, k * CA:(k + 1) * CA])
    return torch.cat(out, 1)


def features(fld, rec, dtype, taps=taps32, mistake=None):
    """basis_mat . products -> [n, 27], unclamped (tir_vm_app_fwd's rad_feat)."""
    return products(fld, rec.xyz, light_rows(fld, rec, mistake), dtype, taps, mistake) @ fld.basis.to(dtype).T


def own13(feat):
    """The decoder's view of the features when kperm_f deals 13 to lane half 0 and the gather still deals 14: feature 13 meets no weight,
    features 14..26 meet the weights of 13..25, the weights of 26 meet nothing."""
    f = torch.zeros_like(feat)
    f[:, :13] = feat[:, :13]
    f[:, 13:26] = feat[:, 14:27]
    return f


def decoder_fixture(rec, dec, feat, w=None):
    """A decoder_reference fixture over the records: features as given, aux = the directions, aux_map = the pair ids."""
    od, act, _ = D.DECODERS[dec]
    return types.SimpleNamespace(name=f"{rec.name}-{dec}", dec=dec, n=rec.n, out_dim=od, act=act, w=w if w is not None else weights(rec.field, dec),
                                 feat=feat, aux=rec.dirs, aux_map=rec.rec_map, aux_mod=rec.aux_mod, kind="map_mod")


def forward(fld, rec, dec, dtype, taps=taps32, w=None, mistake=None):
    """The stage in dtype -> (features [n, 27] clamped, out [n, out_dim])."""
    feat = features(fld, rec, dtype, taps, mistake).clamp(-H_MAX, H_MAX)
    seen = own13(feat) if mistake == "own13" else feat
    out = D.forward(decoder_fixture(rec, dec, seen, w), dtype, "exact", table=True, mistake=mistake if mistake in ("pe_swap", "mod_before_map") else None).out
    return feat, out


# ---- the emulations ------------------------------------------------------------------------------------------------------------------
def _hfma(a, b, c):
    return sat16_free(a * b + c)


def sat16_free(t):
    return t.to(torch.float16).to(F32)


def h16_features(fld, rec):
    """Class "h16": the packed-fp16 gather of k_vm_app_h16 / k_indirect_fused (h16_chunk_pk) -> [n, 27] float32, unclamped."""
    h = sat16_free
    li = light_rows(fld, rec)
    light = sat16(fld.light)[li]
    out = []
    for k in range(3):
        m0, m1 = MAT_MODE[k]
        x0, x1, wx0, wx1 = taps32(rec.xyz[:, m0], fld.grid[m0])
        y0, y1, wy0, wy1 = taps32(rec.xyz[:, m1], fld.grid[m1])
        l0, l1, wl0, wl1 = taps32(rec.xyz[:, VEC_MODE[k]], fld.grid[VEC_MODE[k]])
        pl, ln = sat16(fld.planes[k]), sat16(fld.lines[k])
        acc = h(pl[:, y0, x0] * h(wx0 * wy0))
        acc = _hfma(pl[:, y0, x1], h(wx1 * wy0), acc)
        acc = _hfma(pl[:, y1, x0], h(wx0 * wy1), acc)
        acc = _hfma(pl[:, y1, x1], h(wx1 * wy1), acc)
        lin = _hfma(ln[:, l1], h(wl1), h(ln[:, l0] * h(wl0)))
        out.append(h(h(acc * lin).T * light[:, k * CA:(k + 1) * CA]))
    return torch.cat(out, 1) @ sat16(fld.basis).T


def dense_volume(fld):
    """tir_dense_app_build: fp32 corner features of a one-light field rounded once to fp16 -> [Z, Y, X, 27] float32."""
    X, Y, Z = fld.grid
    ax = {0: torch.arange(X).view(1, 1, X).expand(Z, Y, X), 1: torch.arange(Y).view(1, Y, 1).expand(Z, Y, X),
          2: torch.arange(Z).view(Z, 1, 1).expand(Z, Y, X)}
    terms = []
    for k in range(3):
        m0, m1 = MAT_MODE[k]
        terms.append((fld.planes[k][:, ax[m1], ax[m0]] * fld.lines[k][:, ax[VEC_MODE[k]]]) * fld.light[0, k * CA:(k + 1) * CA, None, None, None])
    return sat16(torch.einsum("jc,czyx->zyxj", fld.basis, torch.cat(terms, 0)))


def dense_features(fld, rec):
    """Class "dense": tir::dense_app_lookup's packed form -> [n, 27] float32 (clamped, as both lookups deliver it)."""
    h = sat16_free
    vol = fld.volume()
    tx, ty, tz = (taps32(rec.xyz[:, a], fld.grid[a]) for a in range(3))
    face = []
    for dz in (0, 1):
        s = None
        for dy in (0, 1):
            for dx in (0, 1):
                w = h(((tz[2 + dz] * ty[2 + dy]) * tx[2 + dx]))[:, None]
                v = vol[tz[dz], ty[dy], tx[dx]]
                s = h(v * w) if s is None else _hfma(v, w, s)
        face.append(s)
    return h(face[0] + face[1]).clamp(-H_MAX, H_MAX)


def hp_features(fld, rec, mistake=None):
    """Class "hp", feature phase: fp32 taps and interpolation, product and basis_mat as fp16 hi + lo, three products -> [n, 27] clamped."""
    x = products(fld, rec.xyz, light_rows(fld, rec), F32).clamp(-H_MAX, H_MAX)
    hi = sat16_free(x)
    lo = sat16_free(x - hi)
    bh = sat16(fld.basis)
    bl = sat16_free(fld.basis - bh)
    f = hi @ bh.T + hi @ bl.T
    if mistake != "hp_drop_product":
        f = f + lo @ bh.T
    return f.clamp(-H_MAX, H_MAX)


def hp_decode(rec, dec, feat, w=None, mistake=None):
    """Class "hp", decoder phase, on float32 features (clamped to +-65504) -> out [n, out_dim]."""
    od, act, _ = D.DECODERS[dec]
    w = w if w is not None else weights(rec.field, dec)
    ai = aux_rows(rec)
    scale = 0.0 if mistake == "hp_no_residue" else (2.0 / F8_SCALE if mistake == "hp_scale_x2" else 1.0 / F8_SCALE)

    def layer(a, a8, wt):
        wh = sat16_free(wt)
        z = sat16_free(a) @ wh.T
        return z + (e4m3(a8) @ e4m3((wt - wh) * F8_SCALE).T) * scale

    x = D.input_row(feat, rec.dirs[ai])[:, D.FEAT_COLS]
    x8 = x.clone()
    x8[:, :FEAT] = x8[:, :FEAT].clamp(-F8_MAX, F8_MAX)
    z1 = D.aux_table(w, rec.dirs, F32)[ai] + layer(x, x8, w["w0"][:, D.FEAT_COLS])
    h1 = z1.clamp(0.0, H_MAX)
    z2 = w["b1"] + layer(h1, h1.clamp(max=F8_MAX), w["w1"])
    z3 = torch.relu(z2) @ w["w2"].T + w["b2"]
    return torch.tanh(z3) if act == 1 else torch.sigmoid(z3)


def f16_decode(rec, dec, feat, w=None):
    return D.forward(decoder_fixture(rec, dec, feat.clamp(-H_MAX, H_MAX), w), F32, "f16", table=True).out


# ---- fields ----------------------------------------------------------------------------------------------------------------------------
def half_range_bound(fld):
    """ops.HalfRange.judge on the field's maxima -> (ok, bound)."""
    lim = HALF_RANGE
    m = [float(t.abs().max()) for t in fld.planes] + [float(t.abs().max()) for t in fld.lines] + [float(fld.light.abs().max()), float(fld.basis.abs().max())]
    b = max(m[i] * m[3 + i] for i in range(3)) * max(1.0, m[6])
    return bool(b < lim and m[7] < lim and all(v < lim for v in m[:7])), b


@functools.lru_cache(maxsize=None)
def field(name):
    """The seeded field `name`: synth.make_checkpoint with 48 appearance components and light_rotation as tests/config_scenes.py builds
    it, its tables scaled into the regime IN the checkpoint (the device model is loaded from fld.ck), basis_mat scaled so that the
    features have rms 0.8 (small: 0.25) at 512 interior points.
      unit    planes and lines x 4
      small   planes and lines x 0.018: every plane * line * light product of the fixtures lies in fp16's subnormal range (features of
              rms 0.25: with 0.8 basis_mat would leave fp16)
      large   one scale on planes and lines puts the range guard's bound at 5.5e4, and one channel carries the maxima of its plane,
              line and light rows at one lattice node (fld.planted): the product there IS the bound
      huge    planes and lines x 24, then basis_mat x 125, row 3 x 10 and row 20 x 1000 on top: raw features beyond 448 and beyond
              65504 with max |basis_mat| still inside fp16"""
    n_lights, regime, grid = FIELDS[name]
    rot = [f"{(i * 360) // n_lights:03d}" for i in range(n_lights)]
    ck = synth.make_checkpoint(grid=grid, seed=_seed("field", name) % (1 << 31), light_rotation=rot, density_n_comp=(4, 4, 4), app_n_comp=(CA,) * 3)
    sd = ck["state_dict"]
    fld = types.SimpleNamespace(name=name, grid=grid, n_lights=n_lights, regime=regime, ck=ck, planted=None)
    s = {"unit": 4.0, "small": 0.018, "large": 1.0, "huge": 24.0}[regime]
    for i in range(3):
        sd[f"app_plane.{i}"] *= s
        sd[f"app_line.{i}"] *= s
    if regime == "large":
        pm = [float(sd[f"app_plane.{i}"].abs().max()) for i in range(3)]
        lm = [float(sd[f"app_line.{i}"].abs().max()) for i in range(3)]
        light_max = max(1.0, float(sd["light_line.weight"].abs().max()))
        k = max(range(3), key=lambda i: pm[i] * lm[i])
        g = (5.5e4 / (pm[k] * lm[k] * light_max)) ** 0.5
        for i in range(3):
            sd[f"app_plane.{i}"] *= g
            sd[f"app_line.{i}"] *= g
        c, node = 5, [grid[a] // 3 for a in range(3)]
        m0, m1 = MAT_MODE[k]
        sd[f"app_plane.{k}"][0, c, node[m1], node[m0]] = float(sd[f"app_plane.{k}"].abs().max())
        sd[f"app_line.{k}"][0, c, node[VEC_MODE[k]], 0] = float(sd[f"app_line.{k}"].abs().max())
        sd["light_line.weight"][:, k * CA + c] = light_max
        fld.planted = torch.tensor([[node[a] / (grid[a] - 1) * 2 - 1 for a in range(3)]], dtype=F32)
        fld.planted_channel = k * CA + c
    fld.planes = [sd[f"app_plane.{i}"][0] for i in range(3)]                    # [48, grid[m1], grid[m0]]  (views: the checkpoint's own)
    fld.lines = [sd[f"app_line.{i}"][0, :, :, 0] for i in range(3)]             # [48, grid[vec]]
    fld.light = sd["light_line.weight"]                                        # [L, 144]
    fld.basis = sd["basis_mat.weight"]                                         # [27, 144]
    cal = types.SimpleNamespace(n=512, xyz=torch.rand(512, 3, generator=torch.Generator().manual_seed(_seed("cal", name))) * 1.8 - 0.9)
    f = products(fld, cal.xyz, torch.zeros(512, dtype=torch.long), F64) @ fld.basis.double().T
    fld.basis *= float((0.25 if regime == "small" else 0.8) / f.pow(2).mean().sqrt())
    if regime == "huge":
        fld.basis *= 125.0
        fld.basis[3] *= 10.0
        fld.basis[20] *= 1000.0
    fld.volume = functools.lru_cache(maxsize=None)(lambda: dense_volume(fld))
    return fld


def points(fld, gen, n_each=120):
    """The point classes of _points in tests/test_gpu_dense_app.py on the field's own grid -> (xyz [m, 3] float32, class id [m])."""
    g = fld.grid
    u = lambda m: torch.rand(m, 3, generator=gen) * 2 - 1
    cls = [u(2 * n_each)]
    cls.append(torch.stack([torch.randint(0, g[a], (n_each,), generator=gen).float() / (g[a] - 1) * 2 - 1 for a in range(3)], 1))
    faces, last = [], []
    for a in range(3):
        for edge in (-1.0, 1.0):
            q = u(n_each // 6)
            q[:, a] = edge
            faces.append(q)
        q = u(n_each // 3)
        q[:, a] = 1.0 - torch.rand(n_each // 3, generator=gen) * 2.0 / (g[a] - 1)
        last.append(q)
    cls += [torch.cat(faces), torch.cat(last), u(n_each) * 1.08]
    cls.append(torch.tensor([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]))
    if fld.planted is not None:
        cls.append(fld.planted.expand(4, 3))
    xyz = torch.cat(cls).float().contiguous()
    ids = torch.cat([torch.full((c.shape[0],), i) for i, c in enumerate(cls)])
    return xyz, ids


@functools.lru_cache(maxsize=None)
def population(fname, addr="nomap", n=POP):
    """The seeded record population of (field, addressing): n records drawn from every point class (the eight corners and the planted
    node among them), pair ids, per-ray light indices with -1 and n_lights + 3 among valid ones, unit directions."""
    fld = field(fname)
    gen = torch.Generator().manual_seed(_seed("records", fname, addr, n))
    xyz, ids = points(fld, gen, max(120, n // 5))
    tail = ids >= POINT_CLASSES.index("corners")                              # corners and the planted node: always in, the rest drawn
    rest = torch.nonzero(~tail).view(-1)
    keep = torch.cat([torch.nonzero(tail).view(-1), rest[torch.randperm(rest.numel(), generator=gen)[:n - int(tail.sum())]]])
    keep = keep[torch.randperm(n, generator=gen)]
    xyz, ids = xyz[keep].contiguous(), ids[keep]
    L = fld.n_lights
    if addr == "nomap":
        rec_map, idx_div, aux_mod, n_rays, n_dirs = None, 1, 0, n, n
    else:
        idx_div, aux_mod, pairs = {"d3": (3, 3, 120), "d16": (16, 16, 320), "div5mod7": (5, 7, 210)}[addr]
        rec_map = torch.randint(0, pairs, (n,), generator=gen)
        n_rays, n_dirs = (pairs + idx_div - 1) // idx_div, aux_mod
        rec_map[0], rec_map[n // 2], rec_map[n - 1] = pairs - 1, 0, 2 * idx_div + idx_div - 1
        rec_map[min(3, n - 1)] = idx_div                                       # ray 1 (light index -1), ray 2 above (n_lights + 3)
        rec_map = rec_map.int()
    light_idx = torch.arange(n_rays) % L                                       # every light row (n_rays >= n_lights + 3 everywhere) ...
    light_idx[0], light_idx[1], light_idx[2] = L - 1, -1, L + 3                # ... and two indices outside [0, n_lights)
    dirs = torch.nn.functional.normalize(torch.randn(n_dirs, 3, generator=gen), dim=-1)
    return types.SimpleNamespace(name=f"{fname}-{addr}-{n}", field=fname, addr=addr, n=n, xyz=xyz, ids=ids, rec_map=rec_map, idx_div=idx_div,
                                 aux_mod=aux_mod, light_idx=light_idx.int(), dirs=dirs.contiguous())


def head(rec, n):
    """The first n records of a population (a launch of n rows): its own pair ids and points, the population's rays and directions."""
    if n == rec.n:
        return rec
    r = types.SimpleNamespace(**rec.__dict__)
    r.name, r.n, r.xyz, r.ids = f"{rec.name}[:{n}]", n, rec.xyz[:n].contiguous(), rec.ids[:n]
    r.rec_map = None if rec.rec_map is None else rec.rec_map[:n].contiguous()
    return r


# ---- decoders ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def saturating_decoder(dec):
    """decoder_reference's weights with six entries each of W0 (feature columns: raw, sin and cos) and W1 set to magnitudes in [8, 16):
    there (W - fp16(W)) 2^17 exceeds 448 and the e4m3 residue saturates.  max |W0| and max |W1| lie in [8, 16)."""
    w = {k: v.clone() for k, v in D.decoder(dec).items()}
    gen = torch.Generator().manual_seed(_seed("saturating", dec))
    vals = torch.tensor([8.0009765625, -9.3, 11.7, -13.1, 15.99, -8.77])
    for key, cols in (("w0", [2, 30 + 7, 30 + 54 + 20, 16, 30 + 41, 30 + 54 + 3]), ("w1", torch.randint(0, D.HID, (6,), generator=gen).tolist())):
        units = torch.randperm(D.HID, generator=gen)[:6].tolist()
        for u, c, v in zip(units, cols, vals.tolist()):
            w[key][u, c] = v
    # layer 3 set again from the float64 pre-activations of a calibration set, as decoder_reference.decoder does: the columns spread
    od, act, _ = D.DECODERS[dec]
    x = D.input_row((torch.randn(700, FEAT, generator=gen) * 0.8).double(), torch.randn(700, 3, generator=gen).double())
    h2 = torch.relu(torch.relu(x @ w["w0"].double().T + w["b0"].double()) @ w["w1"].double().T + w["b1"].double())
    z3 = h2 @ w["w2"].double().T
    scale = (0.8 if act == 1 else 1.5) / z3.std(0)
    w["w2"] = (w["w2"].double() * scale[:, None]).float()
    w["b2"] = (0.2 * torch.arange(1, od + 1) / od - z3.mean(0) * scale).float()
    return w


@functools.lru_cache(maxsize=None)
def huge_decoder(dec):
    """decoder_reference's |feat| ~ 100 weights for the huge regime: the raw-feature columns of the two inflated features (3: x 10,
    20: x 1000, mostly clamped to +-65504) weigh 0.1 and 0.001 as much, so that the hidden layers stay mixed."""
    w = {k: v.clone() for k, v in D.decoder(dec, "large").items()}
    w["w0"][:, 3] *= 0.1
    w["w0"][:, 20] *= 0.001
    return w


def weights(fname, dec, wkind=None):
    if wkind == "saturating":
        return saturating_decoder(dec)
    return huge_decoder(dec) if FIELDS[fname][1] == "huge" else D.decoder(dec)


# ---- yardsticks ------------------------------------------------------------------------------------------------------------------------
def refs(fname, addr="nomap", dec="sig3", n=POP, wkind=None):
    """float64 and the yardsticks of one (field, addressing, decoder, weight set), once: feat / out per class.  Rows are independent, so
    the references of a launch of fewer rows are the first rows of these."""
    return _refs(fname, addr, dec, n, wkind)


@functools.lru_cache(maxsize=None)
def _refs(fname, addr, dec, n, wkind):
    fld, rec = field(fname), population(fname, addr, n)
    w = weights(fname, dec, wkind)
    r = types.SimpleNamespace(rec=rec, w=w)
    r.feat64, r.out64 = forward(fld, rec, dec, F64, w=w)
    r.feat64_raw = features(fld, rec, F64)
    r.feat32, r.out32 = forward(fld, rec, dec, F32, w=w)
    if fld.regime != "huge":
        r.feat_h16 = h16_features(fld, rec)
        r.out_h16 = f16_decode(rec, dec, r.feat_h16, w)
        if fld.n_lights == 1:
            r.feat_dense = dense_features(fld, rec)
            r.out_dense = f16_decode(rec, dec, r.feat_dense, w)
    if fld.n_lights <= 8:
        r.feat_hp = hp_features(fld, rec)
        r.out_hp = hp_decode(rec, dec, r.feat_hp, w)
    return r


def bias_distance(got, f64):
    """max over the output channels of |mean signed deviation| / max |float64|."""
    a, b = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(f64).double()
    return float((a - b).mean(0).abs().max() / b.abs().max())


def bias_bound(yard, f64):
    return 10 * max(bias_distance(yard, f64), 2.0 ** -24)
