"""Material editing on the GPU (tensoir_amd/csrc/tir_materials.hip, tensoir_amd/materials.py): the kernels alone
against the float64 restatement (tests/materials_reference.py), deterministic k-means on the fixture, and the plumbing through
relight_view, bake_atlas / export_textured and the bake command line.

Tolerance of tir_material_edit: ten times the largest deviation of the restatement run in float32 from the one run in float64
on the case's own rows and edit list (the bound of DESIGN 4.17's lighting row); for the map rows, on the rows the error is taken
over (acc > acc_thres).  Where that deviation is 0 -- the empty list, and any case whose float32 run happens to round without
error -- the bound is 0 and the device must equal the float64 restatement exactly: the kernels are built without fused
multiply-adds, so their arithmetic is the float32 restatement's.  Every hard test (feather = 0, palette entry) of the inputs keeps
at least 1e-5 from its boundary, asserted on the restatement; no row is excluded.  Printed per case: the float32 deviation, the
bound and the device's deviation.

k-means: labels after every pass, the number of passes and the counts equal the restatement's; a centroid is within one fp32 ulp
of it (the double sums differ from the exact mean by <= N 2^-53 relative, far below half an ulp, so only a mean on a rounding
boundary may move); the restatement's gap between a row's best and second-best d2 is asserted above the fp32 error of a
difference of two d2 <= 4 (2 x 2e-6) -- for the shapes here it is >= 7.5e-5, for k = 32 on 915 rows 5.2e-6."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import materials_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1001, -1002
KEYS = ("albedo", "roughness", "fresnel", "base", "metal")


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def pool(M=257, seed=11):
    """Surface rows: positions in the unit cube, three albedo families plus noise, roughness in the decoder's range."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    fam = np.float32([[0.8, 0.15, 0.1], [0.15, 0.2, 0.75], [0.5, 0.5, 0.45]])[rng.integers(0, 3, M)]
    a = np.clip(fam + rng.normal(0, 0.04, (M, 3)), 0.01, 0.99).astype(np.float32)
    r = rng.uniform(0.09, 0.99, M).astype(np.float32)
    f = rng.uniform(0.02, 0.08, (M, 3)).astype(np.float32)
    return x, a, r, f


PALETTE = (np.float32([[0.8, 0.15, 0.1, 0.3], [0.15, 0.2, 0.75, 0.6], [0.5, 0.5, 0.45, 0.5], [0.5, 0.5, 0.45, 0.2]]), 0.5)


def edit_list(n):
    from tensoir_amd.materials import EditList, MaterialEdit as E
    one = [E(strength=0.75, sphere_center=(0.1, -0.2, 0.3), sphere_radius=0.6, sphere_feather=0.5, albedo_mode="recolor",
             color=(0.1, 0.3, 0.9), roughness_scale=0.5, roughness_offset=0.1, metallic=0.8)]
    if n <= 1:
        return EditList(one[:n], palette=PALETTE)
    rng = np.random.default_rng(5)
    edits = list(one)
    modes = ("set", "multiply", "recolor", "keep")
    for i in range(1, 16):
        kw = {"strength": float(rng.uniform(0.2, 1.0))}
        which = i % 5
        if which == 0:
            kw.update(sphere_center=tuple(rng.uniform(-0.5, 0.5, 3)), sphere_radius=float(rng.uniform(0.3, 0.9)),
                      sphere_feather=0.0 if i % 2 else 0.3)
        elif which == 1:
            kw.update(box_center=tuple(rng.uniform(-0.5, 0.5, 3)), box_half=tuple(rng.uniform(0.2, 0.8, 3)), box_feather=0.0 if i % 2 else 0.4)
        elif which == 2:
            kw.update(select_color=(0.8, 0.15, 0.1) if i % 2 else (0.15, 0.2, 0.75), color_tolerance=0.12, color_feather=0.0 if i > 8 else 0.2)
        elif which == 3:
            kw.update(roughness_band=(0.3, 0.6), band_feather=0.0 if i % 2 else 0.15, box_center=(0, 0, 0), box_half=(0.9, 0.9, 0.9),
                      box_feather=0.2)
        else:
            kw.update(palette_id=int(i % 4))
        mode = modes[i % 4]
        if mode != "keep":
            kw.update(albedo_mode=mode, color=tuple(rng.uniform(0.05, 0.95 if mode != "multiply" else 1.6, 3)))
        if i % 3 == 0:
            kw.update(metallic=float(rng.uniform(0, 1)))
        if i % 4 == 1:
            kw.update(roughness_scale=float(rng.uniform(0, 1.5)), roughness_offset=float(rng.uniform(-0.2, 0.3)))
        edits.append(E(**kw))
    return EditList(edits, palette=PALETTE)


def restate(el, x, a, r, f, dtype=np.float64):
    return R.apply(el.records(), el.centroids, el.rough_weight, x, a, r, f, dtype)


def deviation(got, want, rows=slice(None), keys=KEYS):
    return max(float(np.abs(np.asarray(got[k], np.float64)[rows] - want[k][rows]).max()) if np.size(want[k][rows]) else 0.0 for k in keys)


def bound_of(el, x, a, r, f, rows=slice(None), keys=KEYS):
    """(10 x the float32 restatement's deviation from the float64 one on `rows` of these inputs, that deviation, the float64
    result); the hard tests of the inputs keep their margin"""
    ref = restate(el, x, a, r, f)
    assert ref["margin"] >= 1e-5, ref["margin"]
    d32 = deviation(restate(el, x, a, r, f, np.float32), ref, rows, keys)
    return 10 * d32, d32, ref


def map_rows(x, a, r, f, seed=3):
    """[M, 20] map rows and rays whose surface points lie at x up to rounding; every third row is background (acc <= 0.5)."""
    M = a.shape[0]
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, (M, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    maps = rng.uniform(0, 1, (M, 20)).astype(np.float32)
    maps[:, 3] = rng.uniform(0.5, 2.5, M)
    rays = np.concatenate([x - maps[:, 3:4].astype(np.float64) * d, d], 1).astype(np.float32)
    maps[:, 7:10], maps[:, 10], maps[:, 11:14] = a, r, f
    maps[:, 14] = np.where(np.arange(M) % 3 == 2, rng.uniform(0, 0.5, M), rng.uniform(0.500001, 1, M))
    maps[min(4, M - 1), 14] = 0.5                                       # AT the threshold: background
    surf = rays[:, :3] + maps[:, 3:4] * rays[:, 3:]                     # float32 numpy: the product and the sum rounded on their own
    return maps, rays, surf.astype(np.float32)


SIZES = [1, 63, 64, 65, 257]
LENGTHS = [0, 1, 16]


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("M", SIZES)
def test_edit_arrays_match_the_restatement(M, n):
    from tensoir_amd import ops
    el = edit_list(n)
    x, a, r, f = (t[:M] for t in pool())
    bound, d32, ref = bound_of(el, x, a, r, f)
    rec, cent = el.on("cuda")
    got = ops.material_edit(rec, cent, el.rough_weight, dev(x), dev(a), dev(r), dev(f))
    # the same rows as column views of wider rows: [M, 20]-style storage at strides 7, 5, 2, 6
    wide = [torch.full((M, s), -3.0, device="cuda") for s in (7, 5, 2, 6)]
    for w, src, c0 in zip(wide, (x, a, r[:, None], f), (2, 1, 1, 3)):
        w[:, c0:c0 + src.shape[1]] = dev(src)
    views = [wide[0][:, 2:5], wide[1][:, 1:4], wide[2][:, 1], wide[3][:, 3:6]]
    strided = ops.material_edit(rec, cent, el.rough_weight, *views)
    torch.cuda.synchronize()
    if M > 1:
        assert views[0].stride(0) == 7 and not views[1].is_contiguous()
    out = {k: got[k].cpu().numpy() for k in KEYS}
    err = deviation(out, ref)
    print(f"\n[material_edit arrays] M {M} edits {n}: float32 restatement {d32:.3e}, bound {bound:.3e}, device {err:.3e}")
    assert err <= bound
    for k in KEYS:
        assert torch.equal(bits(strided[k]), bits(got[k])), k          # the stride changes nothing
    keep = ~ref["touched"]
    for k, src in (("albedo", a), ("base", a), ("roughness", r), ("fresnel", f)):
        assert np.array_equal(out[k][keep].view(np.uint32), src[keep].view(np.uint32)), k     # unselected rows: their bits
    assert (out["metal"][keep] == 0).all()
    if n == 0:
        assert keep.all()
    if n == 16 and M == 257:
        assert ref["touched"].sum() > 20 and ref["metal"].max() > 0.1


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("M", SIZES)
def test_edit_maps_match_the_restatement(M, n):
    from tensoir_amd import ops
    el = edit_list(n)
    x, a, r, f = pool()
    maps, rays, surf = (t[:M] for t in map_rows(x, a, r, f))            # a prefix of the pool's map rows
    a, r, f = a[:M], r[:M], f[:M]
    hit = maps[:, 14] > 0.5
    bound, d32, ref = bound_of(el, surf, a, r, f, hit, ("albedo", "roughness", "fresnel"))     # on the rows the error is taken over
    rec, cent = el.on("cuda")
    dm = dev(maps)
    before = dm.clone()
    ops.material_edit_maps(rec, cent, el.rough_weight, dm, dev(rays), 0.5)
    c = ops.surface_compact(before, dev(rays), 0.5)
    torch.cuda.synchronize()
    got = dm.cpu().numpy()
    n_hit = int(c["n_hit"].item())
    assert n_hit == hit.sum()
    # the position the edit saw is surface_compact's: the float32 restatement's, bit for bit
    assert np.array_equal(c["surf"][:n_hit].cpu().numpy().view(np.uint32), surf[hit].view(np.uint32))
    out = {"albedo": got[:, 7:10], "roughness": got[:, 10], "fresnel": got[:, 11:14]}
    err = max(float(np.abs(out[k][hit].astype(np.float64) - ref[k][hit]).max()) if hit.any() else 0.0 for k in out)
    print(f"\n[material_edit maps] M {M} edits {n}: hit {int(hit.sum())}, float32 restatement {d32:.3e}, bound {bound:.3e}, device {err:.3e}")
    assert err <= bound
    same = ~(hit & ref["touched"])                                      # background rows and unselected rows keep every bit
    assert np.array_equal(got[same].view(np.uint32), maps[same].view(np.uint32))
    other = [c for c in range(20) if c not in (7, 8, 9, 10, 11, 12, 13)]
    assert np.array_equal(got[:, other].view(np.uint32), maps[:, other].view(np.uint32))
    if n > 0 and M >= 63:
        assert (hit & ref["touched"]).sum() > 5 and not np.array_equal(got, maps)


def test_both_instantiations_agree_bit_for_bit():
    """The map rows of a chunk edited in place, then compacted, are the compacted rows edited out of place: one row function,
    and the position of a map row is surface_compact's surf."""
    from tensoir_amd import materials, ops
    el = edit_list(16)
    x, a, r, f = pool()
    maps, rays, _ = map_rows(x, a, r, f)
    dm, dr = dev(maps), dev(rays)
    c0 = ops.surface_compact(dm, dr, 0.5)
    want = materials.apply(c0["surf"], c0["albedo"], c0["rough"], c0["fresnel"], el, m_dev=c0["n_hit"])
    materials.apply_to_maps(dm, dr, el, 0.5)
    c1 = ops.surface_compact(dm, dr, 0.5)
    n = int(c0["n_hit"].item())
    assert n == int(c1["n_hit"].item()) and n > 100
    for k0, k1 in (("albedo", "albedo"), ("roughness", "rough"), ("fresnel", "fresnel")):
        assert torch.equal(bits(want[k0][:n]), bits(c1[k1][:n])), k0
    assert torch.equal(bits(c0["surf"][:n]), bits(c1["surf"][:n]))


def raw_edit(el, x, a, r, f, M, m_dev, outs):
    from tensoir_amd import _lib
    rec, cent = el.on("cuda")
    rc = _lib.lib().tir_material_edit(rec.data_ptr() if len(el) else None, len(el), cent.data_ptr(), cent.shape[0], el.rough_weight,
                                      x.data_ptr(), 3, a.data_ptr(), 3, r.data_ptr(), 1, f.data_ptr(), 3, *[o.data_ptr() for o in outs],
                                      M, None if m_dev is None else m_dev.data_ptr(), None)
    torch.cuda.synchronize()
    return rc


def test_rows_beyond_the_count_are_not_written():
    el = edit_list(16)
    x, a, r, f = (dev(t) for t in pool())
    M = 257
    full = [torch.full(s, 7.0, device="cuda") for s in ((M, 3), (M,), (M, 3), (M, 3), (M,))]
    assert raw_edit(el, x, a, r, f, M, None, full) == 0
    for count in (0, 1, 64, 200, 257, 300, -5):
        outs = [torch.full(s, 7.0, device="cuda") for s in ((M + 2, 3), (M + 2,), (M + 2, 3), (M + 2, 3), (M + 2,))]
        assert raw_edit(el, x, a, r, f, M, torch.tensor([count], dtype=torch.int32, device="cuda"), outs) == 0
        n = min(max(count, 0), M)
        for o, w in zip(outs, full):
            assert torch.equal(bits(o[:n]), bits(w[:n])) and bool((o[n:] == 7.0).all())
    # capacity M smaller than the arrays: rows >= M stay
    outs = [torch.full(s, 7.0, device="cuda") for s in ((M, 3), (M,), (M, 3), (M, 3), (M,))]
    assert raw_edit(el, x, a, r, f, 65, None, outs) == 0
    for o, w in zip(outs, full):
        assert torch.equal(bits(o[:65]), bits(w[:65])) and bool((o[65:] == 7.0).all())
    # base and metal are optional
    from tensoir_amd import _lib
    rec, cent = el.on("cuda")
    three = [torch.full(s, 7.0, device="cuda") for s in ((M, 3), (M,), (M, 3))]
    rc = _lib.lib().tir_material_edit(rec.data_ptr(), len(el), cent.data_ptr(), 4, el.rough_weight, x.data_ptr(), 3, a.data_ptr(), 3,
                                      r.data_ptr(), 1, f.data_ptr(), 3, *[o.data_ptr() for o in three], None, None, M, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and all(torch.equal(bits(o), bits(w)) for o, w in zip(three, full))


def test_palette_selector_label_is_the_assign_kernels():
    """metal = id / 16 where the row's palette entry is id: the labels tir_material_edit selected by are tir_kmeans_assign's, on
    near-tied rows and on a duplicated centroid."""
    from tensoir_amd import ops
    from tensoir_amd.materials import EditList, MaterialEdit as E
    a, r = R.fixture()
    k, wr = 16, 0.7
    cent = ops.kmeans_seed(dev(a), dev(r), k, wr)
    cent[9] = cent[2]                                                   # an exact tie between two entries: the lower index wins
    # rows on the perpendicular bisector of two centroids, up to rounding
    c = cent.cpu().numpy().astype(np.float64)
    mid = np.float32([(c[i] + c[j]) / 2 for i in range(8) for j in range(i + 1, 8)])
    a2 = np.concatenate([a, np.clip(mid[:, :3], 0, 1)]).astype(np.float32)
    r2 = np.concatenate([r, np.clip(mid[:, 3] / wr, 0, 1.4)]).astype(np.float32)
    N = a2.shape[0]
    el = EditList([E(palette_id=j, metallic=j / 16) for j in range(k)], palette=(cent, wr))
    rec, pc = el.on("cuda")
    assert torch.equal(pc, cent)
    out = ops.material_edit(rec, pc, wr, torch.zeros((N, 3), device="cuda"), dev(a2), dev(r2), torch.zeros((N, 3), device="cuda"))
    labels = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    ops.kmeans_assign(dev(a2), dev(r2), cent, labels, ops.kmeans_workspace(N, k, "cuda"), True, wr)
    torch.cuda.synchronize()
    assert torch.equal((out["metal"] * 16).to(torch.int32), labels) and torch.equal(out["metal"] * 16, labels.float())
    lab, _, gap = R.label(a2, r2, cent.cpu().numpy(), wr)
    sure = gap >= 1e-5
    assert np.array_equal(labels.cpu().numpy()[sure], lab[sure]) and (~sure).sum() >= 1 and 9 not in labels.cpu().tolist()
    print(f"\n[palette label] {N} rows, {int((~sure).sum())} within 1e-5 of a tie, labels used {sorted(set(labels.cpu().tolist()))}")


def test_every_refusal_returns_its_code():
    from tensoir_amd import _lib
    L = _lib.lib()
    t = torch.full((64,), 7.0, device="cuda")
    ti = torch.full((64,), 7, dtype=torch.int64, device="cuda")
    p, pi = t.data_ptr(), ti.data_ptr()
    inf, nan = float("inf"), float("nan")

    def edit(n=1, k=0, wr=1.0, strides=(3, 3, 1, 3), M=4, e=p, pal=None, arrays=(p,) * 7):
        return L.tir_material_edit(e, n, pal, k, wr, arrays[0], strides[0], arrays[1], strides[1], arrays[2], strides[2], arrays[3],
                                   strides[3], arrays[4], arrays[5], arrays[6], None, None, M, None, None)
    assert edit(M=0) == 0 and edit(n=0, e=None, M=0) == 0
    for bad in (dict(n=-1), dict(n=17), dict(k=-1), dict(k=33, pal=p), dict(wr=inf), dict(wr=nan), dict(M=-1), dict(e=None),
                dict(k=2, pal=None), dict(strides=(2, 3, 1, 3)), dict(strides=(3, 2, 1, 3)), dict(strides=(3, 3, 0, 3)),
                dict(strides=(3, 3, 1, 2))) + tuple(dict(arrays=tuple(None if j == i else p for j in range(7))) for i in range(7)):
        assert edit(**bad) == ERR_ARG, bad
    assert edit(M=2 ** 31) == ERR_UNSUPPORTED

    def maps(n=1, k=0, wr=1.0, B=2, thres=0.5, e=p, pal=None, m=p, rays=p):
        return L.tir_material_edit_maps(e, n, pal, k, wr, m, rays, B, thres, None)
    assert maps(B=0) == 0 and maps(n=0, e=None) == 0
    for bad in (dict(n=-1), dict(n=17), dict(k=33, pal=p), dict(k=1), dict(wr=nan), dict(B=-1), dict(thres=nan), dict(e=None), dict(m=None),
                dict(rays=None)):
        assert maps(**bad) == ERR_ARG, bad
    assert maps(B=2 ** 31) == ERR_UNSUPPORTED

    def metal(orm=p, size=12, cols=2, T=6, F=4, m=p):
        return L.tir_atlas_metal(orm, size, cols, T, F, m, None)
    assert metal(F=0, m=None) == 0
    for bad in (dict(orm=None), dict(size=5), dict(cols=0), dict(cols=3), dict(F=-1), dict(F=9), dict(orm=p + 1), dict(m=None)):
        assert metal(**bad) == ERR_ARG, bad
    assert metal(T=5) == ERR_UNSUPPORTED and metal(size=8193, cols=1) == ERR_UNSUPPORTED

    assert L.tir_kmeans_groups(-1) == ERR_ARG and L.tir_kmeans_groups(2 ** 31) == ERR_UNSUPPORTED
    assert [L.tir_kmeans_groups(n) for n in (0, 1, 256, 257)] == [0, 1, 1, 2]

    def seed(N=8, wr=1.0, k=2, have=1, ptrs=(p, p, p, p, pi)):
        return L.tir_kmeans_seed(ptrs[0], ptrs[1], N, wr, ptrs[2], k, have, ptrs[3], ptrs[4], None)
    for bad in (dict(N=0), dict(N=-1), dict(k=0), dict(k=33), dict(have=-1), dict(have=2), dict(wr=inf), dict(ptrs=(p, p, p, p, pi + 4))) \
            + tuple(dict(ptrs=tuple(None if j == i else q for j, q in enumerate((p, p, p, p, pi)))) for i in range(5)):
        assert seed(**bad) == ERR_ARG, bad
    assert seed(N=2 ** 31) == ERR_UNSUPPORTED

    def assign(N=8, wr=1.0, k=2, G=1, ptrs=(p,) * 7):
        return L.tir_kmeans_assign(ptrs[0], ptrs[1], N, wr, ptrs[2], k, 1, ptrs[3], ptrs[4], ptrs[5], ptrs[6], G, None)
    for bad in (dict(N=0), dict(N=-1), dict(k=0), dict(k=33), dict(wr=nan), dict(G=2), dict(N=257, G=1)) \
            + tuple(dict(ptrs=tuple(None if j == i else p for j in range(7))) for i in range(7)):
        assert assign(**bad) == ERR_ARG, bad
    assert assign(N=2 ** 31, G=2 ** 23) == ERR_UNSUPPORTED

    def update(G=1, k=2, ptrs=(p,) * 7):
        return L.tir_kmeans_update(ptrs[0], ptrs[1], ptrs[2], G, ptrs[3], k, ptrs[4], ptrs[5], ptrs[6], None)
    for bad in (dict(G=0), dict(G=-1), dict(G=2 ** 23 + 1), dict(k=0), dict(k=33)) + tuple(dict(ptrs=tuple(None if j == i else p for j in range(7))) for i in range(7)):
        assert update(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert bool((t == 7.0).all()) and bool((ti == 7).all())            # nothing was launched


def test_atlas_metal_writes_only_the_b_byte_of_owned_texels():
    from tensoir_amd import ops
    size, F = 27, 7
    cols, T = ops.atlas_layout(F, size)
    n_cells = (F + 1) // 2
    N = n_cells * T * T
    rng = np.random.default_rng(2)
    metal = rng.uniform(-0.2, 1.2, N).astype(np.float32)
    metal[3] = np.nan                                                   # a NaN counts as 0
    before = torch.from_numpy(rng.integers(0, 256, (size, size, 4)).astype(np.uint8)).cuda()
    orm = before.clone()
    ops.atlas_metal(orm, cols, T, F, dev(metal))
    torch.cuda.synchronize()
    want = before.cpu().numpy().copy()
    idx = np.arange(N)
    c, j, i = idx // (T * T), (idx % (T * T)) // T, idx % T
    want[(c // cols) * T + j, (c % cols) * T + i, 2] = np.rint(np.float32(255.0) * np.clip(np.nan_to_num(metal, nan=0.0), 0, 1)).astype(np.uint8)
    assert np.array_equal(orm.cpu().numpy(), want) and want[0, 3, 2] == 0
    assert not np.array_equal(want, before.cpu().numpy())


# ---- k-means ---------------------------------------------------------------------------------------------------------------------
def lloyd_on_device(a, r, k, wr=1.0, max_iters=50):
    """The host loop of materials.palette_of, keeping the labels of every pass."""
    from tensoir_amd import ops
    da, dr = dev(a), dev(r)
    N = a.shape[0]
    cent = ops.kmeans_seed(da, dr, k, wr)
    seeds = cent.clone()
    work = ops.kmeans_workspace(N, k, "cuda")
    labels = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    counts = torch.empty((k,), dtype=torch.int64, device="cuda")
    inertia = torch.empty((1,), dtype=torch.float64, device="cuda")
    changed = torch.empty((1,), dtype=torch.int32, device="cuda")
    history, changes = [], []
    for p in range(max_iters):
        ops.kmeans_assign(da, dr, cent, labels, work, p == 0, wr)
        ops.kmeans_update(work, cent, counts, inertia, changed)
        history.append(labels.cpu().numpy().copy())
        changes.append(int(changed.item()))
        if changes[-1] == 0:
            break
    return {"seeds": seeds.cpu().numpy(), "centroids": cent.cpu().numpy(), "history": history, "changes": changes,
            "counts": counts.cpu().numpy(), "inertia": float(inertia.item())}


def ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def check_kmeans(a, r, k, min_gap):
    ref = R.kmeans(a, r, k)
    assert ref["gap"] >= min_gap and ref["seed_gap"] >= min_gap, (ref["gap"], ref["seed_gap"])
    got = lloyd_on_device(a, r, k)
    assert np.array_equal(got["seeds"], R.features(a, r, 1.0)[ref["seed_rows"]])
    assert len(got["history"]) == ref["passes"]
    for p, (g, w) in enumerate(zip(got["history"], ref["history"])):
        assert np.array_equal(g, w), p
    assert got["changes"][0] == a.shape[0] and got["changes"][-1] == 0 and all(c > 0 for c in got["changes"][:-1])
    assert [int((x != y).sum()) for x, y in zip(got["history"][1:], got["history"][:-1])] == got["changes"][1:]
    assert np.array_equal(got["counts"], ref["counts"])
    u = ulps(got["centroids"], ref["centroids"])
    rel = abs(got["inertia"] - ref["inertia"]) / max(ref["inertia"], 1e-300)
    print(f"\n[kmeans] N {a.shape[0]} k {k}: {ref['passes']} passes, gap {ref['gap']:.3e}, centroids within {u} ulp, inertia "
          f"{got['inertia']:.6f} (relative {rel:.1e} from the float64 restatement's)")
    assert u <= 1 and rel <= 1e-5              # the inertia adds fp32 d2 values: their rounding, 6e-8 relative each, not the sum's
    return ref, got


@pytest.mark.parametrize("k", [4, 6])
def test_kmeans_fixture(k):
    from tensoir_amd import materials
    a, r = R.fixture()
    ref, got = check_kmeans(a, r, k, 1e-5)
    assert ref["passes"] == {4: 13, 6: 9}[k]
    p1, p2 = (materials.palette_of(dev(a), dev(r), k) for _ in range(2))
    torch.cuda.synchronize()
    assert p1.passes == p2.passes == ref["passes"] and p1.inertia == p2.inertia == got["inertia"]
    assert torch.equal(bits(p1.centroids), bits(p2.centroids)) and torch.equal(p1.counts, p2.counts) and torch.equal(p1.labels, p2.labels)
    order = R.order_by_count(ref["counts"])
    assert np.array_equal(p1.counts.cpu().numpy(), ref["counts"][order]) and np.array_equal(p1.centroids.cpu().numpy(), got["centroids"][order])
    assert np.array_equal(order[p1.labels.cpu().numpy()], ref["labels"])
    assert (np.diff(p1.counts.cpu().numpy()) <= 0).all() and p1.labels.dtype == torch.int32


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_kmeans_shapes(N, k):
    from tensoir_amd import materials
    a, r = R.fixture()
    if N < k:
        with pytest.raises(ValueError, match="cannot seed"):
            materials.palette_of(dev(a[:N]), dev(r[:N]), k)
        return
    check_kmeans(a[:N], r[:N], k, 1e-5)


def test_kmeans_32_clusters_and_an_empty_one():
    from tensoir_amd import ops
    a, r = R.fixture()
    check_kmeans(a, r, 32, 4e-6)
    # duplicate rows: the third seed is row 0 again, wins no row (the lower index takes the tie) and keeps its value
    da, dr = np.repeat(np.float32([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9]]), 3, axis=0), np.repeat(np.float32([0.2, 0.8]), 3)
    got = lloyd_on_device(da, dr, 3)
    assert np.array_equal(got["seeds"], R.features(da, dr, 1.0)[[0, 3, 0]])
    assert got["history"][-1].tolist() == [0, 0, 0, 1, 1, 1] and got["counts"].tolist() == [3, 3, 0]
    assert np.array_equal(got["centroids"][2], got["seeds"][2]) and len(got["history"]) == 2
    assert ops.KMEANS_ROWS == 256


# ---- plumbing: relight ---------------------------------------------------------------------------------------------------------
SIDE, SEED = 32, 77


@pytest.fixture(scope="module")
def view_scene():
    import contextlib
    import io
    import tensoir_amd
    from tensoir_amd import synth
    model = tensoir_amd.model_from_checkpoint(synth.make_checkpoint(grid=(96,) * 3), "cuda")
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        model.updateAlphaMask((48,) * 3)
    maps = synth.make_hdr_maps(["one"], 32, 64)
    return model, maps, synth.make_rays(SIDE, SIDE, narrow=1.0).cuda()


def fresh_env(maps, seed=SEED):
    from tensoir_amd import relight
    torch.manual_seed(seed)
    return relight.Environment_Light(hdr_maps=maps, device="cuda")


def view(scene, **kw):
    from tensoir_amd import relight
    model, maps, rays = scene
    return relight.relight_view(model, fresh_env(maps), list(maps), rays, SIDE, SIDE, num_samples=16, **kw)


@torch.no_grad()
def test_view_without_edits_keeps_its_bits(view_scene):
    from tensoir_amd.materials import EditList, MaterialEdit as E
    base = view(view_scene)
    hit = base["acc"] > 0.5
    assert 50 < int(hit.sum()) < hit.numel() - 50
    for edits in (None, EditList(), [], EditList([E(strength=0.0, albedo_mode="set", color=(1, 0, 0), metallic=1.0)])):
        v = view(view_scene, edits=edits)
        for key in ("rgb", "raw", "guide"):
            assert torch.equal(bits(v[key]), bits(base[key])), (key, edits)


@torch.no_grad()
def test_global_set_albedo_is_the_hand_pipeline(view_scene):
    from tensoir_amd import ops, relight
    from tensoir_amd.materials import EditList, MaterialEdit as E
    model, maps, rays = view_scene
    colour = (0.1, 0.6, 0.3)
    el = EditList([E(albedo_mode="set", color=colour)])
    v = view(view_scene, edits=el)
    base = view(view_scene)
    # by hand: primary pass -> the albedo of the compacted rows replaced -> importance-sampled relighting -> composition
    env = fresh_env(maps)
    n = SIDE * SIDE
    lidx = torch.zeros((n, 1), dtype=torch.int32, device="cuda")
    prim, rows = model(rays, lidx, _return_maps=True)
    c = ops.surface_compact(rows, rays, 0.5)
    col = torch.tensor(colour, device="cuda")
    albedo = c["albedo"] + (col - c["albedo"])                          # v += w (target - v) at w = 1, in fp32
    rgb = relight.relight_importance_sampled(model, env, "one", c["surf"], c["normal"], albedo, c["rough"], c["fresnel"], c["rays_d"],
                                             16, m_dev=c["n_hit"])
    out = torch.empty((n, 3), device="cuda")
    ops.env_compose(env.hdr_rgbs["one"], rays, c["slot"], rgb, out, 0)
    assert torch.equal(bits(v["rgb"][0].reshape(n, 3)), bits(out))
    assert not torch.equal(v["rgb"], base["rgb"])
    hit = (base["acc"] > 0.5).view(-1)
    g, g0 = v["guide"].view(n, 12), base["guide"].view(n, 12)
    assert float((g[hit][:, 8:11] - col).abs().max()) <= 2e-7           # the guide is built from the edited albedo
    assert torch.equal(bits(g[~hit]), bits(g0[~hit])) and torch.equal(bits(g[:, :8]), bits(g0[:, :8]))
    assert torch.equal(bits(v["rgb"][0].reshape(n, 3)[~hit]), bits(base["rgb"][0].reshape(n, 3)[~hit]))
    # the chunk call hands back the edited maps on hit rows and the untouched ones on background rows
    _, p1, c1 = relight.relight_chunk(model, fresh_env(maps), ["one"], rays, lidx, num_samples=16, edits=el)
    _, p0, _ = relight.relight_chunk(model, fresh_env(maps), ["one"], rays, lidx, num_samples=16)
    p0 = [t.clone() if torch.is_tensor(t) else t for t in p0]
    assert float((p1[3][hit] - col).abs().max()) <= 2e-7 and torch.equal(bits(p1[3][~hit]), bits(p0[3][~hit]))
    nh = int(c1["n_hit"].item())
    assert torch.equal(bits(c1["albedo"][:nh]), bits(albedo[:nh])) and torch.equal(bits(p1[3][hit]), bits(albedo[:nh]))
    for i in (0, 1, 2, 4, 5, 6):
        assert torch.equal(bits(p1[i]), bits(p0[i])), i                 # nothing the primary pass composited is re-rendered


@torch.no_grad()
def test_metallic_edit_changes_the_image_and_the_fresnel_rows(view_scene):
    from tensoir_amd import materials, ops, relight
    from tensoir_amd.materials import EditList, MaterialEdit as E
    model, maps, rays = view_scene
    n = SIDE * SIDE
    lidx = torch.zeros((n, 1), dtype=torch.int32, device="cuda")
    el = EditList([E(box_center=(1.0, 0.0, 0.0), box_half=(1.0, 3.0, 3.0), box_feather=0.5, metallic=1.0, roughness_scale=0.0,
                     roughness_offset=0.2)])                            # the half of the scene with x > 0, fading out to x = -0.5
    _, rows = model(rays, lidx, _return_maps=True)
    c = ops.surface_compact(rows.clone(), rays, 0.5)
    nh = int(c["n_hit"].item())
    want = materials.apply(c["surf"], c["albedo"], c["rough"], c["fresnel"], el, m_dev=c["n_hit"])
    out1, p1, c1 = relight.relight_chunk(model, fresh_env(maps), ["one"], rays, lidx, num_samples=16, edits=el)
    out0, _, _ = relight.relight_chunk(model, fresh_env(maps), ["one"], rays, lidx, num_samples=16)
    hit = p1[6] > 0.5
    assert float((out1[hit] - out0[hit]).abs().max()) > 0.02 and torch.equal(bits(out1[~hit]), bits(out0[~hit]))
    for key, col, ck in (("fresnel", 5, "fresnel"), ("albedo", 3, "albedo"), ("roughness", 4, "rough")):
        assert torch.equal(bits(p1[col][hit].reshape(nh, -1)), bits(want[key][:nh].reshape(nh, -1))), key
        assert torch.equal(bits(c1[ck][:nh]), bits(want[key][:nh])), key
    assert float(want["metal"][:nh].max()) > 0.5 and float((want["fresnel"][:nh] - c["fresnel"][:nh]).abs().max()) > 0.05


# ---- plumbing: the asset ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    from tests.train_sequence import reconstruct
    return reconstruct()


def asset_edits():
    from tensoir_amd.materials import EditList, MaterialEdit as E
    return EditList([E(box_center=(0.0, 0.0, 0.0), box_half=(0.4, 2.0, 2.0), box_feather=0.3, albedo_mode="recolor", color=(0.1, 0.2, 0.9),
                       metallic=0.9, roughness_scale=0.0, roughness_offset=0.25),
                     E(roughness_band=(0.0, 0.4), band_feather=0.1, albedo_mode="multiply", color=(1.2, 0.8, 0.8), strength=0.5)])


@torch.no_grad()
def test_bake_atlas_with_edits(trained, tmp_path):
    from tensoir_amd import bake, materials, mesh, ops
    m = trained.model
    grid = [int(g) for g in m.gridSize]
    size = 256
    verts, faces, normals = mesh.extract_mesh(m, simplify=3)
    F = faces.shape[0]
    plain = mesh.bake_atlas(m, verts, faces, normals, grid, size=size)
    none = mesh.bake_atlas(m, verts, faces, normals, grid, size=size, edits=None)
    for k in mesh.IMAGE_NAMES:
        assert torch.equal(plain[k], none[k]), k
    el = asset_edits()
    got = mesh.bake_atlas(m, verts, faces, normals, grid, size=size, edits=el)
    diffuse = mesh.bake_atlas(m, verts, faces, normals, grid, size=size, edits=el, color="diffuse")
    cols, T = ops.atlas_layout(F, size)
    point, outward, _ = ops.atlas_texels(verts, normals, faces, size, cols, T)
    p, d = mesh.field_positions(m.aabb, grid, point, outward)
    b = bake.bake_points(m, p.contiguous(), d.contiguous())
    e = materials.apply(b["surface"], b["albedo"], b["roughness"], torch.full_like(b["albedo"], 0.04), el)
    base, orm, normal = ops.atlas_pack(verts, normals, faces, size, cols, T, e["base"], e["roughness"], b["normal"], b["coverage"], ao=b["ao"])
    dbase, _, _ = ops.atlas_pack(verts, normals, faces, size, cols, T, e["albedo"], e["roughness"], b["normal"], b["coverage"],
                                 irradiance=b["irradiance"], ao=b["ao"])
    torch.cuda.synchronize()
    assert torch.equal(got["base"], base) and torch.equal(got["normal"], normal) and torch.equal(got["normal"], plain["normal"])
    assert torch.equal(got["orm"][..., [0, 1, 3]], orm[..., [0, 1, 3]]) and torch.equal(diffuse["base"], dbase)
    assert torch.equal(diffuse["orm"], got["orm"]) and not torch.equal(got["base"], plain["base"])
    N = point.shape[0]
    idx = np.arange(N)
    c, j, i = idx // (T * T), (idx % (T * T)) // T, idx % T
    want_b = np.zeros((size, size), np.uint8)
    metal = e["metal"].cpu().numpy()
    want_b[(c // cols) * T + j, (c % cols) * T + i] = np.rint(np.float32(255.0) * np.clip(metal, 0, 1)).astype(np.uint8)
    got_b = got["orm"][..., 2].cpu().numpy()
    owned = np.zeros((size, size), bool)
    owned[(c // cols) * T + j, (c % cols) * T + i] = True
    assert np.array_equal(got_b, want_b) and (got_b[~owned] == 0).all() and (plain["orm"][..., 2] == 0).all()
    touched = int((metal > 0).sum())
    print(f"\n[atlas edits] {F} faces, T {T}: {touched} of {N} texels carry metal, largest byte {int(got_b.max())}")
    assert 0 < touched < N and got_b.max() > 100
    # the file records the list; the command line writes the same file
    glb, cli, ej = (str(tmp_path / n) for n in ("edited.glb", "cli.glb", "edits.json"))
    mesh.export_textured(m, glb, simplify=3, size=size, edits=el)
    file = mesh.read_glb(glb)
    assert file["json"]["extras"]["tensoir_amd"]["edits"] == el.to_json()
    assert materials.EditList.from_json(file["json"]["extras"]["tensoir_amd"]["edits"]) == el
    for k in mesh.IMAGE_NAMES:
        assert np.array_equal(file["images"][k], got[k].cpu().numpy()), k
    with open(ej, "w") as h:
        json.dump(el.to_json(), h)
    ckpt = str(tmp_path / "trained.th")
    m.save(ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tensoir_amd.bake", ckpt, cli, "--simplify", "3", "--texture-size", str(size), "--edits", ej,
                        "--palette", "3", "--palette-samples", "4096"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(cli, "rb").read() == open(glb, "rb").read()
    line = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith('{"palette"')))
    assert len(line["palette"]["centroids"]) == 3 and sorted(line["palette"]["counts"], reverse=True) == line["palette"]["counts"]


@torch.no_grad()
def test_palette_of_a_model_repeats_and_partitions(trained):
    from tensoir_amd import materials
    m = trained.model
    s = materials.surface_samples(m, samples=8192, simplify=3)
    n = s["albedo"].shape[0]
    p1 = materials.palette(m, 4, samples=8192, max_iters=300, simplify=3)
    p2 = materials.palette(m, 4, samples=8192, max_iters=300, simplify=3)
    assert 1000 < n <= 8192 and p1.labels.shape == (n,) and p1.passes < 300      # converged: the labels are the final centroids'
    assert torch.equal(bits(p1.centroids), bits(p2.centroids)) and torch.equal(p1.counts, p2.counts) and torch.equal(p1.labels, p2.labels)
    assert p1.passes == p2.passes and p1.inertia == p2.inertia
    lab = p1.labels.cpu().numpy()
    assert lab.min() >= 0 and lab.max() < 4                             # disjoint by construction, and every covered sample has one
    assert np.array_equal(np.bincount(lab, minlength=4), p1.counts.cpu().numpy()) and int(p1.counts.sum()) == n
    assert (np.diff(p1.counts.cpu().numpy()) <= 0).all()
    # the palette selects the same rows through an edit list
    el = materials.EditList([materials.MaterialEdit(palette_id=j, metallic=(j + 1) / 4) for j in range(4)], palette=p1)
    out = materials.apply(s["points"], s["albedo"], s["roughness"], torch.zeros_like(s["albedo"]), el)
    assert torch.equal((out["metal"] * 4).to(torch.int32) - 1, p1.labels)
    print(f"\n[palette] {n} covered samples, counts {p1.counts.tolist()}, {p1.passes} passes")
