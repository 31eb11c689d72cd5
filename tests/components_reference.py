"""Connected components of a dense lattice, restated in numpy: the yardstick of tir_ccl_* / ops.label_components /
ops.keep_components (contract: include/tensoir_hip.h) and the named test volumes both test files share.

    label(vol, level, connectivity) -> labels [gx, gy, gz] int32: -1 where not vol > level (fp32; a NaN is outside), otherwise the
                                       smallest linear index ((x * gy + y) * gz + z) of the point's component
    table(labels)                   -> {"roots" [K] ascending, "sizes" [K], "boxes" [K, 6] inclusive (x0, y0, z0, x1, y1, z1)}, int32
    keep(vol, labels, table, keep, fill) -> vol where outside or the component's flag is set, else fill

label is a union-find over the list of links between inside neighbours (built with array slices), run as rounds of
"hang the larger root below the smaller" + full pointer jumping until no link joins two trees: parents only ever decrease, so a
root is the minimum of its set.  It shares nothing with the device code but that invariant; tests/test_components_cpu.py checks
it against scipy.ndimage.label.
"""
import numpy as np

# the 13 neighbours with a smaller linear index; the first three are the face neighbours
BACK = [(-1, 0, 0), (0, -1, 0), (0, 0, -1)] + [(dx, dy, dz) for dx in (-1, 0) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
                                              if (dx, dy, dz) < (0, 0, 0) and abs(dx) + abs(dy) + abs(dz) > 1]
assert len(BACK) == 13


def inside(vol, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(vol, np.float32) > np.float32(level)


def _links(cid, connectivity):
    """Pairs (a, b) of compact ids of inside points that are neighbours."""
    gx, gy, gz = cid.shape
    out = []
    for dx, dy, dz in BACK[:3 if connectivity == 6 else 13]:
        def sl(d, g):           # (slice of the point, slice of its neighbour at offset d)
            return (slice(1, g), slice(0, g - 1)) if d < 0 else (slice(0, g - 1), slice(1, g)) if d > 0 else (slice(0, g),) * 2
        (px, qx), (py, qy), (pz, qz) = sl(dx, gx), sl(dy, gy), sl(dz, gz)
        a, b = cid[px, py, pz], cid[qx, qy, qz]
        m = (a >= 0) & (b >= 0)
        out.append(np.stack([a[m], b[m]], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def label(vol, level, connectivity=6):
    assert connectivity in (6, 26)
    vol = np.asarray(vol)
    assert vol.ndim == 3
    ins = inside(vol, level)
    idx = np.flatnonzero(ins)                                  # ascending linear indices: compact id order = index order
    cid = np.full(vol.shape, -1, np.int64)
    cid.reshape(-1)[idx] = np.arange(len(idx))
    links = _links(cid, connectivity)
    parent = np.arange(len(idx))
    while len(links):
        ra, rb = parent[links[:, 0]], parent[links[:, 1]]
        live = ra != rb
        if not live.any():
            break
        links, ra, rb = links[live], ra[live], rb[live]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:                                            # pointer jumping: every point to its root
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    labels = np.full(vol.shape, -1, np.int32)
    labels.reshape(-1)[idx] = idx[parent].astype(np.int32)
    return labels


def table(labels):
    labels = np.asarray(labels)
    gx, gy, gz = labels.shape
    flat = labels.reshape(-1)
    idx = np.flatnonzero(flat >= 0)
    roots, inv, sizes = np.unique(flat[idx], return_inverse=True, return_counts=True)
    K = len(roots)
    boxes = np.empty((K, 6), np.int32)
    boxes[:, :3], boxes[:, 3:] = np.iinfo(np.int32).max, -1
    coords = np.stack(np.unravel_index(idx, labels.shape), 1).astype(np.int32) if len(idx) else np.zeros((0, 3), np.int32)
    for a in range(3):
        np.minimum.at(boxes[:, a], inv, coords[:, a])
        np.maximum.at(boxes[:, 3 + a], inv, coords[:, a])
    return {"roots": roots.astype(np.int32), "sizes": sizes.astype(np.int32), "boxes": boxes}


def keep(vol, labels, tab, flags, fill=0.0):
    vol = np.asarray(vol, np.float32)
    flags = np.asarray(flags, bool)
    assert flags.shape == tab["roots"].shape
    out = vol.copy()
    ins = labels >= 0
    comp = np.searchsorted(tab["roots"], labels[ins])
    drop = np.zeros(vol.shape, bool)
    drop[ins] = ~flags[comp]
    out[drop] = np.float32(fill)
    return out


def select(tab, keep_largest=None, min_voxels=None):
    """mesh.select_components, restated: the n largest (ties to the smaller root) and / or at least m voxels."""
    sizes = tab["sizes"].astype(np.int64)
    flags = np.ones(len(sizes), bool)
    if min_voxels is not None:
        flags &= sizes >= min_voxels
    if keep_largest is not None:
        ranked = sorted(range(len(sizes)), key=lambda k: (-sizes[k], k))[:keep_largest]
        top = np.zeros(len(sizes), bool)
        top[ranked] = True
        flags &= top
    return flags


# ---- the named volumes -----------------------------------------------------------------------------------------------------
def _checkerboard(shape):
    x, y, z = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    return (((x + y + z) & 1) == 0).astype(np.float32)


def _single():
    v = np.zeros((6, 5, 4), np.float32)
    v[3, 2, 1] = 1
    return v


def _line():
    v = ((np.arange(100) // 5) % 2 == 0).astype(np.float32)     # ten runs of five
    return v.reshape(1, 1, 100)


def _two_blobs(b_origin):
    v = np.zeros((9, 9, 9), np.float32)
    v[1:4, 1:4, 1:4] = 1
    x, y, z = b_origin
    v[x:x + 3, y:y + 3, z:z + 3] = 1
    return v


def serpentine(n=48):
    """One voxel-wide path: the z-rows (x even, y even) joined end to end by single voxels, boustrophedon in y and in x."""
    v = np.zeros((n, n, n), np.float32)
    end = n - 1                                               # z end of the row being left; alternates with every row
    xs = list(range(0, n, 2))
    for i, x in enumerate(xs):
        ys = list(range(0, n, 2))
        if i % 2:
            ys.reverse()
        for j, y in enumerate(ys):
            v[x, y, :] = 1
            if j + 1 < len(ys):
                v[x, (y + ys[j + 1]) // 2, end] = 1           # to the next row of this plane
            elif i + 1 < len(xs):
                v[x + 1, y, end] = 1                          # to the next plane
            end = (n - 1) - end
    return v


def smooth_noise(shape=(37, 50, 91), seed=5, passes=2, quantile=0.90):
    """Seeded white noise, box-filtered (3 taps, `passes` times per axis, edges replicated), thresholded at its own quantile:
    a few hundred irregular components.  -> (vol, level)"""
    v = np.random.default_rng(seed).standard_normal(shape).astype(np.float64)
    for _ in range(passes):
        for a in range(3):
            p = np.pad(v, [(1, 1) if b == a else (0, 0) for b in range(3)], mode="edge")
            n = v.shape[a]
            v = (np.take(p, range(0, n), a) + np.take(p, range(1, n + 1), a) + np.take(p, range(2, n + 2), a)) / 3
    v = v.astype(np.float32)
    return v, float(np.quantile(v, quantile))


def _with_nans():
    rng = np.random.default_rng(11)
    v = rng.random((9, 10, 11)).astype(np.float32)
    v[rng.random(v.shape) < 0.2] = np.nan
    return v


def noisy_blob(n=300, seed=7, speck_seed=23, speck_rate=1.5e-4):
    """tests/test_gpu_mesh.py's noisy_blob_300 formula at n^3 plus sparse specks well above the level (0.3): one dominant
    component and, at 300^3, a few thousand floaters.  -> (vol, level)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    ax = torch.linspace(-1, 1, n)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v = (1 - (x * x / 0.5 + y * y / 0.4 + z * z / 0.6) + 0.05 * torch.rand((n, n, n), generator=g)).float().numpy()
    specks = np.random.default_rng(speck_seed).random((n, n, n)) < speck_rate
    v[specks] = np.float32(0.9)
    return v, 0.3


# name -> (builder of (vol, level), components under connectivity 6, under 26; None = the description states no number)
CASES = {
    "all_outside": (lambda: (np.zeros((5, 6, 7), np.float32), 0.5), 0, 0),
    "all_inside": (lambda: (np.ones((5, 6, 7), np.float32), 0.5), 1, 1),
    "on_level": (lambda: (np.full((3, 4, 5), 0.5, np.float32), 0.5), 0, 0),           # a value AT the level is outside
    "single_voxel": (lambda: (_single(), 0.5), 1, 1),
    "line_1x1xN": (lambda: (_line(), 0.5), 10, 10),
    "slab_8x1x8": (lambda: (_checkerboard((8, 1, 8)), 0.5), 32, 1),
    "checkerboard": (lambda: (_checkerboard((17, 18, 19)), 0.5), 17 * 18 * 19 // 2, 1),
    "face_diagonal": (lambda: (_two_blobs((4, 4, 1)), 0.5), 2, 1),                   # contact along one lattice-face diagonal only
    "body_diagonal": (lambda: (_two_blobs((4, 4, 4)), 0.5), 2, 1),                   # contact through one corner only
    "serpentine": (lambda: (serpentine(48), 0.5), 1, 1),
    "smooth_noise": (lambda: smooth_noise(), None, None),                            # "a few hundred": checked as a range
    "nans": (lambda: (_with_nans(), 0.5), None, None),
}
SMALL = list(CASES)


def case(name):
    vol, level = CASES[name][0]()
    return np.ascontiguousarray(vol, np.float32), float(level)


# ---- the blob scene: a field whose density is a handful of separable Gaussian bumps ----------------------------------------
BLOB_GRID = [40, 48, 56]
BLOB_AABB = [[-1.5, -1.4, -1.3], [1.5, 1.4, 1.6]]
# (centre in normalised [-1, 1] coordinates, sigma): one large blob and five floaters, far apart in x-y as well, so that an
# axis-parallel ray along z meets one of them only
BLOBS = [((0.0, 0.0, 0.0), 0.20),
         ((0.72, 0.70, 0.55), 0.06), ((-0.72, 0.70, -0.50), 0.06), ((0.72, -0.70, -0.20), 0.06), ((-0.72, -0.70, 0.60), 0.06),
         ((0.0, 0.78, 0.70), 0.05)]
BLOB_GAIN = 20.0


def blob_checkpoint(grid=BLOB_GRID, aabb=BLOB_AABB):
    """A reference-format checkpoint as tests/config_scenes.checkpoint builds them (synth.make_checkpoint), with every density
    factor zero except blob k in density component k of all three plane / line pairs: plane_c * line_c is one local bump of
    peak 3 * BLOB_GAIN, far above the softplus shift of -10, and zero density (alpha 1e-5-ish) elsewhere."""
    import torch
    from tensoir_amd import synth
    ck = synth.make_checkpoint(grid=tuple(grid), seed=20240915, light_rotation=["000"], aabb=aabb, density_n_comp=(8, 8, 8),
                               app_n_comp=(48, 48, 48))
    sd = ck["state_dict"]
    for i in range(3):
        m0, m1 = synth.MAT_MODE[i]
        v = synth.VEC_MODE[i]
        sd[f"density_plane.{i}"].zero_()
        sd[f"density_line.{i}"].zero_()
        for c, (centre, sigma) in enumerate(BLOBS):
            def bump(axis):
                return torch.exp(-(torch.linspace(-1, 1, grid[axis]) - centre[axis]) ** 2 / (2 * sigma ** 2))
            sd[f"density_plane.{i}"][0, c] = BLOB_GAIN * bump(m1)[:, None] * bump(m0)[None, :]
            sd[f"density_line.{i}"][0, c, :, 0] = bump(v)
    return ck


def blob_centres_world(aabb=BLOB_AABB):
    lo, hi = np.float32(aabb[0]), np.float32(aabb[1])
    return np.stack([lo + (np.float32(c) + 1) / 2 * (hi - lo) for c, _ in BLOBS])


def blob_alpha_planned(grid=BLOB_GRID, aabb=BLOB_AABB, step_ratio=0.5):
    """The blob scene's alpha lattice at the model's own grid as its recipe plans it (float64 arithmetic; the device's differs in
    the last bits): feature = 3 * BLOB_GAIN * sum_k bump_k(x) bump_k(y) bump_k(z), sigma = softplus(feature - 10), alpha =
    1 - exp(-sigma * step * 25) with step = step_ratio * mean voxel size.  For the counts of the plan, not for comparisons."""
    ax = [np.linspace(-1, 1, g) for g in grid]
    feat = np.zeros(grid)
    for centre, sigma in BLOBS:
        b = [np.exp(-(ax[a] - centre[a]) ** 2 / (2 * sigma ** 2)) for a in range(3)]
        feat += 3 * BLOB_GAIN * b[0][:, None, None] * b[1][None, :, None] * b[2][None, None, :]
    units = (np.float64(aabb[1]) - np.float64(aabb[0])) / (np.float64(grid) - 1)
    sigma = np.logaddexp(0.0, feat - 10.0)
    return (1 - np.exp(-sigma * units.mean() * step_ratio * 25.0)).astype(np.float32)
