"""Material editing restated in numpy (the definition: include/tensoir_hip.h, "Material editing").

Every function takes `dtype`: float64 is the reference, float32 is the same expressions with every numpy operation rounded to
fp32 -- its distance from the float64 run on the same inputs is the yardstick of the device's tolerance (ten times that).
The edit records are the header's: [n, 32] floats, integers stored as the floats that equal them."""
import numpy as np

EDIT_FLOATS, MAX_EDITS, MAX_PALETTE = 32, 16, 32
SPHERE, BOX, COLOUR, BAND, PALETTE = 1, 2, 4, 8, 16
KEEP, SET, MULTIPLY, RECOLOUR = 0, 1, 2, 3
LUMA = (0.2126, 0.7152, 0.0722)
ROUGH_MIN, ROUGH_MAX = 0.09, 0.99


def smoothstep(t):
    return t * t * (3 - 2 * t)


def fall(d, r, f, dtype):
    """1 inside r, 0 beyond r + f, a smoothstep between; f = 0: the hard test d <= r.  -> (value, |d - r| where the test is hard)"""
    d = np.asarray(d, dtype)
    r, f = dtype(r), dtype(f)
    if f > 0:
        t = np.clip((d - r) / f, dtype(0), dtype(1))
        return dtype(1) - smoothstep(t), np.full(d.shape, np.inf)
    return (d <= r).astype(dtype), np.abs(d.astype(np.float64) - np.float64(r))


def features(albedo, rough, wr):
    """[N, 4] float32: (a.r, a.g, a.b, fp32(wr r)) -- the product is one fp32 operation"""
    a = np.asarray(albedo, np.float32).reshape(-1, 3)
    r = np.asarray(rough, np.float32).reshape(-1)
    return np.concatenate([a, (np.float32(wr) * r)[:, None]], 1).astype(np.float32)


def dist2(feat, cent, dtype=np.float64):
    """d2 [N, k] = ((D0 D0 + D1 D1) + D2 D2) + D3 D3 in this order"""
    d = feat.astype(dtype)[:, None, :] - np.asarray(cent, np.float32).astype(dtype)[None, :, :]
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3]


def label(albedo, rough, cent, wr, dtype=np.float64):
    """-> (label [N] int32: the lowest index of the smallest d2, d2 [N, k], gap [N] between the best and the second best d2
    (inf for k = 1))"""
    d2 = dist2(features(albedo, rough, wr), cent, dtype)
    lab = np.argmin(d2, axis=1).astype(np.int32)                       # numpy's argmin returns the first of equals
    if d2.shape[1] > 1:
        s = np.sort(d2.astype(np.float64), axis=1)
        gap = s[:, 1] - s[:, 0]
    else:
        gap = np.full(d2.shape[0], np.inf)
    return lab, d2, gap


def weights(records, palette, wr, x, a0, r0, dtype=np.float64):
    """w [n_edits, M] from the rows' ORIGINAL x, a0, r0, and the smallest distance of any hard test from its boundary."""
    rec = np.asarray(records, np.float32).reshape(-1, EDIT_FLOATS)
    x, a0, r0 = (np.asarray(t, np.float32).astype(dtype) for t in (x, a0, r0))
    M = r0.shape[0]
    w = np.zeros((len(rec), M), dtype)
    margin = np.inf
    lab = gap = None
    for e, E in enumerate(rec):
        E = E.astype(dtype)
        sel = int(E[0])
        we = np.full(M, E[1], dtype)
        hard = []
        if sel & SPHERE:
            d = x - E[2:5]
            v, m = fall(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]), E[5], E[6], dtype)
            we, hard = we * v, hard + [m]
        if sel & BOX:
            q = np.abs(x - E[7:10]) - E[10:13]
            v, m = fall(np.maximum(np.maximum(q[:, 0], q[:, 1]), q[:, 2]), 0, E[13], dtype)
            we, hard = we * v, hard + [m]
        if sel & COLOUR:
            d = a0 - E[14:17]
            v, m = fall(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]), E[17], E[18], dtype)
            we, hard = we * v, hard + [m]
        if sel & BAND:
            v, m = fall(np.maximum(E[19] - r0, r0 - E[20]), 0, E[21], dtype)
            we, hard = we * v, hard + [m]
        if sel & PALETTE:
            if palette is None or len(palette) == 0:
                v = np.zeros(M, dtype)
            else:
                if lab is None:
                    lab, _, gap = label(a0, r0, palette, wr, dtype)
                v = (lab == int(E[22])).astype(dtype)
                hard.append(gap)
            we = we * v
        w[e] = we
        for m in hard:
            if m.size:
                margin = min(margin, float(np.min(m)))
    return w, margin


def apply(records, palette, wr, x, a0, r0, f0, dtype=np.float64):
    """The edit list on M rows -> dict(albedo, roughness, fresnel, base [M, 3] / metal [M], touched [M] bool, w [n, M],
    margin).  Untouched rows are returned as they came (their float32 values, exactly)."""
    rec = np.asarray(records, np.float32).reshape(-1, EDIT_FLOATS)
    a32, r32, f32 = (np.asarray(t, np.float32) for t in (a0, r0, f0))
    w, margin = weights(rec, palette, wr, x, a32, r32, dtype)
    base, rough = a32.astype(dtype).copy(), r32.astype(dtype).copy()
    metal = np.zeros_like(rough)
    touched = np.zeros(rough.shape[0], bool)
    Y = np.asarray(LUMA, dtype)
    for e, E in enumerate(rec):
        E = E.astype(dtype)
        on = w[e] != 0
        touched |= on
        mode, col = int(E[23]), E[24:27]
        if mode == SET:
            t = np.broadcast_to(col, base.shape)
        elif mode == MULTIPLY:
            t = base * col
        elif mode == RECOLOUR:
            yb = Y[0] * base[:, 0] + Y[1] * base[:, 1] + Y[2] * base[:, 2]
            yc = np.maximum(Y[0] * col[0] + Y[1] * col[1] + Y[2] * col[2], dtype(1e-6))
            t = col[None, :] * (yb / yc)[:, None]
        else:
            t = base
        t = np.clip(t, dtype(0), dtype(1))
        tr = np.clip(rough * E[27] + E[28], dtype(ROUGH_MIN), dtype(ROUGH_MAX))
        we = np.where(on, w[e], dtype(0))
        base = base + we[:, None] * (t - base)
        if E[27] != 1 or E[28] != 0:                                    # scale 1, offset 0: the edit leaves rough as it is
            rough = rough + we * (tr - rough)
        if E[29] != 0:
            metal = metal + we * (E[30] - metal)
    f0d = f32.astype(dtype)
    out = {"base": base, "metal": metal, "roughness": rough, "albedo": base * (1 - metal)[:, None],
           "fresnel": f0d * (1 - metal)[:, None] + base * metal[:, None]}
    keep = ~touched
    out["albedo"][keep], out["base"][keep], out["roughness"][keep], out["fresnel"][keep] = a32[keep], a32[keep], r32[keep], f32[keep]
    out.update(touched=touched, w=w, margin=margin)
    return out


# ---- deterministic k-means ---------------------------------------------------------------------------------------------------
def seed(feat, k):
    """Farthest-point seeding from row 0 in float64: centroid j + 1 = the row of largest min-distance to centroids 0..j, the lowest
    index among equals.  -> (centroids [k, 4] float32, the chosen rows, the smallest gap between the largest and the second
    largest min-distance over the steps)."""
    feat = np.asarray(feat, np.float32)
    rows, mind, gap = [0], None, np.inf
    for _ in range(1, k):
        d = dist2(feat, feat[rows[-1]][None], np.float64)[:, 0]
        mind = d if mind is None else np.minimum(mind, d)
        best = int(np.argmax(mind))
        if feat.shape[0] > 1:
            others = np.delete(mind, best)
            gap = min(gap, float(mind[best] - others.max()))
        rows.append(best)
    return feat[rows].copy(), rows, gap


def lloyd(feat, cent, max_iters=50):
    """Lloyd passes from the float32 centroids `cent`: assign (float64 d2, lowest index on ties), then centroid = float32 of the
    float64 mean (an empty cluster keeps its centroid).  The first pass counts every row as changed; the loop ends with the first
    pass that changes no label, or after max_iters passes.
    -> dict(centroids [k, 4] float32, labels [N], history: the labels after every pass, passes, counts [k], inertia (of the last
    assignment, float64), gap: the smallest distance between a row's best and second-best d2 over all passes)."""
    feat = np.asarray(feat, np.float32)
    cent = np.asarray(cent, np.float32).copy()
    k, N = cent.shape[0], feat.shape[0]
    labels, history, gap, passes = None, [], np.inf, 0
    f64 = feat.astype(np.float64)
    for p in range(max_iters):
        d2 = dist2(feat, cent, np.float64)
        new = np.argmin(d2, axis=1).astype(np.int32)
        if k > 1:
            s = np.sort(d2, axis=1)
            gap = min(gap, float((s[:, 1] - s[:, 0]).min()))
        changed = N if labels is None else int((new != labels).sum())
        counts = np.bincount(new, minlength=k).astype(np.int64)
        inertia = float(d2[np.arange(N), new].sum())
        for c in range(k):
            if counts[c] > 0:
                cent[c] = (f64[new == c].sum(0) / counts[c]).astype(np.float32)
        labels, passes = new, p + 1
        history.append(new.copy())
        if changed == 0:
            break
    return {"centroids": cent, "labels": labels, "history": history, "passes": passes, "counts": counts, "inertia": inertia,
            "gap": gap}


def kmeans(albedo, rough, k, wr=1.0, max_iters=50):
    feat = features(albedo, rough, wr)
    if feat.shape[0] < k:
        raise ValueError(f"k-means: {feat.shape[0]} rows for {k} clusters")
    cent, rows, seed_gap = seed(feat, k)
    out = lloyd(feat, cent, max_iters)
    out.update(seed_rows=rows, seed_gap=seed_gap)
    return out


def order_by_count(counts):
    """the palette's order: count descending, the lower original index first among equals -> perm (new index -> old index)"""
    return np.asarray(sorted(range(len(counts)), key=lambda c: (-int(counts[c]), c)), np.int64)


def fixture(seed_=6):
    """The k-means fixture of the material tests: seven Gaussian blobs, 915 rows (three full 256-row groups and a ragged one)."""
    rng = np.random.default_rng(seed_)
    cent = rng.uniform(.1, .9, (7, 4))
    sizes = rng.integers(20, 300, 7)
    X = np.concatenate([c + rng.normal(0, .08, (n, 4)) for c, n in zip(cent, sizes)]).clip(0, 1).astype(np.float32)
    X = X[rng.permutation(len(X))]
    return np.ascontiguousarray(X[:, :3]), np.ascontiguousarray(X[:, 3])
