"""Material editing without a GPU: the numpy restatement (tests/materials_reference.py) against the definition in
include/tensoir_hip.h, the record packing and validation of tensoir_amd.materials, and deterministic k-means on the fixture.

k-means fixture (materials_reference.fixture: 915 rows, seven blobs), float64, row-0 farthest-point seeding: k = 4 reaches its
fixed point in 13 passes, k = 6 in 9 (the last pass is the one that changes no label).  The smallest gap between a row's best and
second-best d2 over all rows and passes is 8.9e-5 (k = 4) and 2.2e-4 (k = 6), the smallest gap in the seeding steps 7.8e-3; an
fp32 evaluation of d2 <= 4 errs by less than 2e-6, so the device must reproduce every label."""
import json

import numpy as np
import pytest

from tests import materials_reference as R


def mt():
    from tensoir_amd import materials
    return materials


def rows(M=200, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    a = rng.uniform(0.05, 0.95, (M, 3)).astype(np.float32)
    r = rng.uniform(0.09, 0.99, M).astype(np.float32)
    f = rng.uniform(0.02, 0.08, (M, 3)).astype(np.float32)
    return x, a, r, f


def run(edits, x, a, r, f, palette=None, dtype=np.float64):
    el = mt().EditList(edits, palette)
    return R.apply(el.records(), el.centroids, el.rough_weight, x, a, r, f, dtype)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_empty_list_and_zero_strength_are_the_identity():
    E = mt().MaterialEdit
    x, a, r, f = rows()
    a[3], f[4, 0] = -0.0, -0.0                                         # bits, not values
    for edits in ([], [E(strength=0.0, albedo_mode="set", color=(1, 0, 0), metallic=1.0, roughness_offset=0.3)]):
        for dtype in (np.float64, np.float32):
            o = run(edits, x, a, r, f, dtype=dtype)
            assert not o["touched"].any()
            for key, src in (("albedo", a), ("base", a), ("roughness", r), ("fresnel", f)):
                assert np.array_equal(bits(o[key]), bits(src)), key
            assert (o["metal"] == 0).all()


def weight_of(edit, x=(0, 0, 0), a=(0.5, 0.5, 0.5), r=0.5):
    el = mt().EditList([edit])
    w, _ = R.weights(el.records(), None, 1.0, np.float32([x]), np.float32([a]), np.float32([r]))
    return float(w[0, 0])


def test_selectors_at_centre_midpoint_and_beyond():
    E = mt().MaterialEdit
    c = (0.25, -0.5, 0.75)
    sphere = lambda d: weight_of(E(sphere_center=c, sphere_radius=0.5, sphere_feather=0.25), x=(c[0] + d, c[1], c[2]))
    assert sphere(0) == 1 and sphere(0.5) == 1 and sphere(0.625) == pytest.approx(0.5, abs=1e-12) and sphere(0.75) == 0 and sphere(2) == 0
    box = lambda d: weight_of(E(box_center=c, box_half=(0.5, 0.25, 0.125), box_feather=0.5), x=(c[0], c[1] + d, c[2]))
    assert box(0) == 1 and box(-0.25) == 1 and box(0.5) == pytest.approx(0.5, abs=1e-12) and box(0.75) == 0 and box(-3) == 0
    col = lambda d: weight_of(E(select_color=(0.5, 0.25, 0.125), color_tolerance=0.125, color_feather=0.25), a=(0.5, 0.25 + d, 0.125))
    assert col(0) == 1 and col(0.125) == 1 and col(0.25) == pytest.approx(0.5, abs=1e-12) and col(0.375) == 0 and col(0.7) == 0
    band = lambda r: weight_of(E(roughness_band=(0.25, 0.5), band_feather=0.25), r=r)
    assert band(0.375) == 1 and band(0.25) == 1 and band(0.5) == 1 and band(0.625) == pytest.approx(0.5, abs=1e-12)
    assert band(0.125) == pytest.approx(0.5, abs=1e-12) and band(0.75) == 0 and band(0.0) == 0
    # hard edges: feather = 0 is the test d <= r
    assert weight_of(E(sphere_center=c, sphere_radius=0.5), x=(c[0] + 0.5, c[1], c[2])) == 1
    assert weight_of(E(sphere_center=c, sphere_radius=0.5), x=(c[0] + 0.5001, c[1], c[2])) == 0
    # the product of selectors, times the strength
    both = E(strength=0.5, sphere_center=c, sphere_radius=0.5, sphere_feather=0.25, roughness_band=(0.25, 0.5), band_feather=0.25)
    assert weight_of(both, x=(c[0] + 0.625, c[1], c[2]), r=0.625) == pytest.approx(0.125, abs=1e-12)


def test_palette_selector_and_label_ties():
    E, cent = mt().MaterialEdit, np.float32([[0.2, 0.2, 0.2, 0.3], [0.8, 0.8, 0.8, 0.6], [0.2, 0.2, 0.2, 0.3]])
    a = np.float32([[0.2, 0.2, 0.2], [0.8, 0.8, 0.8], [0.5, 0.5, 0.5]])
    r = np.float32([0.3, 0.6, 0.45])
    lab, d2, _ = R.label(a, r, cent, 1.0)
    assert lab.tolist() == [0, 1, 0] and d2[0, 0] == d2[0, 2] == 0                  # the duplicate centroid never wins: lower index
    o = run([E(palette_id=1, albedo_mode="set", color=(0, 0, 1))], np.zeros((3, 3), np.float32), a, r, np.zeros((3, 3), np.float32),
            palette=(cent, 1.0))
    assert o["touched"].tolist() == [False, True, False] and o["albedo"][1].tolist() == [0, 0, 1]
    with pytest.raises(ValueError, match="palette_id 3"):
        mt().EditList([E(palette_id=3)], palette=(cent, 1.0))
    with pytest.raises(ValueError, match="palette_id 0"):
        mt().EditList([E(palette_id=0)])


def test_selectors_read_the_original_values():
    """Two edits select by colour and each changes the colour: either order selects the same rows."""
    E = mt().MaterialEdit
    x, a, r, f = rows(300, 3)
    a[:100] = np.float32([0.8, 0.1, 0.1]) + 0.01 * a[:100]
    a[100:200] = np.float32([0.1, 0.1, 0.8]) + 0.01 * a[100:200]
    a[200:] = 0.4 + 0.2 * a[200:]                                      # greys, far from both
    red_to_blue = E(select_color=(0.8, 0.1, 0.1), color_tolerance=0.1, albedo_mode="set", color=(0.1, 0.1, 0.8))
    blue_to_red = E(select_color=(0.1, 0.1, 0.8), color_tolerance=0.1, albedo_mode="set", color=(0.8, 0.1, 0.1))
    o1, o2 = run([red_to_blue, blue_to_red], x, a, r, f), run([blue_to_red, red_to_blue], x, a, r, f)
    assert np.array_equal(o1["w"][0], o2["w"][1]) and np.array_equal(o1["w"][1], o2["w"][0])
    assert o1["w"][0].sum() == 100 and o1["w"][1].sum() == 100 and (o1["w"][0] * o1["w"][1]).sum() == 0
    assert np.array_equal(o1["albedo"], o2["albedo"])
    assert np.allclose(o1["albedo"][:100], [0.1, 0.1, 0.8]) and np.allclose(o1["albedo"][100:200], [0.8, 0.1, 0.1])
    assert np.array_equal(bits(o1["albedo"][200:]), bits(a[200:]))


def test_targets():
    E = mt().MaterialEdit
    x, a, r, f = rows(64, 5)
    m = run([E(albedo_mode="set", color=(0.9, 0.6, 0.2), metallic=1.0)], x, a, r, f)
    assert (m["albedo"] == 0).all() and np.allclose(m["fresnel"], m["base"]) and np.allclose(m["base"], np.float32([0.9, 0.6, 0.2]))
    half = run([E(metallic=0.5)], x, a, r, f)
    assert np.allclose(half["albedo"], 0.5 * a) and np.allclose(half["fresnel"], 0.5 * f + 0.5 * a) and np.allclose(half["metal"], 0.5)
    Y = lambda c: c @ np.asarray(R.LUMA)
    rec = run([E(albedo_mode="recolor", color=(0.1, 0.2, 0.9))], x, 0.2 * a, r, f)       # dark enough that nothing clamps
    assert np.allclose(Y(rec["base"]), Y(0.2 * a.astype(np.float64)), rtol=1e-12)
    assert np.allclose(rec["base"] / rec["base"][:, 2:3], np.float64([0.1, 0.2, 0.9]) / 0.9)
    mul = run([E(albedo_mode="multiply", color=(0.5, 2.0, 1.0))], x, a, r, f)
    assert np.allclose(mul["base"], np.clip(a.astype(np.float64) * [0.5, 2.0, 1.0], 0, 1))
    ro = run([E(roughness_scale=0.5, roughness_offset=0.1)], x, a, r, f)
    assert np.allclose(ro["roughness"], np.clip(0.5 * r.astype(np.float64) + 0.1, 0.09, 0.99))
    lo = run([E(roughness_scale=0.0)], x, a, r, f)
    assert np.allclose(lo["roughness"], 0.09)
    blend = run([E(strength=0.25, albedo_mode="set", color=(1, 1, 1))], x, a, r, f)
    assert np.allclose(blend["base"], a + 0.25 * (1 - a.astype(np.float64)))
    # list order matters for the targets: set then multiply is not multiply then set
    s, mu = E(albedo_mode="set", color=(0.5, 0.5, 0.5)), E(albedo_mode="multiply", color=(0.5, 0.5, 0.5))
    assert np.allclose(run([s, mu], x, a, r, f)["base"], 0.25) and np.allclose(run([mu, s], x, a, r, f)["base"], 0.5)


def test_float32_restatement_stays_close():
    E = mt().MaterialEdit
    x, a, r, f = rows(500, 9)
    edits = [E(sphere_center=(0, 0, 0), sphere_radius=0.4, sphere_feather=0.5, albedo_mode="recolor", color=(0.2, 0.5, 0.9), metallic=0.7),
             E(roughness_band=(0.3, 0.6), band_feather=0.2, roughness_scale=0.5, roughness_offset=0.2, albedo_mode="multiply",
               color=(0.9, 0.8, 1.1))]
    o64, o32 = run(edits, x, a, r, f), run(edits, x, a, r, f, dtype=np.float32)
    dev = max(float(np.abs(o32[k].astype(np.float64) - o64[k]).max()) for k in ("albedo", "roughness", "fresnel", "base", "metal"))
    print(f"float32 restatement against float64: {dev:.3e}")
    assert 0 < dev < 1e-5


def test_json_round_trip():
    M = mt()
    E = M.MaterialEdit
    pal = (np.float32([[0.1, 0.2, 0.3, 0.4], [0.5, 0.6, 0.7, 0.8]]), 0.5)
    el = M.EditList([E(strength=0.5, sphere_center=(1, 2, 3), sphere_radius=0.5, sphere_feather=0.1, albedo_mode="set", color=(0.1, 0.2, 0.3)),
                     E(box_center=(0, 0, 0), box_half=(1, 2, 3), palette_id=1, metallic=1.0, roughness_scale=0.0, roughness_offset=0.2),
                     E(select_color=M.srgb_to_linear((255, 0, 0)), color_tolerance=0.2, roughness_band=(0.2, 0.4), albedo_mode="recolor",
                       color=(0, 0, 1))], palette=pal)
    text = json.dumps(el.to_json())
    back = M.EditList.from_json(json.loads(text))
    assert back == el and np.array_equal(back.records(), el.records()) and np.array_equal(back.centroids, el.centroids)
    assert back.rough_weight == 0.5 and M.EditList.from_json(text) == el
    assert el.to_json()["edits"][1] == {"box_center": [0.0, 0.0, 0.0], "box_half": [1.0, 2.0, 3.0], "palette_id": 1,
                                        "roughness_scale": 0.0, "roughness_offset": 0.2, "metallic": 1.0}
    assert M.EditList.from_json([{"metallic": 1.0}]) == M.EditList([E(metallic=1.0)])
    rec = el.records()
    assert rec.shape == (3, 32) and rec.dtype == np.float32 and rec[:, 0].tolist() == [1, 18, 12] and rec[:, 23].tolist() == [1, 0, 3]
    assert M.srgb_to_linear((255, 0, 0)) == (1.0, 0.0, 0.0) and M.srgb_to_linear((0.5, 0.5, 0.5))[0] == pytest.approx(0.21404114)
    assert len(M.EditList()) == 0 and M.EditList().records().shape == (0, 32)


BAD_EDITS = [
    (dict(strength=1.5), "strength"), (dict(strength=float("nan")), "strength"), (dict(strength=True), "strength"),
    (dict(sphere_center=(0, 0, 0)), "come together"), (dict(sphere_radius=1.0), "come together"),
    (dict(sphere_center=(0, 0), sphere_radius=1.0), "three numbers"), (dict(sphere_center=(0, 0, 0), sphere_radius=-1.0), "sphere_radius"),
    (dict(sphere_center=(0, 0, 0), sphere_radius=1.0, sphere_feather=-0.1), "sphere_feather"),
    (dict(box_center=(0, 0, 0)), "come together"), (dict(box_center=(0, 0, 0), box_half=(1, -1, 1)), "box_half"),
    (dict(select_color=(0, 0, float("inf"))), "select_color"), (dict(color_tolerance=-1.0), "color_tolerance"),
    (dict(roughness_band=(0.5, 0.2)), "lo <= hi"), (dict(roughness_band=0.5), "lo, hi"), (dict(band_feather=-1.0), "band_feather"),
    (dict(palette_id=32), "palette_id"), (dict(palette_id=-1), "palette_id"), (dict(palette_id=1.0), "palette_id"),
    (dict(albedo_mode="paint", color=(0, 0, 0)), "albedo_mode"), (dict(albedo_mode="set"), "color comes with"),
    (dict(color=(0, 0, 0)), "color comes with"), (dict(albedo_mode="set", color=(0, 0, 1.5)), "color"),
    (dict(albedo_mode="multiply", color=(0, 0, -0.5)), "color"), (dict(roughness_scale="1"), "roughness_scale"),
    (dict(metallic=1.5), "metallic"), (dict(metallic=-0.1), "metallic"),
]


@pytest.mark.parametrize("kw, match", BAD_EDITS, ids=[f"{i}-{m.split()[0]}" for i, (_, m) in enumerate(BAD_EDITS)])
def test_edits_are_validated_without_a_device(kw, match):
    with pytest.raises(ValueError, match=match):
        mt().MaterialEdit(**kw)


def test_lists_are_validated_without_a_device():
    M = mt()
    E = M.MaterialEdit
    with pytest.raises(TypeError):
        E(1.0)                                                          # keywords only
    with pytest.raises(ValueError, match="at most 16"):
        M.EditList([E()] * 17)
    with pytest.raises(TypeError, match="MaterialEdit"):
        M.EditList([{"metallic": 1.0}])
    with pytest.raises(ValueError, match="unknown edit field"):
        M.EditList.from_json({"edits": [{"metalic": 1.0}]})
    with pytest.raises(ValueError, match="edit list is"):
        M.EditList.from_json({"edit": []})
    for bad in ((np.zeros((33, 4)), 1.0), (np.zeros((2, 3)), 1.0), (np.full((2, 4), np.nan), 1.0), (np.zeros((2, 4)), -1.0), 5):
        with pytest.raises(ValueError):
            M.EditList([], palette=bad)
    with pytest.raises(TypeError, match="edits"):
        M.as_edit_list(3)
    assert M.as_edit_list(None) is None and len(M.as_edit_list([E()])) == 1
    import torch
    with pytest.raises(ValueError, match="k: expected"):
        M.palette_of(torch.zeros(4, 3), torch.zeros(4), 0)
    with pytest.raises(ValueError, match="k: expected"):
        M.palette_of(torch.zeros(40, 3), torch.zeros(40), 33)
    with pytest.raises(ValueError, match="cannot seed"):
        M.palette_of(torch.zeros(3, 3), torch.zeros(3), 4)              # N < k, refused before the device is asked for
    with pytest.raises(ValueError, match="max_iters"):
        M.palette_of(torch.zeros(4, 3), torch.zeros(4), 2, max_iters=0)


# ---- k-means ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, passes", [(4, 13), (6, 9)])
def test_kmeans_fixture(k, passes):
    a, r = R.fixture()
    assert a.shape == (915, 3)
    o = R.kmeans(a, r, k)
    print(f"k {k}: {o['passes']} passes, smallest d2 gap {o['gap']:.3e}, smallest seeding gap {o['seed_gap']:.3e}, counts "
          f"{o['counts'].tolist()}, inertia {o['inertia']:.6f}")
    assert o["passes"] == passes and o["gap"] >= 1e-5 and o["seed_gap"] >= 1e-5
    assert o["seed_rows"][0] == 0 and len(set(o["seed_rows"])) == k
    assert (o["history"][-1] == o["history"][-2]).all() and (o["history"][-2] != o["history"][-3]).any()
    assert o["counts"].sum() == 915 and (o["counts"] > 0).all()
    again = R.kmeans(a, r, k)
    assert np.array_equal(again["centroids"], o["centroids"]) and np.array_equal(again["labels"], o["labels"])
    # a fixed point: the centroids are the means of their rows
    feat = R.features(a, r, 1.0).astype(np.float64)
    for c in range(k):
        assert np.array_equal(o["centroids"][c], feat[o["labels"] == c].mean(0).astype(np.float32))


def test_kmeans_edge_cases():
    a, r = R.fixture()
    one = R.kmeans(a, r, 1)
    assert one["passes"] == 2 and (one["labels"] == 0).all() and one["counts"].tolist() == [915]
    assert np.array_equal(one["centroids"][0], R.features(a, r, 1.0).astype(np.float64).mean(0).astype(np.float32))
    with pytest.raises(ValueError):
        R.kmeans(a[:3], r[:3], 4)                                       # N < k
    # duplicate rows: a tie goes to the lower index, in the seeding and in the labels
    da, dr = np.repeat(np.float32([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9]]), 3, axis=0), np.repeat(np.float32([0.2, 0.8]), 3)
    cent, chosen, _ = R.seed(R.features(da, dr, 1.0), 3)
    assert chosen == [0, 3, 0]                                          # every min-distance is 0 after two seeds: row 0 again
    o = R.lloyd(R.features(da, dr, 1.0), cent)
    assert o["labels"].tolist() == [0, 0, 0, 1, 1, 1] and o["counts"].tolist() == [3, 3, 0]
    assert np.array_equal(o["centroids"][2], cent[2])                   # wins no row: keeps its value
    far = np.float32([[0.1, 0.1, 0.1, 0.2], [0.9, 0.9, 0.9, 0.8], [5, 5, 5, 5]])
    o = R.lloyd(R.features(da, dr, 1.0), far)
    assert o["counts"].tolist() == [3, 3, 0] and np.array_equal(o["centroids"][2], far[2])
    assert R.order_by_count([5, 9, 5, 0]).tolist() == [1, 0, 2, 3]
