"""What needs no GPU of the asset lighting: the float64 restatement (tests/light_reference.py) pinned to the oracle's
GGX_specular and tone map, the solid angles and the white furnace, the light-cell reduction's invariants, the float32 restatement's
own distance from float64 on every fixture of the GPU tests (printed: ten times it is the device's bound), and Radiance .hdr
reading and writing (tensoir_amd/hdr.py)."""
import math

import numpy as np
import pytest
import torch

from tests import light_reference as L


# ---- the restatement against the oracle ----------------------------------------------------------------------------------------------
def test_specular_term_is_the_oracles():
    """The fixture's N, V and L (L normalised in float64 first: the oracle normalises it, the kernel takes it as stored), roughness
    and fresnel broadcast to three channels: 1e-12 relative."""
    from oracle import tensoir_oracle as O
    for rough in L.ROUGH_CASES:
        g, v, cells = L.surface_rows(65, 33, rough)
        lt = cells[:, 0:3].astype(np.float64)
        lt /= np.linalg.norm(lt, axis=1, keepdims=True)
        S = L.surface(g[:, 5:8], v, g[:, 3])
        mine = L.specular(S, lt, 0.04)
        M, D = mine.shape
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
        ref = O.ggx_specular(T(g[:, 5:8]), T(v), T(np.broadcast_to(lt, (M, D, 3))), T(g[:, 3:4]).expand(M, 3), torch.full((M, 3), 0.04, dtype=torch.float64))
        ref = ref.numpy()
        assert ref.shape == (M, D, 3)
        rel = np.abs(mine[..., None] - ref) / np.abs(ref)
        assert rel.max() < 1e-12, (rough, rel.max())


def test_tone_map_is_the_oracles():
    from oracle import tensoir_oracle as O
    x = np.concatenate([np.linspace(-0.5, 1.5, 4001), [0.0, 0.0031308, 0.00313081, 1.0]])
    assert np.abs(L.linear2srgb(x) - O.linear2srgb(torch.from_numpy(x)).numpy()).max() < 1e-15


# ---- solid angles, white furnace -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 4), (6, 12), (64, 128)])
def test_solid_angles_sum_to_the_sphere(H, W):
    from tensoir_amd import ops
    assert abs(W * L.row_weights(H, W).sum() / (4 * math.pi) - 1) < 1e-12
    assert np.array_equal(ops.env_row_weights(H, W).numpy(), L.row_weights(H, W))
    cells = L.env_cells(np.ones((H, W, 3), np.float32), H, W)
    assert abs(cells[:, 3].sum() / (4 * math.pi) - 1) < 1e-7          # the float32 weights the kernel gets, summed in float64


def _furnace(h, w, normals, views, albedo):
    """The diffuse part (specular term removed) under a constant unit map on an h x w grid, float64 weights."""
    cells = np.zeros((h * w, 8))
    cells[:, 0:3] = L.cell_dirs(h, w).reshape(-1, 3)
    cells[:, 3] = np.repeat(L.row_weights(h, w), w)
    cells[:, 4:7] = 1.0
    g = np.zeros((len(normals), L.ROW))
    g[:, 0:3], g[:, 3], g[:, 4], g[:, 5:8], g[:, 8] = albedo, 0.5, 1.0, normals, 1.0
    S = L.surface(g[:, 5:8], views, g[:, 3])
    c = L._dot(g[:, None, 5:8], cells[None, :, 0:3])
    on = c > L.THRESHOLD
    return (np.where(on, c * cells[None, :, 3], 0.0).sum(1) / math.pi)[:, None] * g[:, 0:3], S


def test_white_furnace():
    """A constant unit map lights a surface of albedo a to a + the integral of the specular term, in every orientation.  The
    diffuse part on 64 x 128 cells must equal a within the midpoint rule's own error, measured here as the difference from the
    128 x 256 grid: agreement to twice that difference."""
    rng = np.random.default_rng(3)
    n = rng.normal(size=(40, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[0], n[1], n[2] = (0, 0, 1), (1, 0, 0), (0, -1, 0)
    v = rng.normal(size=(40, 3))
    a = np.float64([0.8, 0.5, 0.2])
    coarse, _ = _furnace(64, 128, n, v, a)
    fine, _ = _furnace(128, 256, n, v, a)
    rule = np.abs(coarse - fine).max()
    print(f"\n[light furnace] 64 x 128 against albedo {np.abs(coarse - a).max():.3e}, against 128 x 256 {rule:.3e}")
    assert rule > 0 and np.abs(coarse - a).max() <= 2 * rule
    # and through the restatement itself, fresnel 0: the result is a + what the specular term adds, the same for every channel
    g = np.zeros((40, L.ROW), np.float32)
    g[:, 0:3], g[:, 3], g[:, 4], g[:, 5:8], g[:, 8] = a, 0.5, 1.0, n, 1.0
    g64 = g[:, 5:8].astype(np.float64)
    cells = L.env_cells(np.ones((64, 128, 3), np.float32), 64, 128).astype(np.float32)
    full = L.light_gbuffer(g, v.astype(np.float32), cells, 0.0, 0)
    diffuse = L.light_gbuffer(g, v.astype(np.float32), cells, 0.0, 0, specular_on=False)
    assert np.abs(diffuse[:, 0:3] - g[:, 0:3].astype(np.float64)).max() <= 2 * rule + 1e-6       # float32 cells: + their rounding
    extra = full[:, 0:3] - diffuse[:, 0:3]
    assert (extra >= 0).all() and np.abs(extra - extra[:, :1]).max() < 1e-12 and g64.shape == (40, 3)


# ---- the light-cell reduction ---------------------------------------------------------------------------------------------------------
def test_env_cells_restatement():
    hdr = L.hdr_map(12, 24, 5)
    same = L.env_cells(hdr, 12, 24)
    assert np.abs(same[:, 4:7] - hdr.reshape(-1, 3).astype(np.float64)).max() <= 1e-15 * hdr.max()     # factor (1, 1): the map itself
    assert np.array_equal(same[:, 7], np.zeros(12 * 24))
    flux = (same[:, 3:4] * same[:, 4:7]).sum(0)
    for f in (2, 3):
        red = L.env_cells(hdr, 12 // f, 24 // f)
        assert np.abs((red[:, 3:4] * red[:, 4:7]).sum(0) / flux - 1).max() < 1e-12, f
        assert abs(red[:, 3].sum() / same[:, 3].sum() - 1) < 1e-12
        assert np.abs(np.linalg.norm(red[:, 0:3], axis=1) - 1).max() < 1e-15
    with pytest.raises(ValueError):
        L.env_cells(hdr, 5, 24)
    # the centre directions are Environment_Light's (relight.py), on the cell grid
    lat, lng = np.pi / 6, 2 * np.pi / 12
    phi, theta = torch.meshgrid([torch.linspace(np.pi / 2 - 0.5 * lat, -np.pi / 2 + 0.5 * lat, 6, dtype=torch.float64),
                                 torch.linspace(np.pi - 0.5 * lng, -np.pi + 0.5 * lng, 12, dtype=torch.float64)], indexing="ij")
    dirs = torch.stack([torch.cos(theta) * torch.cos(phi), torch.sin(theta) * torch.cos(phi), torch.sin(phi)], dim=-1).numpy()
    assert np.abs(L.cell_dirs(6, 12) - dirs).max() < 1e-14


# ---- the yardstick: float32 against float64 on every fixture of the GPU tests ---------------------------------------------------------
def test_float32_restatement_distances():
    """Printed per fixture (DESIGN 4.9 tabulates them); asserted: no fixture has a pair within 1e-6 of the horizon threshold (so no
    comparison excludes anything), float32 and float64 take the same pairs, and roughness 0.02 reaches the denominator's lower
    clamp."""
    worst = 0.0
    cases = [(M, 33, 0.5, 3) for M in L.M_CASES] + [(65, D, 0.5, 3) for D in L.D_CASES] + \
            [(65, 33, 0.5, f) for f in range(4)] + [(65, 33, r, 3) for r in L.ROUGH_CASES] + [(65, 33, r, 0) for r in L.ROUGH_CASES]
    for M, D, rough, flags in cases:
        g, v, cells = L.surface_rows(M, D, rough)
        s64, s32 = {}, {}
        ref = L.light_gbuffer(g, v, cells, 0.04, flags, np.float64, stats=s64)
        f32 = L.light_gbuffer(g, v, cells, 0.04, flags, np.float32, stats=s32)
        assert f32.dtype == np.float32
        d = L.distance(f32, ref)
        worst = max(worst, d)
        print(f"\n[light float32 M {M} D {D} roughness {rough} flags {flags}] distance {d:.2e}, pairs {s64['pairs']}, excluded "
              f"{s64['near_threshold']}, clamped denominators {s64['nom_low']}")
        assert s64["near_threshold"] == 0 and s32["pairs"] == s64["pairs"]
        if M > 6 and rough == 0.02:
            assert s64["nom_low"] > 0
        if M > 2:
            assert (ref[1] == 0).all() and ref[0, 3] == 1
    for name in L.CELL_CASES:
        hdr, h, w = L.cell_case(name)
        d = L.distance(L.env_cells(hdr, h, w, np.float32), L.env_cells(hdr, h, w, np.float64))
        worst = max(worst, d)
        print(f"\n[light float32 cells {name}] distance {d:.2e}")
    assert worst < 1e-4
    g, v, cells = L.horizon_case()
    out = L.light_gbuffer(g, v, cells, 0.04, 0, np.float32)
    only = L.light_gbuffer(g, v, cells[2:3], 0.04, 0, np.float32)
    assert np.array_equal(out, only) and (out[0, :3] > 0).all()


# ---- Radiance .hdr ------------------------------------------------------------------------------------------------------------------
def _picture(H, W, seed=0):
    rng = np.random.default_rng(seed)
    x = np.exp(rng.normal(0.0, 2.0, (H, W, 3))).astype(np.float32)
    if W >= 8:
        x[0, : W // 2] = x[0, 0]                  # a long run in every channel
    return x


@pytest.mark.parametrize("W", [1, 7, 8, 9, 300])
def test_hdr_round_trip(tmp_path, W):
    from tensoir_amd import hdr
    x = _picture(5, W, W)
    p, q = str(tmp_path / "a.hdr"), str(tmp_path / "b.hdr")
    hdr.write_hdr(p, x)
    y = hdr.read_hdr(p)
    assert y.dtype == np.float32 and y.shape == x.shape
    assert (np.abs(y.astype(np.float64) - x) <= x.max(-1, keepdims=True).astype(np.float64) / 128).all()
    hdr.write_hdr(q, y)
    assert np.array_equal(hdr.read_rgbe(q), hdr.read_rgbe(p)) and open(q, "rb").read() == open(p, "rb").read()
    raw = open(p, "rb").read()
    body = raw[raw.index(b"+X") :].split(b"\n", 1)[1]
    assert (body[:2] == b"\x02\x02") == (W >= 8) and (len(body) == 5 * W * 4 if W < 8 else True)


def test_hdr_pixel_encoding(tmp_path):
    from tensoir_amd import hdr
    x = np.float32([[[0, 0, 0], [1e-38, 0, 0], [6e4, 1.0, 0.5], [1.0, 0.5, 0.25], [0.9, 0.3, 1e-3]]])
    e = hdr.encode_rgbe(x)
    assert e[0, 0].tolist() == [0, 0, 0, 0] and e[0, 1].tolist() == [0, 0, 0, 0]
    assert e[0, 3].tolist() == [128, 64, 32, 129]                                    # frexp(1) = (0.5, 1)
    m, ex = math.frexp(6e4)
    assert e[0, 2].tolist() == [int(np.float32(6e4) * m * 256 / np.float32(6e4)), int(1.0 * 2.0 ** (8 - ex)), int(0.5 * 2.0 ** (8 - ex)), ex + 128]
    y = hdr.decode_rgbe(e)
    assert (y[0, 0] == 0).all() and (y[0, 1] == 0).all()
    assert y[0, 3].tolist() == [128.5 / 256 * 2, 64.5 / 256 * 2, 32.5 / 256 * 2]       # (byte + 0.5) 2^(E - 136)
    live = x.max(-1) >= 1e-32                                                        # below: four zero bytes, by the format
    assert (np.abs(y - x) <= x.max(-1, keepdims=True) / 128)[live].all() and live.tolist() == [[False, False, True, True, True]]
    assert np.array_equal(hdr.encode_rgbe(y), e)


def _file(tmp_path, body, H, W, head=b"#?RADIANCE\n# a comment\nEXPOSURE=2.5\nFORMAT=32-bit_rle_rgbe\n\n", res=None):
    p = str(tmp_path / "hand.hdr")
    with open(p, "wb") as fh:
        fh.write(head + (res or f"-Y {H} +X {W}\n".encode()) + body)
    return p


def test_hdr_hand_assembled_scanlines(tmp_path):
    """A run-length scanline put together from the format description: per channel a run of 200 (127 + 73: a run holds at most
    127), then a literal span of 100; and a flat scanline below it."""
    from tensoir_amd import hdr
    W = 300
    lit = bytes((7 * i) % 251 for i in range(100))
    body = bytes((2, 2, W >> 8, W & 255))
    for ch, value in enumerate((10, 20, 30, 130)):
        body += bytes((128 + 127, value, 128 + 73, value, 100)) + (lit if ch < 3 else bytes([129] * 100))
    flat = bytes(range(4)) * W
    got = hdr.read_rgbe(_file(tmp_path, body + flat, 2, W))
    assert got.shape == (2, W, 4)
    assert (got[0, :200] == (10, 20, 30, 130)).all()
    assert np.array_equal(got[0, 200:, 0], np.frombuffer(lit, np.uint8)) and (got[0, 200:, 3] == 129).all()
    assert (got[1] == (0, 1, 2, 3)).all()
    rgb = hdr.read_hdr(_file(tmp_path, body + flat, 2, W))
    assert rgb[0, 0].tolist() == [10.5 / 64, 20.5 / 64, 30.5 / 64]                     # 2^(130 - 136)
    # written again, the 200-pixel run crosses the 127 limit and comes back as it was
    q = str(tmp_path / "again.hdr")
    hdr.write_rgbe(q, got)
    assert np.array_equal(hdr.read_rgbe(q), got)
    raw = open(q, "rb").read()
    assert bytes((128 + 127, 10, 128 + 73, 10)) in raw


def test_hdr_refusals(tmp_path):
    from tensoir_amd import hdr
    W = 16
    good = bytes((2, 2, 0, W)) + b"".join(bytes((128 + W, v)) for v in (1, 2, 3, 128))
    assert (hdr.read_rgbe(_file(tmp_path, good, 1, W))[0] == (1, 2, 3, 128)).all()
    with pytest.raises(ValueError, match="resolution"):
        hdr.read_hdr(_file(tmp_path, good, 1, W, res=b"+Y 1 +X 16\n"))
    with pytest.raises(ValueError, match="resolution"):
        hdr.read_hdr(_file(tmp_path, good, 1, W, res=b"-X 16 -Y 1\n"))
    with pytest.raises(ValueError, match="truncated"):
        hdr.read_hdr(_file(tmp_path, good[:-3], 1, W))
    with pytest.raises(ValueError, match="truncated"):
        hdr.read_hdr(_file(tmp_path, bytes(4 * 5 - 1), 1, 5))                          # a flat scanline one byte short
    over = bytes((2, 2, 0, W)) + bytes((128 + 10, 1, 128 + 10, 1)) + b"".join(bytes((128 + W, v)) for v in (2, 3, 128))
    with pytest.raises(ValueError, match="overruns"):
        hdr.read_hdr(_file(tmp_path, over, 1, W))
    with pytest.raises(ValueError):
        hdr.read_hdr(_file(tmp_path, good, 1, W, head=b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n"))


def test_relight_read_hdr_falls_back(tmp_path, monkeypatch):
    """relight.read_hdr without OpenCV, and with the launcher's stand-in for it (which raises on use): the same array as
    hdr.read_hdr."""
    import sys
    from tensoir_amd import hdr, relight, shims
    x = _picture(6, 12, 1)
    p = str(tmp_path / "m.hdr")
    hdr.write_hdr(p, x)
    want = hdr.read_hdr(p)
    monkeypatch.setitem(sys.modules, "cv2", None)                                       # import cv2 -> ImportError
    assert np.array_equal(relight.read_hdr(p), want)
    shims._lazy("cv2", IMREAD_UNCHANGED=-1, COLOR_BGR2RGB=4)                            # replaces the entry; undone with the patch
    assert getattr(sys.modules["cv2"], "__tensoir_shim__", False)
    assert np.array_equal(relight.read_hdr(p), want)
