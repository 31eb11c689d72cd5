"""What relighting with multiple importance sampling promises without a GPU: the C ABI of its two entry points and
their argument checks, that both densities of tests/mis_reference.py are densities, that its estimator is unbiased under each
strategy alone and under both, that the fixtures of tests/test_gpu_mis.py leave almost no pair to exempt, and MisConfig."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import mis_reference as R

F32, F64 = torch.float32, torch.float64
ARG, UNSUPPORTED = -1001, -1002


@pytest.fixture(scope="module")
def lib():
    from tensoir_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_both_entry_points_and_the_binding_matches(lib):
    from tensoir_amd import _lib
    # pointers, 32-bit integers, the float and the two 64-bit Philox words, in the header's order (the binding is derived from
    # the header, and tests/test_abi.py holds every entry of it to the compiler's reading of the prototypes)
    kinds = {"tir_env_mis_setup": "PPIIPIPPPPPIIIFUUIPPIIPPPPPPPP", "tir_relight_mis": "PPPPPPPPPPIIIPPP"}
    want = {C.c_void_p: "P", C.c_float: "F", C.c_uint64: "U", C.c_int32: "I"}
    for name in ("tir_env_mis_setup", "tir_relight_mis"):
        assert name in _lib.SIGNATURES, f"{name} is not declared in tensoir_hip.h"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(kinds[name])
        assert hasattr(lib, name)
        assert "".join(want[a] for a in args) == kinds[name], name


def _setup_args(ptr, **kw):
    a = dict(row_cdf=ptr, col_cdf=ptr, H=8, W=16, env_cell=ptr, stride=8, env_pdf=None, row_sin=ptr, normal=ptr, rays_d=ptr, rough=ptr, M=4,
             n_l=32, n_b=32, select=0.5, seed=1, offset=1, block_pairs=512, row_guide=None, col_guide=None, g_rows=0, g_cols=0, dirs=ptr,
             cell=ptr, pdf_mix=ptr, vis=ptr, pair_ids=ptr, n_active=ptr, m_dev=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def test_entry_points_validate_before_any_device_work(lib):
    """Null pointers, N < 1, negative counts, lobe_select outside [0, 1] (a NaN too) and block_pairs outside the LDS layout are
    refused on the host: the pointers below are host addresses, never dereferenced, and no GPU need be present."""
    keep = torch.zeros(64, dtype=torch.float32)
    ptr = keep.data_ptr()
    assert ptr % 16 == 0
    setup = lambda **kw: lib.tir_env_mis_setup(*_setup_args(ptr, **kw))
    for name in ("row_cdf", "col_cdf", "env_cell", "row_sin", "normal", "rays_d", "rough", "dirs", "cell", "pdf_mix", "vis", "pair_ids",
                 "n_active"):
        assert setup(**{name: None}) == ARG, name
    assert setup(stride=3) == ARG                                     # the direction table alone: env_pdf is required
    assert setup(stride=4) == ARG
    assert setup(n_l=0, n_b=0) == ARG                                 # N < 1
    assert setup(n_l=-1) == ARG and setup(n_b=-1) == ARG and setup(n_l=-1, n_b=5) == ARG
    for s in (-0.01, 1.01, float("nan"), float("inf")):
        assert setup(select=s) == ARG, s
    for bp in (0, 255, 32769, -512):
        assert setup(block_pairs=bp) == UNSUPPORTED, bp
    assert setup(M=-1) == ARG and setup(H=0) == ARG
    assert setup(row_guide=ptr) == ARG                                # one guide table without the other
    assert setup(row_guide=ptr, col_guide=ptr, g_rows=6, g_cols=16) == ARG       # not a power of two
    assert setup(M=0) == 0                                            # nothing to do
    assert setup(M=1 << 20, n_l=1 << 10, n_b=1 << 10) == UNSUPPORTED  # 2^31 pairs: 32-bit pair ids
    relight = lambda M=4, N=64, linear=0, **kw: lib.tir_relight_mis(*[kw.get(k, ptr) for k in (
        "normal", "albedo", "rough", "fresnel", "rays_d", "dirs", "cell", "pdf_mix", "env_cell", "vis")], M, N, linear, kw.get("out", ptr), None, None)
    for name in ("normal", "albedo", "rough", "fresnel", "rays_d", "dirs", "cell", "pdf_mix", "env_cell", "vis", "out"):
        assert relight(**{name: None}) == ARG, name
    assert relight(N=0) == ARG and relight(M=-1) == ARG and relight(linear=2) == ARG
    assert relight(env_cell=ptr + 4) == ARG                           # the records are read 16 bytes at a time
    assert relight(M=0) == 0


# ---- MisConfig -----------------------------------------------------------------------------------------------------------------------
def test_mis_config_validation_and_split():
    from tensoir_amd.relight import MisConfig
    cfg = MisConfig()
    assert (cfg.brdf_fraction, cfg.lobe_select, cfg.linear) == (0.5, 0.5, False)
    assert cfg.split(512) == (256, 256) and cfg.split(1) == (1, 0) and cfg.split(3) == (1, 2)     # round(1.5) = 2: half to even
    assert MisConfig(0.0).split(64) == (64, 0) and MisConfig(1.0).split(64) == (0, 64) and MisConfig(0.25).split(130) == (98, 32)
    for n in (1, 2, 7, 16, 64, 513):
        for f in (0.0, 0.1, 0.5, 0.77, 1.0):
            n_l, n_b = MisConfig(f).split(n)
            assert n_l >= 0 and n_b >= 0 and n_l + n_b == n and n_b == round(f * n)
    for bad in (-0.1, 1.1, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError):
            MisConfig(brdf_fraction=bad)
        with pytest.raises(ValueError):
            MisConfig(lobe_select=bad)
    with pytest.raises(ValueError):
        cfg.split(0)


def test_relighting_entry_points_refuse_what_is_not_a_config():
    from tensoir_amd import relight
    z = torch.zeros((0, 3))
    with pytest.raises(TypeError):
        relight.relight_importance_sampled(None, None, "m", z, z, z, z, z, z, mis=0.5)
    with pytest.raises(TypeError):
        relight.relight_view(None, None, ["m"], torch.zeros((4, 6)), 2, 2, mis={"brdf_fraction": 0.5})


def test_mis_needs_the_cell_records(monkeypatch):
    """TENSOIR_ENV_RECORDS=0 together with mis raises, as a device-side point count does; M = 0 still consumes its draw counter."""
    from tensoir_amd import _lib, relight
    lt = R.light("m5x12")
    env = relight.Environment_Light(hdr_maps={"m": lt.hdr}, device="cpu")
    z = torch.zeros((0, 3))
    monkeypatch.setattr(relight.ops, "pack_env_cells", lambda d, c, p: torch.zeros((d.reshape(-1, 3).shape[0], 8)))
    before = env._draws
    out = relight.relight_importance_sampled(None, env, "m", z, z, z, torch.zeros((0, 1)), z, z, mis=relight.MisConfig())
    assert out.shape == (0, 3) and env._draws == before + 1
    monkeypatch.setenv("TENSOIR_ENV_RECORDS", "0")
    with pytest.raises(_lib.TensoirHipError, match="TENSOIR_ENV_RECORDS"):
        relight.relight_importance_sampled(None, env, "m", z, z, z, torch.zeros((0, 1)), z, z, mis=relight.MisConfig())
    with pytest.raises(_lib.TensoirHipError, match="TENSOIR_ENV_RECORDS"):
        env.sample_mis("m", z, z, torch.zeros(0), 16, relight.MisConfig())


# ---- the densities are densities -----------------------------------------------------------------------------------------------------
def _quadrature(fn, n_theta, n_phi, axis=None):
    w, dw = R.sphere_grid(n_theta, n_phi, axis)
    return float((fn(w) * dw).sum())


def _refined(fn, axis, n_theta=500, n_phi=64, step=1e-4, limit=64000):
    """midpoint quadrature about `axis`, the polar grid doubled until the float64 result moves by less than `step`"""
    got = _quadrature(fn, n_theta, n_phi, axis)
    while n_theta < limit:
        n_theta *= 2
        last, got = got, _quadrature(fn, n_theta, n_phi, axis)
        if abs(got - last) < step:
            break
    return got, n_theta


@pytest.mark.parametrize("name", list(R.MAPS))
def test_light_density_integrates_to_one(name):
    lt = R.light(name)

    def p_l(w):
        row, col = R.cell_of(w, lt.H, lt.W)
        return R.pdf_light(lt, w, row * lt.W + col, F64)
    got = _quadrature(p_l, 40 * lt.H, 40 * lt.W)                      # constant per cell in (theta, phi): the midpoint rule is exact
    print(f"\n[mis p_l {name}] integral {got:.9f}")
    assert abs(got - 1.0) <= 1e-3
    assert abs(float(lt.prob.double().sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("rough", [0.1, 0.3, 1.0])
def test_brdf_density_integrates_to_one(rough):
    """At normal incidence every half vector of the lobe reflects (v.h = Nf.h > 0): p_b integrates to 1.  Seen from 60 degrees
    the half vectors with v.h <= 0 give no direction (the sample is inactive), and p_b integrates to s + (1 - s) x the mass of the
    half-vector distribution on v.h > 0, found by its own quadrature over h: the mixture density the estimator divides by is the
    density of the directions that are generated.  Polar grids about the mirror direction, doubled until the result moves by less than 1e-4."""
    n = torch.tensor([0.36, -0.48, 0.8], dtype=F64)
    alpha2 = torch.tensor(rough ** 4, dtype=F64)
    t, b = R.frame(n)
    for label, v, flip in (("normal incidence", n, 1.0), ("60 degrees", 0.5 * n + math.sqrt(0.75) * t, 1.0),
                           ("60 degrees, flipped", -(0.5 * n + math.sqrt(0.75) * t), -1.0)):
        Nf = flip * n
        mirror = 2.0 * torch.sum(v * Nf) * Nf - v
        for s in (0.0, 0.5):
            def half_mass(h):
                noh = torch.sum(h * Nf, -1).clamp(min=0.0)
                cr = torch.linalg.cross(Nf.expand_as(h), h, dim=-1)
                d = alpha2 / (math.pi * (torch.sum(cr * cr, -1) + alpha2 * noh * noh) ** 2)
                return torch.where(torch.sum(h * v, -1) > 0, d * noh, torch.zeros_like(noh))
            n_phi = 64 if label == "normal incidence" else 512
            mass, _ = _refined(half_mass, Nf, n_phi=n_phi)
            want = s + (1.0 - s) * mass
            got, n_theta = _refined(lambda w: R.pdf_brdf(n, Nf, v, alpha2, s, w), mirror, n_phi=n_phi)
            print(f"\n[mis p_b roughness {rough} {label} s {s}] integral {got:.6f} (reflecting mass {mass:.6f}, {n_theta} polar steps)")
            assert abs(got - want) <= 1e-3
            if label == "normal incidence":
                assert abs(got - 1.0) <= 1e-3 and abs(mass - 1.0) <= 1e-3


# ---- the estimator is unbiased -------------------------------------------------------------------------------------------------------
N_UNBIASED = 1 << 16


@pytest.fixture(scope="module")
def unbiased_points():
    pts = R.points(67)
    rows = [i for i in range(67) if float(pts.rough[i]) >= 0.3][:4]
    flipped = [i for i in rows if float((pts.normal[i] * -pts.rays_d[i]).sum()) < 0]
    assert flipped and len(rows) == 4
    return R.take(pts, rows)


@pytest.fixture(scope="module")
def quadratures(unbiased_points):
    """fine-grid midpoint quadrature of the integrand with V = 1, per map: grid lines on every cell border"""
    out = {}
    for name in R.MAPS:
        lt = R.light(name)
        w, dw = R.sphere_grid(80 * lt.H, 80 * lt.W)
        coarse_w, coarse_dw = R.sphere_grid(40 * lt.H, 40 * lt.W)
        fine = (R.integrand(lt, unbiased_points, w) * dw[None, :, None]).sum(1)
        coarse = (R.integrand(lt, unbiased_points, coarse_w) * coarse_dw[None, :, None]).sum(1)
        out[name] = fine, float(((fine - coarse).abs() / fine.abs()).max())
    return out


@pytest.mark.parametrize("n_l,n_b", [(N_UNBIASED, 0), (0, N_UNBIASED), (N_UNBIASED // 2, N_UNBIASED // 2)], ids=["light", "brdf", "half"])
@pytest.mark.parametrize("name", list(R.MAPS))
def test_estimator_is_unbiased(name, n_l, n_b, unbiased_points, quadratures):
    """V = 1, float64, N = 2^16, the linear estimate: within 5 standard errors of the quadrature; the standard error from the
    restatement's own per-sample values, per strategy (the two strata have fixed sizes)."""
    lt, pts = R.light(name), unbiased_points
    want, refinement = quadratures[name]
    s = R.setup(lt, pts, n_l, n_b, R.SELECT, R.SEED, 11, F64)
    x = R.samples(lt, pts, s.dirs, s.cell, s.pdf_mix, s.active.to(F64), F64)            # [M, N, 3]
    N = n_l + n_b
    got = x.mean(1)
    assert torch.allclose(got, R.relight(lt, pts, s.dirs, s.cell, s.pdf_mix, s.active.to(F64), True, F64))
    var = sum(part.var(dim=1, unbiased=True) * part.shape[1] for part in (x[:, :n_l], x[:, n_l:]) if part.shape[1] > 1)
    se = torch.sqrt(var) / N
    z = ((got - want) / se).abs()
    print(f"\n[mis unbiased {name} n_l {n_l} n_b {n_b}] max |estimate - quadrature| / se {float(z.max()):.2f}, relative se "
          f"{float((se / want).max()):.2e}, quadrature moved {refinement:.1e} when refined")
    assert refinement < 0.1 * float((se / want).min())
    assert (z <= 5.0).all(), z


# ---- the GPU fixtures leave almost nothing to exempt ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.MAPS))
def test_exempt_share_and_dtype_agreement(name):
    """On every fixture used on the GPU at most 1 % of the pairs are exempt, and the float32 and float64 restatements agree on cell,
    active and lobe choice for every other pair."""
    for M in R.POINTS:
        for n_l, n_b in R.SPLITS:
            a, b = R.case(name, M, n_l, n_b, F64), R.case(name, M, n_l, n_b, F32)
            share = float(a.exempt.double().mean())
            keep = ~a.exempt
            assert share <= 0.01, (M, n_l, n_b, share)
            for what in ("cell", "active", "lobe"):
                assert torch.equal(getattr(a, what)[keep], getattr(b, what)[keep]), (M, n_l, n_b, what)
            assert torch.equal(a.lobe == R.LIGHT, torch.arange(n_l + n_b).expand(M, -1) < n_l)
            own = (a.lobe == R.LOBE) & a.active                    # a lobe sample's own density is the density of its direction
            assert torch.allclose(a.pdf_lobe_own[own], a.pdf_lobe_w[own], rtol=1e-8, atol=0)
            if M == 67 and n_b >= 30:
                assert (a.lobe == R.COSINE).any() and (a.lobe == R.LOBE).any() and (~a.active[a.lobe == R.LOBE]).any()
    pts = R.points(67)
    nov = (torch.nn.functional.normalize(pts.normal.double(), dim=-1) * torch.nn.functional.normalize(-pts.rays_d.double(), dim=-1)).sum(-1)
    assert (nov < -0.05).sum() > 10 and (nov > 0.05).sum() > 10 and (nov.abs() >= 0.05 - 1e-6).all()
    assert float(pts.rough.min()) >= 0.1 and float(pts.rough.max()) <= 1.0
    hdr = R.light(name).hdr
    assert float(hdr.max()) >= 15 * float(hdr.mean()) and float(hdr.min()) > 0


def test_philox_restatement_is_a_counter_function():
    """Known answer of Philox-4x32-10 (Random123's kat vectors: zero key and counter) through the uniform mapping, and the counter
    layout: one call over many counters equals calls one by one."""
    zero = R.philox_uniform4(0, 0, np.array([0], dtype=np.uint64))[0]
    words = np.array([0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], dtype=np.uint64)
    want = np.minimum((words.astype(np.float32) + np.float32(0.5)) * np.float32(2.3283064365386963e-10), np.float32(0.99999994))
    assert np.array_equal(zero, want)
    many = R.philox_uniform4(R.SEED, 5, np.arange(1000, dtype=np.uint64) + (1 << 33))
    one = np.stack([R.philox_uniform4(R.SEED, 5, np.array([i + (1 << 33)], dtype=np.uint64))[0] for i in (0, 1, 999)])
    assert np.array_equal(many[[0, 1, 999]], one) and many.min() > 0 and many.max() < 1
    assert abs(float(many.mean()) - 0.5) < 0.02
