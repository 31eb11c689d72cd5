"""The appearance gathers on a field with exactly ONE light (every single-light configuration; no row of tests/config_scenes.py
has one).  There light_mean is light_line[0], so the both-features gathers form one product tile, run one contraction and store
it to both outputs (app_mfma_body's single-light mode: k_vm_app_primary_one, k_vm_app_mfma<12, true, true, ..., true>), and the
fused indirect kernels skip the per-record light lookup.  The reference of the bitwise tests is the SINGLE-feature launches
(radiance only, intrinsic only) and the stand-alone jitter launch: they never take the single-light mode.

Record counts: a pass is 16 records, a workgroup 64; at 40 007 every wave of the grid walks several passes of both kinds.
n_dev = 0 (a batch whose rays all miss): the point count is clamped on the device, the pass range is empty and no wave reads a
point, a light index or a tap (app_mfma_body: n_pass = 0 -> xcd_range_at gives first >= end).
"""
import os
import sys

import pytest
import torch

from oracle import tensoir_oracle as O
from tests import config_scenes as CS
from tests.helpers import rel_err
from tests.pointwise_ref import scene64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT_TOL = 2e-5                      # tests/test_gpu_config_matrix.py's bound on a gathered feature against the fp64 oracle
ONE_LIGHT = CS.Row("d16_a48_l1", 16, 48, "softplus", 1, False)
COUNTS = (1, 15, 16, 17, 63, 64, 65, 40_007)
N_RAYS = 4096
# (records, device-side live count, light-index vector): zeros; out-of-range entries (-1 and 5 clamp to row 0); n_dev < n; n_dev = 0
CASES = [(n, n, "zeros") for n in COUNTS] + [(65, 65, "clamped"), (40_007, 40_007, "clamped"), (40_007, 33_333, "zeros"),
                                            (40_007, 0, "zeros")]


class Fields:
    def __init__(self):
        import tensoir_amd
        from tensoir_amd import _lib
        assert torch.cuda.is_available()
        assert _lib.lib().tir_device_check() == 0
        self.models, self.refs = {}, {}
        self.tensoir_amd = tensoir_amd

    def model(self, row):
        if row.name not in self.models:
            m = self.tensoir_amd.model_from_checkpoint(CS.checkpoint(row), "cuda", envmap_h=CS.ENVMAP_HW[0], envmap_w=CS.ENVMAP_HW[1])
            assert int(m.packed_field().n_lights) == row.n_lights and int(m.packed_field().n_acomp) == 48
            self.models[row.name] = m
        return self.models[row.name]

    def inputs(self, row, n, n_live, kind):
        """Points as in the merged-gather test of tests/test_gpu_parity.py, a sorted record -> ray map, per-ray light indices and
        the separate launches' results (computed once per case, never modified)."""
        key = (row.name, n, n_live, kind)
        if key not in self.refs:
            from tensoir_amd import ops
            f = self.model(row).packed_field()
            g = torch.Generator().manual_seed(11 + n)
            xyz = (torch.rand(n, 3, generator=g) * 1.6 - 0.8).cuda()
            rec_ray = torch.sort(torch.randint(0, N_RAYS, (n,), generator=g)).values.int().cuda()
            if kind == "zeros":
                lidx = torch.zeros(N_RAYS, dtype=torch.int32)
            elif kind == "clamped":
                lidx = torch.tensor([0, -1, 5, 0, 5, -1, 0], dtype=torch.int32).repeat(N_RAYS // 7 + 1)[:N_RAYS].contiguous()
            else:
                lidx = torch.randint(0, row.n_lights, (N_RAYS,), generator=g).int()
            lidx = lidx.cuda()
            n_dev = torch.tensor([n_live], dtype=torch.int32, device="cuda")
            state = torch.tensor([99, 3], dtype=torch.int64, device="cuda")
            with torch.no_grad():
                rad0 = ops.vm_app(f, xyz, lidx, rec_ray, True, False, "mfma", 0, n_dev)[0]
                intr0 = ops.vm_app(f, xyz, None, None, False, True, "mfma", 0, n_dev)[1]
                xj0, ij0 = ops.vm_app_jitter(f, xyz, 0.01, 0, 0, state, n_dev)
            self.refs[key] = (f, xyz, rec_ray, lidx, n_dev, state, rad0, intr0, xj0, ij0)
        return self.refs[key]


@pytest.fixture(scope="module")
def fields():
    return Fields()


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("n,n_live,kind", CASES)
def test_merged_launch_one_light(fields, n, n_live, kind):
    from tensoir_amd import ops
    f, xyz, rec_ray, lidx, n_dev, state, rad0, intr0, xj0, ij0 = fields.inputs(ONE_LIGHT, n, n_live, kind)
    rad, intr, xj, ij = ops.vm_app_primary(f, xyz, lidx, rec_ray, 0.01, state, n_dev, exact=True)
    torch.cuda.synchronize()
    w, L = int(f.app_dim), n_live
    assert torch.equal(rad[:L, :w], rad0[:L, :w]) and torch.equal(intr[:L, :w], intr0[:L, :w])
    assert torch.equal(rad[:L], intr[:L])                                     # one contraction, two outputs
    assert torch.equal(xj[:L], xj0[:L]) and torch.equal(ij[:L, :w], ij0[:L, :w])
    for t in (rad, intr, ij):
        assert bool((t[:L, w:] == 0).all())
    if L:
        assert float(rad[:L, :w].abs().max()) > 0.0


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("n,n_live,kind", CASES)
def test_both_features_launch_one_light(fields, n, n_live, kind):
    from tensoir_amd import ops
    f, xyz, rec_ray, lidx, n_dev, state, rad0, intr0, xj0, ij0 = fields.inputs(ONE_LIGHT, n, n_live, kind)
    rad, intr = ops.vm_app(f, xyz, lidx, rec_ray, True, True, "mfma", 0, n_dev)
    torch.cuda.synchronize()
    w, L = int(f.app_dim), n_live
    assert torch.equal(rad[:L, :w], rad0[:L, :w]) and torch.equal(intr[:L, :w], intr0[:L, :w])
    assert torch.equal(rad[:L], intr[:L])
    assert bool((rad[:L, w:] == 0).all()) and bool((intr[:L, w:] == 0).all())


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("n", [17, 65])
def test_three_lights_keep_the_general_route(fields, n):
    from tensoir_amd import ops
    f, xyz, rec_ray, lidx, n_dev, state, rad0, intr0, xj0, ij0 = fields.inputs(CS.ROW["d16_a48"], n, n, "random")
    assert int(f.n_lights) == 3
    rad, intr, xj, ij = ops.vm_app_primary(f, xyz, lidx, rec_ray, 0.01, state, n_dev, exact=True)
    w = int(f.app_dim)
    assert torch.equal(rad[:, :w], rad0[:, :w]) and torch.equal(intr[:, :w], intr0[:, :w])
    assert torch.equal(xj, xj0) and torch.equal(ij[:, :w], ij0[:, :w])
    assert not torch.equal(rad[:, :w], intr[:, :w])                           # a light row is not the mean of three
    both = ops.vm_app(f, xyz, lidx, rec_ray, True, True, "mfma", 0, n_dev)
    assert torch.equal(both[0][:, :w], rad0[:, :w]) and torch.equal(both[1][:, :w], intr0[:, :w])


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("n,n_live", [(17, 17), (65, 65), (40_007, 33_333)])
def test_x3_contraction_one_light(fields, n, n_live):
    """The opt-in fp16 hi + lo contraction: the merged-gather test's bound against the exact result, 5e-6 of the feature scale + 1e-7."""
    from tensoir_amd import ops
    f, xyz, rec_ray, lidx, n_dev, state, rad0, intr0, xj0, ij0 = fields.inputs(ONE_LIGHT, n, n_live, "zeros")
    old_c = ops.APP_CONTRACTION
    try:
        ops.APP_CONTRACTION = "x3"
        assert ops.app_contraction() == "x3"
        rad3, intr3, xj3, ij3 = ops.vm_app_primary(f, xyz, lidx, rec_ray, 0.01, state, n_dev)
    finally:
        ops.APP_CONTRACTION = old_c
    w, L = int(f.app_dim), n_live
    assert torch.equal(xj3[:L], xj0[:L])
    for name, got, ref in (("rad", rad3, rad0), ("intr", intr3, intr0), ("intr_jit", ij3, ij0)):
        scale = float(ref[:L, :w].abs().max())
        err = float((got[:L, :w] - ref[:L, :w]).abs().max())
        print(f"\n[one-light] x3 {name} n={n}: err {err:.2e} scale {scale:.2e}")
        assert err < 5e-6 * scale + 1e-7, (name, n, err, scale)
        assert bool((got[:L, w:] == 0).all())


@pytest.mark.gpu
@torch.no_grad()
def test_one_light_features_match_the_oracle(fields):
    from tensoir_amd import ops
    m = fields.model(ONE_LIGHT)
    f = m.packed_field()
    sc, _ = scene64(m)
    g = torch.Generator().manual_seed(5)
    for n in (600, 17):
        x = torch.rand(n, 3, generator=g) * 1.9 - 0.95
        li = torch.zeros(n, dtype=torch.int32)
        r_ref, i_ref = O.both_feature(sc, x.double(), li, "explicit")
        state = torch.tensor([7, 0], dtype=torch.int64, device="cuda")
        rad, intr, _, _ = ops.vm_app_primary(f, x.cuda(), li.cuda(), None, 0.01, state, None, exact=True)
        r2, i2 = ops.vm_app(f, x.cuda(), li.cuda(), None, True, True, "mfma")
        for name, got, ref in (("merged rad", rad, r_ref), ("merged intr", intr, i_ref), ("both rad", r2, r_ref), ("both intr", i2, i_ref)):
            e = rel_err(got[:, :27], ref)
            print(f"\n[one-light] oracle {name} n={n}: {e:.2e}")
            assert e < FEAT_TOL, (name, n, e)


@pytest.mark.gpu
@torch.no_grad()
@pytest.mark.parametrize("n", [31, 32, 33, 385])
def test_fused_indirect_kernels_one_light(fields, n):
    """A wave is 32 records, a tile 384.  The fused f16 kernel against the two launches it replaces at the bound of
    tests/test_gpu_parity.py (1e-5: that test does not demand bit equality) and against the exact route (5e-4); the hp kernel
    against the exact route at its 3e-4.  Out-of-range light indices clamp to row 0: same bits as zeros."""
    from tensoir_amd import ops
    m = fields.model(ONE_LIGHT)
    fld, fh, pm = m.packed_field(), m.packed_field_half(), m.renderModule.packed()
    assert fh is not None
    gen = torch.Generator().manual_seed(100 + n)
    D, npt = 3, 40
    dirs = torch.nn.functional.normalize(torch.randn(D, 3, generator=gen), dim=-1).cuda()
    pts = (torch.rand(n, 3, generator=gen) * 1.9 - 0.95).cuda()
    pair = torch.randint(0, npt * D, (n,), generator=gen).int().cuda()
    lpt = torch.zeros(npt, dtype=torch.int32, device="cuda")
    odd = torch.tensor([0, -1, 5, 0] * (npt // 4), dtype=torch.int32, device="cuda")
    assert D * 8 <= n                                                        # the two-launch route takes its aux-table decoder
    two = ops.mlp(pm, ops.vm_app_h16(fld, fh, pts, lpt, pair, D), dirs, pair, "f16", D)
    exact = ops.mlp(pm, ops.vm_app(fld, pts, lpt, pair, True, False, "mfma", D)[0], dirs, pair, "mfma", D)
    one = ops.indirect_fused(fld, fh, pm, pts, lpt, pair, D, dirs, D)
    hp = ops.indirect_fused_hp(fld, pm, pts, lpt, pair, D, dirs, D)
    assert one.shape == (n, 3) and bool(torch.isfinite(one).all()) and bool(torch.isfinite(hp).all())
    e2, e1, eh = (float((a - b).abs().max()) for a, b in ((one, two), (one, exact), (hp, exact)))
    print(f"\n[one-light] indirect n={n}: fused - two launches {e2:.2e}, fused - exact {e1:.2e}, hp - exact {eh:.2e}")
    assert e2 < 1e-5 and e1 < 5e-4 and eh < 3e-4, (n, e2, e1, eh)
    assert torch.equal(ops.indirect_fused(fld, fh, pm, pts, odd, pair, D, dirs, D), one)
    assert torch.equal(ops.indirect_fused_hp(fld, pm, pts, odd, pair, D, dirs, D), hp)


def test_single_light_gathers_keep_the_register_budget():
    """No GPU: the single-light instantiations the default route launches, held like tests/test_abi.py holds k_vm_app_primary<12, false>."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from tensoir_amd import _lib
    ks = {k["name"]: k for k in kernel_resources.kernels(_lib.LIB_PATH)}
    mine = [n for n in ks if n.startswith("k_vm_app_primary") and not n.startswith("k_vm_app_primary<")]
    assert "k_vm_app_primary_one<12, false>" in mine, sorted(mine)
    for name in mine + ["k_vm_app_mfma<12, true, true, false, false, true>"]:
        k = ks[name]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 256, k
