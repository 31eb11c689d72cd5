"""Three places of the step that pay, or paid, one memory round trip per element: the ordered record sum
(tir_accumulate_records and the record arm of tir_shade_integrate_records) and the capped scan of the record counts in the last
workgroup of tir_march_primary_fused_fwd now issue their loads in groups; the smoothness means in the last workgroup of
tir_composite_primary_fused were measured that way and left as they were.  Regrouping loads may not change a bit or an integer,
so every case here compares EXACTLY against a restatement of the documented order in numpy (float32, sequential) or against
integer sums, and the file passes on the build before the change as well as after it: that is what shows the restatements
describe the old order -- and what the next attempt at the means has to keep.

Record sums: w and rgb are k / 4096 with k in 1 .. 4095, so every product w * c is exact in float32 and fmaf(w, c, acc) equals the
float32 sum acc + w * c; the partial sums round (up to 96 terms of up to 24 bits each), which makes the result depend on the
order.  The gaps between the segments hold NaN: a load outside [b, e) that reached a sum would show."""
import types

import numpy as np
import pytest
import torch

from tests import shade_reference as S

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 8200)        # rays: around one block of 256, around one round of 4096, two rounds and a rest


def dev(t):
    return None if t is None else torch.as_tensor(t).contiguous().cuda()


# ---- the ordered record sum -------------------------------------------------------------------------------------------------------
REC_M, REC_D = 5, 130                                      # lanes 0-1 take three directions, 2-63 two; D = 130 > 128: a second round
REC_COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 96)      # around the groups of 4 and 8, the cap of the secondary march
_records = {}


def records_fixture():
    """-> off [M * D], cnt [M * D] int32, rec_w [R], rec_rgb [R, 3] float32, want [M * D, 3] float32.  Neighbouring directions of a
    point take different counts (a stride of 5 through the 14 values, shifted per point), so every wave mixes them; point 1 has
    no record at all and point 3 has 96 everywhere.  The segments lie in a shuffled pair order, each behind a gap of 1 - 5 NaN
    records, and the last one ends at the buffer's last record."""
    if _records:
        return _records["v"]
    rng = np.random.default_rng(20240611)
    n = REC_M * REC_D
    cnt = np.empty((REC_M, REC_D), np.int64)
    for m in range(REC_M):
        cnt[m] = np.asarray(REC_COUNTS)[(np.arange(REC_D) * 5 + 3 * m) % len(REC_COUNTS)]
    cnt[1], cnt[3] = 0, 96
    cnt = cnt.reshape(-1)
    order = rng.permutation(n)
    last = int(np.nonzero(cnt[order] > 0)[0][-1])           # a non-empty segment goes last
    order[[last, n - 1]] = order[[n - 1, last]]
    gap = rng.integers(1, 6, n)
    off = np.zeros(n, np.int64)
    pos = 0
    for p in order:
        pos += int(gap[p])
        off[p] = pos
        pos += int(cnt[p])
    R = pos
    assert off[order[-1]] + cnt[order[-1]] == R and cnt[order[-1]] > 0
    w = np.full(R, np.nan, np.float32)
    rgb = np.full((R, 3), np.nan, np.float32)
    want = np.zeros((n, 3), np.float32)
    for p in range(n):
        b, e = int(off[p]), int(off[p] + cnt[p])
        w[b:e] = rng.integers(1, 4096, e - b).astype(np.float32) / np.float32(4096)
        rgb[b:e] = rng.integers(1, 4096, (e - b, 3)).astype(np.float32) / np.float32(4096)
    for j in range(int(cnt.max())):                         # sequential in the record index, all pairs side by side
        on = cnt > j
        i = off[on] + j
        want[on] = want[on] + w[i][:, None] * rgb[i]        # float32 throughout: exact product, one rounding of the sum
    assert np.isnan(w).sum() == gap.sum() and np.isfinite(want).all() and want.dtype == np.float32
    _records["v"] = (off.astype(np.int32), cnt.astype(np.int32), w, rgb, want)
    return _records["v"]


def test_records_fixture_is_order_sensitive():
    """The restatement summed backwards differs: the partial sums do round."""
    off, cnt, w, rgb, want = records_fixture()
    back = np.zeros_like(want)
    for j in range(int(cnt.max())):
        on = cnt > j
        i = off[on] + cnt[on] - 1 - j
        back[on] = back[on] + w[i][:, None] * rgb[i]
    assert (back != want).any() and np.abs(back - want).max() < 1e-4


def test_record_sum_is_the_sequential_float32_sum():
    """tir_accumulate_records equals the restatement bit for bit, is finite (no NaN of a gap reached a sum) and zero where a pair
    has no record; the record arm of tir_shade_integrate_records equals tir_shade_integrate fed that tensor, both weightings."""
    from tensoir_amd import ops
    off, cnt, w, rgb, want = records_fixture()
    n = REC_M * REC_D
    got = ops.accumulate_records(dev(off), dev(cnt), dev(w), dev(rgb), n)
    g = got.cpu().numpy()
    print(f"\n[load chains] record sum: {int((g != want).sum())} of {g.size} values differ, {int(cnt.sum())} records in {len(w)} slots")
    assert np.isfinite(g).all()
    assert (g[cnt == 0] == 0).all()
    assert np.array_equal(g, want)
    fx = S.case(REC_M, REC_D, 3, 0.5)
    for equal_area, srgb in ((False, True), (True, False)):
        args = (dev(fx.maps), dev(fx.rays), dev(fx.dirs), dev(fx.light_idx), dev(fx.vis))
        fused = ops.shade_integrate_records(*args, dev(off), dev(cnt), dev(w), dev(rgb), dev(fx.env), dev(fx.weight_d), equal_area, srgb)
        apart = ops.shade_integrate(*args, got.view(REC_M, REC_D, 3), dev(fx.env), dev(fx.weight_d), equal_area, srgb)
        assert torch.isfinite(fused).all() and torch.equal(fused, apart), equal_area


# ---- the capped scan in the primary march's last workgroup ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(golden):
    """The small golden scene of the parity tests and 8200 rays towards it: the golden rays repeated, origins moved a little."""
    import tensoir_amd
    from tensoir_amd import _lib
    from tests.helpers import golden_checkpoint
    assert torch.cuda.is_available() and _lib.lib().tir_device_check() == 0
    eh, ew = [int(x) for x in golden["scene/envmap_hw"]]
    model = tensoir_amd.model_from_checkpoint(golden_checkpoint(golden), "cuda", envmap_h=eh, envmap_w=ew)
    model.march_t_stop = 0.0
    base = torch.from_numpy(np.array(golden["rays/rays"])).float()
    rays = base[torch.arange(max(SIZES)) % base.shape[0]].clone()
    rays[:, :3] += 0.02 * torch.randn(max(SIZES), 3, generator=torch.Generator().manual_seed(5))
    return types.SimpleNamespace(model=model, rays=rays.cuda())


@torch.no_grad()
@pytest.mark.parametrize("B", SIZES)
def test_capped_scan_of_record_counts(scene, B):
    """offsets[0 .. B] = min(exclusive sum of the counts, cap) and total = their sum, exactly, 64 samples per ray, with the cap
    above the total and at half of it; twice each."""
    from tensoir_amd import ops
    m, rays = scene.model, scene.rays[:B].contiguous()
    f = m.packed_field()
    words = torch.zeros((8,), dtype=torch.int32, device="cuda")
    cnt0 = ops.march_primary_fused(f, rays, 64, m.march_t_stop, 1 << 30, words)[3]
    total = int(cnt0.sum())
    print(f"\n[load chains] scan B {B}: {total} records, largest count {int(cnt0.max())}")
    assert B < 255 or (total > 0 and int(cnt0.max()) > 1)   # the rays do hit the scene
    excl = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), cnt0.long().cumsum(0)])
    for cap in (total + 1000, total // 2):
        want = excl.clamp(max=cap).int()
        for call in range(2):                               # the second call: the ticket re-armed itself
            words[1:3].fill_(7)
            _w, _a, _d, cnt, off, tot, _vd = ops.march_primary_fused(f, rays, 64, m.march_t_stop, cap, words)
            assert off.shape == (B + 1,) and torch.equal(cnt, cnt0), (cap, call)
            assert torch.equal(off, want), (cap, call)
            assert int(tot) == total and int(words[3]) == 0 and int(words[1]) == 0 and int(words[2]) == 0, (cap, call)


# ---- the smoothness means in the compositing kernel's last workgroup -----------------------------------------------------------------
def mean_restated(col):
    """float32 [B] -> the mean as the kernel forms it: thread t sums rays t, t + 256, ... in that order; per wave the xor butterfly
    32, 16, 8, 4, 2, 1 (every lane adds its partner's value; lane 0's result); ((p0 + p1) + (p2 + p3)) / B."""
    B = col.shape[0]
    a = np.zeros(256, np.float32)
    for j in range(0, B, 256):
        seg = col[j:j + 256]
        a[:seg.shape[0]] = a[:seg.shape[0]] + seg
    a = a.reshape(4, 64)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lane ^ d]
    p = a[:, 0]
    assert p.dtype == np.float32
    return ((p[0] + p[1]) + (p[2] + p[3])) / np.float32(B)


@torch.no_grad()
@pytest.mark.parametrize("B", SIZES)
def test_smoothness_means_in_documented_order(B):
    """The two means equal mean_restated of columns 17 and 18 of the map rows the same call returned, bit for bit, on synthetic
    records (0 - 70 per ray)."""
    from tensoir_amd import ops
    rng = np.random.default_rng([7, B])
    cnt = rng.integers(0, 71, B)                             # none, a few, more than the 64 lanes of the ray's wave
    cnt[0] = 70
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    R = int(off[-1])
    u = lambda *shape, hi=1.0: rng.uniform(0.0, hi, shape).astype(np.float32)
    d = u(B, 3) - 0.5
    rays = np.concatenate([u(B, 3), d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(np.float32)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    words = torch.zeros((8,), dtype=torch.int32, device="cuda")
    args = (dev(rays), dev(off), dev(u(R, hi=0.03)), dev(u(R, 3)), dev(u(R, 4)), dev(u(R, 4)), dev(unit(u(R, 3) - 0.5)),
            dev(unit(u(R, 3) - 0.5)), dev(u(B)), dev(u(B, hi=4.0)), True, True, 0.04, words)
    for call in range(2):                                   # the second call: the ticket re-armed itself
        maps, smooth = ops.composite_primary_fused(*args)
        mp, got = maps.cpu().numpy(), smooth.cpu().numpy()
        want = np.array([mean_restated(mp[:, 17]), mean_restated(mp[:, 18])], np.float32)
        print(f"\n[load chains] means B {B} call {call}: device {got.tolist()} restated {want.tolist()}")
        assert (mp[:, 17:19] >= 0).all() and (mp[:, 17] > 0).any() and (mp[:, 18] > 0).any()
        assert np.array_equal(got, want) and int(words[4]) == 0, (call, got, want)
