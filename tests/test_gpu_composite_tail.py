"""The end of the step's two small launches that reserve on one address.

tir_composite_primary_fused runs 1024-thread workgroups (16 rays each, one ticket per workgroup) where tir_composite_primary keeps
its four-ray workgroups: the per-ray arithmetic is the same function, so map columns 0-16 and 19 are bit-equal between the two, the
two smoothness means are the means of columns 17 and 18, and the ticket re-arms itself (a second call gives the same bits).

tir_shade_setup_compact: what any regrouping of its reservations has to keep (the form with four 1024-pair chunks per workgroup was
measured, found slower and taken out; the kernel is the earlier one).  The list is a permutation of the active pairs: whole
1024-pair chunks in any order, thread order inside a chunk."""
import numpy as np
import pytest
import torch

from tests import shade_reference as S

pytestmark = pytest.mark.gpu

RECORDS = (200, 0, 1, 64, 65)             # per ray, cycled: more than three rounds of the ray's wave, none, one, a full wave, one more


def dev(a):
    return torch.as_tensor(a).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@torch.no_grad()
@pytest.mark.parametrize("B", [1, 4, 5, 17, 1023, 1025])
def test_composite_fused_equals_plain(B):
    from tensoir_amd import ops
    rng = np.random.default_rng([12, B])
    cnt = np.array([RECORDS[i % len(RECORDS)] for i in range(B)])
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    R = int(off[-1])
    u = lambda *shape, hi=1.0: rng.uniform(0.0, hi, shape).astype(np.float32)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    rays = np.concatenate([u(B, 3), unit(u(B, 3) - 0.5)], axis=1).astype(np.float32)
    args = (dev(rays), dev(off), dev(u(R, hi=0.01)), dev(u(R, 3)), dev(u(R, 4)), dev(u(R, 4)), dev(unit(u(R, 3) - 0.5)),
            dev(unit(u(R, 3) - 0.5)), dev(u(B)), dev(u(B, hi=4.0)), True, True, 0.04)
    plain = ops.composite_primary(*args)
    words = torch.zeros((8,), dtype=torch.int32, device="cuda")
    first = None
    for call in range(2):
        maps, smooth = ops.composite_primary_fused(*args, words)
        assert int(words[4]) == 0, (B, call, "ticket not re-armed")
        cols = list(range(17)) + [19]
        assert torch.equal(bits(maps[:, cols]), bits(plain[:, cols])), (B, call)
        assert torch.equal(bits(maps[:, 17:19]), bits(plain[:, 17:19])), (B, call)       # the same values, stored write-through
        want = maps[:, 17:19].cpu().double().mean(0)
        got = smooth.cpu().double()
        rel = ((got - want).abs() / want.abs()).max()
        print(f"\n[composite tail] B {B} call {call}: means {smooth.tolist()} float64 {want.tolist()} rel {float(rel):.2e}")
        assert bool((want > 0).all()) and float(rel) <= 1e-6, (B, call, got, want)
        if first is None:
            first = smooth.clone()
        assert torch.equal(bits(smooth), bits(first)), (B, call, "second call differs")


@torch.no_grad()
@pytest.mark.parametrize("M", [1, 7, 300])
def test_shade_setup_compact_chunks(M):
    from tensoir_amd import ops
    D = 128
    gen = torch.Generator().manual_seed(1200 + M)
    nrm = lambda t: torch.nn.functional.normalize(t, dim=-1)
    maps = torch.zeros((M, ops.MAP_STRIDE))
    maps[:, 3] = torch.rand(M, generator=gen) * 3 + 0.5
    maps[:, 4:7] = nrm(torch.randn(M, 3, generator=gen))
    maps[:, 14] = 1.0
    rays = torch.cat([torch.rand(M, 3, generator=gen), nrm(torch.randn(M, 3, generator=gen))], -1)
    dirs = nrm(torch.randn(D, 3, generator=gen))
    active = S.shade_setup(maps, rays, dirs, 0.5, torch.float32)[1]
    assert torch.equal(active, S.shade_setup(maps, rays, dirs, 0.5, torch.float64)[1])
    want = torch.nonzero(active.reshape(-1)).reshape(-1)
    assert 0.3 * M * D < want.numel() < 0.7 * M * D                  # about half of the pairs pass
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    surf, act, ids, vis, rec_cnt = ops.shade_setup_compact(dev(maps), dev(rays), dev(dirs), 0.5, n)
    assert int(n) == want.numel() and torch.equal(act.cpu().bool(), active)
    ids = ids.cpu()[:int(n)].long()
    assert torch.equal(torch.sort(ids).values, want), "the list is not the set of active pairs"
    off = ~active.reshape(-1)
    assert bool((vis.cpu()[off] == 0).all()) and bool((rec_cnt.cpu()[off] == 0).all())
    # thread order (direction-major, the default): pair (m, d) is thread d * M + m; a chunk = 1024 consecutive threads
    assert ops.TUNE["pair_order"] in (0, 1)
    t = (ids % D) * M + ids // D
    chunk = t // 1024
    starts = torch.nonzero(torch.cat([torch.tensor([True]), chunk[1:] != chunk[:-1]])).reshape(-1)
    assert starts.numel() == torch.unique(chunk).numel(), "a chunk's pairs are not contiguous in the list"
    same = chunk[1:] == chunk[:-1]
    assert bool((t[1:][same] > t[:-1][same]).all()), "thread order broken inside a chunk"
    print(f"\n[shade setup chunks] M {M}: {int(n)} of {M * D} pairs active, {starts.numel()} chunks")
