"""Host logic of round 5 that needs no GPU: the verdict state machine of the indirect-light precision policy
(indirect.mode / set_verdict), its self-check ladder and record estimate (indirect.establish / record_estimate), the
record-capacity hint and protocol (capacity.learn_capacity, capacity.PassCapacity, capacity.check_site), the range guard's bound (ops.HalfRange.judge), the shard layout used by the image
all-gather (dist._layout / gather_records at world 1) and the arithmetic of bench.simulate_ranks."""
import math
import os
import sys
import time
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Dec:
    def __init__(self):
        self._key = ((100, 0),)

    def packed(self):
        return None


class _Model:
    """The three attributes the state machine reads: the packed-field key (first element: one (ptr, version, shape) per parameter),
    the radiance decoder's key, and a __dict__ for the state."""

    def __init__(self):
        self._field_key = (((1000, 0, (1, 48, 8, 8)), (2000, 0, (1, 48, 8, 1))), "rest")
        self.renderModule = _Dec()

    def step(self):                      # an optimizer step: same storage, next version
        self._field_key = (tuple((p, v + 1, s) for p, v, s in self._field_key[0]), "rest")

    def realloc(self):                   # upsample / shrink: new storage
        self._field_key = (tuple((p + 64, 0, s) for p, v, s in self._field_key[0]), "rest")

    def packed_field(self):
        return None


@pytest.fixture
def auto_policy(monkeypatch):
    from tensoir_amd import ops
    monkeypatch.setattr(ops, "INDIRECT_GUARD", True)
    monkeypatch.setattr(ops, "SECONDARY_MLP_IMPL", "f16")
    monkeypatch.setattr(ops, "SECONDARY_APP_IMPL", "h16")
    monkeypatch.setattr(ops, "MLP_IMPL", "bf16x3")
    return ops


def test_verdict_state_machine(auto_policy):
    from tensoir_amd import indirect
    ops, m = auto_policy, _Model()
    assert indirect.mode(m) == "probe"                          # nothing known yet
    indirect.set_verdict(m, "f16", "probe", {"map_max_abs": 1e-6})
    assert indirect.mode(m) == "f16" and indirect.mode(m, training=True) == "f16"
    # inference: a verdict belongs to exactly one parameter version
    m.step()
    assert indirect.mode(m) == "probe"
    # training: carried over for `interval` versions of the same storage, then re-established
    for _ in range(ops.INDIRECT_PROBE["interval"]):
        assert indirect.mode(m, training=True) == "f16"
        assert indirect.mode(m, training=True) == "f16"         # (asking twice for one version does not age it twice)
        m.step()
    assert indirect.mode(m, training=True) == "probe"
    # ... and an inference pass never inherits a CARRIED verdict: strict verdict at v0, five training steps, inference at v5 probes
    m2 = _Model()
    indirect.set_verdict(m2, "f16", "probe", {"map_max_abs": 1e-6})
    for _ in range(5):
        m2.step()
        assert indirect.mode(m2, training=True) == "f16"
    assert indirect.mode(m2) == "probe"
    assert indirect.mode(m2, training=True) == "f16"            # (the training loop still rides on it)
    indirect.set_verdict(m, "full", "probe", {"map_max_abs": 9e-5})
    assert indirect.state(m)["fallbacks"] == 1
    m.step()
    assert indirect.mode(m, training=True) == "full"
    # new storage (upsample, shrink, a model rebuilt from a checkpoint): at once
    m.realloc()
    assert indirect.mode(m, training=True) == "probe"
    # a verdict taken with the TRAINING limit never serves an inference pass of the same version
    indirect.set_verdict(m, "f16", "probe", {"map_max_abs": 6e-5}, train_limit=True)
    assert indirect.mode(m, training=True) == "f16" and indirect.mode(m) == "probe"
    indirect.set_verdict(m, "full", "probe", {"map_max_abs": 6e-5})
    assert indirect.mode(m) == "full"


def test_forced_policies_bypass_the_state_machine(monkeypatch):
    from tensoir_amd import indirect, ops
    m = _Model()
    monkeypatch.setattr(ops, "MLP_IMPL", "bf16x3")
    monkeypatch.setattr(ops, "INDIRECT_GUARD", False)
    monkeypatch.setattr(ops, "SECONDARY_MLP_IMPL", "f16")
    monkeypatch.setattr(ops, "SECONDARY_APP_IMPL", "h16")
    assert indirect.mode(m) == "f16"
    monkeypatch.setattr(ops, "SECONDARY_MLP_IMPL", None)
    monkeypatch.setattr(ops, "SECONDARY_APP_IMPL", None)
    assert indirect.mode(m) == "full"
    monkeypatch.setattr(ops, "SECONDARY_MLP_IMPL", "f16")
    monkeypatch.setattr(ops, "SECONDARY_APP_IMPL", "h16")
    monkeypatch.setattr(ops, "MLP_IMPL", "mfma")                        # the exact decoder modes stay exact end to end
    assert indirect.mode(m) == "full"


class _Ladder:
    """decode / measure of indirect.establish on the CPU: one small distinct tensor per tier, the tiers asked for in order, and a
    scripted measurement per candidate tier (a callable is evaluated on the spot, as the real comparisons are)."""

    def __init__(self, script):
        self.rows = {k: torch.full((4, 3), float(i)) for i, k in enumerate(("f16", "hp", "full"))}
        self.script, self.asked = script, []

    def decode(self, kind):
        self.asked.append(kind)
        return self.rows[kind]

    def measure(self, rows):
        tier = next(k for k, v in self.rows.items() if v is rows)
        ok, stats = self.script[tier]
        return (ok() if callable(ok) else ok), dict(stats)


def test_ladder_keeps_f16_when_it_passes(auto_policy):
    from tensoir_amd import indirect
    m, lad = _Model(), _Ladder({"f16": (True, {"kind": "map", "map_max_abs": 1e-6})})
    verdict, rows = indirect.establish(m, lad.decode, lad.measure, try_hp=True, train_limit=False)
    assert verdict == "f16" and rows is lad.rows["f16"] and lad.asked == ["f16"]
    st = indirect.state(m)
    assert st["verdict"] == "f16" and st["why"] == "probe" and st["stats"] == {"kind": "map", "map_max_abs": 1e-6}
    assert st["fallbacks"] == 0 and st["probes"] == 1 and st["train_limit"] is False
    assert indirect.mode(m) == "f16" and indirect.verdict(m) == "f16"


def test_ladder_falls_back_to_hp_then_full(auto_policy):
    from tensoir_amd import indirect
    f16_stats, hp_stats = {"kind": "map", "map_max_abs": 7e-5}, {"kind": "map", "map_max_abs": 8e-6}
    m, lad = _Model(), _Ladder({"f16": (False, f16_stats), "hp": (True, hp_stats)})
    verdict, rows = indirect.establish(m, lad.decode, lad.measure, try_hp=True, train_limit=False)
    assert verdict == "hp" and rows is lad.rows["hp"] and lad.asked == ["f16", "hp"]
    st = indirect.state(m)
    assert st["stats"] == {**hp_stats, "f16": f16_stats} and st["fallbacks"] == 1 and st["probes"] == 1
    assert indirect.mode(m) == "hp"
    # both fail: the primary-stage kernels, and the caller gets the full rows object
    m, lad = _Model(), _Ladder({"f16": (False, f16_stats), "hp": (False, hp_stats)})
    verdict, rows = indirect.establish(m, lad.decode, lad.measure, try_hp=True, train_limit=False)
    assert verdict == "full" and rows is lad.rows["full"] and lad.asked == ["f16", "hp", "full"]
    assert indirect.state(m)["stats"] == {**hp_stats, "f16": f16_stats} and indirect.state(m)["fallbacks"] == 1
    assert indirect.mode(m) == "full"
    # the hp tier switched off: never decoded
    m, lad = _Model(), _Ladder({"f16": (False, f16_stats), "hp": (True, hp_stats)})
    verdict, rows = indirect.establish(m, lad.decode, lad.measure, try_hp=False, train_limit=False)
    assert verdict == "full" and rows is lad.rows["full"] and lad.asked == ["f16", "full"]
    assert indirect.state(m)["stats"] == f16_stats and indirect.state(m)["fallbacks"] == 1


def test_ladder_rejects_a_nan_measurement(auto_policy):
    from tensoir_amd import indirect
    nan, limit = float("nan"), 2.5e-5
    m, lad = _Model(), _Ladder({"f16": (lambda: nan <= limit, {"map_max_abs": nan}), "hp": (lambda: nan <= limit, {"map_max_abs": nan})})
    verdict, rows = indirect.establish(m, lad.decode, lad.measure, try_hp=True, train_limit=False)
    assert verdict == "full" and rows is lad.rows["full"] and lad.asked == ["f16", "hp", "full"]


def test_ladder_training_limit_and_probe_count(auto_policy):
    from tensoir_amd import indirect
    m, lad = _Model(), _Ladder({"f16": (True, {"map_max_abs": 6e-5})})
    attrs = set(m.__dict__)
    assert indirect.verdict(m) is None and set(m.__dict__) == attrs                     # (reading creates no state)
    indirect.establish(m, lad.decode, lad.measure, try_hp=True, train_limit=True)
    assert indirect.state(m)["train_limit"] is True
    assert indirect.mode(m) == "probe" and indirect.mode(m, training=True) == "f16"
    for n in (2, 3):                                                     # one per pass that ran the self-check, hp tried or not
        lad.script = {"f16": (False, {}), "hp": (n == 2, {})}
        indirect.establish(m, lad.decode, lad.measure, try_hp=True, train_limit=False)
        assert indirect.state(m)["probes"] == n and indirect.report(m)["probes_run"] == n
    assert indirect.report(m)["mode"] == "full" and indirect.report(m)["fallbacks"] == 2
    indirect.reset(m)
    assert indirect.verdict(m) is None and indirect.report(m)["probes_run"] == 0


def test_record_estimate_statistics(auto_policy, monkeypatch):
    """10 records, at most 4 probed: stride 10 // 4 = 2 -> records 0, 2, 4, 6; the four statistics and the estimate of
    ops.INDIRECT_PROBE's formula, computed here in fp64."""
    from tensoir_amd import indirect
    ops = auto_policy
    monkeypatch.setitem(ops.INDIRECT_PROBE, "records", 4)
    gen = torch.Generator().manual_seed(11)
    ref_all = torch.rand(10, 3, generator=gen)
    cand = ref_all + 1e-5 * torch.randn(10, 3, generator=gen) + torch.tensor([2e-5, 0.0, -1e-5])
    cand = torch.cat([cand, torch.full((2, 3), 9.0)])                   # rows beyond n_valid: never read
    asked = []

    def decode_full_subset(sel):
        asked.append(sel.tolist())
        return ref_all[sel]
    ok, st = indirect.record_estimate(cand, 10, decode_full_subset)
    assert asked == [[0, 2, 4, 6]] and st["kind"] == "records" and st["records"] == 4 and st["of"] == 10
    sel = torch.tensor([0, 2, 4, 6])
    d = (cand[sel] - ref_all[sel]).double()
    bias, rms, mx = float(d.mean(0).abs().max()), float(d.pow(2).mean().sqrt()), float(d.abs().max())
    lim = ops.INDIRECT_PROBE
    est = max(lim["w_bias"] * bias + lim["w_rms"] * rms, lim["w_max"] * mx)
    assert st["bias"] == pytest.approx(bias, rel=1e-12) and st["rms"] == pytest.approx(rms, rel=1e-12)
    assert st["max"] == pytest.approx(mx, rel=1e-12) and st["estimate"] == pytest.approx(est, rel=1e-12)
    assert st["radiance_rms"] == pytest.approx(float(ref_all[sel].double().pow(2).mean().sqrt()), rel=1e-12)
    assert ok == (est <= lim["limit"]) and ok                           # (a few 1e-5: inside the 2.5e-5 limit)
    # outside the limit, and a NaN row: rejected
    assert not indirect.record_estimate(cand + 1e-3, 10, decode_full_subset)[0]
    bad = cand.clone()
    bad[2, 1] = float("nan")
    assert not indirect.record_estimate(bad, 10, decode_full_subset)[0]
    # fewer valid records than rows, and none at all
    assert indirect.record_estimate(cand, 3, decode_full_subset)[1]["records"] == 3 and asked[-1] == [0, 1, 2]
    assert indirect.record_estimate(cand, 0, decode_full_subset) == (True, {"records": 0})


def test_learn_capacity():
    """The record-capacity hint of every stage (primary forward, training forward, secondary march, bake)."""
    from tensoir_amd.capacity import learn_capacity
    h = {}
    learn_capacity(h, "k", 1000, 1.25, max_entries=64)
    assert h == {"k": 16384}                                             # the floor of 16 k rows
    learn_capacity(h, "k", 100000, 1.25, max_entries=64)
    assert h["k"] == 129096                                              # 1.25 x the count + 4096
    learn_capacity(h, "c", 100000, 1.25, ceiling=120000, max_entries=64)
    assert h["c"] == 120000
    h["d"] = 1000000
    learn_capacity(h, "d", 1000, 1.25, max_entries=64)
    assert h["d"] == 970000                                              # decays slowly from a heavy call
    h["d"] = 1000000
    learn_capacity(h, "d", 1000, 1.5, decay=0, max_entries=32)
    assert h["d"] == 16384                                               # ... unless the caller asks for no memory
    learn_capacity(h, "s", 100000, 1.5, max_entries=32)
    assert h["s"] == 154096
    # a table above max_entries is emptied BEFORE the old value is read
    h = {i: 1000000 for i in range(33)}
    learn_capacity(h, 5, 1000, 1.5, max_entries=32)
    assert h == {5: 16384}
    h = {i: 1000000 for i in range(32)}
    learn_capacity(h, 5, 1000, 1.5, max_entries=32)
    assert len(h) == 32 and h[5] == 970000


class _Count:
    """A count source of capacity.PassCapacity that needs no device: answers a chosen integer, remembers what was queued."""
    made = []

    def __init__(self, counter):
        self.counter, self.gets = counter, 0
        _Count.made.append(self)

    def get(self):
        self.gets += 1
        return self.counter["total"]


@pytest.fixture
def counts():
    _Count.made = []
    return _Count.made


PRIMARY = dict(ceiling=4096 * 512, max_entries=64)


def test_pass_capacity_without_a_hint(counts):
    from tensoir_amd.capacity import PassCapacity, learn_capacity
    hints = {"other": 7}
    rc = PassCapacity(hints, (4096, 512), 1.25, count_source=_Count, **PRIMARY)
    assert rc.hinted() is None and counts == [] and hints == {"other": 7}
    # the caller's exact route hands its own count in: learnt, nothing queued
    assert rc.settle(30000) is True and counts == []
    want = {"other": 7}
    learn_capacity(want, (4096, 512), 30000, 1.25, **PRIMARY)
    assert hints == want


@pytest.mark.parametrize("site", [(1.25, dict(ceiling=4096 * 512, max_entries=64)), (1.5, dict(max_entries=32)),
                                  (1.5, dict(decay=0, max_entries=32))], ids=["primary", "secondary", "bake"])
def test_pass_capacity_hinted_and_fits(counts, site):
    from tensoir_amd.capacity import PassCapacity, learn_capacity
    growth, learn = site
    hints, want = {"k": 500000, "other": 7}, {"k": 500000, "other": 7}
    rc = PassCapacity(hints, "k", growth, count_source=_Count, **learn)
    cap = rc.hinted()
    assert cap == 500000
    counter = {"total": 123456}
    rc.watch(counter, cap)
    assert len(counts) == 1 and counts[0].counter is counter and counts[0].gets == 0       # queued at watch(), not read yet
    assert rc.settle() is True and counts[0].gets == 1
    learn_capacity(want, "k", 123456, growth, **learn)
    assert hints == want and hints["k"] != 500000
    counter["total"] = cap                                               # exactly full still fits
    rc.watch(counter, cap)
    assert rc.settle() is True


def test_pass_capacity_overflow_drops_the_hint_and_learns_nothing(counts):
    from tensoir_amd.capacity import PassCapacity
    hints = {i: 1000000 for i in range(70)}                              # (above max_entries: a learn would empty the table)
    rc = PassCapacity(hints, 5, 1.25, count_source=_Count, **PRIMARY)
    rc.watch({"total": 1000001}, rc.hinted())
    assert rc.settle() is False
    assert hints == {i: 1000000 for i in range(70) if i != 5}
    assert rc.regrow(1000001) == int(1000001 * 1.25) + 1024 and PassCapacity.regrow(0) == 1024


def test_pass_capacity_while_capturing(counts):
    from tensoir_amd._lib import TensoirHipError
    from tensoir_amd.capacity import PassCapacity
    checks, hints, counter = [], {77: 20000}, object()
    rc = PassCapacity(hints, 77, 1.5, max_entries=32, capture=checks, check_key=("secondary", 77), count_source=_Count)
    rc.watch(counter, rc.hinted())
    assert len(checks) == 1 and checks[0][0] is counter and checks[0][1:] == (20000, ("secondary", 77))
    assert counts == [] and hints == {77: 20000}                         # no host read is queued inside a capture
    with pytest.raises(TensoirHipError):
        PassCapacity({}, 77, 1.5, max_entries=32, capture=checks, check_key=("secondary", 77), count_source=_Count).hinted()
    assert len(checks) == 1 and counts == []


def test_pass_capacity_ceiling_caps_the_hint(counts):
    from tensoir_amd.capacity import PassCapacity
    hints = {(64, 100): 6300}
    rc = PassCapacity(hints, (64, 100), 1.25, ceiling=64 * 100, max_entries=64, count_source=_Count)
    rc.watch({"total": 6000}, rc.hinted())
    assert rc.settle() is True and hints[(64, 100)] == 6400              # 1.25 x 6000 + 4096 and the 16 k floor are both above B * S


def test_check_site_maps_graph_keys():
    from tensoir_amd.capacity import check_site
    m = types.SimpleNamespace(_app_cap_hints={(4096, 512): 1}, _rec_cap_hints={524288: 2})
    hints, key, need = check_site(m, ("primary", 4096, 512), 100000)
    assert hints is m._app_cap_hints and key == (4096, 512) and need == int(100000 * 1.25) + 4096
    assert check_site(m, ("primary", 64, 100), 6000)[2] == 6400          # never more than rays x samples
    hints, key, need = check_site(m, ("secondary", 524288), 3000000)
    assert hints is m._rec_cap_hints and key == 524288 and need == int(3000000 * 1.25) + 4096
    assert key in hints


def test_half_range_bound():
    from tensoir_amd.ops import HalfRange
    lim = 6.0e4
    ok, b = HalfRange.judge([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 0.5, 0.1], lim)
    assert ok and b == 18.0                                              # a light row below 1 does not shrink the bound
    ok, b = HalfRange.judge([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 0.1], lim)
    assert ok and b == 144.0
    assert not HalfRange.judge([300.0, 1.0, 1.0, 300.0, 1.0, 1.0, 1.0, 0.1], lim)[0]          # plane x line alone leaves the range
    assert not HalfRange.judge([100.0, 1.0, 1.0, 100.0, 1.0, 1.0, 7.0, 0.1], lim)[0]          # ... or with the light row
    assert not HalfRange.judge([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 7.0e4], lim)[0]            # basis_mat is cast to fp16 too
    assert not HalfRange.judge([float("nan"), 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.1], lim)[0]     # a NaN anywhere fails
    assert not HalfRange.judge([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, float("nan"), 0.1], lim)[0]


@pytest.mark.parametrize("tile", [0, 5, 16])
def test_layout_reassembles_every_sharding(tile):
    from tensoir_amd import dist as tdist
    n, world = 103, 4
    cap, index = tdist._layout(n, world, tile, torch.device("cpu"))
    assert cap == tdist.shard_capacity(n, world, tile) and index.shape == (n,)
    # what the all-gather would deliver: rank r's rows, padded to cap
    rows = torch.arange(n, dtype=torch.float32).view(-1, 1).repeat(1, 3)
    gathered = torch.full((world * cap, 3), -1.0)
    for r in range(world):
        mine = tdist.shard_rows(n, r, world, tile)
        gathered[r * cap: r * cap + mine.numel()] = rows[mine]
    assert torch.equal(gathered.index_select(0, index), rows)
    one = tdist.gather_records(rows, n, 0, 1, tile)
    assert torch.equal(one, rows) and one.data_ptr() != rows.data_ptr()


def test_simulate_ranks_arithmetic(monkeypatch):
    import bench
    n, chunk = 16000, 1000
    cost = torch.ones(n)
    cost[:4000] = 0.0                                                    # the first quarter of the "image" is background: free
    # a clock that only the "render" advances (plus a fixed call overhead): the arithmetic is what is tested, and a sleep-based
    # version of this test failed once on a loaded host
    clock = {"t": 0.0}

    def render_shard(mine):
        clock["t"] += float(cost[mine].sum()) * 2e-6 + 5e-5
    monkeypatch.setattr(bench.time, "perf_counter", lambda: clock["t"])
    t1 = float(cost.sum()) * 2e-6 + 5e-5
    sim = bench.simulate_ranks(render_shard, n, chunk, t1, 96, 4, passes=2, tiles=[0, chunk])
    assert [c["world"] for c in sim["configs"]] == [2, 2, 4, 4]
    by = {(c["world"], c["tile"]): c for c in sim["configs"]}
    # row tiles: rank 0 of 4 holds only background, the others a full quarter each -> max / mean = 4 / 3
    assert by[(4, 0)]["imbalance_max_over_mean"] == pytest.approx(4 / 3, rel=0.25)
    # tiles of one chunk dealt round-robin: every rank gets exactly one of the four background tiles
    assert by[(4, chunk)]["imbalance_max_over_mean"] == pytest.approx(1.0, abs=1e-3)
    assert by[(4, chunk)]["predicted_speedup"] > by[(4, 0)]["predicted_speedup"]
    for c in sim["configs"]:
        assert len(c["per_shard_ms"]) == c["world"] and c["predicted_ms"] >= c["max_ms"]
        wire = (c["world"] - 1) / c["world"] * n * 96 / (0.6 * 153e9 * (c["world"] - 1))
        assert c["exchange_model_ms"] == pytest.approx(1e3 * wire, abs=1e-3)
    assert set(sim["best_per_world"]) == {"2", "4"}


def test_single_ray_bisect_finds_the_ray():
    """bench.single_ray_bisect / grad_deviation (the follow-up of a strict miss of the train workload's gradient check): per-ray
    gradients whose mean is the batch gradient, one ray deviating -> that ray is found, the others agree."""
    import bench
    gen = torch.Generator().manual_seed(3)
    n = 128
    per_ray = {"renderModule.mlp.0.weight": torch.randn(n, 16, 10, generator=gen), "app_plane.0": torch.randn(n, 1, 4, 9, 9, generator=gen),
               "basis_mat.weight": torch.randn(n, 5, 12, generator=gen)}
    bad = {k: v.clone() for k, v in per_ray.items()}
    bad["renderModule.mlp.0.weight"][37] *= 1.6                      # one unit's share of one ray
    bad["app_plane.0"][37] += 0.3 * torch.randn(1, 4, 9, 9, generator=gen)
    calls = []

    def dev_of(idx):
        calls.append(int(idx.numel()))
        return bench.grad_deviation({k: v[idx].mean(0) for k, v in bad.items()}, {k: v[idx].mean(0) for k, v in per_ray.items()})
    full = dev_of(torch.arange(n))
    assert full["dense"] > 2e-3 and full["l2"] > 3e-3
    ray, alone, rest = bench.single_ray_bisect(n, dev_of)
    assert ray == 37
    assert alone["dense"] > 0.3 and rest["dense"] == 0.0 and rest["l2"] == 0.0 and rest["abs"] == 0.0
    assert sum(calls[1:]) == 2 * (n - 1) + (n - 1)                   # rays evaluated: every level's two halves + all rays but one
    assert bench.single_ray_bisect(1, dev_of)[0] == 0
