"""The record-capacity protocol of every pass that records w > thres samples, host logic only.

The record count is only known on the device.  A pass sizes its buffers from the hint its previous call of the same problem size
left (`hinted`), bounds every kernel by the device-side count, sends the count to the host right behind the kernel that produces it
(`watch`) and reads it once, after everything has been queued (`settle`): an overflow drops the hint and the caller runs again.
Capturing a HIP graph, `watch` reads nothing and hands (counter, capacity, check key) to the graph's owner (graph.py, `check_site`).
What a pass does WITHOUT a hint is its own: the primary passes count exactly, the secondary march and the bake read back and `regrow`."""
from __future__ import annotations

import torch

from ._lib import TensoirHipError


class AsyncCount:
    """A device-side int32 counter on its way to the host: the copy into pinned memory and an event are queued NOW, on the
    current stream, right behind the kernel that produced the counter.  `get()` waits for that event only -- not for the
    launches queued afterwards -- so a capacity check at the end of a pass does not drain the launch queue (with
    `tensor.item()` it does: the GPU then idles while the host queues the next stage)."""

    def __init__(self, counter):
        self.pin = torch.empty(1, dtype=torch.int32, pin_memory=True)
        self.pin.copy_(counter.view(-1)[:1], non_blocking=True)
        self.ev = torch.cuda.Event()
        self.ev.record(torch.cuda.current_stream(counter.device))      # the counter's device, which need not be current
        self.value = None

    def get(self) -> int:
        if self.value is None:
            self.ev.synchronize()
            self.value = int(self.pin[0])
            self.pin = None
        return self.value


def learn_capacity(hints, key, total, growth, *, ceiling=None, decay=0.97, max_entries):
    """Record capacity for the next call of problem size `key`, learnt from this call's count `total`: growth x the count plus
    slack, never below 16 k rows, and decaying slowly from the previous hint (a heavy batch after a light one must not
    overflow); at most `ceiling` rows where the caller knows a bound.  `hints` is the caller's plain dict; it is emptied
    when it holds more than `max_entries` sizes."""
    if len(hints) > max_entries:
        hints.clear()
    cap = max(int(total * growth) + 4096, 1 << 14, int(decay * hints.get(key, 0)))
    hints[key] = cap if ceiling is None else min(cap, ceiling)


class PassCapacity:
    """One pass's view of its hint: `hints[key]` in the caller's plain dict, `learn` the site's learn_capacity parameters,
    `capture` the graph owner's check list while a HIP graph is captured (else None), `check_key` the pass's name in it,
    `count` the watched count on its way to the host (`count.get()` waits for its producer only; None while capturing)."""

    def __init__(self, hints, key, growth, *, capture=None, check_key=None, count_source=AsyncCount, **learn):
        self.hints, self.key, self.learn = hints, key, dict(growth=growth, **learn)
        self.capture, self.check_key, self.count_source = capture, check_key, count_source
        self.cap = self.count = None

    def hinted(self):
        """The capacity the previous call left, or None: the caller takes its own exact / first route (not while capturing)."""
        cap = self.hints.get(self.key)
        if cap is None and self.capture is not None:
            raise TensoirHipError(f"graph capture needs a warmed-up record-capacity hint for {self.check_key} (run one eager call first)")
        return cap

    def watch(self, counter, cap):
        """This attempt runs with `cap` rows, `counter` holds its count: queue the read HERE, behind the producer (capturing: register it)."""
        self.cap = cap
        if self.capture is not None:
            self.capture.append((counter, cap, self.check_key))
        else:
            self.count = self.count_source(counter)

    def settle(self, total=None):
        """The one end-of-pass rule.  total: a count the caller already holds (a route without `watch`), else the watched one.
        Overflow: the hint is dropped, nothing is learnt, False (run again).  Otherwise the hint is learnt, True."""
        total = self.count.get() if total is None else total
        if self.cap is not None and total > self.cap:
            self.hints.pop(self.key, None)
            return False
        learn_capacity(self.hints, self.key, total, **self.learn)
        return True

    @staticmethod
    def regrow(total):
        """Room for a march that is repeated at once after `total` records did not fit (eager secondary march, bake)."""
        return int(total * 1.25) + 1024


def check_site(model, check_key, total=0):
    """A graph check key -- ("primary", B, S) or ("secondary", n_rays) -> (the model's hint dict, the key in it, the capacity
    the next capture needs after a replay produced `total` records: never more than rays x samples for a primary pass)."""
    need = int(total * 1.25) + 4096
    if check_key[0] == "primary":
        return model._app_cap_hints, tuple(check_key[1:]), min(need, check_key[1] * check_key[2])
    return model._rec_cap_hints, check_key[1], need
