"""Skewed stream timing for tests: delays behind the forks and joins the product makes by hand, so that a missing wait, a
wait on the wrong event or a missing record_stream changes a number at test sizes - where a step is host-bound and runs
serially on the GPU whatever its events say.

    with Skew(monkeypatch, main, "side_late", delay_ms) as sk:
        ... the pass ...
    sk.count, sk.sites

patches torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream and torch.cuda.Event.record at class level (they are
Python methods of torch/cuda/streams.py) for the length of the block.  `main` is the stream the test treats as the main one.

  side_late     after any stream OTHER than main executes wait_event / wait_stream, a delay is enqueued on that stream: the
                forked work starts late, the forking stream runs ahead to its join.
  main_late     after Event.record on main, a delay is enqueued on main: the forked work runs ahead of the stream that forked it.
  count         no delay: the hooks only count what side_late (`.count`) and main_late (`.records`) would have delayed.
  replay_late   no hook delays; sk.replay_late(streams) enqueues one delay on each given stream, each behind the one before
                (they would otherwise run side by side and main would see only one of them): the backward nodes that autograd
                replays on those streams queue behind it.  Autograd's own cross-stream waits are C++ and are not hooked.

A delay is one torch.cuda._sleep: one thread, one block, bounded.  Its length comes from calibrate(), once per process.  A
Skew refuses to queue more than BUDGET_MS in all: what goes beyond is counted in `.refused` and the run's check fails.

Importing this module makes no HIP call."""
import collections
import os
import sys
import time

import torch

MIN_MS, MAX_MS = 2.0, 20.0      # the clamp of one delay
BUDGET_MS = 2000.0              # of one test, all its delays together
MODES = ("side_late", "main_late", "count", "replay_late")

_ORIG = {}                      # the unpatched methods, for the harness's own events and waits
_cycles_per_ms = None


def _orig(cls, name):
    """The method as torch defines it (also while a Skew is active)."""
    return _ORIG.get((cls, name)) or getattr(cls, name)


def calibrate() -> float:
    """torch.cuda._sleep cycles per millisecond, measured once: a sleep long enough (>= 5 ms) to hide its launch."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        record = _orig(torch.cuda.Event, "record")
        cycles = 1_000_000
        torch.cuda._sleep(cycles)       # (the first launch loads the kernel)
        for _ in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            record(a)
            torch.cuda._sleep(cycles)
            record(b)
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0:
                break
            cycles = int(cycles * min(100.0, 8.0 / max(ms, 1e-3)))
        assert ms >= 5.0, f"torch.cuda._sleep({cycles}) took {ms} ms: no calibration"
        _cycles_per_ms = cycles / ms
    return _cycles_per_ms


def sleep_on(stream, ms: float):
    """One bounded delay of `ms` on `stream`."""
    assert 0 < ms <= 1000.0, ms
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * calibrate()))


def shares_queue(stream, other, ms: float = 3.0) -> bool:
    """Does work on `stream` wait for work on `other` although no event says so?  A process has fewer hardware queues than it may
    have streams; two streams on one queue run one behind the other.  One short sleep on `other`, one empty launch on `stream`."""
    record = _orig(torch.cuda.Event, "record")
    torch.cuda.synchronize()
    sleep_on(other, ms)
    over, done = torch.cuda.Event(), torch.cuda.Event()
    record(over, other)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(1)
    record(done, stream)
    done.synchronize()
    waited = over.query()        # the sleep was over when the empty launch had finished: it ran behind it
    torch.cuda.synchronize()
    return waited


def draw_until_shared(other, tries: int = 40) -> int:
    """torch hands out its streams from a fixed pool in turn, and the runtime spreads that pool over the hardware queues in
    turn: draw streams until one shares `other`'s queue - the next few drawn (one fewer than there are queues) then do not.
    -> how many were drawn.  What this achieves is checked by the caller with shares_queue, not assumed."""
    for i in range(tries):
        if shares_queue(torch.cuda.Stream(), other):
            return i + 1
    return tries


def clamp_delay(wall_ms: float, n: int = 0, budget_ms: float = BUDGET_MS) -> float:
    """The delay for a pass of `wall_ms` with `n` places to delay: the pass's wall time within [MIN_MS, MAX_MS], and no more
    than what keeps n delays inside the budget (never below MIN_MS: a pass with more places than that has to shrink)."""
    d = min(max(wall_ms, MIN_MS), MAX_MS)
    if n:
        d = max(MIN_MS, min(d, 0.9 * budget_ms / n))
    return d


def _site() -> str:
    """file:line of the code that called the hooked method: the first frame outside this file and torch's streams.py."""
    f = sys._getframe(1)
    while f.f_back is not None and os.path.basename(f.f_code.co_filename) in ("stream_skew.py", "streams.py"):
        f = f.f_back
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno}"


class Skew:
    def __init__(self, monkeypatch, main, mode, delay_ms=MIN_MS, budget_ms=BUDGET_MS):
        assert mode in MODES, mode
        assert mode == "count" or MIN_MS <= delay_ms <= MAX_MS, delay_ms
        self._mp, self.main, self.mode, self.delay_ms, self.budget_ms = monkeypatch, main, mode, float(delay_ms), float(budget_ms)
        self.count = 0              # delays injected (mode count: waits on streams other than main)
        self.records = 0            # Event.record calls on main (what main_late delays)
        self.replays = 0            # mode count: the streams replay_late was given
        self.refused = 0            # delays not injected because the budget was spent
        self.queued_ms = 0.0
        self.sites = collections.Counter()      # "file:line" -> delays injected (or counted) there
        self.delayed = []           # the streams that got a delay, in order, each once
        self.streams = []           # every stream a hook saw, each once
        self._ctx = None

    # -- the delay ----------------------------------------------------------
    def _delay(self, stream, site):
        if self.queued_ms + self.delay_ms > self.budget_ms:
            self.refused += 1
            return
        sleep_on(stream, self.delay_ms)
        self.queued_ms += self.delay_ms
        self.count += 1
        self.sites[site] += 1
        if not any(s == stream for s in self.delayed):
            self.delayed.append(stream)

    def _saw(self, stream):
        if not any(s == stream for s in self.streams):
            self.streams.append(stream)

    def _after_wait(self, stream, site):
        self._saw(stream)
        if stream == self.main:
            return
        if self.mode == "side_late":
            self._delay(stream, site)
        elif self.mode == "count":
            self.count += 1
            self.sites[site] += 1

    def replay_late(self, streams):
        """One delay on each stream, the k-th behind the (k-1)-th.  (Mode count: counted only.)"""
        streams = list(streams)
        if self.mode == "count":
            self.replays += len(streams)
            return
        assert self.mode == "replay_late", self.mode
        record, wait = _orig(torch.cuda.Event, "record"), _orig(torch.cuda.Stream, "wait_event")
        prev = None
        for s in streams:
            if prev is not None:
                wait(s, prev)
            self._delay(s, "replay_late")
            prev = torch.cuda.Event()
            record(prev, s)

    def join_delayed(self):
        """main waits for every stream that got a delay (for a pass whose product code joins nobody - on purpose)."""
        record, wait = _orig(torch.cuda.Event, "record"), _orig(torch.cuda.Stream, "wait_event")
        for s in self.delayed:
            if s != self.main:
                ev = torch.cuda.Event()
                record(ev, s)
                wait(self.main, ev)

    # -- the hooks ----------------------------------------------------------
    def __enter__(self):
        sk = self
        for key in ((torch.cuda.Stream, "wait_event"), (torch.cuda.Stream, "wait_stream"), (torch.cuda.Event, "record")):
            _ORIG.setdefault(key, getattr(*key))
        wait_event, record = _ORIG[torch.cuda.Stream, "wait_event"], _ORIG[torch.cuda.Event, "record"]

        def hooked_wait_event(self, event):
            wait_event(self, event)
            sk._after_wait(self, _site())

        def hooked_wait_stream(self, stream):
            # (torch's own body, self.wait_event(stream.record_event()), with the caller's site: the record goes through the
            # hook below, the wait is delayed once)
            wait_event(self, stream.record_event())
            sk._after_wait(self, _site())

        def hooked_record(self, stream=None):
            if stream is None:
                stream = torch.cuda.current_stream()
            record(self, stream)
            sk._saw(stream)
            if stream == sk.main:
                sk.records += 1
                if sk.mode == "main_late":
                    sk._delay(stream, _site())

        self._ctx = self._mp.context()
        mp = self._ctx.__enter__()
        mp.setattr(torch.cuda.Stream, "wait_event", hooked_wait_event)
        mp.setattr(torch.cuda.Stream, "wait_stream", hooked_wait_stream)
        mp.setattr(torch.cuda.Event, "record", hooked_record)
        return self

    def __exit__(self, *exc):
        ctx, self._ctx = self._ctx, None
        return ctx.__exit__(*exc)

    def report(self) -> str:
        top = ", ".join(f"{k} x{v}" for k, v in self.sites.most_common(12))
        return f"{self.mode}: {self.count} delays of {self.delay_ms:.1f} ms ({self.refused} refused, {self.records} records on main) at {top}"


class Timed:
    """Elapsed time of a block on `stream` (events, through the unpatched record) and on the host, host-synchronised at both
    ends (sync: the device by default; a stream's own synchronize where the device must not be waited for): .gpu_ms, .wall_ms."""

    def __init__(self, stream=None, before_end=None, sync=None):
        self.stream, self.before_end, self.sync = stream, before_end, sync or torch.cuda.synchronize
        self.gpu_ms = self.wall_ms = None

    def __enter__(self):
        self.stream = torch.cuda.current_stream() if self.stream is None else self.stream
        self._a, self._b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.sync()
        self._t0 = time.perf_counter()
        _orig(torch.cuda.Event, "record")(self._a, self.stream)
        return self

    def __exit__(self, et, ev, tb):
        if et is None and self.before_end is not None:
            self.before_end()
        _orig(torch.cuda.Event, "record")(self._b, self.stream)
        self.sync()
        self.wall_ms = (time.perf_counter() - self._t0) * 1e3
        self.gpu_ms = self._a.elapsed_time(self._b)
        return False


def assert_skewed(sk: Skew, gpu_ms: float, ref_gpu_ms: float, what=""):
    """A skew that did not happen is a failure: the pass took at least the reference's time plus half of what was queued."""
    need = ref_gpu_ms + 0.5 * sk.count * sk.delay_ms
    print(f"{what}: {sk.report()}; on main {gpu_ms:.1f} ms, reference {ref_gpu_ms:.1f} ms, needed {need:.1f} ms")
    assert sk.refused == 0, f"{what}: {sk.refused} delays beyond the budget of {sk.budget_ms:.0f} ms ({sk.report()})"
    assert sk.count > 0, f"{what}: no delay was injected - the pass forked nothing ({sk.report()})"
    assert sk.queued_ms <= sk.budget_ms
    assert gpu_ms >= need, f"{what}: the skew did not take place: {gpu_ms:.1f} ms on main, needed {need:.1f} ms ({sk.report()})"
