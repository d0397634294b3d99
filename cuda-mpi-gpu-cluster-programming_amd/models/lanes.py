"""Stream lanes: the one place that says which stream waits for what when a model splits a batch.

A model with ``L`` lanes has L engines. :class:`Lanes` owns the HIP streams they run on (one per side lane
1..L-1, and lane 0's own stream, created by the first free run) and offers the two ways to run a batch:
:meth:`Lanes.run_joined` forks the side lanes from the current stream and joins them back within the call
(graph capturable), :meth:`Lanes.run_free` leaves every lane running on its own stream until
:meth:`Lanes.join`. The models supply only the per-lane work: ``AlexNetBlocks`` and ``AlexNetFull`` contain no
stream operation of their own, and ``tests/test_lanes_cpu.py`` pins the order of the operations below.
"""
from __future__ import annotations

import torch


def split(n: int, lanes: int, min_per_lane: int) -> list[int]:
    """Image boundaries [0, ..., n] of ``n`` images over ``lanes`` lanes: one lane below
    ``lanes * min_per_lane`` images, else contiguous near-equal slices."""
    if lanes <= 1 or n < lanes * min_per_lane:
        return [0, n]
    return [n * i // lanes for i in range(lanes + 1)]


def handover(st):
    """Record an event on ``st`` here; returns what a lane's ``run`` hands to :meth:`Lanes.run_free` to make the
    next lane's stream wait for this point."""
    ev = torch.cuda.Event()
    ev.record(st)
    return lambda s: s.wait_event(ev)


class Lanes:
    def __init__(self, device, lanes: int, min_per_lane: int, priority: int = 0):
        self.device, self.count, self.min_per_lane = device, lanes, min_per_lane
        # priority < 0: side lanes on high-priority streams (their waves dispatch first)
        self.side = [torch.cuda.Stream(device, priority=priority) for _ in range(lanes - 1)]
        self.own = None  # lane 0's stream in run_free (run_joined runs lane 0 on the current stream)

    def bounds(self, n: int) -> list[int]:
        """Image boundaries [0, ..., n] of the lanes both run modes put ``n`` images on."""
        return split(n, self.count, self.min_per_lane)

    def run_joined(self, n: int, run) -> None:
        """One batch of ``n`` images, forked from and joined back to the current stream: ``run(i, lo, hi)``
        enqueues images [lo, hi) on lane i's engine and the current stream. Side lanes first, each on its
        stream after that stream waits for the current one (inputs produced, outputs free there); then lane 0
        on the current stream, which finally waits for every side stream, so later work on it (reuse of the
        buffers included) follows all lanes. Too few images to split: ``run(0, 0, n)`` and nothing else."""
        bounds = self.bounds(n)
        if len(bounds) == 2:
            run(0, 0, n)
            return
        cur = torch.cuda.current_stream(self.device)
        for i, st in enumerate(self.side, start=1):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                run(i, bounds[i], bounds[i + 1])
        run(0, 0, bounds[1])
        for st in self.side:
            cur.wait_stream(st)

    def run_free(self, n: int, run, pre_lane=None, on_lane=None, prepare=None) -> None:
        """Throughput form for a loop of calls on the same buffers (``forward_async`` of both models).

        Each lane enqueues its slice on its own stream and is NOT joined back: consecutive calls
        pipeline instead of being realigned by a join every call. When every lane is idle (the first
        call, or after any device synchronisation) each lane's stream first waits for the current stream,
        and then for the point lane i-1 handed over, if it did: ``run(i, lo, hi, st, lead)`` enqueues images
        [lo, hi) on stream ``st``; ``lead`` (lanes idle, and a lane follows) asks it to publish its
        mid-forward point by returning a callable that makes a given stream wait for it (the lanes then run
        half a forward apart: one lane's transforms and pools under the other's GEMMs). Busy lanes get no
        waits and ``lead`` false. ``prepare(i, lo, hi)`` runs before lane i's waits (it may synchronise
        the device).

        Contract: the outputs hold a call's results once :meth:`join` has made the current stream wait
        for the lanes (or after a device synchronisation); inputs and outputs must not be written by
        other work until then. ``pre_lane(i, lo, hi)`` / ``on_lane(i, lo, hi)``, if given, run with
        lane i's stream current right before / after it enqueues images [lo, hi) (e.g. waiting for a
        collective still reading that output slice / a per-lane collective on it). Too few images to split:
        ``run(0, 0, n, None, False)`` on the current stream between the hooks, and no stream operation."""
        bounds = self.bounds(n)
        if len(bounds) == 2:
            if pre_lane is not None:
                pre_lane(0, 0, n)
            run(0, 0, n, None, False)
            if on_lane is not None:
                on_lane(0, 0, n)
            return
        if self.own is None:
            self.own = torch.cuda.Stream(self.device)
        streams = (self.own, *self.side)
        fresh = all(st.query() for st in streams)
        cur = torch.cuda.current_stream(self.device)
        handed = None
        for i, st in enumerate(streams):
            lo, hi = bounds[i], bounds[i + 1]
            if prepare is not None:
                prepare(i, lo, hi)
            if fresh:
                st.wait_stream(cur)
                if handed is not None:
                    handed(st)
            with torch.cuda.stream(st):
                if pre_lane is not None:
                    pre_lane(i, lo, hi)
                handed = run(i, lo, hi, st, fresh and i + 1 < self.count)
                if on_lane is not None:
                    on_lane(i, lo, hi)

    def join(self) -> None:
        """Make the current stream wait for every lane of :meth:`run_free`."""
        streams = ([self.own] if self.own is not None else []) + self.side
        if streams:
            cur = torch.cuda.current_stream(self.device)
            for st in streams:
                cur.wait_stream(st)
