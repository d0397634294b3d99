"""What each stream is made to wait for when a model splits a batch over lanes (:mod:`anx.models.lanes`), pinned
down without a GPU: ``torch.cuda`` as that module sees it is replaced by a recording stand-in, and every test
asserts the whole sequence of stream operations and callbacks, written out. A dropped or reordered wait usually
leaves the output bits of the GPU tests intact; it cannot pass here.

Log entries are ``(stream, op, argument)``: for a stream operation the stream it is enqueued on, for a callback
the stream that is current while it runs (``"cur"`` is the caller's stream). The stand-in numbers streams ``s1``,
``s2``, ... and events ``e1``, ... in creation order: the side lanes' streams come first (``Lanes`` creates them),
lane 0's own stream last (the first free run creates it)."""
import contextlib
import types

import pytest

from anx.models import lanes as lanes_mod
from anx.models.lanes import Lanes


class FakeStream:
    def __init__(self, cuda, name):
        self.cuda, self.name, self.idle = cuda, name, True

    def wait_stream(self, other):
        self.cuda.log.append((self.name, "wait_stream", other.name))

    def wait_event(self, ev):
        self.cuda.log.append((self.name, "wait_event", ev.name))

    def query(self):
        self.cuda.log.append((self.name, "query", None))
        return self.idle


class FakeEvent:
    def __init__(self, cuda, name):
        self.cuda, self.name = cuda, name

    def record(self, st):
        self.cuda.log.append((st.name, "record_event", self.name))


class FakeCuda:
    """The ``torch.cuda`` names lanes.py uses: Stream, current_stream, the stream(...) context, Event."""

    def __init__(self):
        self.log, self.streams, self.events = [], [], 0
        self.current = FakeStream(self, "cur")

    def Stream(self, device=None, priority=0):
        self.streams.append(FakeStream(self, f"s{len(self.streams) + 1}"))
        return self.streams[-1]

    def Event(self):
        self.events += 1
        return FakeEvent(self, f"e{self.events}")

    def current_stream(self, device=None):
        return self.current

    @contextlib.contextmanager
    def stream(self, st):
        prev, self.current = self.current, st
        try:
            yield
        finally:
            self.current = prev


@pytest.fixture
def cuda(monkeypatch):
    fake = FakeCuda()
    monkeypatch.setattr(lanes_mod, "torch", types.SimpleNamespace(cuda=fake))
    return fake


def joined_run(cuda):
    return lambda i, lo, hi: cuda.log.append((cuda.current.name, "run", (i, lo, hi)))


def free_args(cuda, handover="mark"):
    """run / pre_lane / on_lane / prepare that record themselves. A leading lane hands over a native-style mark
    (``"mark"``, as AlexNetFull), an event recorded on its stream (``"event"``, as staggered AlexNetBlocks) or
    nothing (``None``, as AlexNetBlocks without stagger)."""
    def hook(op):
        return lambda i, lo, hi: cuda.log.append((cuda.current.name, op, (i, lo, hi)))

    def run(i, lo, hi, st, lead):
        cuda.log.append((cuda.current.name, "run", (i, lo, hi, st and st.name, lead)))
        if lead and handover == "mark":
            return lambda s: cuda.log.append((s.name, "wait_mark", i))
        if lead and handover == "event":
            return lanes_mod.handover(st)

    return dict(run=run, pre_lane=hook("pre"), on_lane=hook("on"), prepare=hook("prepare"))


@pytest.mark.parametrize("L,n,min_per_lane,bounds,expected", [
    (2, 5, 1, [0, 2, 5], [
        ("s1", "wait_stream", "cur"), ("s1", "run", (1, 2, 5)),
        ("cur", "run", (0, 0, 2)),
        ("cur", "wait_stream", "s1")]),
    (3, 5, 1, [0, 1, 3, 5], [
        ("s1", "wait_stream", "cur"), ("s1", "run", (1, 1, 3)),
        ("s2", "wait_stream", "cur"), ("s2", "run", (2, 3, 5)),
        ("cur", "run", (0, 0, 1)),
        ("cur", "wait_stream", "s1"), ("cur", "wait_stream", "s2")]),
    (2, 48, 16, [0, 24, 48], [
        ("s1", "wait_stream", "cur"), ("s1", "run", (1, 24, 48)),
        ("cur", "run", (0, 0, 24)),
        ("cur", "wait_stream", "s1")]),
    (3, 48, 16, [0, 16, 32, 48], [
        ("s1", "wait_stream", "cur"), ("s1", "run", (1, 16, 32)),
        ("s2", "wait_stream", "cur"), ("s2", "run", (2, 32, 48)),
        ("cur", "run", (0, 0, 16)),
        ("cur", "wait_stream", "s1"), ("cur", "wait_stream", "s2")]),
])
def test_joined(cuda, L, n, min_per_lane, bounds, expected):
    """Fork, side lanes in order, lane 0 on the caller's stream, joins in stream order (the order graph capture
    relies on)."""
    ln = Lanes("dev", L, min_per_lane)
    assert ln.bounds(n) == bounds
    ln.run_joined(n, joined_run(cuda))
    assert cuda.log == expected
    assert ln.own is None  # the joined form never needs lane 0's own stream


@pytest.mark.parametrize("L,n,min_per_lane", [(2, 1, 1), (2, 31, 16), (1, 64, 16)])
def test_below_threshold_no_stream_operation(cuda, L, n, min_per_lane):
    ln = Lanes("dev", L, min_per_lane)
    assert ln.bounds(n) == [0, n]
    ln.run_joined(n, joined_run(cuda))
    assert cuda.log == [("cur", "run", (0, 0, n))]
    del cuda.log[:]
    ln.run_free(n, **free_args(cuda))
    assert cuda.log == [("cur", "pre", (0, 0, n)), ("cur", "run", (0, 0, n, None, False)), ("cur", "on", (0, 0, n))]
    assert ln.own is None and len(cuda.streams) == L - 1
    del cuda.log[:]
    ln.run_free(n, free_args(cuda)["run"])  # the hooks are optional
    assert cuda.log == [("cur", "run", (0, 0, n, None, False))]


def test_free_fresh_two_lanes(cuda):
    ln = Lanes("dev", 2, 1)
    ln.run_free(5, **free_args(cuda))
    assert cuda.log == [
        ("s2", "query", None), ("s1", "query", None),
        ("cur", "prepare", (0, 0, 2)),
        ("s2", "wait_stream", "cur"),
        ("s2", "pre", (0, 0, 2)), ("s2", "run", (0, 0, 2, "s2", True)), ("s2", "on", (0, 0, 2)),
        ("cur", "prepare", (1, 2, 5)),
        ("s1", "wait_stream", "cur"), ("s1", "wait_mark", 0),
        ("s1", "pre", (1, 2, 5)), ("s1", "run", (1, 2, 5, "s1", False)), ("s1", "on", (1, 2, 5))]


def test_free_fresh_three_lanes(cuda):
    ln = Lanes("dev", 3, 16)
    ln.run_free(48, **free_args(cuda))
    assert cuda.log == [
        ("s3", "query", None), ("s1", "query", None), ("s2", "query", None),
        ("cur", "prepare", (0, 0, 16)),
        ("s3", "wait_stream", "cur"),
        ("s3", "pre", (0, 0, 16)), ("s3", "run", (0, 0, 16, "s3", True)), ("s3", "on", (0, 0, 16)),
        ("cur", "prepare", (1, 16, 32)),
        ("s1", "wait_stream", "cur"), ("s1", "wait_mark", 0),
        ("s1", "pre", (1, 16, 32)), ("s1", "run", (1, 16, 32, "s1", True)), ("s1", "on", (1, 16, 32)),
        ("cur", "prepare", (2, 32, 48)),
        ("s2", "wait_stream", "cur"), ("s2", "wait_mark", 1),
        ("s2", "pre", (2, 32, 48)), ("s2", "run", (2, 32, 48, "s2", False)), ("s2", "on", (2, 32, 48))]


def test_free_fresh_event_handover_and_none(cuda):
    """The event form of the hand-over (staggered AlexNetBlocks), and a leading lane that hands nothing over
    (AlexNetBlocks without stagger): then the next lane waits for the caller's stream only."""
    ln = Lanes("dev", 2, 16)
    args = free_args(cuda, handover="event")
    ln.run_free(32, args["run"])
    assert cuda.log == [
        ("s2", "query", None), ("s1", "query", None),
        ("s2", "wait_stream", "cur"),
        ("s2", "run", (0, 0, 16, "s2", True)), ("s2", "record_event", "e1"),
        ("s1", "wait_stream", "cur"), ("s1", "wait_event", "e1"),
        ("s1", "run", (1, 16, 32, "s1", False))]
    del cuda.log[:]
    ln.run_free(32, free_args(cuda, handover=None)["run"])
    assert cuda.log == [
        ("s2", "query", None), ("s1", "query", None),
        ("s2", "wait_stream", "cur"), ("s2", "run", (0, 0, 16, "s2", True)),
        ("s1", "wait_stream", "cur"), ("s1", "run", (1, 16, 32, "s1", False))]


def test_free_busy_no_waits(cuda):
    """One lane still busy: the idle check (made once, before anything else) fails, so no wait of any kind is
    enqueued and no lane is asked to publish its mid-forward point."""
    ln = Lanes("dev", 3, 1)
    ln.side[1].idle = False
    ln.run_free(5, **free_args(cuda))
    assert cuda.log == [
        ("s3", "query", None), ("s1", "query", None), ("s2", "query", None),
        ("cur", "prepare", (0, 0, 1)),
        ("s3", "pre", (0, 0, 1)), ("s3", "run", (0, 0, 1, "s3", False)), ("s3", "on", (0, 0, 1)),
        ("cur", "prepare", (1, 1, 3)),
        ("s1", "pre", (1, 1, 3)), ("s1", "run", (1, 1, 3, "s1", False)), ("s1", "on", (1, 1, 3)),
        ("cur", "prepare", (2, 3, 5)),
        ("s2", "pre", (2, 3, 5)), ("s2", "run", (2, 3, 5, "s2", False)), ("s2", "on", (2, 3, 5))]


def test_own_stream_and_join(cuda):
    """Lane 0's own stream appears with the first free run and is reused; join() waits for it first once it
    exists, then for the side streams in order."""
    ln = Lanes("dev", 3, 1)
    ln.join()
    assert cuda.log == [("cur", "wait_stream", "s1"), ("cur", "wait_stream", "s2")]
    run = free_args(cuda)["run"]
    ln.run_free(5, run)
    own = ln.own
    assert own is cuda.streams[2] and len(cuda.streams) == 3
    ln.run_free(5, run)
    assert ln.own is own and len(cuda.streams) == 3
    del cuda.log[:]
    ln.join()
    assert cuda.log == [("cur", "wait_stream", "s3"), ("cur", "wait_stream", "s1"), ("cur", "wait_stream", "s2")]
    del cuda.log[:]
    Lanes("dev", 1, 16).join()  # one lane (any model on the CPU): nothing to wait for
    assert cuda.log == []
