"""What TrainEngine queues, on which stream, behind which event -- recorded on the CPU and
checked against the row-index ring's hazard rules.  Host only: no GPU, no librae_hip.so.

The engine under test is the real one: an object made with ``TrainEngine.__new__`` whose
``run``, ``prefetch_index``, ``_index_ready``, ``_mark_built``, ``_queue_window``, ``_graph``,
``_dp_caps_check``, ``train_call`` ... are the methods of rae/engine.py, running over fakes of
what they call:

* ``FakeLib``: every ``rae_*`` entry returns 0 and is logged with its stream.  It models the
  device cursor, so a cursor-relative ``rae_step_forward(plan, i, st)`` resolves to its absolute
  batch, and the argument rules of the C entries that matter here (csrc/rae.hip launch_index,
  check_batch).  ``rae_check`` and ``rae_dp_list_max`` are blocking host reads (TrainEngine.check:
  "waits for all the device's queued work"), ``rae_check_on`` waits for its stream only.
* ``FakeCuda``: ``torch.cuda`` as the engine module sees it -- streams, events, the current
  stream, ``CUDAGraph`` and ``torch.cuda.graph``.  A capture records the calls made inside it;
  ``replay()`` issues them again on the current stream against the cursor at replay time, so the
  engine's own graph keys and ``_graphs.clear()`` run for real.
* ``FakeExchange``: ``barrier``, ``max_int``, ``rows`` and ``__call__`` as step-stream operations.

Happens-before.  Every device operation gets a number and the set (a Python int used as a bit
mask) of the operations that are certain to have finished before it starts: the earlier ones of
its stream, those an event or stream wait of its stream covered, and those the host had waited
for when it queued the operation.  Two operations are concurrent iff neither is in the other's
set.  Only one rank's own queue is modelled, not the peers' signals.

The rules, and where the project states them:

R1  A step-side operation reading batch r (forward, update, pack, unpack, rae_p2p_prologue; the
    pipelined form's forward / update also read batch r + 1 inside the epoch) is never concurrent
    with a rae_build_index writing slot r % ring.  (TrainEngine.prefetch_index docstring: steps
    queued after the point the build waits for "may read batches >= first_batch + count -
    index_window only"; include/rae.h rae_p2p_prologue: "the row index of a step's batch + 1
    must be built before the step runs".)
R2  For every such read the newest build of the slot that precedes the reader is a build of
    batch r itself under the negatives current when the step was queued.  (include/rae.h
    rae_build_index: "Batch b uses slot b % window"; TrainEngine._covered / _new_negatives.)
R3  One build's batches map to distinct slots.  (include/rae.h: "count <= rae_index_window()".)
R4  No two builds are concurrent (they share the plan's index scratch: TrainEngine.
    _drain_prefetch docstring) and no build is concurrent with a write of the negative buffers
    (the build "reads the negatives", same docstring; set_epoch_negatives,
    sample_epoch_negatives, train_call all call _new_negatives first).
R5  The forwards and the updates of a run are exactly its batches, once each, in order, inside
    the epoch, and after the run the engine's ``_cursor_at`` (when it claims to know) is where
    the device cursor is.  (TrainEngine.run docstring; the comment on ``_cursor_at``.)
R6  A graph captured before a rae_set_dp_buffers call is never replayed after it.
    (TrainEngine._dp_caps_check: "a resize drops the captured graphs, which hold the old
    buffers".)
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import types

import numpy as np
import pytest
import torch as real_torch

from rae import _lib
from rae import engine as engine_mod
from rae.engine import TrainEngine

FORMS = ("single", "partitioned", "p2p", "p2p_pipe")

Violation = collections.namedtuple("Violation", "rule text")


class Op:
    __slots__ = ("id", "kind", "stream", "reads", "need", "first", "count", "token", "pred",
                 "stale_graph", "run")

    def __init__(self, **kw):
        self.reads, self.need, self.first, self.count, self.token = (), None, 0, 0, None
        self.stale_graph, self.run = False, None
        for k, v in kw.items():
            setattr(self, k, v)

    def __repr__(self):
        what = f"[{self.first},{self.first + self.count})" if self.kind == "build" else \
            (f"({self.reads[0]})" if self.reads else "")
        return f"#{self.id} {self.kind}{what} on {self.stream}"


class Recorder:
    """The log and the happens-before state shared by the fakes."""

    def __init__(self, nb: int, ring: int, pipelined: bool):
        self.nb, self.ring, self.pipelined = nb, ring, pipelined
        self.ops = []
        self.host = 0                    # operations the host has waited for
        self.streams = {}
        self.default = FakeStream(self, name="step")
        self.current = [self.default]
        self.capture = None              # (graph, stream) while torch.cuda.graph is open
        self.cursor = None               # the device cursor (None: never set)
        self.moves = 0                   # rae_cursor_moves
        self.neg_content = 0             # bumped by every write of the epoch negative buffers
        self.neg_mode = None             # ("epoch",) or ("call", k): rae_set_negatives
        self.calls = 0
        self.dp_gen = 0                  # bumped by rae_set_dp_buffers
        self.built_since_read = []       # batches built since the last rae_dp_list_max
        self.run_id = None
        self.runs = []                   # [first, count, claimed cursor, device cursor]
        self.problems = []               # violations seen while recording
        self.host_log = []

    def launch(self, kind, stream, **info):
        op = Op(id=len(self.ops), kind=kind, stream=stream.name, run=self.run_id, **info)
        op.pred = stream.pred | self.host
        stream.pred = op.pred | (1 << op.id)
        self.ops.append(op)
        return op

    def sync_all(self):
        for s in self.streams.values():
            self.host |= s.pred

    def stream_of(self, st):
        sid = st.value if isinstance(st, C.c_void_p) else st
        return self.streams[int(sid)]


class FakeStream:
    def __init__(self, rec, device=None, priority=0, name=None):
        self.rec = rec
        self.cuda_stream = len(rec.streams) + 1      # never 0: c_void_p(0).value is None
        self.name = name or f"s{self.cuda_stream}"
        self.pred = 0
        self.gate = True                 # False: its waits are dropped (a planted fault)
        rec.streams[self.cuda_stream] = self

    @staticmethod
    def priority_range():
        return (0, -1)

    def wait_stream(self, other):
        if self.gate:
            self.pred |= other.pred

    def wait_event(self, ev):
        if self.gate:
            self.pred |= ev.pred

    def synchronize(self):
        self.rec.host |= self.pred


class FakeEvent:
    def __init__(self, rec, **kw):
        self.rec, self.pred = rec, 0

    def record(self, stream=None):
        stream = stream or self.rec.current[-1]
        self.pred = stream.pred | self.rec.host

    def synchronize(self):
        self.rec.host |= self.pred


class FakeGraph:
    def __init__(self, rec):
        self.rec, self.nodes, self.gen = rec, [], None

    def replay(self):
        rec = self.rec
        st = rec.current[-1]
        for name, args in self.nodes:
            if name.startswith("exchange."):
                rec.launch(name, st)
            else:
                rec.lib.execute(name, args, st, graph=self)

    def raw_cuda_graph_exec(self):
        return 0


class FakeCuda:
    """torch.cuda as rae/engine.py uses it."""

    def __init__(self, rec):
        self.rec = rec
        outer = self

        class Stream(FakeStream):
            def __init__(self, device=None, priority=0):
                super().__init__(outer.rec, device, priority)

        class Event(FakeEvent):
            def __init__(self, **kw):
                super().__init__(outer.rec, **kw)

        self.Stream, self.Event = Stream, Event
        self.CUDAGraph = lambda: FakeGraph(rec)

    def current_stream(self, device=None):
        return self.rec.current[-1]

    @contextlib.contextmanager
    def stream(self, s):
        self.rec.current.append(s)
        try:
            yield
        finally:
            self.rec.current.pop()

    @contextlib.contextmanager
    def graph(self, g, stream=None):
        rec = self.rec
        assert rec.capture is None, "nested capture"
        g.gen = rec.dp_gen
        rec.capture = (g, stream)
        rec.current.append(stream)
        try:
            yield
        finally:
            rec.current.pop()
            rec.capture = None

    def synchronize(self, device=None):
        self.rec.sync_all()


class FakeTorch:
    """The engine module's ``torch``: the real one with ``cuda`` replaced."""

    def __init__(self, cuda):
        self.cuda = cuda

    def __getattr__(self, name):
        return getattr(real_torch, name)


class FakeBuf:
    """A negative buffer: copy_ is a write on the current stream."""

    def __init__(self, rec, kind):
        self.rec, self.kind = rec, kind
        self.ptr = 0x1000                # only ever passed on to the fake library

    def data_ptr(self):
        return self.ptr

    def copy_(self, src):
        rec = self.rec
        rec.launch("neg_write" if self.kind == "epoch" else "call_write", rec.current[-1])
        if self.kind == "epoch":
            rec.neg_content += 1
        return self


class FakeCosts:
    """engine.costs: reading an element back is a blocking host read."""

    def __init__(self, rec):
        self.rec = rec

    def __getitem__(self, i):
        rec = self.rec
        return types.SimpleNamespace(item=lambda: (rec.sync_all(), 0.0)[1])


class FakeExchange:
    def __init__(self, rec):
        self.rec = rec

    def _op(self, name):
        rec = self.rec
        if rec.capture is not None and rec.current[-1] is rec.capture[1]:
            rec.capture[0].nodes.append((name, ()))
        else:
            rec.launch(name, rec.current[-1])

    def __call__(self, buf):
        self._op("exchange.records")

    def rows(self, send, recv):
        self._op("exchange.rows")

    def barrier(self):
        self.rec.host_log.append("exchange.barrier")

    def max_int(self, v):
        self.rec.host_log.append("exchange.max_int")
        return int(v)


_STEP_KIND = {"rae_step_forward": "forward", "rae_step_update": "update",
              "rae_dp_pack": "pack", "rae_dp_unpack": "unpack"}


class FakeLib:
    """librae_hip.so's entries as TrainEngine's training path calls them."""

    def __init__(self, rec, list_max=None):
        self.rec = rec
        rec.lib = self
        self.list_max = list_max or (lambda batches: (8, 8))
        self.error = b""

    # ---- plumbing
    def _fail(self, msg):
        self.error = msg.encode()
        return 2

    def rae_last_error(self):
        return self.error

    def _entry(self, name, args, st):
        """An ABI call: recorded when its stream is capturing, else executed."""
        rec = self.rec
        stream = rec.stream_of(st)
        rc = self._validate(name, args)
        if rc:
            return rc
        if name in ("rae_set_cursor", "rae_advance_cursor"):
            rec.moves += 1               # counted at the call, captured or not (csrc/rae.hip)
        if rec.capture is not None and stream is rec.capture[1]:
            rec.capture[0].nodes.append((name, args))
            return 0
        return self.execute(name, args, stream)

    def _validate(self, name, args):
        rec = self.rec
        if name == "rae_build_index":
            first, count = args
            if first < 0 or count < 0 or first + count > rec.nb:
                return self._fail("batch range out of the epoch")
            if count > rec.ring:
                return self._fail("more batches than the index window holds")
        elif name.endswith("_at") or name == "rae_p2p_prologue":
            if not 0 <= args[0] < rec.nb:
                return self._fail("batch index out of the epoch")
        return 0

    def execute(self, name, args, stream, graph=None):
        rec = self.rec
        if name == "rae_set_cursor":
            rec.cursor = args[0]
            op = rec.launch("set_cursor", stream)
        elif name == "rae_advance_cursor":
            if rec.cursor is None:
                rec.problems.append(Violation("R5", "rae_advance_cursor on a cursor never set"))
            else:
                rec.cursor += args[0]
            op = rec.launch("advance_cursor", stream)
        elif name == "rae_build_index":
            first, count = args
            if count == 0:
                return 0
            rec.built_since_read += range(first, first + count)
            op = rec.launch("build", stream, first=first, count=count,
                            token=self._build_token())
        elif name == "rae_p2p_prologue":
            op = rec.launch("prologue", stream, reads=(args[0],), need=("epoch", rec.neg_content))
        else:
            base = name[:-3] if name.endswith("_at") else name
            kind = _STEP_KIND[base]
            if name.endswith("_at"):
                b = args[0]
            elif rec.cursor is None:
                rec.problems.append(Violation("R5", f"{name} on a device cursor never set"))
                b = 0
            else:
                b = rec.cursor + args[0]
            if not 0 <= b < rec.nb:
                rec.problems.append(Violation("R5", f"{kind} of batch {b} outside the epoch's "
                                                    f"{rec.nb} batches"))
            reads = (b,)
            if rec.pipelined and kind in ("forward", "update") and b + 1 < rec.nb:
                reads = (b, b + 1)
            op = rec.launch(kind, stream, reads=reads, need=("epoch", rec.neg_content))
        if graph is not None and graph.gen != rec.dp_gen:
            op.stale_graph = True
        return 0

    def _build_token(self):
        rec = self.rec
        return ("epoch", rec.neg_content) if rec.neg_mode == ("epoch",) else rec.neg_mode

    # ---- the entries
    def rae_index_window(self, plan):
        return self.rec.ring

    def rae_cursor_moves(self, plan):
        return self.rec.moves

    def rae_set_cursor(self, plan, batch, st):
        return self._entry("rae_set_cursor", (int(batch),), st)

    def rae_advance_cursor(self, plan, count, st):
        return self._entry("rae_advance_cursor", (int(count),), st)

    def rae_build_index(self, plan, first, count, st):
        return self._entry("rae_build_index", (int(first), int(count)), st)

    def rae_p2p_prologue(self, plan, batch, drain, st):
        return self._entry("rae_p2p_prologue", (int(batch), int(drain)), st)

    def rae_set_negatives(self, plan, n1, n2, mode, stride):
        self.rec.neg_mode = ("epoch",) if mode == _lib.RAE_NEG_PER_EPOCH else ("call", -1)
        return 0

    def rae_train_step(self, plan, batch, n1, n2, st):
        rec = self.rec
        b = int(batch)
        if not 0 <= b < rec.nb:
            return self._fail("batch index out of range")
        stream = rec.stream_of(st)
        rec.calls += 1
        rec.neg_mode = ("call", rec.calls)           # rae_set_negatives(RAE_NEG_PER_CALL)
        rec.launch("build", stream, first=b, count=1, token=rec.neg_mode)
        rec.launch("forward", stream, reads=(b,), need=rec.neg_mode)
        rec.launch("update", stream, reads=(b,), need=rec.neg_mode)
        return 0

    def _neg_sample(self, st):
        rec = self.rec
        rec.launch("neg_write", rec.stream_of(st))
        rec.neg_content += 1
        return 0

    def rae_neg_sample(self, cum, n, u, count, out, st):
        return self._neg_sample(st)

    def rae_neg_sample_philox(self, cum, n, seed, off, count, out, st):
        return self._neg_sample(st)

    def rae_check(self, plan):
        self.rec.sync_all()
        return 0

    def rae_check_on(self, plan, st):
        self.rec.host |= self.rec.stream_of(st).pred
        return 0

    def rae_dp_list_max(self, plan, ma, mw):
        rec = self.rec
        rec.sync_all()
        a, w = self.list_max(rec.built_since_read)
        rec.built_since_read = []
        ma._obj.value, mw._obj.value = int(a), int(w)
        return 0

    def rae_set_dp_buffers(self, plan, send, recv, ca, cw):
        self.rec.dp_gen += 1
        return 0

    def rae_dp_block_floats(self, cfg, ca, cw):
        return 4

    def __getattr__(self, name):
        if name.startswith("rae_") and (name[4:9] == "step_" or name[4:7] == "dp_"):
            return lambda plan, x, st: self._entry(name, (int(x),), st)
        raise AttributeError(name)


class Scheduled:
    """A bare TrainEngine over the fakes.  Use inside ``patched()``."""

    def __init__(self, form: str, nb: int, index_window: int = 0, index_overlap: bool = True,
                 graph_chunk: int = 1, graph_absolute: bool = False, list_max=None):
        assert form in FORMS
        part = form != "single"
        # the plan's ring (csrc/rae_plan.hpp plan_resolve): clamped to the epoch
        ring = max(1, min(index_window if index_window > 0 else (256 if part else 2048), nb))
        self.rec = rec = Recorder(nb, ring, form == "p2p_pipe")
        self.cuda = FakeCuda(rec)
        self.torch = FakeTorch(self.cuda)
        self.lib = FakeLib(rec, list_max)
        self._ctor = (index_window, index_overlap, graph_chunk, graph_absolute, form, nb)
        self.eng = None

    @contextlib.contextmanager
    def patched(self):
        """The engine module over the fakes; everything is put back on exit."""
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(engine_mod, "torch", self.torch)
            mp.setattr(engine_mod, "_upload_graph", lambda g, s: None)
            mp.setattr(_lib, "_lib", self.lib)              # _lib.check reads rae_last_error
            yield self

    def make(self):
        """The fields __init__ sets for run(); the ring's window comes from the engine's own
        _set_index_schedule / resolve_index_schedule (a ValueError there refuses the config)."""
        index_window, index_overlap, graph_chunk, graph_absolute, form, nb = self._ctor
        rec = self.rec
        e = TrainEngine.__new__(TrainEngine)
        e.lib, e.plan, e.device = self.lib, C.c_void_p(1), real_torch.device("cpu")
        e.world_size = 1 if form == "single" else 2
        e.dp_rank = 0
        e.exchange = None if form == "single" else FakeExchange(rec)
        e.graph_chunk, e.graph_absolute = int(graph_chunk), bool(graph_absolute)
        e.s, e.l = 2, 4
        e.L = e.l * e.world_size
        e.nb = nb
        e.N = nb * e.L
        e._dp = form != "single"
        e._p2p = form in ("p2p", "p2p_pipe")
        e._pipe = form == "p2p_pipe"
        if e._pipe and int(index_window) == 1:              # as __init__ does, before the plan
            engine_mod.resolve_index_schedule(1, index_overlap, True, nb)
        e._p2p_next, e._p2p_valid = None, False
        e.cfg = _lib.RaeConfig()
        e.neg1, e.neg2 = FakeBuf(rec, "epoch"), FakeBuf(rec, "epoch")
        e.call_neg = [FakeBuf(rec, "call"), FakeBuf(rec, "call")]
        e.costs = FakeCosts(rec)
        e.exchange_buf = None
        e._dp_caps, e._dp_send, e._dp_recv = None, None, None
        e._stale = set()
        e._dp_cap_max = (1 << 20, 1 << 20)
        e.index_window = int(self.lib.rae_index_window(e.plan))
        e._graphs = {}
        e._epoch_mode = None
        e._cursor_at = None
        e._moves_seen = e._moves()
        e._set_index_schedule(index_overlap)
        e._cum_dev = real_torch.zeros(4, dtype=real_torch.float64)
        e.run = self.run
        self.eng = e
        return e

    # ---- drivers
    def new_negatives(self, sampled=False):
        e = self.eng
        if sampled:
            e.sample_epoch_negatives(None, "philox", seed=1, epoch=self.rec.neg_content)
        else:
            z = np.zeros((e.s, 1), dtype=np.int32)
            e.set_epoch_negatives(z, z)

    def run(self, first, count, *a, **kw):
        """TrainEngine.run, its operations tagged for R5 (make() puts it on the engine object,
        so callers that hold the engine alone, bench.warm_up, are recorded too)."""
        rec, e = self.rec, self.eng
        rec.run_id = len(rec.runs)
        try:
            TrainEngine.run(e, first, count, *a, **kw)
        finally:
            rec.run_id = None
        rec.runs.append((first, count, e._cursor_at, rec.cursor,
                         e._moves_seen == rec.moves))

    def train_call(self, b):
        e = self.eng
        z = np.zeros((e.s, e.l), dtype=np.int32)
        return e.train_call(b, z, z)

    def external_set_cursor(self, batch):
        """Someone else drives the plan's cursor through the ABI (not through the engine)."""
        e = self.eng
        assert self.lib.rae_set_cursor(e.plan, int(batch), e._stream()) == 0


def _first(rec, mask):
    """The earliest operation of a mask."""
    return rec.ops[(mask & -mask).bit_length() - 1]


def check(rec: Recorder):
    """Every violation of R1-R6 in the recorded schedule (an empty list: the schedule is safe)."""
    out = list(rec.problems)
    ring = rec.ring
    slot_builds = collections.defaultdict(int)      # slot -> mask of the builds writing it
    slot_readers = collections.defaultdict(int)     # slot -> mask of the operations reading it
    builds = negw = 0
    seen = set()

    def add(rule, text):
        if (rule, text) not in seen:
            seen.add((rule, text))
            out.append(Violation(rule, text))

    for op in rec.ops:
        bit = 1 << op.id
        if op.kind == "build":
            slots = {b % ring for b in range(op.first, op.first + op.count)}
            if len(slots) != op.count:
                add("R3", f"{op!r}: {op.count} batches share {len(slots)} slots of the ring of "
                          f"{ring}")
            other = builds & ~op.pred
            if other:
                add("R4", f"{op!r} beside {_first(rec, other)!r} (one index scratch)")
            other = negw & ~op.pred
            if other:
                add("R4", f"{op!r} beside {_first(rec, other)!r} (reads the negatives)")
            for s in slots:
                other = slot_readers[s] & ~op.pred
                if other:
                    add("R1", f"{op!r} beside {_first(rec, other)!r}, slot {s}")
                slot_builds[s] |= bit
            builds |= bit
        elif op.kind == "neg_write":
            other = builds & ~op.pred
            if other:
                add("R4", f"{op!r} beside {_first(rec, other)!r} (reads the negatives)")
            negw |= bit
        for r in op.reads:
            s = r % ring
            other = slot_builds[s] & ~op.pred
            if other:
                add("R1", f"{_first(rec, other)!r} beside {op!r}, slot {s}")
            before = slot_builds[s] & op.pred
            if not before:
                add("R2", f"{op!r} reads batch {r}: slot {s} was never built before it")
            else:
                b = rec.ops[before.bit_length() - 1]
                if not b.first <= r < b.first + b.count:
                    add("R2", f"{op!r} reads batch {r}: slot {s} holds {b!r}")
                elif b.token != op.need:
                    add("R2", f"{op!r} reads batch {r} built under negatives {b.token}, current "
                              f"{op.need}")
            slot_readers[s] |= bit
        if op.stale_graph:
            add("R6", f"{op!r} replayed from a graph captured before rae_set_dp_buffers")
    for i, (first, count, claimed, cursor, in_sync) in enumerate(rec.runs):
        want = list(range(first, first + count))
        for kind in ("forward", "update"):
            got = [o.reads[0] for o in rec.ops if o.run == i and o.kind == kind]
            if got != want:
                add("R5", f"run({first}, {count}): {kind}s of batches {got}")
        fw = [o for o in rec.ops if o.run == i and o.kind in ("forward", "update")]
        if any(a.kind == b.kind for a, b in zip(fw, fw[1:])) or (fw and fw[0].kind != "forward"):
            add("R5", f"run({first}, {count}): forwards and updates do not alternate")
        if any(not (b.pred >> a.id) & 1 for a, b in zip(fw, fw[1:])):
            add("R5", f"run({first}, {count}): steps not ordered one behind the other")
        if claimed is not None and in_sync and claimed != cursor:
            add("R5", f"run({first}, {count}): engine holds the cursor at {claimed}, the device "
                      f"at {cursor}")
    return out


def rules(violations):
    return sorted({v.rule for v in violations})
