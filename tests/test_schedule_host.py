"""TrainEngine's launch schedule against the index ring's hazard rules (tests/_schedule.py: the
real run() / prefetch_index / _index_ready / _queue_window / _graph over recording fakes, then a
happens-before check of rules R1-R6).  No GPU.

Every (ring, epoch length, graph form, overlap, data-parallel form, call pattern) either passes
R1-R6 or is refused with a ValueError when its schedule is resolved -- and only the pipelined
form on an explicit ring of one batch with more than one batch to run is refused.  A config
that fails later, inside rae_build_index ("more batches than the index window holds"), fails
the sweep."""
import collections
import inspect
import itertools

import pytest

import bench
from rae import engine as engine_mod
from rae.engine import TrainEngine, resolve_index_schedule
from _schedule import FORMS, Scheduled, check, rules

RINGS = (1, 2, 3, 4, 5, 6, 8, 9, 16, 0)          # 0: the plan's default, i.e. ring = nb here
NBS = (1, 2, 3, 7, 20, 45)
# (graph_chunk, graph_absolute, index_overlap, growing row lists): every graph_chunk with
# graph_absolute off and on (chunk 1 runs eagerly: graph_absolute changes nothing there), each
# graph_chunk with overlap on and off, growing lists (dp forms) with and without graphs and
# overlap.  Paired and not crossed, so that the file stays a test of seconds; no ring, epoch
# length, form or call pattern is left out.
PAIRED = ((1, False, True, False), (1, False, False, True),
          (2, False, True, False), (2, True, True, True), (2, True, False, False),
          (4, False, True, True), (4, False, False, False), (4, True, True, True))


def _grow(batches):
    """rae_dp_list_max maxima that outgrow _dp_caps_check's 4 % + 16 headroom every third batch:
    the row-exchange buffers are resized (and the graphs dropped) in the middle of a run."""
    m = 8 + 40 * (max(batches) // 3) if batches else 0
    return m, m


def _cuts(nb):
    return sorted({k for k in (nb // 2, nb - 1) if 0 < k < nb})


# ---- call patterns: each yields the drivers of one scenario (a callable over a Scheduled)
def p_one_run(nb):
    def go(h):
        h.new_negatives()
        h.run(0, nb)
    yield "", go


def p_split_run(nb):
    for k in _cuts(nb):
        def go(h, k=k):
            h.new_negatives()
            h.run(0, k)
            h.run(k, nb - k)
        yield f"cut {k}", go


def p_per_batch_eager(nb):
    def go(h):                                   # frequentEval mode 2 (inducer.learn)
        h.new_negatives()
        for b in range(nb):
            h.run(b, 1, graph=False)
    yield "", go


def p_two_epochs(nb):
    def go(h):
        h.new_negatives()
        h.run(0, nb)
        h.new_negatives(sampled=True)
        h.run(0, nb)
    yield "", go


def p_negatives_mid_epoch(nb):
    for k in _cuts(nb):
        def go(h, k=k):
            h.new_negatives()
            h.run(0, k)
            h.new_negatives(sampled=True)
            h.run(k, nb - k)
        yield f"cut {k}", go


def p_external_cursor(nb):
    for k in _cuts(nb):
        def go(h, k=k):
            h.new_negatives()
            h.run(0, k)
            h.external_set_cursor(0)
            h.run(k, nb - k)
        yield f"cut {k}", go


def p_train_call(nb):
    for k in _cuts(nb):
        for b in sorted({k - 1, k}):
            def go(h, k=k, b=b):
                h.new_negatives()
                h.run(0, k)
                h.train_call(b)
                h.run(k, nb - k)
            yield f"cut {k} call {b}", go


def _bench(h, W, K):
    """bench.py main()'s use of the engine around its timed region (its own warm_up and
    batch_spans; the lines between are pinned by test_bench_pattern_is_bench_py's)."""
    eng, nb = h.eng, h.eng.nb
    h.new_negatives(sampled=True)
    wrapped = K + W > nb
    look = max(0, min(eng._look, nb - W - K))
    prebuilt = not wrapped and W + K + look <= eng.index_window
    if prebuilt:
        eng.build_index(0, W + K + look)
        eng.check()
    if eng._dp:
        if not prebuilt:
            eng.build_index(0, min(eng.index_window, W + K, nb))
        if not eng._p2p:
            eng.exchange.rows(eng._dp_send, eng._dp_recv)
        h.cuda.synchronize()
    graphed = bench.warm_up(eng, W, K, prebuilt, eng.graph_chunk > 1)
    assert graphed == (eng.graph_chunk > 1)
    tspans = bench.batch_spans(W, K, nb)
    h.cuda.synchronize()
    npref = 0
    if prebuilt and eng.index_overlap and 2 * K <= eng.index_window and K >= bench.OVERLAP_MIN_STEPS:
        npref = max(0, min(K, nb - W - K))
    for i, (b, n) in enumerate(tspans):
        eng.run(b, n, index=not prebuilt, last_advance=i + 1 < len(tspans),
                prefetch=None if not prebuilt else npref > 0, sync_peers=False)
    h.cuda.synchronize()
    eng.check()
    eng.build_index(0, min(eng.index_window, nb))
    return npref


BENCH_LINES = (
    "look = max(0, min(eng._look, nb - W - K))",
    "prebuilt = not wrapped and W + K + look <= eng.index_window",
    "eng.build_index(0, W + K + look)",
    "eng.build_index(0, min(eng.index_window, W + K, nb))",
    "graphed = warm_up(eng, W, K, prebuilt, args.graph_chunk > 1)",
    "if prebuilt and eng.index_overlap and 2 * K <= eng.index_window and K >= OVERLAP_MIN_STEPS:",
    "npref = max(0, min(K, nb - W - K))",
    "eng.run(b, n, index=not prebuilt, last_advance=i + 1 < len(tspans),",
    "prefetch=None if not prebuilt else npref > 0, sync_peers=False)",
    "eng.build_index(0, nwin)",
)


def p_bench(nb):
    for W, K in sorted({(0, nb), (min(1, nb - 1), max(1, nb // 2)), (nb // 3 + 1, nb)}):
        yield f"W {W} K {K}", lambda h, W=W, K=K: _bench(h, W, K)


PATTERNS = {"one_run": p_one_run, "split_run": p_split_run, "per_batch_eager": p_per_batch_eager,
            "two_epochs": p_two_epochs, "negatives_mid_epoch": p_negatives_mid_epoch,
            "external_cursor": p_external_cursor, "train_call": p_train_call, "bench": p_bench}


def _scenario(form, nb, iw, overlap, chunk, absolute, go, grow=False):
    """(refused message or None, violations) of one scenario."""
    h = Scheduled(form, nb, index_window=iw, index_overlap=overlap, graph_chunk=chunk,
                  graph_absolute=absolute, list_max=_grow if grow else None)
    with h.patched():
        try:
            h.make()
        except ValueError as e:
            return str(e), []
        go(h)
        return None, check(h.rec)


def _matrix(form, pattern):
    """Every ring at every epoch length, times the paired factors of PAIRED."""
    for nb in NBS:
        for iw in sorted({min(r, nb) if r else 0 for r in RINGS}):
            if iw == nb:
                continue                         # the same ring as iw = 0, which is kept
            for chunk, absolute, overlap, grow in PAIRED:
                if pattern == "per_batch_eager" and chunk > 1:
                    continue                     # graph=False runs: the graph form is unused
                if pattern == "external_cursor" and absolute:
                    continue                     # absolute graphs never read the cursor
                yield nb, iw, overlap, chunk, absolute, grow and form != "single"


# train_call is the single-rank func['train'] path (it raises on more than one rank)
CASES = [(p, f) for p in PATTERNS for f in FORMS if p != "train_call" or f == "single"]


@pytest.mark.parametrize("pattern,form", CASES)
def test_every_schedule_keeps_the_ring_rules(pattern, form):
    bad, n, refused = [], 0, 0
    for nb, iw, overlap, chunk, absolute, grow in _matrix(form, pattern):
        family = f"index_window {iw} overlap {overlap}"
        for tag, go in PATTERNS[pattern](nb):
            n += 1
            name = (f"{form} nb {nb} {family} chunk {chunk} absolute {absolute} grow {grow} "
                    f"{tag}")
            try:
                msg, v = _scenario(form, nb, iw, overlap, chunk, absolute, go, grow)
            except Exception as e:               # e.g. RaeError out of rae_build_index
                bad.append((family, f"{name}: {type(e).__name__}: {e}"))
                continue
            # the one config refused: the pipelined form cannot keep its lookahead in one slot
            want_refused = form == "p2p_pipe" and iw == 1 and nb > 1
            if (msg is not None) != want_refused:
                bad.append((family, f"{name}: refused={msg!r}, expected {want_refused}"))
            elif msg is not None:
                refused += 1
                assert "lookahead" in msg
            elif v:
                bad.append((family, f"{name}: {rules(v)} first: {v[0].text}"))
    print(f"{pattern} / {form}: {n} schedules, {refused} refused, {len(bad)} bad")
    families = collections.Counter(f for f, _ in bad)
    first = {}
    for f, line in bad:
        first.setdefault(f, line)
    assert not bad, (f"{len(bad)} of {n} schedules, by family {dict(families)}; the first of "
                     f"each:\n" + "\n".join(first.values()))


@pytest.mark.parametrize("form", FORMS)
def test_bench_prefetch_beside_a_long_timed_region(form):
    """bench.py builds the next K batches' index beside its timed steps only from
    OVERLAP_MIN_STEPS steps on a ring of twice that: the default rings (2048, partitioned 256)."""
    W, K = 64, bench.OVERLAP_MIN_STEPS
    out = {}

    def go(h):
        out["npref"] = _bench(h, W, K)
    msg, v = _scenario(form, 700, 0, True, 64, False, go, grow=form != "single")
    assert msg is None and not v, v[:3]
    assert out["npref"] == K


def test_bench_pattern_is_bench_py():
    """_bench restates the engine calls of bench.py's main(); they are still what it does."""
    src = inspect.getsource(bench.main)
    for line in BENCH_LINES:
        assert line in src, line


# ---- the resolution itself
def test_overlap_leaves_room_for_the_window_its_lookahead_and_the_build():
    for ring, ov, pipe in itertools.product(range(1, 70), (True, False), (True, False)):
        if pipe and ring == 1:
            with pytest.raises(ValueError, match="lookahead"):
                resolve_index_schedule(ring, ov, pipe, 5)
            with pytest.raises(ValueError, match="lookahead"):
                resolve_index_schedule(ring, ov, pipe)
            assert resolve_index_schedule(ring, ov, pipe, 1) == (False, 1, 1)
            continue
        s = resolve_index_schedule(ring, ov, pipe, 100)
        assert s.lookahead == (1 if pipe else 0) and s.window >= 1
        assert s.window + s.lookahead <= ring
        if s.overlap:
            assert ov and 2 * s.window + s.lookahead <= ring
        else:
            assert s.window == ring - s.lookahead
        assert s.overlap == (ov and ring >= 2 + s.lookahead)
    assert resolve_index_schedule(2, True, True, 8) == (False, 1, 1)
    assert resolve_index_schedule(8, True, False) == (True, 4, 0)
    assert resolve_index_schedule(6, True, True) == (True, 2, 1)


# ---- planted faults: the checker sees each one
def _clean_then(form, nb, iw, go, plant, chunk=2, overlap=True, grow=False, absolute=False):
    """The scenario is clean as the engine stands; `plant(h, mp)` then breaks it."""
    msg, v = _scenario(form, nb, iw, overlap, chunk, absolute, go, grow)
    assert msg is None and not v, v[:3]
    h = Scheduled(form, nb, index_window=iw, index_overlap=overlap, graph_chunk=chunk,
                  graph_absolute=absolute, list_max=_grow if grow else None)
    with h.patched(), pytest.MonkeyPatch.context() as mp:
        plant(h, mp, before=True)
        h.make()
        plant(h, mp, before=False)
        try:
            go(h)
        except engine_mod._lib.RaeError as e:
            return ["refused by the library: " + str(e)], check(h.rec)
        return [], check(h.rec)


# odd pipelined rings are left out: there 2 * (window + 1) + 1 still fits the ring
@pytest.mark.parametrize("form,iw", [("single", 2), ("single", 3), ("single", 8), ("single", 16),
                                     ("partitioned", 4), ("p2p", 9), ("p2p_pipe", 4),
                                     ("p2p_pipe", 6), ("p2p_pipe", 8), ("p2p_pipe", 16)])
def test_fault_overlap_window_one_batch_too_long(form, iw):
    """R1 fires: the side build of the next window writes a slot the window in flight reads."""
    def plant(h, mp, before):
        if before:
            real = engine_mod.resolve_index_schedule

            def longer(*a, **k):
                s = real(*a, **k)
                return s._replace(window=s.window + 1) if s.overlap else s
            mp.setattr(engine_mod, "resolve_index_schedule", longer)
    _, v = _clean_then(form, 45, iw, next(p_one_run(45))[1], plant)
    assert "R1" in rules(v), v[:3]


@pytest.mark.parametrize("iw,chunk", [(2, 1), (4, 2), (8, 4), (16, 2)])
def test_fault_side_build_gate_dropped(iw, chunk):
    """R1 fires: without its gate the build of window w + 1 runs beside the steps of window
    w - 1, whose slots it writes.  (Single rank: the partitioned forms' blocking
    rae_dp_list_max read at every window happens to order the same pair.)"""
    def plant(h, mp, before):
        if not before:
            h.eng._idx_stream.gate = False
    _, v = _clean_then("single", 45, iw, next(p_one_run(45))[1], plant, chunk=chunk)
    assert "R1" in rules(v), v[:3]


@pytest.mark.parametrize("form", FORMS)
def test_fault_drain_prefetch_is_a_no_op(form):
    """R4 fires: new negatives are written while the side build that reads them is in flight."""
    def plant(h, mp, before):
        if before:
            mp.setattr(TrainEngine, "_drain_prefetch", lambda self: None)
    go = dict(p_negatives_mid_epoch(20))["cut 10"]
    _, v = _clean_then(form, 20, 8, go, plant)
    assert "R4" in rules(v), v[:3]


@pytest.mark.parametrize("form,overlap", [("single", True), ("single", False), ("p2p_pipe", True)])
def test_fault_covered_ignores_the_negatives_version(form, overlap):
    """R2 fires: with the whole epoch in the ring the second epoch's steps read the index built
    under the first epoch's negatives."""
    def plant(h, mp, before):
        if before:
            def covered(self, b, e):
                rd = self._ready
                return rd is not None and rd[0] <= b and e <= rd[1]
            mp.setattr(TrainEngine, "_covered", covered)
    _, v = _clean_then(form, 7, 0, next(p_two_epochs(7))[1], plant, overlap=overlap)
    assert "R2" in rules(v), v[:3]


@pytest.mark.parametrize("form", ["partitioned", "p2p", "p2p_pipe"])
def test_fault_resize_keeps_the_captured_graphs(form):
    """R6 fires: a graph holding the old row-exchange buffers is replayed after the resize."""
    def plant(h, mp, before):
        if before:
            real = TrainEngine._dp_caps_check

            def keeps(self):
                held = dict(self._graphs)
                real(self)
                self._graphs.update(held)
            mp.setattr(TrainEngine, "_dp_caps_check", keeps)
    _, v = _clean_then(form, 20, 4, next(p_one_run(20))[1], plant, grow=True)
    assert "R6" in rules(v), v[:3]


@pytest.mark.parametrize("form", ["single", "p2p_pipe"])
def test_fault_last_graph_bookkeeping_off_by_one(form):
    """R5 fires: after a run whose last graph does not advance the cursor, the engine believes
    the cursor one batch off; the next run then skips rae_set_cursor and steps wrong batches."""
    def plant(h, mp, before):
        if before:
            real = TrainEngine._queue_window

            def off(self, b, n, wi, replays, graph):
                real(self, b, n, wi, replays, graph)
                if self._cursor_at is not None and not replays[wi][-1][1]:
                    self._cursor_at += 1
            mp.setattr(TrainEngine, "_queue_window", off)

    def go(h):
        h.new_negatives()
        h.run(0, 9, last_advance=False)
        h.run(9, 5)
    _, v = _clean_then(form, 20, 8, go, plant)
    assert "R5" in rules(v), v[:3]
