"""G data-parallel ranks in one process, on one GPU and one stream.

The collective forms of the ranks' exchange are "the caller moves bytes between the step's
launches" (include/rae.h RAE_XCHG_COLLECTIVE; TrainEngine._steps_eager).  Between ranks that
live in one process the caller can move them with plain device copies: no process group, no
host staging, no process start per case.

  Loopback   the three movers over the ranks' buffers (CPU or device tensors; bitwise copies)
             with the semantics rae/dist.py documents -- gather (Exchange.__call__), rows
             (Exchange.rows), sync_rows (Exchange.sync_rows) -- and port(k), rank k's object with
             the interface of rae.dist.Exchange.  A port's collective completes when every rank
             has entered it, in rank order (one thread: ranks 0 .. G-2 leave their buffers, rank
             G-1 moves the bytes).  max_int answers with the bound the harness set and records
             what each rank asked with.
  Ranks      owns G ReconstructInducers / TrainEngines (rank 0 .. G-1, each with its own model
             and optimizer, so its own parameter and accumulator replicas; the factory returns
             either an inducer or a ready TrainEngine) and drives global
             batches for all of them in lockstep through the ABI's absolute-batch launches, in
             the order of TrainEngine._steps_eager.  The engines never call a collective from
             inside a step.

The peer-to-peer exchanges (dp_xchg p2p / p2p_pipe) are refused: their wait kernels spin for a
peer that runs concurrently, and ranks that share one stream never do.
"""
import torch


class Loopback:
    def __init__(self, G):
        if G < 2:
            raise ValueError("a loopback joins at least two ranks")
        self.G = int(G)
        self.bounds = None          # (entity rows, feature rows): what max_int answers
        self.maxima = []            # (rank, table 0 / 1, value) of every max_int call
        self._asked = [0] * self.G
        self._entered = {}          # collective -> the buffers of the ranks that have entered

    # ---------------------------------------------------------------- the movers
    def gather(self, bufs):
        """All-gather in place: slice [k n, (k+1) n) of rank k's buffer, n = numel / G, into the
        same slice of every peer's."""
        G = self.G
        n = bufs[0].numel() // G
        for k in range(G):
            src = bufs[k][k * n:(k + 1) * n]
            for j in range(G):
                if j != k:
                    bufs[j][k * n:(k + 1) * n].copy_(src)

    def rows(self, sends, recvs):
        """All-to-all of G equal blocks: block k of rank j's send buffer arrives as block j of
        rank k's receive buffer."""
        G = self.G
        blk = sends[0].numel() // G
        for j in range(G):
            for k in range(G):
                recvs[k][j * blk:(j + 1) * blk].copy_(sends[j][k * blk:(k + 1) * blk])

    def sync_rows(self, tensor_lists):
        """tensor_lists[k]: rank k's tensors, in the same order on every rank (None entries
        skipped).  Row x of every tensor is copied from rank x % G to all others."""
        G = self.G
        for ts in zip(*tensor_lists):
            if ts[0] is None:
                continue
            for x in range(G):
                for j in range(G):
                    if j != x:
                        ts[j][x::G] = ts[x][x::G]

    # ---------------------------------------------------------------- the ranks' side
    def port(self, rank):
        return _Port(self, rank)

    def _enter(self, what, rank, arg):
        have = self._entered.setdefault(what, [])
        if len(have) != rank:
            raise RuntimeError(f"loopback {what}: rank {rank} entered after {len(have)} ranks "
                               "(every rank enters a collective once, in rank order)")
        have.append(arg)
        if len(have) < self.G:
            return
        del self._entered[what]
        if what == "gather":
            self.gather(have)
        elif what == "rows":
            self.rows([a[0] for a in have], [a[1] for a in have])
        else:
            self.sync_rows(have)

    def _max_int(self, rank, v):
        if self.bounds is None:
            raise RuntimeError("loopback max_int before the harness set the capacities' bounds")
        table = self._asked[rank] % 2       # TrainEngine._dp_caps_check: entity rows, then features
        self._asked[rank] += 1
        self.maxima.append((rank, table, int(v)))
        return int(self.bounds[table])


class _Port:
    """Rank `rank`'s end of a Loopback: the interface of rae.dist.Exchange."""

    def __init__(self, hub, rank):
        self.hub, self.world_size, self.rank, self.group = hub, hub.G, int(rank), None

    def __call__(self, buf):
        self.hub._enter("gather", self.rank, buf)

    def rows(self, send, recv):
        self.hub._enter("rows", self.rank, (send, recv))

    def sync_rows(self, tensors):
        self.hub._enter("sync_rows", self.rank, list(tensors))

    def max_int(self, v):
        return self.hub._max_int(self.rank, v)

    def barrier(self):
        pass

    def all_gather_object(self, obj):
        raise RuntimeError("all_gather_object serves the peer-to-peer exchange's set-up, which "
                           "the loopback does not run")


def refuse_p2p(kernel_forms):
    xchg = (kernel_forms or {}).get("dp_xchg", "collective")
    if xchg != "collective":
        raise ValueError(f"dp_xchg={xchg!r}: the peer-to-peer wait kernels spin for a peer that "
                         "runs concurrently; ranks on one stream would hang")


class Ranks:
    """G ranks of one data-parallel plan.  make_inducer(rank, exchange) returns rank's
    ReconstructInducer (world_size = G, that rank and exchange, graph_chunk = 1,
    index_overlap = False: no side stream), not yet compiled; kernel_forms is what those
    inducers are given (looked at only to refuse a peer-to-peer exchange before any plan
    exists).  The factory may return a TrainEngine of the same description instead (a test that
    builds its model from device tensors): inds is then empty."""

    def __init__(self, G, make_inducer, kernel_forms=None):
        refuse_p2p(kernel_forms)
        self.G = int(G)
        self.lb = Loopback(G)
        made = [make_inducer(k, self.lb.port(k)) for k in range(self.G)]
        for x in made:
            refuse_p2p(x.kernel_forms)
        self.inds = [x for x in made if hasattr(x, "compile_function")]
        assert len(self.inds) in (0, self.G)
        for ind in self.inds:
            ind.compile_function()
        self.engines = [ind.engine for ind in self.inds] if self.inds else made
        e0 = self.engines[0]
        self.part = e0._dp
        assert all(e.world_size == self.G and e.dp_rank == k and e._dp == self.part and
                   not e._p2p and e._idx_stream is None for k, e in enumerate(self.engines))
        # the row lists' capacities: equal on all ranks, any value at or above the lists
        # (include/rae.h rae_set_dp_buffers) -- the worst case of one rank's l examples
        self.lb.bounds = (e0.l * (2 + 2 * e0.s), e0.index_dims()["RW"])
        self.nb = e0.nb

    def close(self):
        for ind in self.inds:
            ind._drop_engine()
        if not self.inds:
            for eng in self.engines:
                eng.close()

    def set_negatives(self, negs):
        """negs[k]: rank k's (neg1, neg2), each (s, N) -- the same arrays on every rank."""
        for eng, (n1, n2) in zip(self.engines, negs):
            eng.set_epoch_negatives(n1, n2)

    def _each(self, fn, b, what):
        from rae import _lib
        for eng in self.engines:
            _lib.check(getattr(eng.lib, fn)(eng.plan, int(b), eng._stream()), what)

    def step(self, b):
        """Global batch b on every rank, then the device error word of every plan."""
        engs = self.engines
        for eng in engs:
            eng.build_index(b, 1)
        if self.part:
            for rank, table, v in self.lb.maxima:
                assert v <= self.lb.bounds[table], (rank, table, v, self.lb.bounds)
            self._each("rae_dp_pack_at", b, "rae_dp_pack_at")
            self.lb.rows([e._dp_send for e in engs], [e._dp_recv for e in engs])
            self._each("rae_dp_unpack_at", b, "rae_dp_unpack_at")
        self._each("rae_step_forward_at", b, "rae_step_forward_at")
        self.lb.gather([e.exchange_buf for e in engs])
        self._each("rae_step_update_at", b, "rae_step_update_at")
        torch.cuda.synchronize()
        for eng in engs:
            eng.check()
            if self.part:
                eng._stale.update(("params", "acc"))

    def sync(self):
        """Partitioned update: every replica made whole (TrainEngine.sync_replicas on every
        rank; the last rank's call moves the rows)."""
        for eng in self.engines:
            eng.sync_replicas()
        assert not self.lb._entered

    def cost(self, rank, b):
        return float(self.engines[rank].costs[b].item())

    def forms(self):
        return [eng.kernel_forms_in_use() for eng in self.engines]
