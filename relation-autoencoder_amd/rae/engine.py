"""The device training step behind ``func['train']`` and ``func['label_<split>']``.

Owns the HBM-resident dataset arrays, the exchange and cost buffers, and the C-ABI plan
(include/rae.h).  Two ways to drive it:

* ``train_call(batch, neg1, neg2)`` -- exactly the reference's compiled function signature
  (learning/OieInduction.py:146-149,189): host negatives for one batch in, cost out.
* ``run(first_batch, count)`` -- many steps back to back on per-epoch negatives resident in
  HBM, captured into HIP graphs (torch.cuda.CUDAGraph) so a step costs two kernel launches
  and no host round trip; per-batch costs stay on the device until the epoch ends.

Data-parallel: each rank computes its l examples of every global batch of L = G*l
examples; ``exchange`` (dist.py) all-gathers the per-example records between the forward
and the update kernels, so every rank applies the identical update.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import socket

import numpy as np
import torch

from . import _lib
from .data import batch_nnz_stats


_hip = None

# TrainEngine.evaluate's result: cost = reconstruction + entropy (Python floats), the
# (nrows, 3) terms tensor (or None) and the three double column sums (S_pos, S_H, S_neg)
EvalResult = collections.namedtuple("EvalResult", "cost reconstruction entropy terms sums")
# TrainEngine.rank: mrr / mean_rank / logp are (side 1, side 2, combined), hits {k: such a tuple}
RankResult = collections.namedtuple(
    "RankResult", "mrr mean_rank hits logp nrows summary greater equal target lse")
# TrainEngine.cluster_metrics' result: B^3 f1 / precision / recall (Python floats), the number
# of clustered elements (int), the cluster sizes (numpy int64, relations) and the
# (relations, n_gold + 1) contingency table (numpy int64, or None when not asked for)
ClusterResult = collections.namedtuple("ClusterResult",
                                       "f1 precision recall n_elements sizes table")
# TrainEngine.cluster_profiles' result: per cluster the `top` most frequent keys and their counts,
# both (relations, top) numpy int32, padded with (-1, 0) (rae.evaluation.topk_from_table's order)
ProfileResult = collections.namedtuple("ProfileResult", "keys counts")
ExemplarResult = collections.namedtuple("ExemplarResult", "rows scores")


def _upload_graph(g, stream):
    """hipGraphUpload the instantiated graph now, so its first replay does not pay for
    putting the kernel packets on the device (a first replay is otherwise ~1-2 us per step
    slower at 20 steps).  Best effort: a runtime without it just uploads on first replay."""
    global _hip
    try:
        if _hip is None:
            _hip = C.CDLL("libamdhip64.so")
            _hip.hipGraphUpload.argtypes = [C.c_void_p, C.c_void_p]
            _hip.hipGraphUpload.restype = C.c_int
        ex = g.raw_cuda_graph_exec()
        if ex:
            _hip.hipGraphUpload(C.c_void_p(ex), C.c_void_p(stream.cuda_stream))
            stream.synchronize()
    except (OSError, AttributeError, RuntimeError):
        pass


def check_p2p_devices(identities, cross_device: bool):
    """The peer-to-peer exchange's device guard: ranks whose GPUs differ are
    refused unless cross_device -- the kernels' stores into a peer GPU's memory have run on
    ranks sharing one GPU only (rae_p2p.hpp "Visibility across GPUs")."""
    devs = sorted(set(identities))
    if len(devs) > 1 and not cross_device:
        raise ValueError(
            f"dp_xchg='p2p' across {len(devs)} GPUs: the peer-to-peer exchange is verified on "
            "ranks sharing one GPU only; pass p2p_cross_device=True to run it across GPUs (or "
            "use dp_xchg='collective', the default)")


IndexSchedule = collections.namedtuple("IndexSchedule", "overlap window lookahead")


def resolve_index_schedule(index_window: int, index_overlap: bool, pipelined: bool,
                           nb: int | None = None) -> IndexSchedule:
    """How run() walks a row-index ring of `index_window` batches (the plan's value,
    rae_index_window: already clamped to the epoch): IndexSchedule(overlap, window, lookahead).

    A window's steps read `window + lookahead` slots: their own batches and, pipelined
    peer-to-peer form, the row lists of the batch after the last one (every step pushes the
    NEXT batch's rows).  With overlap the side stream writes up to `window` further slots while
    those steps run, and a build must never write a slot a queued step reads (prefetch_index),
    so overlap needs  index_window >= 2 * window + lookahead  with window >= 1: a ring of 2
    batches, of 3 pipelined.  A smaller ring runs serial windows of index_window - lookahead
    batches, each built on the step stream right before its steps.

    Pipelined, a ring of one batch cannot hold a step's own batch beside the next one's lists:
    refused unless the epoch is that one batch (nb: the epoch's batches, None: not known)."""
    ring, look = int(index_window), 1 if pipelined else 0
    if ring < 1:
        raise ValueError(f"index_window must be at least 1, got {ring}")
    if look and ring < 2 and nb != 1:
        raise ValueError(
            "dp_xchg='p2p_pipe' needs an index_window of at least 2: every step reads the row "
            "lists of the batch after its own (a lookahead of one batch), so one slot cannot "
            "hold a step's index")
    overlap = bool(index_overlap) and ring >= 2 + look
    if overlap:
        # half the ring each for the window in flight and the build beside it; pipelined, the
        # window gives one slot to its lookahead batch (2 * window + 1 <= index_window)
        win = ring // 2 - look
    else:
        win = ring - look
    return IndexSchedule(overlap, max(1, win), look)


class DeviceSplit:
    """One split's CSR + entity ids in HBM (int32; values kept only if not all 1.0)."""

    def __init__(self, split, device):
        x = split.xFeats
        self.N = int(x.shape[0])
        self.d = int(x.shape[1])
        self.indptr_np = np.asarray(x.indptr, dtype=np.int64)
        if self.indptr_np[-1] >= 2 ** 31:
            raise ValueError("nnz exceeds int32 CSR addressing")
        self.indptr = torch.as_tensor(self.indptr_np.astype(np.int32), device=device)
        self.indices = torch.as_tensor(np.asarray(x.indices, dtype=np.int32), device=device)
        vals = np.asarray(x.data, dtype=np.float32)
        self.values = None if (vals.size == 0 or np.all(vals == 1.0)) else \
            torch.as_tensor(vals, device=device)
        self.args1 = torch.as_tensor(split.args1, device=device)
        self.args2 = torch.as_tensor(split.args2, device=device)


class TrainEngine:
    def __init__(self, model, optimizer, train_split, *, learning_rate, lambda1=0.0,
                 lambda2=0.0, world_size=1, rank=0, exchange=None, graph_chunk=64,
                 index_window=0, device=None, mfma_bf16=False, kernel_forms=None,
                 graph_absolute=False, dp_update="replicated", index_overlap=True,
                 p2p_cross_device=False, p2p_timeout=5.0):
        self.lib = _lib.load()
        self.model = model
        self.device = device if device is not None else model.params[0].device
        self.world_size = int(world_size)
        self.dp_rank = int(rank)     # data-parallel rank (rank() is the argument ranking)
        self.exchange = exchange
        self.graph_chunk = int(graph_chunk)
        dec = model.decoder
        self.m, self.r, self.s, self.l = model.m, model.r, model.s, model.l
        self.L = self.l * self.world_size
        self.split = train_split if isinstance(train_split, DeviceSplit) else \
            DeviceSplit(train_split, self.device)
        self.N = self.split.N
        self.nb = self.N // self.L                                     # OieInduction.py:98
        mbn, mrn = batch_nnz_stats(self.split.indptr_np, self.L)
        named = model.named_params()
        acc = {}
        if optimizer.accumulator is not None:
            acc = dict(zip(model.param_names, optimizer.accumulator))
        cfg = _lib.RaeConfig()
        cfg.decoder = _lib.RAE_DEC[dec.model_type]
        cfg.optimizer = _lib.RAE_OPT[optimizer.name]
        cfg.n_examples = self.N
        cfg.n_features = self.split.d
        cfg.n_entities = model.n
        cfg.relations = self.m
        cfg.embed = self.r
        cfg.neg_samples = self.s
        cfg.batch_size = self.l
        cfg.world_size = self.world_size
        cfg.rank = self.dp_rank
        cfg.learning_rate = float(learning_rate)
        cfg.alpha = float(model.alpha)
        cfg.lambda1 = float(lambda1)
        cfg.lambda2 = float(lambda2)
        cfg.ext_reg = 1 if model.extended_reg else 0
        cfg.max_batch_nnz = mbn
        cfg.max_row_nnz = mrn
        cfg.neg_mode = _lib.RAE_NEG_PER_EPOCH
        cfg.neg_stride = self.N
        cfg.index_window = int(index_window)
        cfg.mfma_bf16 = 1 if mfma_bf16 else 0
        # kernel forms (include/rae.h RAE_SPFWD_* ...): {"sp_forward": "split", ...}; the
        # plan picks for the shape when a form is not named
        self.kernel_forms = dict(kernel_forms or {})
        if dp_update not in _lib.KERNEL_FORMS["dp_update"]:
            raise ValueError(f"dp_update must be one of {sorted(_lib.KERNEL_FORMS['dp_update'])}")
        self.kernel_forms.setdefault("dp_update", dp_update)
        # partitioned update with peers: rows are pulled from their owners before each forward
        self._dp = self.kernel_forms["dp_update"] == "partitioned" and self.world_size > 1
        if self._dp and exchange is None:
            raise ValueError("the partitioned data-parallel update needs the ranks' Exchange")
        # peer-to-peer exchange (include/rae.h RAE_XCHG_P2P): the kernels store rows and
        # records straight into the peers' IPC-mapped buffers -- no collective inside a step
        xchg = self.kernel_forms.get("dp_xchg", "collective")
        self._p2p = xchg != "collective" and self.world_size > 1
        if xchg != "collective" and self.kernel_forms["dp_update"] != "partitioned":
            raise ValueError("the peer-to-peer exchange runs the partitioned update")
        # pipelined form (RAE_XCHG_P2P_PIPE): every step pushes the NEXT batch's rows, so a
        # step needs the row lists of its batch + 1 (run() builds one batch past each window)
        # and a run whose first batch the previous step did not push starts with
        # rae_p2p_prologue (_p2p_start)
        self._pipe = self._p2p and xchg == "p2p_pipe"
        if self._pipe and int(index_window) == 1:    # refused before any plan or peer exists
            resolve_index_schedule(1, index_overlap, True, self.nb)
        self._p2p_next = None        # batch the last queued step pushed rows for (signal out)
        self._p2p_valid = False      # ... pushed from the current negatives' lists
        self._ipc_bases = {}         # handle bytes -> this process's mapping of a peer allocation
        # ranks on different GPUs: the kernels' xGMI stores into a peer's memory (rae_p2p.hpp
        # "Visibility across GPUs") have run on ranks sharing one GPU only -- opt-in
        self._p2p_cross_device = bool(p2p_cross_device)
        self._p2p_timeout = float(p2p_timeout)
        for key, val in self.kernel_forms.items():
            if key not in _lib.KERNEL_FORMS or val not in _lib.KERNEL_FORMS[key]:
                raise ValueError(f"unknown kernel form {key}={val!r}")
            setattr(cfg, key, _lib.KERNEL_FORMS[key][val])
        self.cfg = cfg
        self.rec_floats = int(self.lib.rae_exchange_record_floats(C.byref(cfg)))
        self.exchange_buf = torch.zeros(int(self.lib.rae_exchange_floats(C.byref(cfg))),
                                        dtype=torch.float32, device=self.device)
        self.costs = torch.zeros(max(self.nb, 1), dtype=torch.float32, device=self.device)
        # per-epoch negatives live in fixed buffers (captured graphs keep their pointers)
        self.neg1 = torch.zeros((self.s, self.N), dtype=torch.int32, device=self.device)
        self.neg2 = torch.zeros((self.s, self.N), dtype=torch.int32, device=self.device)
        self.call_neg = torch.zeros((2, self.s, self.L), dtype=torch.int32, device=self.device)
        R3 = named.get("R", named.get("C"))
        bufs = _lib.RaeBuffers()
        p = _lib.ptr
        bufs.W, bufs.Wb, bufs.A, bufs.Ab = p(named["W"]), p(named["Wb"]), p(named["A"]), p(named["Ab"])
        bufs.C1, bufs.C2, bufs.R3 = p(named.get("C1")), p(named.get("C2")), p(R3)
        bufs.acc_W, bufs.acc_Wb = p(acc.get("W")), p(acc.get("Wb"))
        bufs.acc_A, bufs.acc_Ab = p(acc.get("A")), p(acc.get("Ab"))
        bufs.acc_C1, bufs.acc_C2 = p(acc.get("C1")), p(acc.get("C2"))
        bufs.acc_R3 = p(acc.get("R", acc.get("C")))
        bufs.indptr, bufs.indices = p(self.split.indptr), p(self.split.indices)
        bufs.values = p(self.split.values)
        bufs.args1, bufs.args2 = p(self.split.args1), p(self.split.args2)
        bufs.neg1, bufs.neg2 = p(self.neg1), p(self.neg2)
        bufs.exchange, bufs.costs = p(self.exchange_buf), p(self.costs)
        self._bufs = bufs
        self._keep = (named, acc, R3)
        self._named, self._acc = named, acc
        # row-exchange buffers of the partitioned update (sized from the row lists: _dp_caps)
        self._dp_caps = None
        self._dp_send = self._dp_recv = None
        self._stale = set()          # partitioned: {"params", "acc"} not gathered since a run
        self._dp_cap_max = (self.l * (2 + 2 * self.s), max(int(mbn), 1))   # rae.hip LA / LW
        handle = C.c_void_p()
        _lib.check(self.lib.rae_plan_create(C.byref(cfg), C.byref(bufs), C.byref(handle)),
                   "rae_plan_create")
        self.plan = handle
        if self._p2p:
            self._p2p_setup()
        self.index_window = int(self.lib.rae_index_window(self.plan))
        # a batch's row index is hash-partitioned (rae_index.hpp RAE_IDX_PART records per
        # partition) and a partition can overflow its LDS sort (a Zipf-heavy row at a large global
        # batch): run() checks the device error word after building each window's index, before
        # any step of the window applies an update (one host sync per window)
        self._graphs = {}
        self._epoch_mode = None
        # graph_absolute: every captured step carries its absolute batch index in the launch
        # (rae_step_*_at: no dependent device-cursor load at kernel start), one graph per
        # graph_chunk-step chunk of the epoch; otherwise one graph per chunk size, replayed
        # along the epoch by the device cursor
        self.graph_absolute = bool(graph_absolute)
        # batch the device cursor holds after this engine's last cursor-driven run (None:
        # unknown); run() skips its rae_set_cursor launch when the cursor already points at
        # the requested batch (consecutive runs of an epoch).  The plan counts every cursor
        # move made through the ABI (rae_cursor_moves): a move by anyone but this engine --
        # a direct rae_set_cursor / rae_advance_cursor on its plan -- changes the count, and
        # run() then sets the cursor again (cursor_moved() forces the same).
        self._cursor_at = None
        self._moves_seen = self._moves()
        self._set_index_schedule(index_overlap)

    def _set_index_schedule(self, index_overlap: bool):
        """index_overlap: run() builds the next window's row index on a lowest-priority side
        stream while the current window's steps run (the index is parameter independent; a
        batch's slot is batch % index_window).  Otherwise each window is built on the step
        stream right before its steps.  The window and the lookahead the ring allows:
        resolve_index_schedule."""
        self.index_overlap, self._win, self._look = resolve_index_schedule(
            self.index_window, index_overlap, self._pipe, self.nb)
        self._idx_stream = None
        if self.index_overlap:
            lo, _ = torch.cuda.Stream.priority_range()
            self._idx_stream = torch.cuda.Stream(self.device, priority=lo)
            # the runtime sets a stream's hardware queue up at its first use: 0.2-5.6 ms of
            # host time measured (tools/probes/bench_host_trace.py) -- here, not inside a run
            self._idx_stream.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self._idx_stream):
                torch.zeros(1, device=self.device).add_(1)
            self._idx_stream.synchronize()
        self._ready = None           # (lo, hi, negatives version, side-stream event): _mark_built
        self._neg_version = 0

    # ------------------------------------------------------------------ peer-to-peer exchange
    def _ipc_export(self, ptr: int):
        h = (C.c_char * _lib.RAE_IPC_HANDLE_BYTES)()
        off = C.c_int64()
        _lib.check(self.lib.rae_ipc_export(C.c_void_p(ptr), h, C.byref(off)), "rae_ipc_export")
        return bytes(h), int(off.value)

    def _ipc_map(self, handle: bytes, offset: int) -> int:
        base = self._ipc_bases.get(handle)
        if base is None:
            b = C.c_void_p()
            _lib.check(self.lib.rae_ipc_open(C.c_char_p(handle), C.byref(b)), "rae_ipc_open")
            base = self._ipc_bases[handle] = int(b.value)
        return base + offset

    def _device_identity(self):
        try:
            return str(torch.cuda.get_device_properties(self.device).uuid)
        except (AttributeError, RuntimeError):
            return f"{socket.gethostname()}:{self.device.index}"

    def _p2p_setup(self):
        """Trade IPC handles of this rank's exchange buffer, W, A, Ab and signal counters with
        every peer (a collective over the ranks' process group, once) and hand the peers'
        mappings to the plan (rae_set_peer).  Tensors sharing one allocation map it once.
        Ranks on different GPUs are refused unless p2p_cross_device=True (the
        cross-GPU stores have not run on hardware)."""
        named = self._named
        sig = self.lib.rae_p2p_signals(self.plan)
        mine = {"ex": self._ipc_export(self.exchange_buf.data_ptr()),
                "W": self._ipc_export(named["W"].data_ptr()),
                "A": self._ipc_export(named["A"].data_ptr()),
                "Ab": self._ipc_export(named["Ab"].data_ptr()),
                "sig": self._ipc_export(int(sig)),
                "dev": self._device_identity()}
        everyone = self.exchange.all_gather_object(mine)
        check_p2p_devices([e["dev"] for e in everyone], self._p2p_cross_device)
        _lib.check(self.lib.rae_set_p2p_timeout(self.plan, C.c_double(self._p2p_timeout)),
                   "rae_set_p2p_timeout")
        for p, e in enumerate(everyone):
            if p == self.dp_rank:
                continue
            ptr = {k: self._ipc_map(*e[k]) for k in ("ex", "W", "A", "Ab", "sig")}
            _lib.check(self.lib.rae_set_peer(self.plan, p, C.c_void_p(ptr["ex"]),
                                             C.c_void_p(ptr["W"]), C.c_void_p(ptr["A"]),
                                             C.c_void_p(ptr["Ab"]), C.c_void_p(ptr["sig"])),
                       "rae_set_peer")

    # ------------------------------------------------------------------ partitioned update
    def _dp_caps_check(self):
        """After a row-index build: the longest peer row list of the batches just built,
        agreed over the ranks; (re)size the all-to-all blocks when a list would not fit (a
        resize drops the captured graphs, which hold the old buffers)."""
        ma, mw = C.c_int32(), C.c_int32()
        _lib.check(self.lib.rae_dp_list_max(self.plan, C.byref(ma), C.byref(mw)), "rae_dp_list_max")
        need_a = self.exchange.max_int(ma.value)
        need_w = self.exchange.max_int(mw.value)
        ca, cw = self._dp_caps or (0, 0)
        if self._dp_caps is not None and need_a <= ca and need_w <= cw:
            return
        # headroom: the first window's longest list is already the tail of many batches, and
        # a longer one later only re-sizes (a one-off): every padded row travels every step
        ca = min(max(ca, int(need_a * 1.04) + 16), self._dp_cap_max[0])
        cw = min(max(cw, int(need_w * 1.04) + 16), self._dp_cap_max[1])
        if self._p2p:                # capacities only: rows go straight into the peers' replicas
            _lib.check(self.lib.rae_set_dp_buffers(self.plan, None, None, ca, cw),
                       "rae_set_dp_buffers")
        else:
            blk = int(self.lib.rae_dp_block_floats(C.byref(self.cfg), ca, cw))
            self._dp_send = torch.zeros(self.world_size * blk, dtype=torch.float32,
                                        device=self.device)
            self._dp_recv = torch.zeros_like(self._dp_send)
            _lib.check(self.lib.rae_set_dp_buffers(self.plan, C.c_void_p(self._dp_send.data_ptr()),
                                                   C.c_void_p(self._dp_recv.data_ptr()), ca, cw),
                       "rae_set_dp_buffers")
        self._dp_caps = (ca, cw)
        self._graphs.clear()

    def stale(self, accumulators: bool = True) -> bool:
        """Partitioned update: whether this rank's replica misses rows its peers own that
        changed since the last sync_replicas (parameters; with `accumulators`, their AdaGrad
        state too).  Always False for the replicated update."""
        if not self._dp:
            return False
        return "params" in self._stale or (accumulators and "acc" in self._stale)

    def sync_replicas(self, accumulators: bool = True):
        """Partitioned update: gather every A / Ab / W row (and AdaGrad accumulator) from its
        owner, so every rank holds the whole current model (labelling, checkpoints, tests).
        A COLLECTIVE when anything is stale: every rank must call it (ReconstructInducer.gather
        before a rank-0-only save).  No-op when nothing is stale, and for the replicated update
        (replicas are identical after every step)."""
        if not self.stale(accumulators):
            return
        torch.cuda.synchronize(self.device)
        ts = [self._named["W"], self._named["A"], self._named["Ab"]]
        self._stale.discard("params")
        if accumulators and self._acc:
            ts += [self._acc.get("W"), self._acc.get("A"), self._acc.get("Ab")]
            self._stale.discard("acc")
        self.exchange.sync_rows(ts)

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "plan", None):
            rd = getattr(self, "_ready", None)
            if rd is not None and rd[3] is not None:
                rd[3].synchronize()
            self._ready = None
            self._graphs.clear()
            self.lib.rae_plan_destroy(self.plan)
            self.plan = None
            for base in self._ipc_bases.values():
                self.lib.rae_ipc_close(C.c_void_p(base))
            self._ipc_bases = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kernel_forms_in_use(self):
        """The kernel forms the plan resolved for its shape (rae_plan_forms), named as
        _lib.KERNEL_FORMS names them -- so the dict can be fed back as
        TrainEngine(kernel_forms=...) / bench.py --kernel-form to pin the same run:
        sp_forward fused|split (SP), bil_dp strided|staged|mtile (bilinear), bil_prep
        auto|kernel (bf16 bilinear: the forward writes the R-gradient operands, or k_bil_prep
        does), dp_update replicated|partitioned, priv_rows on|off (rows one record of the
        batch references updated per example, or by the row tasks), dp_dense records|partials
        (data-parallel SP: dw1 / dw2 per example in the exchange, or each rank's reduced dense
        gradients), heavy_chunk off|on (rows with at least 256 records of the global batch
        summed as parallel 128-record chunks).  Keys of forms that do not apply to the plan are left out."""
        out = _lib.RaeConfig()
        _lib.check(self.lib.rae_plan_forms(self.plan, C.byref(out)), "rae_plan_forms")
        F = _lib.KERNEL_FORMS
        name = {key: {code: n for n, code in F[key].items()} for key in F}
        sp = self.cfg.decoder == 0
        res = {}
        if sp:
            res["sp_forward"] = name["sp_forward"][out.sp_forward]
        else:
            res["bil_dp"] = name["bil_dp"][out.bil_dp]
            if self.cfg.mfma_bf16:
                res["bil_prep"] = name["bil_prep"][out.bil_prep]
        res["dp_update"] = name["dp_update"][out.dp_update]
        res["priv_rows"] = name["priv_rows"][out.priv_rows]
        if sp and self.world_size > 1:
            res["dp_dense"] = name["dp_dense"][out.dp_dense]
        if self.world_size > 1:
            res["dp_xchg"] = name["dp_xchg"][out.dp_xchg]
        res["heavy_chunk"] = name["heavy_chunk"][out.heavy_chunk]
        return res

    def _moves(self):
        return int(self.lib.rae_cursor_moves(self.plan))

    def set_cursor(self, batch: int):
        """Point the device cursor at global batch `batch` (stream-ordered)."""
        _lib.check(self.lib.rae_set_cursor(self.plan, int(batch), self._stream()), "rae_set_cursor")
        self._cursor_at = int(batch)
        self._moves_seen = self._moves()

    def cursor_moved(self):
        """Tell the engine the device cursor was driven outside run() (direct rae_set_cursor /
        rae_step_* calls on its plan): the next run() sets it again."""
        self._cursor_at = None

    def check(self, stream=None):
        """Raise if the plan's device error word is set.  stream=None: a blocking read (waits
        for all the device's queued work); else a read ordered on that stream only."""
        if stream is None:
            _lib.check(self.lib.rae_check(self.plan), "rae_check")
        else:
            _lib.check(self.lib.rae_check_on(self.plan, C.c_void_p(stream.cuda_stream)),
                       "rae_check_on")

    # ------------------------------------------------------------------ func['train']
    def train_call(self, batch_index, neg1, neg2) -> float:
        """One ``func['train'](batch_index, neg1, neg2)`` call (OieInduction.py:146-149):
        neg1/neg2 are (s, l) int32 host arrays; returns the batch cost as a Python float."""
        if self.world_size != 1:
            raise RuntimeError("train_call is the single-rank func['train'] path")
        n1 = np.ascontiguousarray(neg1, dtype=np.int32)
        n2 = np.ascontiguousarray(neg2, dtype=np.int32)
        if n1.shape != (self.s, self.l) or n2.shape != (self.s, self.l):
            raise ValueError(f"neg arrays must be ({self.s}, {self.l}), got {n1.shape}, {n2.shape}")
        b = int(batch_index)
        if not 0 <= b < self.nb:
            raise IndexError(f"batch index {b} out of range [0, {self.nb})")
        self._cl_labels_of = None        # labels of the old parameters are not reused
        self._new_negatives()            # its index slot is rebuilt with the call's negatives
        self.call_neg[0].copy_(torch.from_numpy(n1))
        self.call_neg[1].copy_(torch.from_numpy(n2))
        st = self._stream()
        _lib.check(self.lib.rae_train_step(self.plan, b, C.c_void_p(self.call_neg[0].data_ptr()),
                                           C.c_void_p(self.call_neg[1].data_ptr()), st),
                   "rae_train_step")
        self._epoch_mode = None
        cost = float(self.costs[b].item())
        self.check()
        return cost

    # ------------------------------------------------------------------ epoch path
    def set_epoch_negatives(self, neg1, neg2):
        """(s, N) negatives of one epoch (OieInduction.py:183-184), host or device."""
        self._new_negatives()
        self.neg1.copy_(torch.as_tensor(np.asarray(neg1, dtype=np.int32)) if not
                        torch.is_tensor(neg1) else neg1)
        self.neg2.copy_(torch.as_tensor(np.asarray(neg2, dtype=np.int32)) if not
                        torch.is_tensor(neg2) else neg2)
        self._ensure_epoch_mode()

    def sample_epoch_negatives(self, sampler, mode: str = "device", seed: int = 0,
                               epoch: int = 0):
        """Fill the (s, N) per-epoch negative buffers on the device.
        mode "device": the shared RandomState draws neg1's then neg2's uniforms exactly as
          the reference does (OieInduction.py:183-184), the CDF search runs in HBM
          (rae_neg_sample) -- bit-identical to the host sampler, ~50x faster;
        mode "philox": uniforms generated on the device (rae_neg_sample_philox, counter =
          (epoch, buffer, draw)) -- no host work at all, not the reference's stream."""
        count = self.N * self.s
        self._new_negatives()
        if getattr(self, "_cum_dev", None) is None:
            self._cum_dev = torch.as_tensor(np.asarray(sampler.cum, dtype=np.float64),
                                            device=self.device)
        cum = C.c_void_p(self._cum_dev.data_ptr())
        n = int(self._cum_dev.numel())
        st = self._stream()
        for which, buf in enumerate((self.neg1, self.neg2)):
            if mode == "philox":
                off = (2 * int(epoch) + which) * count
                _lib.check(self.lib.rae_neg_sample_philox(cum, n, int(seed), off, count,
                                                          C.c_void_p(buf.data_ptr()), st),
                           "rae_neg_sample_philox")
            else:
                u = torch.from_numpy(sampler.draw_uniforms(count))
                if getattr(self, "_u_dev", None) is None or self._u_dev.numel() != count:
                    self._u_dev = torch.empty(count, dtype=torch.float64, device=self.device)
                self._u_dev.copy_(u)
                _lib.check(self.lib.rae_neg_sample(cum, n, C.c_void_p(self._u_dev.data_ptr()), count,
                                                   C.c_void_p(buf.data_ptr()), st), "rae_neg_sample")
        self._ensure_epoch_mode()

    def _ensure_epoch_mode(self):
        if self._epoch_mode is not True:
            _lib.check(self.lib.rae_set_negatives(self.plan, C.c_void_p(self.neg1.data_ptr()),
                                                  C.c_void_p(self.neg2.data_ptr()),
                                                  _lib.RAE_NEG_PER_EPOCH, self.N),
                       "rae_set_negatives")
            self._epoch_mode = True

    def _steps_eager(self, count, st, first=None, advance=True):
        """count steps from the device cursor (which then advances past them unless
        advance=False: a run's last graph, whose successor sets the cursor anyway), or (first
        given) at absolute batches first, first+1, ... (the cursor is not touched: every
        cursor-driven run sets it first)."""
        for i in range(count):
            if self._dp and not self._p2p:   # pull the rows this step's examples read
                if first is None:
                    _lib.check(self.lib.rae_dp_pack(self.plan, i, st), "rae_dp_pack")
                else:
                    _lib.check(self.lib.rae_dp_pack_at(self.plan, first + i, st), "rae_dp_pack_at")
                self.exchange.rows(self._dp_send, self._dp_recv)
                if first is None:
                    _lib.check(self.lib.rae_dp_unpack(self.plan, i, st), "rae_dp_unpack")
                else:
                    _lib.check(self.lib.rae_dp_unpack_at(self.plan, first + i, st),
                               "rae_dp_unpack_at")
            if first is None:
                _lib.check(self.lib.rae_step_forward(self.plan, i, st), "rae_step_forward")
            else:
                _lib.check(self.lib.rae_step_forward_at(self.plan, first + i, st),
                           "rae_step_forward_at")
            if self.exchange is not None and not self._p2p:
                self.exchange(self.exchange_buf)
            if first is None:
                _lib.check(self.lib.rae_step_update(self.plan, i, st), "rae_step_update")
            else:
                _lib.check(self.lib.rae_step_update_at(self.plan, first + i, st),
                           "rae_step_update_at")
        if first is None and advance:
            _lib.check(self.lib.rae_advance_cursor(self.plan, count, st), "rae_advance_cursor")

    def _graph(self, count, first=None, advance=True):
        key = (count if advance else ("last", count)) if first is None else (int(first), count)
        g = self._graphs.get(key)
        if g is None:
            # the capture calls rae_advance_cursor once (recorded, not run): not a real move
            in_sync = self._moves_seen == self._moves()
            g = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.graph(g, stream=s):
                self._steps_eager(count, self._stream(), first, advance)
            torch.cuda.current_stream(self.device).wait_stream(s)
            _upload_graph(g, s)
            self._graphs[key] = g
            if in_sync:
                self._moves_seen = self._moves()
        return g

    def _chunks(self, first_batch: int, count: int):
        """(first batch, steps) of every graph run() replays for these batches."""
        out = []
        for b, n in self.windows(first_batch, count):
            full, rem = divmod(n, self.graph_chunk)
            out += [(b + k * self.graph_chunk, self.graph_chunk) for k in range(full)]
            if rem:
                out.append((b + full * self.graph_chunk, rem))
        return out

    def _cursor_replays(self, first_batch: int, count: int, last_advance: bool = True):
        """Per window of run(first_batch, count): [(steps, advance), ...] of its cursor-driven
        graph replays.  last_advance=False: the run's very last graph does not advance the cursor
        (one node less; for a run no cursor-driven run follows directly -- run() records where
        the cursor stays, and the next run sets it)."""
        wins = self.windows(first_batch, count)
        out = []
        for wi, (_, n) in enumerate(wins):
            full, rem = divmod(n, self.graph_chunk)
            reps = [(self.graph_chunk, True)] * full + ([(rem, True)] if rem else [])
            if not last_advance and wi == len(wins) - 1 and reps:
                reps[-1] = (reps[-1][0], False)
            out.append(reps)
        return out

    def capture(self, count: int | None = None):
        """Capture the HIP graph of ``count`` steps (default: graph_chunk) without running it."""
        self._ensure_epoch_mode()
        self._graph(int(count or self.graph_chunk))

    def windows(self, first_batch: int, count: int):
        """The index windows run() walks: [(first batch, batches), ...] (resolve_index_schedule:
        half the ring each with index_overlap, less the pipelined form's lookahead slot)."""
        out, b, end = [], int(first_batch), int(first_batch) + int(count)
        while b < end:
            n = min(self._win, end - b)
            out.append((b, n))
            b += n
        return out

    def graph_sizes(self, first_batch: int, count: int):
        """Step counts of the graphs run() replays for these batches: graph_chunk-step
        graphs, plus one graph for each window's remainder (so no step runs eagerly)."""
        if self.graph_chunk <= 1:
            return []
        sizes = []
        for _, n in self.windows(first_batch, count):
            full, rem = divmod(n, self.graph_chunk)
            sizes += [self.graph_chunk] * full + ([rem] if rem else [])
        return sizes

    def capture_for(self, first_batch: int, count: int, last_advance: bool = True):
        """Capture (without running) every graph run(first_batch, count, last_advance=...)
        will replay, so no capture lands inside a timed region."""
        self._ensure_epoch_mode()
        if self.graph_chunk <= 1:
            return
        if self.graph_absolute:
            for b, n in self._chunks(first_batch, count):
                self._graph(n, b)
            return
        for reps in self._cursor_replays(first_batch, count, last_advance):
            for n, adv in reps:
                self._graph(n, advance=adv)

    def build_index(self, first_batch: int, count: int):
        """Row index of batches [first_batch, first_batch+count) (one window at most)."""
        self._drain_prefetch()
        _lib.check(self.lib.rae_build_index(self.plan, int(first_batch), int(count), self._stream()),
                   "rae_build_index")
        self._mark_built(int(first_batch), int(first_batch) + int(count))
        if self._dp:
            self._dp_caps_check()

    def index_dims(self):
        """The row index's dimensions as the plan resolved them (rae_index_dims)."""
        v = (C.c_int64 * len(_lib.INDEX_DIMS))()
        _lib.check(self.lib.rae_index_dims(self.plan, v, len(_lib.INDEX_DIMS)), "rae_index_dims")
        return dict(zip(_lib.INDEX_DIMS, (int(x) for x in v)))

    def index_region(self, batch: int, region: str):
        """One region of `batch`'s index slot as a host int32 array (rae_index_read; waits for
        the device).  A read-back for tests and diagnosis: no step path calls it."""
        d = self.index_dims()
        H = _lib.RAE_IDX_HMAX
        shape = {"srecA": (d["RA"],), "srecW": (d["RW"],), "segA": (d["RA"], 4),
                 "segW": (d["RW"], 4), "countA": (H,), "countW": (H,), "pclsA": (H, 4),
                 "pclsW": (H, 4), "thdr": (4,), "task": (d["TC"], 4), "vtask": (d["NVC"], 4),
                 "hfin": (d["HF"], 4), "desc": (d["dnx"], d["dstride"]), "pmask": (d["L"], 4),
                 "dpl": (2, d["G"], d["LA"] + d["LW"]), "dpc": (2, d["G"], 2),
                 "dpmax": (2,)}[region]
        out = np.empty(shape, dtype=np.int32)
        _lib.check(self.lib.rae_index_read(self.plan, int(batch), _lib.INDEX_REGIONS[region],
                                           out.ctypes.data_as(C.c_void_p), out.nbytes),
                   "rae_index_read")
        return out

    def run(self, first_batch: int, count: int, graph: bool = True, index: bool = True,
            last_advance: bool = True, prefetch: bool | None = None, sync_peers: bool = True):
        """Run ``count`` consecutive global batches starting at ``first_batch`` on the epoch
        negatives; costs land in self.costs[first_batch:first_batch+count].  The row index
        of each window of batches is ready before the window's steps (index=False: the caller
        built it already, e.g. bench.py ahead of its timed region).  With index_overlap and
        prefetch (default: index), the index of the batches after each window -- the run's
        next window, or as many batches as the window after the run's last -- is built on the
        side stream, queued in front of the window's steps so it runs beside them.  With
        graph, every step runs inside a replayed HIP graph: graph_chunk-step graphs and one
        graph per window remainder (last_advance: see _cursor_replays).  sync_peers (the
        peer-to-peer exchange only): a host barrier of the ranks first -- a caller that has
        just met its peers (bench.py's timed region) may skip it."""
        self._ensure_epoch_mode()
        self._cl_labels_of = None        # labels of the old parameters are not reused
        if self._dp:
            self._stale.update(("params", "acc"))
        if self._p2p and sync_peers:
            # a peer may have spent any time in host code since its last step (per-batch
            # evaluation, checkpoints): meet here so no wait kernel of this run starts its
            # bounded spin (rae_set_p2p_timeout) while a peer is still away
            self.exchange.barrier()
        pre = (index if prefetch is None else prefetch) and self.index_overlap
        replays = self._cursor_replays(first_batch, count, last_advance)
        wins = self.windows(first_batch, count)
        for wi, (b, n) in enumerate(wins):
            if index:
                self._index_ready(b, min(n + self._look, self.nb - b))
            if wi == 0 and self._pipe:
                self._p2p_start(b)
            nn_ = 0
            if pre:
                nn_ = wins[wi + 1][1] if wi + 1 < len(wins) else min(n, self.nb - (b + n))
            gate = None
            if nn_ > 0:
                # the next window's build may start once everything queued BEFORE this
                # window's steps is done (the previous window's steps read the slots it
                # writes); it is queued AFTER this window's replays, so its host calls never
                # stand between the GPU and the steps (66 vs 34 us of host queue
                # in front of a 20-step timed region)
                gate = torch.cuda.Event()
                gate.record(torch.cuda.current_stream(self.device))
            self._queue_window(b, n, wi, replays, graph)
            if gate is not None:
                self.prefetch_index(b + n, min(nn_ + self._look, self.nb - (b + n)), after=gate)
        if self._pipe and count > 0:
            # the run's last step pushed (and signalled) the rows of the batch after it
            self._p2p_next, self._p2p_valid = first_batch + count, True

    def _p2p_start(self, b: int):
        """Pipelined p2p: unless the previous step already pushed batch b's rows (from the
        current negatives' lists), push them now -- after consuming that step's signal for
        another batch (every rank runs the same batches, so every rank decides alike)."""
        if self._p2p_valid and self._p2p_next == b:
            return
        _lib.check(self.lib.rae_p2p_prologue(self.plan, int(b), 1 if self._p2p_next is not None else 0,
                                             self._stream()), "rae_p2p_prologue")

    def _queue_window(self, b, n, wi, replays, graph):
        """Queue the steps of window [b, b+n) (graph replays or eager launches)."""
        if graph and self.graph_chunk > 1 and self.graph_absolute:
            for cb, cn in self._chunks(b, n):
                self._graph(cn, cb).replay()
            return
        if self._cursor_at != b or self._moves_seen != self._moves():
            self.set_cursor(b)
        self._cursor_at = None              # until the window's launches are queued
        if not graph or self.graph_chunk <= 1:
            self._steps_eager(n, self._stream())
            self._cursor_at = b + n
        else:
            reps = replays[wi]
            for cnt, adv in reps:
                self._graph(cnt, advance=adv).replay()
            self._cursor_at = b + n - (0 if reps[-1][1] else reps[-1][0])
        self._moves_seen = self._moves()

    # ------------------------------------------------------------------ index overlap
    # self._ready = (lo, hi, negatives version, event): batches [lo, hi) have their row index
    # in the ring; event (or None) marks the end of a side-stream build not yet waited for.
    def _mark_built(self, x: int, y: int, event=None):
        lo, hi, ver, ev = self._ready if self._ready else (x, x, self._neg_version, None)
        if ver != self._neg_version or x != hi:      # not contiguous: a new range
            lo, ev = x, None
        self._ready = (max(lo, y - self.index_window), y, self._neg_version, event or ev)

    def _covered(self, b: int, e: int) -> bool:
        rd = self._ready
        return rd is not None and rd[2] == self._neg_version and rd[0] <= b and e <= rd[1]

    def prefetch_index(self, first_batch: int, count: int, after=None):
        """Start the row index of batches [first_batch, first_batch+count) -- the part not
        already built -- on the side stream, behind everything queued on the step stream so
        far (or, `after` given, behind that event of the step stream), in front of whatever is
        queued after.  Steps queued after the point it waits for may read batches
        >= first_batch + count - index_window only (run()'s windows satisfy that, the
        pipelined form's lookahead batch counted in: resolve_index_schedule)."""
        if not self.index_overlap:
            raise RuntimeError("prefetch_index needs index_overlap")
        x, y = int(first_batch), int(first_batch) + int(count)
        rd = self._ready
        if rd is not None and rd[2] == self._neg_version and rd[0] <= x <= rd[1]:
            x = max(x, rd[1])                        # extend the built range
        if y <= x:
            return
        if after is None:
            self._idx_stream.wait_stream(torch.cuda.current_stream(self.device))
        else:
            self._idx_stream.wait_event(after)
        _lib.check(self.lib.rae_build_index(self.plan, x, y - x,
                                            C.c_void_p(self._idx_stream.cuda_stream)),
                   "rae_build_index")
        done = torch.cuda.Event()
        done.record(self._idx_stream)
        self._mark_built(x, y, done)

    def _index_ready(self, b: int, n: int):
        """The window [b, b+n)'s index before its steps: already in the ring (a side-stream
        build the step stream then waits for), else built on the step stream; then the
        overflow check (host sync) and, partitioned, the row-list capacities.  The check of a
        side-stream build reads the error word on the side stream: the host waits for that
        build only, not for the steps still queued on the step stream (a blocking
        null-stream read there left a GPU bubble at every window boundary)."""
        if self._covered(b, b + n):
            ev = self._ready[3]
            if ev is not None:
                torch.cuda.current_stream(self.device).wait_event(ev)
                self._ready = self._ready[:3] + (None,)
                self.check(self._idx_stream)
            else:
                self.check()
        else:
            self._drain_prefetch()
            _lib.check(self.lib.rae_build_index(self.plan, b, n, self._stream()),
                       "rae_build_index")
            self._mark_built(b, b + n)
            self.check()
        if self._dp:
            self._dp_caps_check()

    def _drain_prefetch(self):
        """A side-stream build still in flight: the step stream waits for it (it uses the
        plan's index scratch and reads the negatives)."""
        if self._ready is not None and self._ready[3] is not None:
            torch.cuda.current_stream(self.device).wait_event(self._ready[3])
            self._ready = self._ready[:3] + (None,)

    def _new_negatives(self):
        self._drain_prefetch()
        self._neg_version += 1
        self._p2p_valid = False      # rows pushed from the old lists: push the next run's again

    # ------------------------------------------------------------------ labelling
    def label(self, split: DeviceSplit, row0: int, nrows: int, probs: bool = True):
        """labels (int64) and probs (fp32) of rows [row0, row0+nrows) of a split with the
        current W/Wb (RelationClassifier.py:39-48).  Partitioned update with stale rows: the
        W rows are gathered from their owners first -- a collective, so every rank labels (or
        ReconstructInducer.gather() ran on every rank before a single rank labels)."""
        if self.stale(accumulators=False):   # partitioned update: gather W from its owners
            self.sync_replicas(accumulators=False)
        lab = torch.empty(nrows, dtype=torch.int64, device=self.device)
        pr = torch.empty((nrows, self.m), dtype=torch.float32, device=self.device) if probs else None
        W, Wb = self.model.params[0], self.model.params[1]
        _lib.check(self.lib.rae_label(
            C.c_void_p(split.indptr.data_ptr()), C.c_void_p(split.indices.data_ptr()),
            C.c_void_p(split.values.data_ptr()) if split.values is not None else None,
            C.c_void_p(W.data_ptr()), C.c_void_p(Wb.data_ptr()), self.m, int(row0), int(nrows),
            C.c_void_p(lab.data_ptr()), C.c_void_p(pr.data_ptr()) if pr is not None else None,
            self._stream()), "rae_label")
        return lab, pr

    # ------------------------------------------------------------------ held-out objective
    EVAL_SEED = 0x5EEDE7A1           # Philox key of the evaluation negatives (not the model's RNG)

    def eval_negatives(self, split: DeviceSplit, sampler=None, seed: int | None = None):
        """Two (s, N_split) int32 device arrays of negatives for scoring `split`, drawn over
        negSamplingCum with rae_neg_sample_philox at a fixed key (neg1 at counter offset 0, neg2
        at s * N_split) and cached per split: every epoch scores against the same negatives.
        Never touches the model's RandomState (only sampler.cum is read)."""
        seed = self.EVAL_SEED if seed is None else int(seed)
        cache = self.__dict__.setdefault("_eval_negs", {})
        hit = cache.get(id(split))
        if hit is not None and hit[0] is split and hit[1] == seed:
            return hit[2], hit[3]
        sampler = sampler if sampler is not None else getattr(self, "eval_sampler", None)
        if getattr(self, "_cum_dev", None) is None:
            if sampler is None:
                raise ValueError("eval_negatives needs a sampler (its negSamplingCum)")
            self._cum_dev = torch.as_tensor(np.asarray(sampler.cum, dtype=np.float64),
                                            device=self.device)
        count = self.s * split.N
        out = []
        for which in range(2):
            buf = torch.empty((self.s, split.N), dtype=torch.int32, device=self.device)
            if count:
                _lib.check(self.lib.rae_neg_sample_philox(
                    C.c_void_p(self._cum_dev.data_ptr()), int(self._cum_dev.numel()), seed,
                    which * count, count, C.c_void_p(buf.data_ptr()), self._stream()),
                    "rae_neg_sample_philox")
            out.append(buf)
        cache[id(split)] = (split, seed, out[0], out[1])
        return out[0], out[1]

    def _eval_neg_arg(self, neg):
        if torch.is_tensor(neg):
            t = neg.to(device=self.device, dtype=torch.int32)
        else:
            t = torch.as_tensor(np.ascontiguousarray(neg, dtype=np.int32), device=self.device)
        t = t.contiguous()
        if t.dim() != 2 or t.shape[0] != self.s:
            raise ValueError(f"negatives must be ({self.s}, columns), got {tuple(t.shape)}")
        return t

    def evaluate(self, split: DeviceSplit, row0: int = 0, nrows: int | None = None, neg1=None,
                 neg2=None, seed: int | None = None, terms: bool = False,
                 neg_per_call: bool = False):
        """The forward-only objective (rae_eval_cost) of rows [row0, row0+nrows) of `split` at
        the current parameters: EvalResult(cost, reconstruction, entropy, terms, sums) with
        cost = reconstruction + entropy = -(S_pos + S_neg)/D - 2 S_H/D, D = nrows (4 + 2s) --
        the data term func['train'] returns, without the L1 / L2 regularisers; Python floats
        from the double sums.  terms=True: also the (nrows, 3) fp32 tensor (pos, H, neg).
        neg1 / neg2: (s, >= row0+nrows) arrays whose column is the row within the split
        (default: eval_negatives(split)); neg_per_call: (s, nrows) arrays whose column is the
        example within the range (func['train']'s convention).  Touches no parameter,
        accumulator, plan state, cursor, row index, training negative or prefetch, and not the
        model's RNG.  Partitioned update with stale rows: gathers the parameters first (a
        collective, like label)."""
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        row0 = int(row0)
        nrows = split.N - row0 if nrows is None else int(nrows)
        if row0 < 0 or nrows < 0 or row0 + nrows > split.N:
            raise IndexError(f"rows [{row0}, {row0 + nrows}) out of the split's {split.N}")
        if (neg1 is None) != (neg2 is None):
            raise ValueError("give both neg1 and neg2 or neither")
        if neg1 is None:
            n1, n2 = self.eval_negatives(split, seed=seed)
        else:
            n1, n2 = self._eval_neg_arg(neg1), self._eval_neg_arg(neg2)
        if n1.shape != n2.shape:
            raise ValueError("neg1 and neg2 differ in shape")
        shift = row0 if neg_per_call else 0     # the range as rows [0, nrows) of a shifted view
        if n1.shape[1] < row0 - shift + nrows:
            raise ValueError(f"negatives have {n1.shape[1]} columns, rows need "
                             f"{row0 - shift + nrows}")
        out = torch.empty((nrows, 3), dtype=torch.float32, device=self.device) if terms else None
        self.queue_evaluate(split, row0 - shift, nrows, n1, n2, out, shift)
        sp_, sh_, sn_ = (float(x) for x in self._eval_sums.cpu().numpy())
        D = float(nrows * (4 + 2 * self.s))
        rec = -(sp_ + sn_) / D if nrows else 0.0
        ent = -2.0 * sh_ / D if nrows else 0.0
        return EvalResult(rec + ent, rec, ent, out, (sp_, sh_, sn_))

    def _eval_args(self, split: DeviceSplit | None, row0: int = 0, nrows: int = 0,
                   shift: int = 0):
        """rae_eval_args of the plan-free evaluation entries: the engine's shapes and parameters,
        and rows [row0, row0+nrows) of `split` viewed from row `shift` on (None: no rows).
        Negatives, outputs and the workspace are the caller's to add."""
        named = self._named
        R3 = named.get("R", named.get("C"))
        a = _lib.RaeEvalArgs()
        a.decoder = self.cfg.decoder
        a.relations, a.embed = self.m, self.r
        a.n_entities = self.cfg.n_entities
        a.alpha = self.cfg.alpha
        p = _lib.ptr
        a.W, a.Wb, a.A, a.Ab = p(named["W"]), p(named["Wb"]), p(named["A"]), p(named["Ab"])
        a.C1, a.C2, a.R3 = p(named.get("C1")), p(named.get("C2")), p(R3)
        if split is not None:
            a.indptr = split.indptr.data_ptr() + 4 * shift
            a.indices, a.values = p(split.indices), p(split.values)
            a.args1 = split.args1.data_ptr() + 4 * shift
            a.args2 = split.args2.data_ptr() + 4 * shift
        a.row0, a.nrows = int(row0), int(nrows)
        return a

    def _workspace(self, a, attr: str, what: str, size):
        """Point a's workspace at the device buffer self.<attr>, allocated once per engine with
        the bytes the sizing call size() asks for (`what` names it in the error)."""
        if getattr(self, attr, None) is None:
            need = int(size())
            if need < 0:
                _lib.check(-1, what)
            setattr(self, attr, torch.empty(max(need, 256), dtype=torch.uint8, device=self.device))
        ws = getattr(self, attr)
        a.workspace, a.workspace_bytes = _lib.ptr(ws), int(ws.numel())

    def queue_evaluate(self, split: DeviceSplit, row0: int, nrows: int, n1, n2, out=None,
                       shift: int = 0):
        """Queue rae_eval_cost on the current stream (no host synchronisation): rows
        [row0, row0+nrows) of `split` viewed from row `shift` on, negatives n1 / n2 (device int32,
        (s, stride)), terms into `out` ((nrows, 3) fp32 or None), the sums into self._eval_sums.
        evaluate() is this plus the read-back; tools/eval_bench.py times it alone."""
        a = self._eval_args(split, row0, nrows, shift)
        a.neg_samples = self.s
        a.neg1, a.neg2, a.neg_stride = _lib.ptr(n1), _lib.ptr(n2), int(n1.shape[1])
        self._workspace(a, "_eval_ws", "rae_eval_workspace_bytes",
                        lambda: self.lib.rae_eval_workspace_bytes(C.byref(a)))
        if getattr(self, "_eval_sums", None) is None:    # once per engine
            self._eval_sums = torch.zeros(3, dtype=torch.float64, device=self.device)
        a.terms_out = _lib.ptr(out)
        a.sums_out = _lib.ptr(self._eval_sums)
        _lib.check(self.lib.rae_eval_cost(C.byref(a), self._stream()), "rae_eval_cost")

    # ------------------------------------------------------------------ argument ranking
    def rank(self, split: DeviceSplit, row0: int = 0, nrows: int | None = None,
             ks=(1, 10, 100), per_query: bool = False):
        """Where the true argument ranks among ALL entities, and its exact softmax
        log-likelihood, for rows [row0, row0+nrows) of `split` at the current parameters
        (rae_eval_rank; the scores are rae_eval_cost's).  RankResult: mrr, mean_rank, hits
        ({k: fraction}), logp (mean log-likelihood), each a (side 1, side 2, combined) tuple;
        per_query=True: also the (nrows, 2) tensors greater, equal, target, lse.  Reads back 16
        doubles once.  Touches no parameter, accumulator, plan state, cursor, negative or RNG.
        Partitioned update with stale rows: gathers the parameters first (a collective, like
        evaluate; every rank ranks the whole range)."""
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        row0 = int(row0)
        nrows = split.N - row0 if nrows is None else int(nrows)
        if row0 < 0 or nrows < 0 or row0 + nrows > split.N:
            raise IndexError(f"rows [{row0}, {row0 + nrows}) out of the split's {split.N}")
        ks = tuple(int(k) for k in ks)
        if len(ks) > 4 or any(k < 1 for k in ks):
            raise ValueError("ks: at most four thresholds, each >= 1")
        out = self.queue_rank(split, row0, nrows, ks, per_query)
        s = self._rank_summary.cpu().numpy()
        n = float(nrows)

        def three(j, scale=1.0):
            a, b = float(s[j]), float(s[8 + j])
            if nrows == 0:
                return (0.0, 0.0, 0.0)
            return (a / n * scale, b / n * scale, (a + b) / (2.0 * n) * scale)
        hits = {k: three(3 + j) for j, k in enumerate(ks)}
        return RankResult(three(0), three(1), hits, three(2), nrows, tuple(float(x) for x in s),
                          *(out if per_query else (None, None, None, None)))

    def queue_rank(self, split: DeviceSplit, row0: int, nrows: int, ks=(1, 10, 100),
                   per_query: bool = False, out=None):
        """Queue rae_eval_rank on the current stream (no host synchronisation): the summary
        into self._rank_summary (16 doubles), the per-query outputs into `out` = (greater, equal,
        target, lse), (nrows, 2) each (allocated here unless given; target / lse only with
        per_query).  Returns `out`.  rank() is this plus the read-back;
        tools/rank_eval_bench.py times it alone."""
        a = self._eval_args(split, row0, nrows)
        p = _lib.ptr
        self._workspace(a, "_rank_ws", "rae_rank_workspace_bytes",
                        lambda: self.lib.rae_rank_workspace_bytes(None, C.byref(a)))
        if getattr(self, "_rank_summary", None) is None:  # once per engine
            self._rank_summary = torch.zeros(16, dtype=torch.float64, device=self.device)
        if out is None:
            mk = lambda dt: torch.empty((nrows, 2), dtype=dt, device=self.device)
            out = (mk(torch.int32), mk(torch.int32),
                   mk(torch.float32) if per_query else None,
                   mk(torch.float32) if per_query else None)
        o = _lib.RaeRankOut()
        o.greater, o.equal, o.target, o.lse = p(out[0]), p(out[1]), p(out[2]), p(out[3])
        o.summary = p(self._rank_summary)
        for j in range(4):
            o.hits_k[j] = int(ks[j]) if j < len(ks) else 0
        _lib.check(self.lib.rae_eval_rank(C.byref(a), C.byref(o), self._stream()), "rae_eval_rank")
        return out

    # ------------------------------------------------------------------ top-k entity retrieval
    def _topk_args(self, split: DeviceSplit | None, row0: int = 0, nrows: int = 0):
        """rae_eval_args of rae_eval_topk (the fields rae_eval_rank reads) with the engine's
        top-k workspace, allocated once per engine for top = 32."""
        a = self._eval_args(split, row0, nrows)

        def need():                                      # for both entries
            q = _lib.RaeTopkArgs()
            q.n_entities, q.embed = self.cfg.n_entities, self.r
            size = self.lib.rae_topk_workspace_bytes
            return max(int(size(None, C.byref(a), _lib.RAE_ETK_MAXTOP)),
                       int(size(C.byref(q), None, _lib.RAE_ETK_MAXTOP)))
        self._workspace(a, "_topk_ws", "rae_topk_workspace_bytes", need)
        return a

    @staticmethod
    def _check_top(top):
        top = int(top)
        if not 1 <= top <= _lib.RAE_ETK_MAXTOP:
            raise ValueError(f"top must be in [1, {_lib.RAE_ETK_MAXTOP}]")
        return top

    def topk_entities(self, Q, top: int, add=None, skip=None):
        """The `top` best-scoring entities of every row of Q ((nq, r) fp32) against the engine's
        A / Ab (rae_topk_queries): score <Q[q], A[e]> + add[q] + Ab[e], entity skip[q] left out.
        Returns (ents int32, scores fp32), both (nq, top), ordered by score descending then
        entity ascending, padded with (-1, -inf).  Queued on the current stream, no host
        synchronisation.  Touches no parameter, accumulator, plan state, cursor, negative or RNG;
        partitioned update with stale rows: gathers the parameters first (a collective)."""
        top = self._check_top(top)
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        Q = torch.as_tensor(Q, dtype=torch.float32, device=self.device)
        if Q.dim() != 2 or Q.shape[1] != self.r:
            raise ValueError(f"Q must be (nq, {self.r}), got {tuple(Q.shape)}")
        nq = int(Q.shape[0])
        ldq = (self.r + 3) & ~3
        if ldq != self.r or not Q.is_contiguous() or Q.data_ptr() % 16:
            Qp = torch.zeros((nq, ldq), dtype=torch.float32, device=self.device)
            Qp[:, :self.r] = Q
            Q = Qp
        vec = lambda x, dt: None if x is None else torch.as_tensor(
            x, device=self.device).to(dt).contiguous().reshape(nq)
        add, skip = vec(add, torch.float32), vec(skip, torch.int32)
        e = self._topk_args(None)
        ents = torch.empty((nq, top), dtype=torch.int32, device=self.device)
        scores = torch.empty((nq, top), dtype=torch.float32, device=self.device)
        p = _lib.ptr
        a = _lib.RaeTopkArgs()
        a.Q, a.ldq, a.nq = p(Q), ldq, nq
        a.add, a.skip = p(add), p(skip)
        a.A, a.Ab = e.A, e.Ab
        a.n_entities, a.embed, a.top = self.cfg.n_entities, self.r, top
        a.ents_out, a.scores_out = p(ents), p(scores)
        a.workspace, a.workspace_bytes = e.workspace, e.workspace_bytes
        _lib.check(self.lib.rae_topk_queries(C.byref(a), self._stream()), "rae_topk_queries")
        return ents, scores

    def predict_arguments(self, split: DeviceSplit, row0: int = 0, nrows: int | None = None,
                          top: int = 10, skip_true: bool = False):
        """The `top` entities the model puts in each argument slot of rows [row0, row0+nrows) of
        `split`, given the other argument and the induced relation (rae_eval_topk; the scores are
        rae_eval_rank's).  Returns (ents int32, scores fp32), both (nrows, 2, top); skip_true
        leaves the row's true argument out.  Queued on the current stream.  Touches no parameter,
        accumulator, plan state, cursor, negative or RNG; partitioned update with stale rows:
        gathers the parameters first (a collective, like rank)."""
        top = self._check_top(top)
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        row0 = int(row0)
        nrows = split.N - row0 if nrows is None else int(nrows)
        if row0 < 0 or nrows < 0 or row0 + nrows > split.N:
            raise IndexError(f"rows [{row0}, {row0 + nrows}) out of the split's {split.N}")
        a = self._topk_args(split, row0, nrows)
        ents = torch.empty((nrows, 2, top), dtype=torch.int32, device=self.device)
        scores = torch.empty((nrows, 2, top), dtype=torch.float32, device=self.device)
        o = _lib.RaeTopkOut()
        o.ents, o.scores, o.top, o.skip_true = _lib.ptr(ents), _lib.ptr(scores), top, int(skip_true)
        _lib.check(self.lib.rae_eval_topk(C.byref(a), C.byref(o), self._stream()), "rae_eval_topk")
        return ents, scores

    def relation_preferences(self, top: int = 10):
        """The selectional preferences of every induced relation: for relation k and slot t the
        `top` entities e with the highest SP score <A[e], C_t[:, k]> + Ab[e] ('sp' and
        'rescal+sp'; the queries are the columns of C1 / C2).  Returns (ents int32, scores fp32),
        both (2, m, top).  'rescal' has no per-relation vector: ValueError."""
        top = self._check_top(top)
        named = self._named
        if "C1" not in named or "C2" not in named:
            raise ValueError("relation_preferences needs the selectional-preference matrices "
                             "C1 / C2 ('sp' or 'rescal+sp'); 'rescal' has no per-relation vector")
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        Q = torch.cat([named["C1"].detach().t(), named["C2"].detach().t()]).contiguous()
        ents, scores = self.topk_entities(Q, top)
        return ents.reshape(2, self.m, top), scores.reshape(2, self.m, top)

    # ------------------------------------------------------------------ relation scores
    label_with = "encoder"           # which labels the cluster evaluation / profiles count

    def _rel_eval_args(self, split: DeviceSplit, row0: int, nrows: int):
        """rae_eval_args of rae_eval_relations with the engine's workspace (once per engine)."""
        a = self._eval_args(split, row0, nrows)
        self._workspace(a, "_rel_ws", "rae_relscore_workspace_bytes",
                        lambda: self.lib.rae_relscore_workspace_bytes(None, C.byref(a)))
        return a

    def relation_scores(self, e1, e2):
        """psi ((nq, m) fp32): the decoder's score of every relation for the entity pairs
        (e1[q], e2[q]) at the current parameters (rae_relation_scores; include/rae.h has the
        definition per decoder).  Ids outside [0, n_entities) raise IndexError on the host.
        Queued on the current stream.  Touches no training state; partitioned update with stale
        rows: gathers the parameters first (a collective, like cluster_metrics)."""
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        ids = []
        for e in (e1, e2):
            h = np.ascontiguousarray(e.cpu().numpy() if torch.is_tensor(e) else e).reshape(-1)
            if h.size and (h.min() < 0 or h.max() >= self.cfg.n_entities):
                raise IndexError(f"entity ids must be in [0, {self.cfg.n_entities})")
            ids.append(torch.as_tensor(h.astype(np.int32), device=self.device))
        if ids[0].numel() != ids[1].numel():
            raise ValueError("e1 and e2 differ in length")
        nq = int(ids[0].numel())
        key = ("psi", nq)
        bufs = self.__dict__.setdefault("_rel_bufs", {})
        if key not in bufs:                  # once per shape
            bufs[key] = torch.empty((nq, self.m), dtype=torch.float32, device=self.device)
        psi = bufs[key]
        named = self._named
        p = _lib.ptr
        a = _lib.RaeRelscoreArgs()
        a.decoder, a.relations, a.embed = self.cfg.decoder, self.m, self.r
        a.n_entities = self.cfg.n_entities
        a.A, a.C1, a.C2 = p(named["A"]), p(named.get("C1")), p(named.get("C2"))
        a.R3 = p(named.get("R", named.get("C")))
        a.e1, a.e2, a.nq = p(ids[0]), p(ids[1]), nq
        a.psi_out, a.ldp = p(psi), self.m
        _lib.check(self.lib.rae_relation_scores(C.byref(a), self._stream()), "rae_relation_scores")
        self._rel_keep = ids                 # the id arrays live until the next call
        return psi

    def top_relations(self, e1, e2, top: int = 5):
        """(psi, values, relations): relation_scores and its `top` largest columns per pair
        (torch.topk: m <= 512 needs no kernel)."""
        psi = self.relation_scores(e1, e2)
        vals, rel = torch.topk(psi, min(int(top), self.m), dim=1)
        return psi, vals, rel

    def queue_label_relations(self, split: DeviceSplit, row0: int, nrows: int, mode: str,
                              labels=None):
        """Queue the labels of rows [row0, row0+nrows) of `split` under `mode` on the current
        stream (no host synchronisation) into `labels` (default: the engine's label buffer
        self._cl_labels, allocated once per shape): 'encoder' is rae_label, 'decoder' / 'joint'
        are rae_eval_relations' argmax of psi / of the joint score."""
        if mode not in _lib.LABEL_MODES:
            raise ValueError(f"mode must be one of {_lib.LABEL_MODES}")
        row0, nrows = int(row0), int(nrows)
        if row0 < 0 or nrows < 0 or row0 + nrows > split.N:
            raise IndexError(f"rows [{row0}, {row0 + nrows}) out of the split's {split.N}")
        if labels is None:
            if getattr(self, "_cl_labels", None) is None or self._cl_labels.numel() < nrows:
                self._cl_labels = torch.empty(max(nrows, 1), dtype=torch.int64,
                                              device=self.device)
            labels = self._cl_labels
        st = self._stream()
        if mode == "encoder":
            W, Wb = self.model.params[0], self.model.params[1]
            _lib.check(self.lib.rae_label(
                C.c_void_p(split.indptr.data_ptr()), C.c_void_p(split.indices.data_ptr()),
                C.c_void_p(split.values.data_ptr()) if split.values is not None else None,
                C.c_void_p(W.data_ptr()), C.c_void_p(Wb.data_ptr()), self.m, row0, nrows,
                C.c_void_p(labels.data_ptr()), None, st), "rae_label")
            return labels
        a = self._rel_eval_args(split, row0, nrows)
        o = _lib.RaeRelOut()
        if mode == "decoder":
            o.labels_dec = labels.data_ptr()
        else:
            o.labels_joint = labels.data_ptr()
        _lib.check(self.lib.rae_eval_relations(C.byref(a), C.byref(o), st), "rae_eval_relations")
        return labels

    def label_relations(self, split: DeviceSplit, row0: int = 0, nrows: int | None = None,
                        mode: str = "joint"):
        """Labels (int64 tensor) of rows [row0, row0+nrows) of `split` under `mode` in
        encoder | decoder | joint.  Touches no training state; partitioned update with stale
        rows: gathers the parameters first (a collective, like cluster_metrics)."""
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        row0 = int(row0)
        nrows = split.N - row0 if nrows is None else int(nrows)
        out = torch.empty(max(nrows, 1), dtype=torch.int64, device=self.device)
        self.queue_label_relations(split, row0, nrows, mode, out)
        return out[:nrows]

    def eval_relations(self, split: DeviceSplit, row0: int = 0, nrows: int | None = None):
        """(psi, joint, labels_dec, labels_joint) of rows [row0, row0+nrows) of `split`
        (rae_eval_relations, every output).  Touches no training state."""
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        row0 = int(row0)
        nrows = split.N - row0 if nrows is None else int(nrows)
        if row0 < 0 or nrows < 0 or row0 + nrows > split.N:
            raise IndexError(f"rows [{row0}, {row0 + nrows}) out of the split's {split.N}")
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        psi, joint = mk((nrows, self.m), torch.float32), mk((nrows, self.m), torch.float32)
        ld, lj = mk(max(nrows, 1), torch.int64), mk(max(nrows, 1), torch.int64)
        a = self._rel_eval_args(split, row0, nrows)
        o = _lib.RaeRelOut()
        o.psi, o.joint = psi.data_ptr(), joint.data_ptr()
        o.labels_dec, o.labels_joint = ld.data_ptr(), lj.data_ptr()
        _lib.check(self.lib.rae_eval_relations(C.byref(a), C.byref(o), self._stream()),
                   "rae_eval_relations")
        return psi, joint, ld[:nrows], lj[:nrows]

    # ------------------------------------------------------------------ cluster evaluation
    def _gold_dev(self, split: DeviceSplit, gold_index):
        """The gold ids (int32, split.N; -1 past the index's rows) and sizes (int64) of
        `gold_index` in HBM, uploaded once per (split, gold_index) like eval_negatives."""
        cache = self.__dict__.setdefault("_gold_cache", {})
        key = (id(split), id(gold_index))
        hit = cache.get(key)
        if hit is not None and hit[0] is split and hit[1] is gold_index:
            return hit[2], hit[3]
        ids = np.full(max(split.N, 1), -1, dtype=np.int32)
        k = min(split.N, int(gold_index.ids.shape[0]))
        ids[:k] = gold_index.ids[:k]
        ids_d = torch.as_tensor(ids, device=self.device)
        sizes_d = torch.as_tensor(np.ascontiguousarray(gold_index.sizes, dtype=np.int64),
                                  device=self.device)
        if sizes_d.numel() == 0:             # a pointer even for an empty gold standard
            sizes_d = torch.zeros(1, dtype=torch.int64, device=self.device)
        cache[key] = (split, gold_index, ids_d, sizes_d)
        return ids_d, sizes_d

    def queue_cluster_metrics(self, split: DeviceSplit, gold_index, row0: int = 0,
                              nrows: int | None = None, form: str = "auto"):
        """Queue rae_label(probs=None) -> rae_cluster_count -> rae_b3_metrics for rows
        [row0, row0+nrows) of `split` on the current stream (no host synchronisation, no
        allocation after the first call of a shape: capturable).  The table lands in
        self._cl_table[:relations * (n_gold + 1)], the four metric doubles and the cluster sizes
        in self._cl_out (int64 words: [0:4] the doubles' bits, [4:4+relations] the sizes).
        cluster_metrics() is this plus the read-back; tools/cluster_eval_bench.py times it."""
        if form not in _lib.CCOUNT_FORMS:
            raise ValueError(f"form must be one of {sorted(_lib.CCOUNT_FORMS)}")
        row0 = int(row0)
        nrows = split.N - row0 if nrows is None else int(nrows)
        if row0 < 0 or nrows < 0 or row0 + nrows > split.N:
            raise IndexError(f"rows [{row0}, {row0 + nrows}) out of the split's {split.N}")
        ng = int(gold_index.n_gold)
        ids_d, sizes_d = self._gold_dev(split, gold_index)
        cells = self.m * (ng + 1)
        if getattr(self, "_cl_out", None) is None:       # once per engine
            self._cl_out = torch.zeros(4 + self.m, dtype=torch.int64, device=self.device)
            self._cl_table = None
            self._cl_labels = None
        if self._cl_table is None or self._cl_table.numel() < cells:
            self._cl_table = torch.zeros(cells, dtype=torch.int64, device=self.device)
        if self._cl_labels is None or self._cl_labels.numel() < nrows:
            self._cl_labels = torch.empty(max(nrows, 1), dtype=torch.int64, device=self.device)
        st = self._stream()
        W, Wb = self.model.params[0], self.model.params[1]
        lab = self._cl_labels
        if self.label_with != "encoder":     # the same buffer, from rae_eval_relations
            self.queue_label_relations(split, row0, nrows, self.label_with, lab)
        else:
            _lib.check(self.lib.rae_label(
                C.c_void_p(split.indptr.data_ptr()), C.c_void_p(split.indices.data_ptr()),
                C.c_void_p(split.values.data_ptr()) if split.values is not None else None,
                C.c_void_p(W.data_ptr()), C.c_void_p(Wb.data_ptr()), self.m, row0, nrows,
                C.c_void_p(lab.data_ptr()), None, st), "rae_label")
        self._cl_labels_of = (id(split), row0, nrows)    # queue_cluster_profiles(reuse_labels)
        _lib.check(self.lib.rae_cluster_count(
            C.c_void_p(lab.data_ptr()), C.c_void_p(ids_d.data_ptr() + 4 * row0), nrows, self.m,
            ng, _lib.CCOUNT_FORMS[form], C.c_void_p(self._cl_table.data_ptr()), st),
            "rae_cluster_count")
        _lib.check(self.lib.rae_b3_metrics(
            C.c_void_p(self._cl_table.data_ptr()), C.c_void_p(sizes_d.data_ptr()),
            int(gold_index.n_assessable), self.m, ng, C.c_void_p(self._cl_out.data_ptr()),
            C.c_void_p(self._cl_out.data_ptr() + 32), st), "rae_b3_metrics")

    def cluster_metrics(self, split: DeviceSplit, gold_index, row0: int = 0,
                        nrows: int | None = None, table: bool = False, form: str = "auto"):
        """B^3 of the induced clusters of rows [row0, row0+nrows) of `split` at the current
        W / Wb against `gold_index` (rae.evaluation.GoldIndex), all on the device:
        ClusterResult(f1, precision, recall, n_elements, sizes, table) with compute_metrics'
        values (rae.evaluation.b3_from_table is the host oracle), sizes the cluster sizes
        (get_clusters_size) and, table=True, the contingency table.  One read-back (the four
        doubles and the sizes; the table only when asked).  Touches no training state.
        Partitioned update with stale rows: gathers W first (a collective, like label)."""
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        self.queue_cluster_metrics(split, gold_index, row0, nrows, form)
        self._cl_labels_of = None        # the queued sequence ends here: no later reuse
        ng = int(gold_index.n_gold)
        host = self._cl_out.cpu().numpy()
        f1, pre, rec, nel = (float(x) for x in host[:4].view(np.float64))
        tb = None
        if table:
            tb = self._cl_table[:self.m * (ng + 1)].cpu().numpy().reshape(self.m, ng + 1)
        return ClusterResult(f1, pre, rec, int(nel), host[4:].copy(), tb)

    # ------------------------------------------------------------------ cluster profiles
    def _keys_dev(self, split: DeviceSplit, key_index):
        """The key of every row of `split` (int32, split.N) under `key_index`
        (rae.evaluation.KeyIndex) in HBM: rae_row_keys over the whole split, or the upload of
        the index's own per-row keys (from_gold; -1 past them) -- once per (split, key_index),
        cached like _gold_dev: an example's key is static."""
        cache = self.__dict__.setdefault("_key_cache", {})
        key = (id(split), id(key_index))
        hit = cache.get(key)
        if hit is not None and hit[0] is split and hit[1] is key_index:
            return hit[2]
        if key_index.rows is not None:
            rows = np.full(max(split.N, 1), -1, dtype=np.int32)
            k = min(split.N, int(key_index.rows.shape[0]))
            rows[:k] = key_index.rows[:k]
            keys_d = torch.as_tensor(rows, device=self.device)
        else:
            kof = key_index.key_of_feature
            if kof.shape[0] != split.d:
                raise ValueError(f"key index over {kof.shape[0]} features, split has {split.d}")
            kof_d = torch.as_tensor(kof, device=self.device)
            keys_d = torch.empty(max(split.N, 1), dtype=torch.int32, device=self.device)
            _lib.check(self.lib.rae_row_keys(
                C.c_void_p(split.indptr.data_ptr()), C.c_void_p(split.indices.data_ptr()),
                C.c_void_p(split.values.data_ptr()) if split.values is not None else None,
                C.c_void_p(kof_d.data_ptr()), split.d, 0, split.N,
                C.c_void_p(keys_d.data_ptr()), self._stream()), "rae_row_keys")
        cache[key] = (split, key_index, keys_d)
        return keys_d

    def queue_cluster_profiles(self, split: DeviceSplit, key_index, row0: int = 0,
                               nrows: int | None = None, top: int = 5,
                               reuse_labels: bool = False):
        """Queue rae_label(probs=None) -> rae_cluster_key_count -> rae_cluster_topk for rows
        [row0, row0+nrows) of `split` on the current stream (no host synchronisation; no
        allocation after the first call of a shape, the split's row keys included: capturable
        from the second call on).  The table lands in self._pf_table[:relations * n_keys], the
        result in self._pf_out (int32 words: [0 : relations * top] the keys, [relations * 32 :
        relations * 32 + relations * top] the counts).  reuse_labels: skip the labelling pass
        and count the labels queue_cluster_metrics queued just before for the same rows -- in
        one queued sequence only (the mark is consumed here and dropped by every training step:
        labels are never reused across a parameter update)."""
        row0 = int(row0)
        nrows = split.N - row0 if nrows is None else int(nrows)
        top = int(top)
        if row0 < 0 or nrows < 0 or row0 + nrows > split.N:
            raise IndexError(f"rows [{row0}, {row0 + nrows}) out of the split's {split.N}")
        if not 1 <= top <= _lib.RAE_TOPK_MAX:
            raise ValueError(f"top must be in [1, {_lib.RAE_TOPK_MAX}]")
        nk = int(key_index.n_keys)
        if nk < 1:
            raise ValueError("the key index has no keys")
        keys_d = self._keys_dev(split, key_index)
        cells = self.m * nk
        if getattr(self, "_pf_out", None) is None:       # once per engine
            self._pf_out = torch.zeros(2 * self.m * _lib.RAE_TOPK_MAX, dtype=torch.int32,
                                       device=self.device)
            self._pf_table = None
        if self._pf_table is None or self._pf_table.numel() < cells:
            self._pf_table = torch.zeros(cells, dtype=torch.int32, device=self.device)
        st = self._stream()
        mark = (id(split), row0, nrows)
        if reuse_labels:
            if getattr(self, "_cl_labels_of", None) != mark:
                raise RuntimeError("reuse_labels: queue_cluster_metrics was not queued for these "
                                   "rows just before")
        else:
            if getattr(self, "_cl_labels", None) is None or self._cl_labels.numel() < nrows:
                self._cl_labels = torch.empty(max(nrows, 1), dtype=torch.int64,
                                              device=self.device)
            W, Wb = self.model.params[0], self.model.params[1]
            if self.label_with != "encoder":
                self.queue_label_relations(split, row0, nrows, self.label_with, self._cl_labels)
            else:
                _lib.check(self.lib.rae_label(
                    C.c_void_p(split.indptr.data_ptr()), C.c_void_p(split.indices.data_ptr()),
                    C.c_void_p(split.values.data_ptr()) if split.values is not None else None,
                    C.c_void_p(W.data_ptr()), C.c_void_p(Wb.data_ptr()), self.m, row0, nrows,
                    C.c_void_p(self._cl_labels.data_ptr()), None, st), "rae_label")
        self._cl_labels_of = None
        _lib.check(self.lib.rae_cluster_key_count(
            C.c_void_p(self._cl_labels.data_ptr()), C.c_void_p(keys_d.data_ptr() + 4 * row0),
            nrows, self.m, nk, 0, C.c_void_p(self._pf_table.data_ptr()), st),
            "rae_cluster_key_count")
        half = self.m * _lib.RAE_TOPK_MAX
        _lib.check(self.lib.rae_cluster_topk(
            C.c_void_p(self._pf_table.data_ptr()), self.m, nk, nk, top,
            C.c_void_p(self._pf_out.data_ptr()), C.c_void_p(self._pf_out.data_ptr() + 4 * half),
            st), "rae_cluster_topk")

    def _profile_result(self, top: int):
        host = self._pf_out.cpu().numpy()
        half, n = self.m * _lib.RAE_TOPK_MAX, self.m * top
        return ProfileResult(host[:n].reshape(self.m, top).copy(),
                             host[half:half + n].reshape(self.m, top).copy())

    def cluster_profiles(self, split: DeviceSplit, key_index, row0: int = 0,
                         nrows: int | None = None, top: int = 5):
        """Per induced cluster the `top` most frequent keys (triggers, or gold labels) of rows
        [row0, row0+nrows) of `split` at the current W / Wb, all on the device:
        ProfileResult(keys, counts), both (relations, top) int32 -- count descending, then key
        ascending, padded with (-1, 0); rae.evaluation.key_table + topk_from_table over the
        downloaded labels is the host oracle.  One read-back of 2 * relations * 32 words.
        Touches no training state.  Partitioned update with stale rows: gathers W first (a
        collective, like label)."""
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        self.queue_cluster_profiles(split, key_index, row0, nrows, top)
        return self._profile_result(int(top))

    def cluster_metrics_and_profiles(self, split: DeviceSplit, gold_index, key_index,
                                     row0: int = 0, nrows: int | None = None, top: int = 5,
                                     form: str = "auto"):
        """cluster_metrics and cluster_profiles of the same rows from ONE labelling pass:
        label -> count -> b3 -> key count -> top-k queued back to back, then the two
        read-backs.  Returns (ClusterResult, ProfileResult)."""
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        self.queue_cluster_metrics(split, gold_index, row0, nrows, form)
        self.queue_cluster_profiles(split, key_index, row0, nrows, top, reuse_labels=True)
        host = self._cl_out.cpu().numpy()
        f1, pre, rec, nel = (float(x) for x in host[:4].view(np.float64))
        return (ClusterResult(f1, pre, rec, int(nel), host[4:].copy(), None),
                self._profile_result(int(top)))

    # ------------------------------------------------------------------ relation feature profiles
    def feature_support(self, split: DeviceSplit):
        """support[f] of `split` in HBM (int32, max(split.d, 1) words): the number of its rows
        that store a non-zero value in column f (rae_feature_support over the whole split) --
        once per split, cached like _keys_dev: the support is static."""
        cache = self.__dict__.setdefault("_support_cache", {})
        hit = cache.get(id(split))
        if hit is not None and hit[0] is split:
            return hit[1]
        sup = torch.zeros(max(split.d, 1), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.rae_feature_support(
            C.c_void_p(split.indptr.data_ptr()), C.c_void_p(split.indices.data_ptr()),
            C.c_void_p(split.values.data_ptr()) if split.values is not None else None,
            split.d, 0, split.N, 0, C.c_void_p(sup.data_ptr()), self._stream()),
            "rae_feature_support")
        cache[id(split)] = (split, sup)
        return sup

    def relation_features(self, top: int = 10, centre: bool = True, min_support: int = 0,
                          split: DeviceSplit | None = None):
        """What the encoder keys on: per induced relation k the `top` features f with the highest
        weight W[f, k] -- centre: the row-centred weight W[f, k] - mean_k' W[f, k'], the
        identifiable one (softmax ignores a constant added to a row of W) -- among the features
        with at least min_support rows in `split` (None: no filter).  rae_feature_topk: returns
        (feats int32, scores fp32), both (m, top), score descending then feature ascending,
        padded with (-1, -inf); rae.evaluation.feature_topk is the host oracle.  Queued on the
        current stream, no host synchronisation.  Touches no parameter, accumulator, plan state,
        cursor, negative or RNG; partitioned update with stale rows: gathers W first (a
        collective, like label)."""
        top = self._check_top(top)
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        W = self.model.params[0]
        d = int(W.shape[0])
        sup = None
        if split is not None:
            if split.d != d:
                raise ValueError(f"split over {split.d} features, W has {d}")
            sup = self.feature_support(split)
        feats = torch.empty((self.m, top), dtype=torch.int32, device=self.device)
        scores = torch.empty((self.m, top), dtype=torch.float32, device=self.device)
        a = _lib.RaeFtopkArgs()
        a.W, a.n_features, a.relations, a.ldw = _lib.ptr(W), d, self.m, int(W.stride(0))
        a.support, a.min_support = _lib.ptr(sup), int(min_support)
        a.centre, a.top = 1, _lib.RAE_FT_MAXTOP         # the workspace: sized for every call
        self._workspace(a, "_ftopk_ws", "rae_feature_topk_workspace_bytes",
                        lambda: self.lib.rae_feature_topk_workspace_bytes(C.byref(a)))
        a.centre, a.top = int(bool(centre)), top
        a.feats_out, a.scores_out = _lib.ptr(feats), _lib.ptr(scores)
        _lib.check(self.lib.rae_feature_topk(C.byref(a), self._stream()), "rae_feature_topk")
        return feats, scores

    # ------------------------------------------------------------------ cluster exemplars
    def _row_range(self, split: DeviceSplit, row0, nrows):
        row0 = int(row0)
        nrows = split.N - row0 if nrows is None else int(nrows)
        if row0 < 0 or nrows < 0 or row0 + nrows > split.N:
            raise IndexError(f"rows [{row0}, {row0 + nrows}) out of the split's {split.N}")
        return row0, nrows

    def label_stats(self, split: DeviceSplit, row0: int = 0, nrows: int | None = None):
        """The encoder's labels with its confidence in them (rae_label_stats) for rows
        [row0, row0+nrows) of `split` at the current W / Wb: device tensors (labels int64, margin
        fp32, pmax fp32).  labels and pmax are bitwise label()'s labels and probs[i, label]; margin
        is the logit margin S[label] - S[second], what still separates rows whose posterior has
        saturated at 1.0f.  rae.evaluation.label_stats is the host oracle.  Queued on the current
        stream, no host synchronisation; partitioned update with stale rows: gathers W first (a
        collective, like label)."""
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        row0, nrows = self._row_range(split, row0, nrows)
        lab = torch.empty(nrows, dtype=torch.int64, device=self.device)
        margin = torch.empty(nrows, dtype=torch.float32, device=self.device)
        pmax = torch.empty(nrows, dtype=torch.float32, device=self.device)
        self._queue_label_stats(split, row0, nrows, lab, margin, pmax)
        return lab, margin, pmax

    def _queue_label_stats(self, split, row0, nrows, lab, margin, pmax):
        if nrows == 0:
            return
        W, Wb = self.model.params[0], self.model.params[1]
        _lib.check(self.lib.rae_label_stats(
            C.c_void_p(split.indptr.data_ptr()), C.c_void_p(split.indices.data_ptr()),
            C.c_void_p(split.values.data_ptr()) if split.values is not None else None,
            C.c_void_p(W.data_ptr()), C.c_void_p(Wb.data_ptr()), self.m, row0, nrows,
            _lib.ptr(lab), _lib.ptr(margin), _lib.ptr(pmax), self._stream()), "rae_label_stats")

    def queue_cluster_exemplars(self, split: DeviceSplit, top: int = 5, by="margin",
                                largest: bool = True, labels=None, row0: int = 0,
                                nrows: int | None = None):
        """Queue rae_label_stats (unless `by` is a tensor and labels are given) ->
        rae_cluster_exemplars for rows [row0, row0+nrows) of `split` on the current stream (no host
        synchronisation).  by: "margin" or "pmax" of the encoder, or a device float tensor of nrows
        per-row scores (psi / J of eval_relations, a term of evaluate(terms=True), ...).  labels:
        a device int64 tensor of nrows cluster ids (default: the encoder's own).  The result lands
        in self._cx_out (int32 words: [0 : relations * top] the rows within the range,
        [relations * 32 : relations * 32 + relations * top] the scores' bits)."""
        row0, nrows = self._row_range(split, row0, nrows)
        top = self._check_top(top)
        scores = None
        if torch.is_tensor(by):
            scores = by.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
            if scores.numel() != nrows:
                raise ValueError(f"by has {scores.numel()} scores, the range {nrows} rows")
        elif by not in ("margin", "pmax"):
            raise ValueError('by must be "margin", "pmax" or a device tensor of per-row scores')
        if labels is not None:
            labels = labels.to(device=self.device, dtype=torch.int64).contiguous().reshape(-1)
            if labels.numel() != nrows:
                raise ValueError(f"labels has {labels.numel()} entries, the range {nrows} rows")
        if scores is None or labels is None:
            lab = torch.empty(nrows, dtype=torch.int64, device=self.device)
            st = torch.empty(nrows, dtype=torch.float32, device=self.device)
            if scores is None:
                self._queue_label_stats(split, row0, nrows, lab, st if by == "margin" else None,
                                        st if by == "pmax" else None)
                scores = st
            else:
                self._queue_label_stats(split, row0, nrows, lab, None, None)
            labels = lab if labels is None else labels
        half = self.m * _lib.RAE_CX_MAXTOP
        if getattr(self, "_cx_out", None) is None:       # once per engine
            self._cx_out = torch.zeros(2 * half, dtype=torch.int32, device=self.device)
        a = _lib.RaeExemplarArgs()
        a.relations, a.largest = self.m, 1
        a.nrows, a.top = (1 << 31) - 1, _lib.RAE_CX_MAXTOP     # the workspace: sized for every call
        self._workspace(a, "_cx_ws", "rae_cluster_exemplars_workspace_bytes",
                        lambda: self.lib.rae_cluster_exemplars_workspace_bytes(C.byref(a)))
        a.nrows, a.top, a.largest = nrows, top, int(bool(largest))
        a.labels, a.scores = _lib.ptr(labels) or None, _lib.ptr(scores) or None
        a.rows_out = self._cx_out.data_ptr()
        a.scores_out = self._cx_out.data_ptr() + 4 * half
        _lib.check(self.lib.rae_cluster_exemplars(C.byref(a), self._stream()),
                   "rae_cluster_exemplars")
        self._cx_keep = (labels, scores)     # alive until the queued kernels have read them

    def cluster_exemplars(self, split: DeviceSplit, top: int = 5, by="margin",
                          largest: bool = True, labels=None, row0: int = 0,
                          nrows: int | None = None):
        """Per induced cluster its `top` rows by a per-row score, all on the device:
        ExemplarResult(rows, scores), rows (relations, top) int32 row ids of the split (row0 added;
        padding -1), scores (relations, top) fp32 -- score descending (largest) or ascending, then
        row ascending, padded with (-1, -inf).  by="margin": the clearest members of every cluster
        (largest) or its boundary rows (largest=False) by the encoder's logit margin; "pmax" by its
        posterior; a device tensor: any per-row score.  rae.evaluation.cluster_exemplars is the
        host oracle.  One read-back of 2 * relations * 32 words.  Touches no training state.
        Partitioned update with stale rows: gathers W first (a collective, like label)."""
        if self.stale(accumulators=False):
            self.sync_replicas(accumulators=False)
        self.queue_cluster_exemplars(split, top, by, largest, labels, row0, nrows)
        top = int(top)
        host = self._cx_out.cpu().numpy()
        self._cx_keep = None
        half, n = self.m * _lib.RAE_CX_MAXTOP, self.m * top
        rows = host[:n].reshape(self.m, top).copy()
        rows[rows >= 0] += int(row0)
        return ExemplarResult(rows, host[half:half + n].view(np.float32).reshape(self.m, top).copy())

    def cluster_confidence(self, split: DeviceSplit, bins: int = 10, row0: int = 0,
                           nrows: int | None = None):
        """Per induced cluster the histogram of its rows' posterior pmax: a (relations, bins)
        int32 device tensor, bin = min(int(pmax * bins), bins - 1) (a NaN pmax is not counted).
        rae_label_stats, the binning in torch on the device, then the existing
        rae_cluster_key_count with the bin as the per-row key: no kernel of its own.  A collapsed
        encoder shows as one row of the table holding every count."""
        bins = int(bins)
        if not 1 <= bins <= _lib.RAE_KEYCOUNT_MAX_KEYS:
            raise ValueError(f"bins must be in [1, {_lib.RAE_KEYCOUNT_MAX_KEYS}]")
        lab, _, pmax = self.label_stats(split, row0, nrows)
        n = int(lab.numel())
        key = torch.clamp((pmax * bins).to(torch.int32), max=bins - 1)
        key = torch.where(torch.isnan(pmax), torch.full_like(key, -1), key).contiguous()
        table = torch.zeros((self.m, bins), dtype=torch.int32, device=self.device)
        if n:
            _lib.check(self.lib.rae_cluster_key_count(
                C.c_void_p(lab.data_ptr()), C.c_void_p(key.data_ptr()), n, self.m, bins, 0,
                C.c_void_p(table.data_ptr()), self._stream()), "rae_cluster_key_count")
        return table
