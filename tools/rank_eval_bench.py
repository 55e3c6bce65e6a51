#!/usr/bin/env python
"""Argument ranking over all entities: the rank kernel alone, the split entry end to end, and a
torch path on the same GPU.

One JSON line per measurement:
  rank_queries   rae_rank_queries alone (HIP events, 2 warm-ups, median of 5) on random Q at the
                 headline r = 200 and at r = 1024, n = 200,000 entities (the headline dataset's),
                 nq = 8192, with and without the log-sum-exp:
                   tflops            2 nq n r / time -- the GEMM's flops only
                   frac_of_155       ... over the 155 TFLOP/s measured fp32-MFMA rate
                   torch_us          torch.mm(Q_chunk, A.T) + add, compare, sum (and logsumexp) over
                                     the same Q in chunks of 1024 queries (the product is stored)
                   torch_over_kernel torch_us / kernel_us  (> 1: the kernel is faster)
                   count_mismatches  queries whose `greater` differs between the two paths
                                     (near-ties under the BLAS's other summation order)
                 torch.mm unavailable: torch_error holds the exception and the ratio is null.
  eval_rank      rae_eval_rank end to end (TrainEngine.queue_rank: query build, rank kernel, lse
                 finish, summary) on 16384 rows of a synthetic split, K = 100, r = 200: HIP events
                 around the queued call, and the host clock around TrainEngine.rank (with the
                 read-back of the 16 doubles).
No threshold: the numbers are what was measured.

    python tools/rank_eval_bench.py [--out profiles/rank_eval_bench.json] [--examples 1000000]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "relation-autoencoder_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_TF = 155.0              # measured v_mfma_f32_32x32x2_f32 rate of an MI355X
NQ, N_ENT = 8192, 200000
TORCH_CHUNK = 1024


def event_us(torch, st, fn, warm=2, reps=5):
    """Median HIP-event time of fn() in microseconds."""
    for _ in range(warm):
        fn()
    ev = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(2)) for _ in range(reps)]
    for a, b in ev:
        a.record(st)
        fn()
        b.record(st)
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)


def bench_queries(torch, dev, lib, r, with_lse):
    from rae import _lib
    g = torch.Generator(device=dev)
    g.manual_seed(1 + r)
    Q = torch.randn((NQ, r), generator=g, device=dev) * 0.3
    A = torch.randn((N_ENT, r), generator=g, device=dev) * 0.3
    add = torch.randn(NQ, generator=g, device=dev)
    Ab = torch.randn(N_ENT, generator=g, device=dev)
    target = torch.randn(NQ, generator=g, device=dev)
    gr = torch.empty(NQ, dtype=torch.int32, device=dev)
    eq = torch.empty(NQ, dtype=torch.int32, device=dev)
    lse = torch.empty(NQ, dtype=torch.float32, device=dev) if with_lse else None
    a = _lib.RaeRankArgs()
    a.Q, a.ldq, a.nq = _lib.ptr(Q), r, NQ
    a.add, a.target, a.skip = _lib.ptr(add), _lib.ptr(target), None
    a.A, a.Ab, a.n_entities, a.embed = _lib.ptr(A), _lib.ptr(Ab), N_ENT, r
    a.greater, a.equal, a.lse = _lib.ptr(gr), _lib.ptr(eq), _lib.ptr(lse)
    need = int(lib.rae_rank_workspace_bytes(C.byref(a), None))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), need
    st = torch.cuda.current_stream()
    sp_ = C.c_void_p(st.cuda_stream)

    def kernel():
        _lib.check(lib.rae_rank_queries(C.byref(a), sp_), "rae_rank_queries")

    kernel_us = event_us(torch, st, kernel)
    flops = 2.0 * NQ * N_ENT * r
    line = {"what": "rank_queries", "embed": r, "nq": NQ, "n_entities": N_ENT, "lse": with_lse,
            "kernel_us": kernel_us, "tflops": flops / (kernel_us * 1e-6) / 1e12,
            "frac_of_155": flops / (kernel_us * 1e-6) / 1e12 / PEAK_TF}
    tg = torch.empty(NQ, dtype=torch.int64, device=dev)
    te = torch.empty(NQ, dtype=torch.int64, device=dev)
    tl = torch.empty(NQ, dtype=torch.float32, device=dev)

    def torch_path():
        At = A.t()
        for c0 in range(0, NQ, TORCH_CHUNK):
            s = slice(c0, c0 + TORCH_CHUNK)
            S = torch.mm(Q[s], At)
            S += add[s, None]
            S += Ab[None, :]
            tg[s] = (S > target[s, None]).sum(dim=1)
            te[s] = (S == target[s, None]).sum(dim=1)
            if with_lse:
                tl[s] = torch.logsumexp(S, dim=1)

    try:
        torch_us = event_us(torch, st, torch_path)
        kernel()
        torch.cuda.synchronize()
        line.update(torch_us=torch_us, torch_over_kernel=torch_us / kernel_us,
                    torch_chunk=TORCH_CHUNK,
                    count_mismatches=int((tg != gr.long()).sum().item()))
    except Exception as exc:                                    # no BLAS for torch.mm here
        line.update(torch_us=None, torch_over_kernel=None, torch_error=repr(exc)[:300])
    return line


def bench_split(torch, dev, examples, rows):
    from rae.data import synthetic_dataset
    from rae.inducer import ReconstructInducer
    data, gold = synthetic_dataset(examples, 2 ** 17, 10, seed=1234)
    ind = ReconstructInducer(data, gold, np.random.RandomState(2), 1, 0.1, 100, 200, 100, 20, 0.0,
                             0.0, "adagrad", "rankbench", "sp", False, True, False, 1.0,
                             device=dev, neg_sampler="philox")
    ind.compile_function()
    eng = ind.engine
    split = eng.split
    rows = min(rows, split.N)
    st = torch.cuda.current_stream()
    out = eng.queue_rank(split, 0, rows)
    queued_us = event_us(torch, st, lambda: eng.queue_rank(split, 0, rows, out=out))
    for _ in range(2):
        eng.rank(split, 0, rows)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        res = eng.rank(split, 0, rows)
        ts.append(time.perf_counter() - t0)
    n = data.get_arg_voc_size()
    flops = 2.0 * (2 * rows) * n * 200
    line = {"what": "eval_rank", "decoder": "sp", "relations": 100, "embed": 200, "rows": rows,
            "examples": split.N, "n_entities": n, "queued_us": queued_us,
            "wall_s": float(np.median(ts)), "tflops_end_to_end": flops / (queued_us * 1e-6) / 1e12,
            "mrr": res.mrr[2], "mean_rank": res.mean_rank[2], "logp": res.logp[2],
            "how": "HIP events around TrainEngine.queue_rank (2 warm-ups, median of 5); host clock "
                   "around TrainEngine.rank, which ends in the read-back (2 warm-ups, median of 5); "
                   "parameters at their initial values"}
    eng.close()
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--examples", type=int, default=1000000,
                    help="examples of the synthetic split (entities = examples / 5)")
    ap.add_argument("--rows", type=int, default=16384)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge
    ge.build()
    from rae import _lib
    assert torch.cuda.is_available(), "rank_eval_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _lib.load()
    lines = []

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        lines.append(text)

    for r in (200, 1024):
        for with_lse in (False, True):
            emit(bench_queries(torch, dev, lib, r, with_lse))
    emit(bench_split(torch, dev, args.examples, args.rows))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
