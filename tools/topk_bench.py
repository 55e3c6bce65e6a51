#!/usr/bin/env python
"""Top-k entity retrieval: rae_topk_queries beside the rank kernel (the same tile without the
selection: this design's floor) and a torch path, then the two engine entries end to end.

One JSON line per measurement, all in one process and run:
  topk_queries   rae_topk_queries alone (HIP events, 2 warm-ups, median of 5) on nq = 8192 random
                 queries against n = 200,000 entities at r = 200 and r = 1024, top = 1, 10, 32:
                   rank_us / rank_lse_us  rae_rank_queries on the same Q and A without / with the
                                          log-sum-exp, timed in the same run
                   over_rank              kernel_us / rank_us  (the cost of the selection)
                   lse_over_rank          rank_lse_us / rank_us  (what the other epilogue costs)
                   torch_us               torch.mm(Q_chunk, A.T) + add + torch.topk over the same Q
                                          in chunks of 1024 queries (the product is stored)
                   torch_over_kernel      torch_us / kernel_us  (> 1: the kernel is faster)
                   set_mismatches         queries whose entity row differs from torch.topk's
                                          (near-ties under the BLAS's other summation order)
                 torch.mm unavailable: torch_error holds the exception and the ratio is null.
  predict_arguments     TrainEngine.predict_arguments (rae_eval_topk: query build, selection,
                        merge) on 16384 rows of a synthetic split, K = 100, r = 200, top = 10: HIP
                        events around the queued call.
  relation_preferences  TrainEngine.relation_preferences at m = 100 (200 queries), top = 10.
No threshold: the numbers are what was measured.

    python tools/topk_bench.py [--out profiles/topk_bench.json] [--examples 1000000]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "relation-autoencoder_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rank_eval_bench import event_us  # noqa: E402

NQ, N_ENT = 8192, 200000
TORCH_CHUNK = 1024
TOPS = (1, 10, 32)


def bench_queries(torch, dev, lib, r, emit):
    from rae import _lib
    g = torch.Generator(device=dev)
    g.manual_seed(1 + r)
    Q = torch.randn((NQ, r), generator=g, device=dev) * 0.3
    A = torch.randn((N_ENT, r), generator=g, device=dev) * 0.3
    add = torch.randn(NQ, generator=g, device=dev)
    Ab = torch.randn(N_ENT, generator=g, device=dev)
    target = torch.randn(NQ, generator=g, device=dev)
    st = torch.cuda.current_stream()
    sp_ = C.c_void_p(st.cuda_stream)
    # the rank kernel on the same operands: the tile without the selection
    gr = torch.empty(NQ, dtype=torch.int32, device=dev)
    eq = torch.empty(NQ, dtype=torch.int32, device=dev)
    lse = torch.empty(NQ, dtype=torch.float32, device=dev)
    ra = _lib.RaeRankArgs()
    ra.Q, ra.ldq, ra.nq = _lib.ptr(Q), r, NQ
    ra.add, ra.target, ra.skip = _lib.ptr(add), _lib.ptr(target), None
    ra.A, ra.Ab, ra.n_entities, ra.embed = _lib.ptr(A), _lib.ptr(Ab), N_ENT, r
    ra.greater, ra.equal = _lib.ptr(gr), _lib.ptr(eq)
    need = int(lib.rae_rank_workspace_bytes(C.byref(ra), None))
    rws = torch.empty(need, dtype=torch.uint8, device=dev)
    ra.workspace, ra.workspace_bytes = _lib.ptr(rws), need

    def rank(with_lse):
        ra.lse = _lib.ptr(lse) if with_lse else None
        _lib.check(lib.rae_rank_queries(C.byref(ra), sp_), "rae_rank_queries")

    rank_us = event_us(torch, st, lambda: rank(False))
    rank_lse_us = event_us(torch, st, lambda: rank(True))
    flops = 2.0 * NQ * N_ENT * r
    for top in TOPS:
        ents = torch.empty((NQ, top), dtype=torch.int32, device=dev)
        scores = torch.empty((NQ, top), dtype=torch.float32, device=dev)
        a = _lib.RaeTopkArgs()
        a.Q, a.ldq, a.nq = _lib.ptr(Q), r, NQ
        a.add, a.skip = _lib.ptr(add), None
        a.A, a.Ab, a.n_entities, a.embed, a.top = _lib.ptr(A), _lib.ptr(Ab), N_ENT, r, top
        a.ents_out, a.scores_out = _lib.ptr(ents), _lib.ptr(scores)
        need = int(lib.rae_topk_workspace_bytes(C.byref(a), None, top))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        a.workspace, a.workspace_bytes = _lib.ptr(ws), need

        def kernel():
            _lib.check(lib.rae_topk_queries(C.byref(a), sp_), "rae_topk_queries")

        kernel_us = event_us(torch, st, kernel)
        rank_again_us = event_us(torch, st, lambda: rank(False))    # the floor, after as before
        line = {"what": "topk_queries", "embed": r, "nq": NQ, "n_entities": N_ENT, "top": top,
                "kernel_us": kernel_us, "workspace_bytes": need,
                "gemm_tflops": flops / (kernel_us * 1e-6) / 1e12,
                "rank_us": rank_us, "rank_again_us": rank_again_us, "rank_lse_us": rank_lse_us,
                "over_rank": kernel_us / rank_us, "lse_over_rank": rank_lse_us / rank_us}
        te = torch.empty((NQ, top), dtype=torch.int64, device=dev)
        tv = torch.empty((NQ, top), dtype=torch.float32, device=dev)

        def torch_path():
            At = A.t()
            for c0 in range(0, NQ, TORCH_CHUNK):
                s = slice(c0, c0 + TORCH_CHUNK)
                S = torch.mm(Q[s], At)
                S += add[s, None]
                S += Ab[None, :]
                tv[s], te[s] = torch.topk(S, top, dim=1)

        try:
            torch_us = event_us(torch, st, torch_path)
            kernel()
            torch.cuda.synchronize()
            line.update(torch_us=torch_us, torch_over_kernel=torch_us / kernel_us,
                        torch_chunk=TORCH_CHUNK,
                        set_mismatches=int((te != ents.long()).any(dim=1).sum().item()),
                        max_score_diff=float((tv - scores).abs().max().item()))
        except Exception as exc:                                    # no BLAS for torch.mm here
            line.update(torch_us=None, torch_over_kernel=None, torch_error=repr(exc)[:300])
        emit(line)


def bench_engine(torch, dev, examples, rows, emit):
    from rae.data import synthetic_dataset
    from rae.inducer import ReconstructInducer
    data, gold = synthetic_dataset(examples, 2 ** 17, 10, seed=1234)
    ind = ReconstructInducer(data, gold, np.random.RandomState(2), 1, 0.1, 100, 200, 100, 20, 0.0,
                             0.0, "adagrad", "topkbench", "sp", False, True, False, 1.0,
                             device=dev, neg_sampler="philox")
    ind.compile_function()
    eng = ind.engine
    split = eng.split
    rows = min(rows, split.N)
    st = torch.cuda.current_stream()
    n = data.get_arg_voc_size()
    how = ("HIP events around the queued call, output allocation included (2 warm-ups, median "
           "of 5); parameters at their initial values")
    us = event_us(torch, st, lambda: eng.predict_arguments(split, 0, rows, top=10))
    emit({"what": "predict_arguments", "decoder": "sp", "relations": 100, "embed": 200,
          "rows": rows, "examples": split.N, "n_entities": n, "top": 10, "queued_us": us,
          "gemm_tflops_end_to_end": 2.0 * (2 * rows) * n * 200 / (us * 1e-6) / 1e12, "how": how})
    us = event_us(torch, st, lambda: eng.relation_preferences(10))
    emit({"what": "relation_preferences", "decoder": "sp", "relations": 100, "embed": 200,
          "queries": 200, "n_entities": n, "top": 10, "queued_us": us, "how": how})
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_bench.json"),
                    help="the JSON lines are also written to this file")
    ap.add_argument("--examples", type=int, default=1000000,
                    help="examples of the synthetic split (entities = examples / 5)")
    ap.add_argument("--rows", type=int, default=16384)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge
    ge.build()
    from rae import _lib
    assert torch.cuda.is_available(), "topk_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _lib.load()
    lines = []

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        lines.append(text)
        with open(args.out, "w") as fh:                             # kept if a later step fails
            fh.write("\n".join(lines) + "\n")

    for r in (200, 1024):
        bench_queries(torch, dev, lib, r, emit)
    bench_engine(torch, dev, args.examples, args.rows, emit)


if __name__ == "__main__":
    main()
