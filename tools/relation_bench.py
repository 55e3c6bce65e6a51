#!/usr/bin/env python
"""Relation scores from the decoder: rae_relation_scores beside the project's other fp32-MFMA GEMM
(the rank kernel) and a torch path, rae_eval_relations beside rae_label, and B^3 of the sample under
the three --label-with modes.

One JSON line per measurement, all in one process and run (HIP events, 2 warm-ups, median of 5):
  relation_scores   rae_relation_scores at nq = 16384 pairs over 50,000 entities:
                      kernel_us, tflops = 2 nq K m / time, of_peak = tflops / 155 (the fp32-MFMA
                                        rate of the MI355X guide)
                      rank_us / rank_tflops / rank_of_peak   rae_rank_queries (no log-sum-exp) on
                                        an equal-flop problem (8192 queries, the same embed, as
                                        many entities as make 2 nq n r equal), timed in the same run
                      vs_rank           of_peak / rank_of_peak
                      torch_us          (a1[:, :, None] * a2[:, None, :]).reshape(-1, r*r) @
                                        R3.view(r*r, m) (+ the SP terms) in chunks of 1024 pairs
                      torch_over_kernel torch_us / kernel_us  (> 1: the kernel is faster)
                      max_diff          max |psi - torch's|
  eval_relations    TrainEngine.eval_relations' entry (rae_eval_relations, every output) queued on
                    16384 rows of the 1M synthetic split at the C5 shape, beside rae_label (labels
                    only) on the same rows.
  b3_label_with     tests/golden/data-sample.txt.gz trained as README's config 1; B^3 of the train
                    split under label_with = encoder, decoder, joint (TrainEngine.cluster_metrics).
                    Reported, not asserted.
No threshold: the numbers are what was measured.

    python tools/relation_bench.py [--out profiles/relation_scores_bench.json] [--examples 1000000]
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "relation-autoencoder_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rank_eval_bench import event_us  # noqa: E402

NQ, N_ENT, RANK_NQ = 16384, 50000, 8192
TORCH_CHUNK = 1024
PEAK_TFLOPS = 155.0
CASES = (("rescal", 200, 100), ("rescal+sp", 200, 100), ("rescal", 1024, 16), ("sp", 200, 100))


def bench_scores(torch, dev, lib, dec, r, m, emit):
    from rae import _lib
    g = torch.Generator(device=dev)
    g.manual_seed(1 + r + m)
    rnd = lambda *shape: torch.randn(shape, generator=g, device=dev) * 0.3
    A = rnd(N_ENT, r)
    C1 = C2 = R3 = None
    if dec != "rescal":
        C1, C2 = rnd(r, m), rnd(r, m)
    if dec != "sp":
        R3 = rnd(r, r, m)
    e1 = torch.randint(0, N_ENT, (NQ,), generator=g, device=dev, dtype=torch.int32)
    e2 = torch.randint(0, N_ENT, (NQ,), generator=g, device=dev, dtype=torch.int32)
    psi = torch.empty((NQ, m), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream()
    sp_ = C.c_void_p(st.cuda_stream)
    a = _lib.RaeRelscoreArgs()
    a.decoder, a.relations, a.embed, a.n_entities = _lib.RAE_DEC[dec], m, r, N_ENT
    a.A, a.C1, a.C2, a.R3 = _lib.ptr(A), _lib.ptr(C1), _lib.ptr(C2), _lib.ptr(R3)
    a.e1, a.e2, a.nq = _lib.ptr(e1), _lib.ptr(e2), NQ
    a.psi_out, a.ldp = _lib.ptr(psi), m

    def kernel():
        _lib.check(lib.rae_relation_scores(C.byref(a), sp_), "rae_relation_scores")

    K = {"sp": 2 * r, "rescal": r * r, "rescal+sp": r * r + 2 * r}[dec]
    flops = 2.0 * NQ * K * m
    kernel_us = event_us(torch, st, kernel)
    # the rank kernel on an equal-flop problem
    n_rank = max(128, int(round(flops / (2.0 * RANK_NQ * r))))
    Q = rnd(RANK_NQ, r)
    Ar = rnd(n_rank, r)
    target = rnd(RANK_NQ)
    gr = torch.empty(RANK_NQ, dtype=torch.int32, device=dev)
    eq = torch.empty(RANK_NQ, dtype=torch.int32, device=dev)
    ra = _lib.RaeRankArgs()
    ra.Q, ra.ldq, ra.nq = _lib.ptr(Q), r, RANK_NQ
    ra.add, ra.target, ra.skip = None, _lib.ptr(target), None
    ra.A, ra.Ab, ra.n_entities, ra.embed = _lib.ptr(Ar), None, n_rank, r
    ra.greater, ra.equal, ra.lse = _lib.ptr(gr), _lib.ptr(eq), None
    need = int(lib.rae_rank_workspace_bytes(C.byref(ra), None))
    rws = torch.empty(need, dtype=torch.uint8, device=dev)
    ra.workspace, ra.workspace_bytes = _lib.ptr(rws), need
    rank_us = event_us(torch, st, lambda: _lib.check(
        lib.rae_rank_queries(C.byref(ra), sp_), "rae_rank_queries"))
    rank_flops = 2.0 * RANK_NQ * n_rank * r
    kernel_again_us = event_us(torch, st, kernel)
    tf = flops / (kernel_us * 1e-6) / 1e12
    rtf = rank_flops / (rank_us * 1e-6) / 1e12
    line = {"what": "relation_scores", "decoder": dec, "embed": r, "relations": m, "nq": NQ,
            "n_entities": N_ENT, "K": K, "kernel_us": kernel_us, "kernel_again_us": kernel_again_us,
            "tflops": tf, "of_peak": tf / PEAK_TFLOPS, "peak_tflops": PEAK_TFLOPS,
            "rank_n_entities": n_rank, "rank_nq": RANK_NQ, "rank_us": rank_us, "rank_tflops": rtf,
            "rank_of_peak": rtf / PEAK_TFLOPS, "vs_rank": tf / rtf}
    tp = torch.empty((NQ, m), dtype=torch.float32, device=dev)

    def torch_path():
        for c0 in range(0, NQ, TORCH_CHUNK):
            s = slice(c0, c0 + TORCH_CHUNK)
            a1, a2 = A[e1[s].long()], A[e2[s].long()]
            if dec == "sp":
                tp[s] = a1 @ C1 + a1 @ C2
                continue
            out = (a1[:, :, None] * a2[:, None, :]).reshape(-1, r * r) @ R3.view(r * r, m)
            if dec == "rescal+sp":
                out += a1 @ C1 + a2 @ C2
            tp[s] = out

    try:
        torch_us = event_us(torch, st, torch_path)
        kernel()
        torch.cuda.synchronize()
        line.update(torch_us=torch_us, torch_over_kernel=torch_us / kernel_us,
                    torch_chunk=TORCH_CHUNK, max_diff=float((tp - psi).abs().max().item()),
                    max_abs_psi=float(psi.abs().max().item()))
    except Exception as exc:                                        # no BLAS for torch.mm here
        line.update(torch_us=None, torch_over_kernel=None, torch_error=repr(exc)[:300])
    emit(line)


def bench_engine(torch, dev, examples, rows, emit):
    from rae.data import synthetic_dataset
    from rae.inducer import ReconstructInducer
    data, gold = synthetic_dataset(examples, 2 ** 17, 10, seed=1234)
    ind = ReconstructInducer(data, gold, np.random.RandomState(2), 1, 0.1, 100, 200, 100, 20, 0.0,
                             0.0, "adagrad", "relbench", "rescal", False, True, False, 1.0,
                             device=dev, neg_sampler="philox")
    ind.compile_function()
    eng = ind.engine
    split = eng.split
    rows = min(rows, split.N)
    st = torch.cuda.current_stream()
    how = ("HIP events around the queued call, output allocation included (2 warm-ups, median "
           "of 5); parameters at their initial values")
    us = event_us(torch, st, lambda: eng.eval_relations(split, 0, rows))
    lab_us = event_us(torch, st, lambda: eng.label(split, 0, rows, probs=False))
    joint_us = event_us(torch, st, lambda: eng.label_relations(split, 0, rows, "joint"))
    emit({"what": "eval_relations", "decoder": "rescal", "relations": 100, "embed": 200,
          "rows": rows, "examples": split.N, "n_entities": data.get_arg_voc_size(),
          "queued_us": us, "joint_labels_only_us": joint_us, "rae_label_us": lab_us,
          "over_label": us / lab_us,
          "tflops_end_to_end": 2.0 * rows * 200 * 200 * 100 / (us * 1e-6) / 1e12, "how": how})
    eng.close()


def bench_b3(torch, dev, emit):
    from rae import preprocess as P
    from rae.evaluation import GoldIndex
    from rae.inducer import ReconstructInducer
    sample = os.path.join(ROOT, "tests", "golden", "data-sample.txt.gz")
    with tempfile.TemporaryDirectory() as tmp:
        plain, out = os.path.join(tmp, "data-sample.txt"), os.path.join(tmp, "ds.json.gz")
        with gzip.open(sample, "rb") as src, open(plain, "wb") as dst:
            shutil.copyfileobj(src, dst)
        P.preprocess(plain, out)
        data, gold = P.load_data(out)
    for dec in ("sp", "rescal", "rescal+sp"):
        # README's config 1 (sp); the other decoders at the same sizes
        ind = ReconstructInducer(data, gold, np.random.RandomState(2), 10, 0.1, 100, 10, 10, 5, 0.0,
                                 0.1, "adagrad", "c1", dec, False, True, False, 0.1, device=dev)
        ind.learn(verbose=False)
        eng, ds = ind.engine, ind.engine.split
        gi = GoldIndex((gold or {}).get("train", {}), ds.N)
        nrows = (ds.N // 100) * 100
        line = {"what": "b3_label_with", "decoder": dec, "relations": 10, "embed": 10,
                "epochs": 10, "rows": nrows, "n_gold": gi.n_gold,
                "n_assessable": int(gi.n_assessable)}
        for mode in ("encoder", "decoder", "joint"):
            eng.label_with = mode
            res = eng.cluster_metrics(ds, gi, 0, nrows)
            line["label_with_" + mode] = {"f1": res.f1, "precision": res.precision, "recall": res.recall,
                          "clusters_used": int((np.asarray(res.sizes) > 0).sum())}
        eng.label_with = "encoder"
        emit(line)
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relation_scores_bench.json"),
                    help="the JSON lines are also written to this file")
    ap.add_argument("--examples", type=int, default=1000000,
                    help="examples of the synthetic split (entities = examples / 5)")
    ap.add_argument("--rows", type=int, default=16384)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge
    ge.build()
    from rae import _lib
    assert torch.cuda.is_available(), "relation_bench needs a GPU"
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

    for dec, r, m in CASES:
        bench_scores(torch, dev, lib, dec, r, m, emit)
    bench_b3(torch, dev, emit)
    bench_engine(torch, dev, args.examples, args.rows, emit)


if __name__ == "__main__":
    main()
