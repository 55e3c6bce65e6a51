#!/usr/bin/env python
"""Cluster exemplars: rae_label_stats and rae_cluster_exemplars on their own, and the path they
replace.

One JSON line, on the synthetic split of N = 1,000,000 rows at the C3 shape (K = 100 induced
relations) after 500 training steps.  HIP events around each call, 2 warm-ups, median of 5, all in
one run.
  copy_GBs           rae_stream_copy (1 GiB read + 1 GiB written), measured first
  label              (a) rae_label_stats (labels, margin, pmax) beside rae_label(probs = NULL) on
                     the same rows: both times, stats_over_label their ratio, and the two calls
                     timed a second time in the other order (the label pass's own run-to-run spread)
  exemplars          (b) rae_cluster_exemplars at top 1 / 5 / 32, highest first, on three inputs:
                     "trained" (the trained labels and their margins), "uniform" (uniform labels,
                     standard-normal scores) and "one-cluster-ascending" (every row in cluster 0
                     with ascending scores: every row is admitted, the slow case).  Per case: us,
                     GBs (12 bytes per row per second) and frac_of_copy; count_us is
                     rae_cluster_count (no gold standard) on the same labels; the result is
                     compared with the numpy oracle first
  today              (c) the path that exists today: rae_label(probs), torch gather of pmax, a sort
                     by (label, -pmax) and the first `top` rows per cluster -- today_us beside
                     label_stats + exemplars by pmax (rae_us), today_over_rae their ratio; the two
                     paths' rows are compared first (ties in pmax: by row, both paths)

    python tools/exemplar_bench.py [--rows 1000000] [--out profiles/exemplar_bench.json]
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

M, R, S, L, NTRUE = 100, 30, 5, 100, 40
D = 2 ** 17
TRAIN_STEPS = 500
TOPS = (1, 5, 32)


def run(N, torch, dev, copy_gbs):
    from feature_bench import event_us
    from rae import _lib
    from rae.data import synthetic_dataset
    from rae.evaluation import cluster_exemplars
    from rae.inducer import ReconstructInducer
    data, gold = synthetic_dataset(N, D, NTRUE, seed=1234)
    ind = ReconstructInducer(data, gold, np.random.RandomState(2), 1, 0.1, L, R, M, S, 0.0, 0.0,
                             "adagrad", "exemplarbench", "sp", False, True, False, 1.0,
                             device=dev, neg_sampler="philox")
    ind.compile_function()
    eng, lib = ind.engine, ind.engine.lib
    eng.sample_epoch_negatives(ind.negativeSampler, "philox", 0, 0)
    eng.run(0, min(TRAIN_STEPS, eng.nb))
    torch.cuda.synchronize()
    eng.check()
    split = eng.split
    rows = (split.N // L) * L
    print(f"[N={N}] trained", file=sys.stderr, flush=True)
    st = torch.cuda.current_stream()
    sp_ = C.c_void_p(st.cuda_stream)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
    W, Wb = eng.model.params[0], eng.model.params[1]
    lab = torch.empty(rows, dtype=torch.int64, device=dev)
    lab2 = torch.empty(rows, dtype=torch.int64, device=dev)
    margin = torch.empty(rows, dtype=torch.float32, device=dev)
    pmax = torch.empty(rows, dtype=torch.float32, device=dev)
    probs = torch.empty((rows, M), dtype=torch.float32, device=dev)

    def label(pr=None, out=lab2):
        _lib.check(lib.rae_label(P(split.indptr), P(split.indices), P(split.values), P(W), P(Wb), M,
                                 0, rows, P(out), P(pr), sp_), "rae_label")

    def stats():
        _lib.check(lib.rae_label_stats(P(split.indptr), P(split.indices), P(split.values), P(W),
                                       P(Wb), M, 0, rows, P(lab), P(margin), P(pmax), sp_),
                   "rae_label_stats")

    # (a)
    label_us = event_us(torch, st, label)
    stats_us = event_us(torch, st, stats)
    stats_us_2 = event_us(torch, st, stats)
    label_us_2 = event_us(torch, st, label)
    assert torch.equal(lab, lab2)
    line = {"N": split.N, "rows": rows, "relations": M, "train_steps": min(TRAIN_STEPS, eng.nb),
            "measured_copy_GBs": copy_gbs,
            "nonempty_clusters": int((torch.bincount(lab, minlength=M) > 0).sum()),
            "margin_zero_rows": int((margin == 0).sum()), "pmax_one_rows": int((pmax == 1).sum()),
            "label": {"label_us": label_us, "stats_us": stats_us, "label_us_again": label_us_2,
                      "stats_us_again": stats_us_2, "stats_over_label": stats_us / label_us,
                      "stats_over_label_again": stats_us_2 / label_us_2}}
    # (b)
    a = _lib.RaeExemplarArgs()
    a.nrows, a.relations, a.top, a.largest = rows, M, 32, 1
    ws = torch.empty(int(lib.rae_cluster_exemplars_workspace_bytes(C.byref(a))), dtype=torch.uint8,
                     device=dev)
    ro = torch.empty((M, 32), dtype=torch.int32, device=dev)
    so = torch.empty((M, 32), dtype=torch.float32, device=dev)
    a.workspace, a.workspace_bytes = P(ws), ws.numel()
    a.rows_out, a.scores_out = P(ro), P(so)
    table = torch.zeros(M, dtype=torch.int64, device=dev)
    nogold = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    inputs = {
        "trained": (lab, margin),
        "uniform": (torch.randint(0, M, (rows,), generator=g, device=dev),
                    torch.randn(rows, generator=g, device=dev)),
        "one-cluster-ascending": (torch.zeros(rows, dtype=torch.int64, device=dev),
                                  torch.arange(rows, dtype=torch.float32, device=dev)),
    }
    cases = {}
    for name, (lb, sc) in inputs.items():
        a.labels, a.scores = P(lb), P(sc)

        def exemplars():
            _lib.check(lib.rae_cluster_exemplars(C.byref(a), sp_), "rae_cluster_exemplars")

        def count():
            _lib.check(lib.rae_cluster_count(P(lb), P(nogold), rows, M, 0, 0, P(table), sp_),
                       "rae_cluster_count")

        c = {"count_us": event_us(torch, st, count)}
        lbh, sch = lb.cpu().numpy(), sc.cpu().numpy()
        for top in TOPS:
            a.top = top
            ro.fill_(-9)
            exemplars()
            torch.cuda.synchronize()
            wr, wo = cluster_exemplars(lbh, sch, M, top)
            assert np.array_equal(ro.view(-1)[:M * top].view(M, top).cpu().numpy(), wr), (name, top)
            assert np.array_equal(so.view(-1)[:M * top].view(M, top).cpu().numpy(), wo), (name, top)
            us = event_us(torch, st, exemplars)
            gbs = 12.0 * rows / (us * 1e-6) / 1e9
            c[f"top{top}"] = {"us": us, "GBs": gbs, "frac_of_copy": gbs / copy_gbs,
                              "over_count": us / c["count_us"]}
        cases[name] = c
        print(f"[N={N}] {name}: {c}", file=sys.stderr, flush=True)
    line["exemplars"] = cases
    # (c)
    top = 5
    a.labels, a.scores, a.top = P(lab), P(pmax), top
    ar = torch.arange(rows, device=dev)

    def today():
        label(probs, lab2)
        pm = probs.gather(1, lab2[:, None])[:, 0]
        # by (label, -pmax, row): a stable sort by -pmax, then a stable sort by label
        o1 = torch.sort(-pm, stable=True).indices
        o2 = o1[torch.sort(lab2[o1], stable=True).indices]
        sl = lab2[o2]
        start = torch.searchsorted(sl, torch.arange(M, device=dev))
        rank = ar - start[sl]
        keep = rank < top
        out = torch.full((M, top), -1, dtype=torch.int64, device=dev)
        out[sl[keep], rank[keep]] = o2[keep]
        return out

    def rae():
        stats()
        _lib.check(lib.rae_cluster_exemplars(C.byref(a), sp_), "rae_cluster_exemplars")

    want = today()
    rae()
    torch.cuda.synchronize()
    got = ro.view(-1)[:M * top].view(M, top).to(torch.int64)
    assert torch.equal(got, want), "the two paths pick different rows"
    today_us = event_us(torch, st, today)
    rae_us = event_us(torch, st, rae)
    line["today"] = {"top": top, "today_us": today_us, "rae_us": rae_us,
                     "today_over_rae": today_us / rae_us, "probs_bytes": 4.0 * rows * M}
    line["how"] = ("HIP events around each call on the current stream, 2 warm-ups, median of 5, one "
                   "run; (c) today = rae_label(probs) + gather + two stable torch sorts + scatter, "
                   "rae = rae_label_stats + rae_cluster_exemplars by pmax at top 5")
    eng.close()
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge
    ge.build()
    from eval_bench import copy_rate
    from rae import _lib
    assert torch.cuda.is_available(), "exemplar_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    copy_gbs = copy_rate(_lib.load(), torch, dev, torch.cuda.current_stream())
    line = json.dumps(run(args.rows, torch, dev, copy_gbs))
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
