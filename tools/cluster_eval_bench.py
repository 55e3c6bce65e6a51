#!/usr/bin/env python
"""Cluster evaluation of one split: the host path against the device path.

For synthetic datasets of N = 1,000,000 and 100,000 examples (K = 100 induced relations, 40
planted gold classes, 2 % of the examples gold-labelled) one JSON line each:
  host_wall_s            get_clusters_sets + _evaluate as learn() runs them with
                         cluster_eval="host": the label pass, its download, the Python sets and
                         SingleLabelClusterEvaluation (host clock, 1 warm-up, median of 3)
  device_wall_s          TrainEngine.cluster_metrics: label -> count -> metrics and the one
                         read-back (host clock around the call, which ends in the blocking copy;
                         3 warm-ups, median of 10)
  label_us               HIP events around rae_label(probs=None) over the same rows
  count_lds_us / count_global_us
                         HIP events around rae_cluster_count, per form (3 warm-ups, median of 10)
  b3_us                  HIP events around rae_b3_metrics
  count_GBs_*            12 bytes per example over the count time, next to measured_copy_GBs
                         (rae_stream_copy, read + written bytes, as bench.py measures its ceiling)
  stream_count_GBs_*     the count kernel alone on a long stream: the split's labels and gold ids
                         tiled to 2^25 rows (403 MB), so the launch does not dominate the time
  meets_criterion        device_wall_s < host_wall_s (the acceptance condition at N = 1,000,000)
The two paths' (f1, precision, recall) are compared (rel 1e-12) before anything is reported.

    python tools/cluster_eval_bench.py [--out profiles/cluster_eval_bench.json] [--sizes 1000000,100000]
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

M, R, S, L, NTRUE = 100, 30, 5, 100, 40
TRAIN_STEPS = 500            # a short run off the initial weights, so the clusters are uneven


def event_us(torch, st, fn, warm=3, reps=10):
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


def wall_s(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [float(t) for t in ts]


def run_size(N, torch, dev, copy_gbs):
    from rae import _lib
    from rae.data import synthetic_dataset
    from rae.evaluation import GoldIndex
    from rae.inducer import ReconstructInducer
    data, gold = synthetic_dataset(N, 2 ** 17, NTRUE, seed=1234)
    ind = ReconstructInducer(data, gold, np.random.RandomState(2), 1, 0.1, L, R, M, S, 0.0, 0.0,
                             "adagrad", "clusterbench", "sp", False, True, False, 1.0, device=dev,
                             neg_sampler="philox")
    ind.compile_function()
    eng, lib = ind.engine, ind.engine.lib
    eng.sample_epoch_negatives(ind.negativeSampler, "philox", 0, 0)
    eng.run(0, min(TRAIN_STEPS, eng.nb))
    torch.cuda.synchronize()
    eng.check()
    split = eng.split
    rows = (split.N // L) * L
    gi = GoldIndex(gold["train"], split.N)
    host_score = []

    def host():
        ind.cluster["train"] = ind.get_clusters_sets("train")
        host_score.append(ind._evaluate("train", verbose=False))

    def device():
        return eng.cluster_metrics(split, gi, 0, rows)

    host_s, host_all = wall_s(host, 1, 3)
    dev_s, dev_all = wall_s(device, 3, 10)
    res = device()
    want = host_score[-1]
    got = (res.f1, res.precision, res.recall)
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got, want)), (got, want)
    # the three calls alone, on the buffers the engine's path uses
    st = torch.cuda.current_stream()
    sp_ = C.c_void_p(st.cuda_stream)
    ids_d, sizes_d = eng._gold_dev(split, gi)
    lab, tb, out = eng._cl_labels, eng._cl_table, eng._cl_out
    W, Wb = eng.model.params[0], eng.model.params[1]
    P = lambda t: C.c_void_p(t.data_ptr())

    def label():
        _lib.check(lib.rae_label(P(split.indptr), P(split.indices),
                                 P(split.values) if split.values is not None else None, P(W), P(Wb),
                                 M, 0, rows, P(lab), None, sp_), "rae_label")

    def count(form):
        def go():
            _lib.check(lib.rae_cluster_count(P(lab), P(ids_d), rows, M, gi.n_gold, form, P(tb), sp_),
                       "rae_cluster_count")
        return go

    def b3():
        _lib.check(lib.rae_b3_metrics(P(tb), P(sizes_d), gi.n_assessable, M, gi.n_gold, P(out),
                                      C.c_void_p(out.data_ptr() + 32), sp_), "rae_b3_metrics")

    label_us = event_us(torch, st, label)
    lds_us = event_us(torch, st, count(_lib.RAE_CCOUNT_LDS))
    glb_us = event_us(torch, st, count(_lib.RAE_CCOUNT_GLOBAL))
    b3_us = event_us(torch, st, b3)
    nbytes = 12.0 * rows
    # the same kernel on a stream long enough to time its bandwidth
    big = 1 << 25
    reps = -(-big // rows)
    lab_big = lab[:rows].repeat(reps)[:big].contiguous()
    ids_big = ids_d[:rows].repeat(reps)[:big].contiguous()

    def count_big(form):
        def go():
            _lib.check(lib.rae_cluster_count(P(lab_big), P(ids_big), big, M, gi.n_gold, form, P(tb),
                                             sp_), "rae_cluster_count")
        return go

    big_lds_us = event_us(torch, st, count_big(_lib.RAE_CCOUNT_LDS))
    big_glb_us = event_us(torch, st, count_big(_lib.RAE_CCOUNT_GLOBAL))
    count(_lib.RAE_CCOUNT_AUTO)()
    line = {"N": split.N, "rows": rows, "relations": M, "n_gold": gi.n_gold,
            "n_assessable": gi.n_assessable, "train_steps": min(TRAIN_STEPS, eng.nb),
            "nonempty_clusters": int((res.sizes > 0).sum()),
            "f1": res.f1, "precision": res.precision, "recall": res.recall,
            "host_wall_s": host_s, "host_wall_all_s": host_all,
            "device_wall_s": dev_s, "device_wall_all_s": dev_all,
            "host_over_device": host_s / dev_s, "meets_criterion": bool(dev_s < host_s),
            "label_us": label_us, "count_lds_us": lds_us, "count_global_us": glb_us,
            "b3_us": b3_us, "count_bytes": nbytes,
            "count_GBs_lds": nbytes / (lds_us * 1e-6) / 1e9,
            "count_GBs_global": nbytes / (glb_us * 1e-6) / 1e9,
            "stream_rows": big, "stream_count_lds_us": big_lds_us,
            "stream_count_global_us": big_glb_us,
            "stream_count_GBs_lds": 12.0 * big / (big_lds_us * 1e-6) / 1e9,
            "stream_count_GBs_global": 12.0 * big / (big_glb_us * 1e-6) / 1e9,
            "stream_count_lds_frac_of_copy": 12.0 * big / (big_lds_us * 1e-6) / 1e9 / copy_gbs,
            "measured_copy_GBs": copy_gbs,
            "count_lds_frac_of_copy": nbytes / (lds_us * 1e-6) / 1e9 / copy_gbs,
            "how": "host: host clock around get_clusters_sets + _evaluate, 1 warm-up, median of "
                   "3; device: host clock around cluster_metrics (ends in the read-back), 3 "
                   "warm-ups, median of 10; kernels: HIP events around each call (they include "
                   "the table-zeroing launch for the count), 3 warm-ups, median of 10"}
    eng.close()
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="1000000,100000")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge
    ge.build()
    from eval_bench import copy_rate
    from rae import _lib
    assert torch.cuda.is_available(), "cluster_eval_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    copy_gbs = copy_rate(_lib.load(), torch, dev, torch.cuda.current_stream())
    lines = []
    for n in args.sizes.split(","):
        line = json.dumps(run_size(int(n), torch, dev, copy_gbs))
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
