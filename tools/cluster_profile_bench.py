#!/usr/bin/env python
"""Per-cluster trigger profiles of one split: the host path against the device path.

For synthetic datasets of N = 1,000,000 and 100,000 examples (K = 100 induced relations, 500
training steps) one JSON line each.  Every example gets one extra "trigger" feature drawn
Zipf(1) over 30,000 features appended to the feature space; KeyIndex.from_mask marks those.
  host_wall_s        the label pass, its download, key_table + topk_from_table and
                     format_cluster_profiles (host clock, 1 warm-up, median of 3);
                     host_row_keys_s is the one-off row_keys over the split
  device_wall_s      TrainEngine.cluster_profiles (label -> key count -> top-k and the one
                     read-back) and format_cluster_profiles (host clock, 3 warm-ups, median of 10)
  row_keys_us        HIP events around rae_row_keys over the split (the one-off)
  label_us           HIP events around rae_label(probs=None) over the same rows
  keycount_us / topk_us
                     HIP events around rae_cluster_key_count (with its table-zeroing launch) and
                     rae_cluster_topk on the trained labels; zero_us the zeroing alone
                     (a call with nrows = 0)
  cases              the count kernel alone per input: "trained" (the labels above), "uniform"
                     (uniform labels and keys) and "one-cluster" (every row in cluster 0, Zipf
                     keys: the worst skew) -- at the split's rows, and tiled to 2^25 rows (403 MB,
                     accumulate: no zeroing) for the bandwidth, 12 bytes per row against
                     measured_copy_GBs (rae_stream_copy, read + written bytes); top-k per table
  variant            with --variant-lib (a build with -DRAE_CK_AGG=0: no LDS aggregation, only a
                     wave instruction whose lanes all agree is merged), the same count calls
                     through it, timed in the same process right after the product build's
The two paths' text is compared before anything is reported.

    python tools/cluster_profile_bench.py [--out profiles/cluster_profile_bench.json]
                                          [--sizes 1000000,100000] [--variant-lib PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "relation-autoencoder_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

M, R, S, L, NTRUE = 100, 30, 5, 100, 40
D, NKEYS, TOP = 2 ** 17, 30000, 5
TRAIN_STEPS = 500


def zipf(g, n, size):
    w = 1.0 / np.arange(1, n + 1, dtype=np.float64)
    cdf = np.cumsum(w)
    cdf /= cdf[-1]
    return np.searchsorted(cdf, g.random_sample(size), side="right").clip(0, n - 1)


def keyed_dataset(N):
    """synthetic_dataset(N) with one Zipf-drawn trigger column per row appended (d + NKEYS
    features); the trigger ranks are shuffled over the columns, as a lexicon's are."""
    from rae.data import DatasetManager, synthetic_dataset
    data, gold = synthetic_dataset(N, D, NTRUE, seed=1234)
    tr = data.split["train"]
    g = np.random.RandomState(77)
    col = D + g.permutation(NKEYS)[zipf(g, NKEYS, tr.xFeats.shape[0])]
    extra = sp.csr_matrix((np.ones(len(col), np.float32), (np.arange(len(col)), col)),
                          shape=(len(col), D + NKEYS))
    X = sp.hstack([tr.xFeats, sp.csr_matrix((len(col), NKEYS), dtype=np.float32)],
                  format="csr") + extra
    out = DatasetManager.from_arrays(X.tocsr(), tr.args1, tr.args2,
                                     n_entities=data.get_arg_voc_size(), n_features=D + NKEYS)
    return out, gold


def run_size(N, torch, dev, copy_gbs, variant):
    from cluster_eval_bench import event_us, wall_s
    from rae import _lib
    from rae.evaluation import (KeyIndex, format_cluster_profiles, key_table, row_keys,
                                topk_from_table)
    from rae.inducer import ReconstructInducer
    import time
    data, gold = keyed_dataset(N)
    print(f"[N={N}] dataset ready", file=sys.stderr, flush=True)
    ind = ReconstructInducer(data, gold, np.random.RandomState(2), 1, 0.1, L, R, M, S, 0.0, 0.0,
                             "adagrad", "profilebench", "sp", False, True, False, 1.0,
                             device=dev, neg_sampler="philox")
    ind.compile_function()
    eng, lib = ind.engine, ind.engine.lib
    eng.sample_epoch_negatives(ind.negativeSampler, "philox", 0, 0)
    eng.run(0, min(TRAIN_STEPS, eng.nb))
    torch.cuda.synchronize()
    eng.check()
    split = eng.split
    rows = (split.N // L) * L
    mask = np.zeros(D + NKEYS, bool)
    mask[D:] = True
    ki = KeyIndex.from_mask(mask)
    X = data.split["train"].xFeats
    t0 = time.perf_counter()
    host_keys = row_keys(X, ki.key_of_feature)
    host_row_keys_s = time.perf_counter() - t0
    text = {}

    def host():
        table = key_table(ind._labels("train"), host_keys[:rows], M, ki.n_keys)
        k, c = topk_from_table(table, TOP)
        text["host"] = format_cluster_profiles(k, c, ki.names)

    def device():
        res = eng.cluster_profiles(split, ki, 0, rows, TOP)
        text["device"] = format_cluster_profiles(res.keys, res.counts, ki.names)

    print(f"[N={N}] trained, host keys in {host_row_keys_s:.2f} s", file=sys.stderr, flush=True)
    host_s, host_all = wall_s(host, 1, 3)
    dev_s, dev_all = wall_s(device, 3, 10)
    print(f"[N={N}] host {host_s:.4f} s, device {dev_s:.6f} s", file=sys.stderr, flush=True)
    assert text["host"] == text["device"], "the two paths print different profiles"
    # the calls alone, on the buffers the engine's path uses
    st = torch.cuda.current_stream()
    sp_ = C.c_void_p(st.cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    keys_d = eng._keys_dev(split, ki)
    assert np.array_equal(keys_d[:split.N].cpu().numpy(), host_keys)
    kof_d = torch.as_tensor(ki.key_of_feature, device=dev)
    scratch_keys = torch.empty_like(keys_d)
    lab, tb, out = eng._cl_labels, eng._pf_table, eng._pf_out
    W, Wb = eng.model.params[0], eng.model.params[1]
    vals = P(split.values) if split.values is not None else None

    def rowkeys():
        _lib.check(lib.rae_row_keys(P(split.indptr), P(split.indices), vals, P(kof_d), split.d, 0,
                                    split.N, P(scratch_keys), sp_), "rae_row_keys")

    def label():
        _lib.check(lib.rae_label(P(split.indptr), P(split.indices), vals, P(W), P(Wb), M, 0, rows,
                                 P(lab), None, sp_), "rae_label")

    def count(which, labels, keys, n, acc=0):
        def go():
            _lib.check(which.rae_cluster_key_count(P(labels), P(keys), n, M, ki.n_keys, acc, P(tb),
                                                   sp_), "rae_cluster_key_count")
        return go

    def topk():
        _lib.check(lib.rae_cluster_topk(P(tb), M, ki.n_keys, ki.n_keys, TOP, P(out),
                                        C.c_void_p(out.data_ptr() + 4 * M * _lib.RAE_TOPK_MAX),
                                        sp_), "rae_cluster_topk")

    row_keys_us = event_us(torch, st, rowkeys)
    label_us = event_us(torch, st, label)                   # leaves the trained labels in lab
    g = np.random.RandomState(5)
    inputs = {
        "trained": (lab[:rows], keys_d[:rows]),
        "uniform": (torch.as_tensor(g.randint(0, M, rows).astype(np.int64), device=dev),
                    torch.as_tensor(g.randint(0, NKEYS, rows).astype(np.int32), device=dev)),
        "one-cluster": (torch.zeros(rows, dtype=torch.int64, device=dev),
                        torch.as_tensor(zipf(g, NKEYS, rows).astype(np.int32), device=dev)),
    }
    big = 1 << 25
    reps = -(-big // rows)
    cases = {}
    for name, (lb, ky) in inputs.items():
        lb_big = lb.repeat(reps)[:big].contiguous()
        ky_big = ky.repeat(reps)[:big].contiguous()
        c = {}
        for tag, which in (("", lib), ("variant_", variant)):
            if which is None:
                continue
            us = event_us(torch, st, count(which, lb, ky, rows))
            count(which, lb, ky, rows)()
            torch.cuda.synchronize()
            table = tb[:M * ki.n_keys].cpu().numpy()
            want = key_table(lb.cpu().numpy(), ky.cpu().numpy(), M, ki.n_keys).reshape(-1)
            assert np.array_equal(table, want), (name, tag)
            big_us = event_us(torch, st, count(which, lb_big, ky_big, big, acc=1), warm=1, reps=5)
            c[tag + "keycount_us"] = us
            c[tag + "keycount_GBs"] = 12.0 * rows / (us * 1e-6) / 1e9
            c[tag + "stream_keycount_us"] = big_us
            c[tag + "stream_keycount_GBs"] = 12.0 * big / (big_us * 1e-6) / 1e9
            c[tag + "stream_keycount_frac_of_copy"] = c[tag + "stream_keycount_GBs"] / copy_gbs
        count(lib, lb, ky, rows)()
        c["max_cell"] = int(tb[:M * ki.n_keys].max())
        c["topk_us"] = event_us(torch, st, topk)
        cases[name] = c
    zero_us = event_us(torch, st, count(lib, lab, keys_d, 0))
    tr = cases["trained"]
    line = {"N": split.N, "rows": rows, "relations": M, "n_keys": ki.n_keys, "top": TOP,
            "train_steps": min(TRAIN_STEPS, eng.nb),
            "nonempty_clusters": int(sum(1 for ln in text["device"] if "(" in ln)),
            "host_wall_s": host_s, "host_wall_all_s": host_all, "host_row_keys_s": host_row_keys_s,
            "device_wall_s": dev_s, "device_wall_all_s": dev_all,
            "host_over_device": host_s / dev_s,
            "row_keys_us": row_keys_us, "label_us": label_us, "zero_us": zero_us,
            "keycount_us": tr["keycount_us"], "topk_us": tr["topk_us"],
            "keycount_over_label": tr["keycount_us"] / label_us,
            "topk_over_label": tr["topk_us"] / label_us,
            "table_bytes": 4 * M * ki.n_keys, "count_bytes": 12.0 * rows,
            "stream_rows": big, "measured_copy_GBs": copy_gbs, "cases": cases,
            "variant": None if variant is None else "RAE_CK_AGG=0",
            "how": "host: host clock around the label download + key_table + topk_from_table + "
                   "format, 1 warm-up, median of 3; device: host clock around cluster_profiles "
                   "(ends in the read-back) + format, 3 warm-ups, median of 10; kernels: HIP "
                   "events around each call, 3 warm-ups, median of 10 (the 2^25-row stream: 1 "
                   "warm-up, median of 5, accumulating so nothing is zeroed)"}
    eng.close()
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="1000000,100000")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--variant-lib", default=None,
                    help="a second build of the library whose key count is timed beside the product's")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge
    ge.build()
    from eval_bench import copy_rate
    from rae import _lib
    assert torch.cuda.is_available(), "cluster_profile_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    variant = _lib.load(args.variant_lib) if args.variant_lib else None
    if variant is not None:
        variant.rae_cluster_key_count.argtypes = _lib.load().rae_cluster_key_count.argtypes
    copy_gbs = copy_rate(_lib.load(), torch, dev, torch.cuda.current_stream())
    lines = []
    for n in args.sizes.split(","):
        line = json.dumps(run_size(int(n), torch, dev, copy_gbs, variant))
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
