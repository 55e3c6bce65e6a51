#!/usr/bin/env python
"""Relation feature profiles: rae_feature_topk and rae_feature_support on their own.

One JSON line.  HIP events around each call, 2 warm-ups, median of 5, all in one run.
  copy_GBs           rae_stream_copy (1 GiB read + 1 GiB written), measured first
  topk               rae_feature_topk on a standard-normal W at the C3 shape (d = the feature space
                     of the synthetic split below, m = 100) and the C4 shape (2^20 x 300), at top
                     1 / 10 / 32, centred and raw, every feature eligible; and at top 10 with a
                     support filter that keeps about a fifth of the features ("filtered").  Per
                     case: us, W_GBs (bytes of W once per second), frac_of_copy (W_GBs over
                     copy_GBs: a centred call reads W twice, so 0.5 is the copy rate there),
                     torch_us and torch_over_rae for the torch path
                     (W - W.double().mean(1, keepdim=True)).float() (raw: W), ineligible rows set
                     to -inf, .topk(top, dim=0); the two paths' scores are compared first
  parts              at top 10: the row-statistics pass alone (a centred call minus a raw one)
  support            rae_feature_support over the synthetic split (N rows, d = 2^17, about 14
                     entries per row) beside rae_label(probs=None, m = 100) over the same rows:
                     "uniform" as generated, "hot" with one more feature stored in every row

    python tools/feature_bench.py [--rows 1000000] [--out profiles/feature_topk_bench.json]
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

D_C3, M_C3 = 2 ** 17, 100
D_C4, M_C4 = 2 ** 20, 300
TOPS = (1, 10, 32)


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


def bench_topk(torch, dev, lib, st, d, m, copy_gbs):
    from rae import _lib
    g = torch.Generator(device=dev)
    g.manual_seed(d + m)
    W = torch.randn((d, m), generator=g, device=dev)
    # a Zipf-like support: about a fifth of the features have at least 5 rows
    sup = torch.floor(1.0 / torch.rand(d, generator=g, device=dev).clamp_min(1e-6)).clamp_max(1e6)
    sup = sup.to(torch.int32)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
    sp_ = C.c_void_p(st.cuda_stream)
    feats = torch.empty((m, 32), dtype=torch.int32, device=dev)
    scores = torch.empty((m, 32), dtype=torch.float32, device=dev)
    a = _lib.RaeFtopkArgs()
    a.W, a.n_features, a.relations, a.ldw = P(W), d, m, m
    a.centre, a.top = 1, 32
    ws = torch.empty(int(lib.rae_feature_topk_workspace_bytes(C.byref(a))), dtype=torch.uint8,
                     device=dev)
    a.workspace, a.workspace_bytes = P(ws), ws.numel()
    a.feats_out, a.scores_out = P(feats), P(scores)
    nbytes = 4.0 * d * m
    out = {"d": d, "m": m, "W_bytes": nbytes, "eligible_fraction_filtered": float((sup >= 5).float().mean()),
           "cases": {}}

    def case(centre, top, filtered):
        a.centre, a.top = centre, top
        a.support, a.min_support = (P(sup), 5) if filtered else (None, 0)

        def rae():
            _lib.check(lib.rae_feature_topk(C.byref(a), sp_), "rae_feature_topk")

        def ref():
            s = (W - W.double().mean(1, keepdim=True)).float() if centre else W.clone()
            if filtered:
                s[sup < 5] = -float("inf")
            return s.topk(top, dim=0)

        rae()
        want = ref().values.t()
        got = scores.reshape(-1)[:m * top].reshape(m, top)
        # the torch path sums the row in another order: the scores agree to fp32 rounding
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-5), (centre, top, filtered)
        us = event_us(torch, st, rae)
        tus = event_us(torch, st, ref)
        gbs = nbytes / (us * 1e-6) / 1e9
        return {"us": us, "W_GBs": gbs, "frac_of_copy": gbs / copy_gbs, "torch_us": tus,
                "torch_over_rae": tus / us}

    for centre in (1, 0):
        for top in TOPS:
            out["cases"][f"{'centred' if centre else 'raw'}_top{top}"] = case(centre, top, False)
        out["cases"][f"{'centred' if centre else 'raw'}_top10_filtered"] = case(centre, 10, True)
    c = out["cases"]
    out["parts"] = {"rowstat_us_top10": c["centred_top10"]["us"] - c["raw_top10"]["us"],
                    "one_pass_at_copy_rate_us": nbytes / (copy_gbs * 1e9) * 1e6}
    return out


def bench_support(torch, dev, lib, st, rows):
    from rae import _lib
    from rae.data import synthetic_dataset
    from rae.engine import DeviceSplit
    from rae.evaluation import feature_support
    data, _ = synthetic_dataset(rows, D_C3, 40, seed=1234)
    tr = data.split["train"]
    X = tr.xFeats.tocsr()
    n = X.shape[0]
    hot = (X + sp.csr_matrix((np.ones(n, np.float32), (np.arange(n), np.full(n, 4321))),
                             shape=X.shape)).tocsr()
    hot.data[:] = 1.0
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    W = torch.randn((D_C3, M_C3), generator=g, device=dev) * 0.1
    Wb = torch.zeros(M_C3, device=dev)
    lab = torch.empty(n, dtype=torch.int64, device=dev)
    sup = torch.empty(D_C3, dtype=torch.int32, device=dev)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
    sp_ = C.c_void_p(st.cuda_stream)
    out = {"rows": n, "d": D_C3}

    class _S:                                                 # what DeviceSplit reads
        def __init__(self, x):
            self.xFeats, self.args1, self.args2 = x, tr.args1, tr.args2

    for name, x in (("uniform", X), ("hot", hot)):
        ds = DeviceSplit(_S(x), dev)

        def support():
            _lib.check(lib.rae_feature_support(P(ds.indptr), P(ds.indices), P(ds.values), D_C3, 0, n,
                                               0, P(sup), sp_), "rae_feature_support")

        def label():
            _lib.check(lib.rae_label(P(ds.indptr), P(ds.indices), P(ds.values), P(W), P(Wb), M_C3, 0,
                                     n, P(lab), None, sp_), "rae_label")

        support()
        want = feature_support(x)
        assert np.array_equal(sup.cpu().numpy(), want), name
        s_us, l_us = event_us(torch, st, support), event_us(torch, st, label)
        nnz = int(x.nnz)
        out[name] = {"nnz": nnz, "max_support": int(want.max()), "support_us": s_us,
                     "support_GBs": 4.0 * nnz / (s_us * 1e-6) / 1e9, "label_us": l_us,
                     "support_over_label": s_us / l_us}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1000000, help="rows of the synthetic split")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge
    ge.build()
    from eval_bench import copy_rate
    from rae import _lib
    assert torch.cuda.is_available(), "feature_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib, st = _lib.load(), torch.cuda.current_stream()
    copy_gbs = copy_rate(lib, torch, dev, st)
    line = {"copy_GBs": copy_gbs,
            "topk": {"C3": bench_topk(torch, dev, lib, st, D_C3, M_C3, copy_gbs),
                     "C4": bench_topk(torch, dev, lib, st, D_C4, M_C4, copy_gbs)},
            "support": bench_support(torch, dev, lib, st, args.rows),
            "how": "HIP events around each call, 2 warm-ups, median of 5; W standard normal; "
                   "frac_of_copy = bytes of W once / time / copy_GBs (read + written bytes of "
                   "rae_stream_copy)"}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
