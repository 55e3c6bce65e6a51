#!/usr/bin/env python
"""Throughput of the forward-only objective (rae_eval_cost) against the training forward phase.

For the C2, C3 and C5 shapes (synthetic datasets, bench.py's CONFIGS K / embed / neg / decoder)
one JSON line each:
  eval_ex_per_s          examples per second of rae_eval_cost over the whole train split (HIP
                         events around the call, 3 warm-ups, median of 10)
  bytes_per_example      algorithmic bytes: CSR ids, W rows, A rows, Ab, entity / negative ids,
                         the three terms
  frac_of_measured_copy  eval_ex_per_s * bytes_per_example over the rae_stream_copy rate measured
                         in this process
  mfma_tflops            RESCAL: (2 r^2 m + 4 r^2) flops per example at that rate
  train_fwd_ex_per_s     l / (the forward phase of a training step at the same shape, l = 100,
                         rae_time_next on rae_step_forward, median of 10 steps)
  meets_criterion        eval_ex_per_s >= train_fwd_ex_per_s

    python tools/eval_bench.py [--out profiles/eval_cost_bench.json] [--shapes c2,c3,c5]
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

# K / embed / neg / decoder of BASELINE's configs 2, 3 and 5; N sized for a few-second run
SHAPES = {
    "c2": dict(N=100_000, d=2 ** 17, m=30, r=100, s=10, dec="sp", ntrue=30, bf16=False),
    "c3": dict(N=200_000, d=2 ** 17, m=100, r=200, s=20, dec="sp", ntrue=100, bf16=False),
    "c5": dict(N=100_000, d=2 ** 17, m=100, r=200, s=20, dec="rescal", ntrue=100, bf16=True),
}
L = 100


def copy_rate(lib, torch, dev, st):
    """GB/s of rae_stream_copy (1 GiB read + 1 GiB written, median of 7)."""
    nbytes = 1 << 30
    src = torch.ones(nbytes // 4, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    sp_ = C.c_void_p(st.cuda_stream)

    def go():
        assert lib.rae_stream_copy(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), nbytes,
                                   sp_) == 0, lib.rae_last_error()
    go()
    torch.cuda.synchronize()
    ev = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(2)) for _ in range(7)]
    for a, b in ev:
        a.record(st)
        go()
        b.record(st)
    torch.cuda.synchronize()
    ms = float(np.median([a.elapsed_time(b) for a, b in ev]))
    return 2 * nbytes / (ms * 1e-3) / 1e9


def train_forward_us(eng, torch, steps=10, warm=3):
    """Median span of the forward phase of a training step (rae_time_next), eager steps."""
    lib, plan = eng.lib, eng.plan
    sp_ = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = min(steps + warm, eng.nb, eng.index_window)
    eng.build_index(0, n)
    eng.set_cursor(0)
    evs = []
    for i in range(n):
        a, b = C.c_void_p(), C.c_void_p()
        assert lib.rae_event_create(C.byref(a)) == 0 and lib.rae_event_create(C.byref(b)) == 0
        assert lib.rae_time_next(plan, a, b) == 0, lib.rae_last_error()
        assert lib.rae_step_forward(plan, i, sp_) == 0, lib.rae_last_error()
        assert lib.rae_step_update(plan, i, sp_) == 0, lib.rae_last_error()
        evs.append((a, b))
    torch.cuda.synchronize()
    eng.check()
    eng.cursor_moved()
    ms = []
    for a, b in evs:
        v = C.c_float()
        assert lib.rae_event_elapsed_ms(a, b, C.byref(v)) == 0, lib.rae_last_error()
        ms.append(v.value)
        lib.rae_event_destroy(a)
        lib.rae_event_destroy(b)
    return float(np.median(ms[warm:]) * 1e3)


def run_shape(name, cfg, torch, dev, copy_gbs):
    from rae.data import synthetic_dataset
    from rae.inducer import ReconstructInducer
    data, gold = synthetic_dataset(cfg["N"], cfg["d"], cfg["ntrue"], seed=1234)
    m, r, s, dec = cfg["m"], cfg["r"], cfg["s"], cfg["dec"]
    ind = ReconstructInducer(data, gold, np.random.RandomState(2), 1, 0.1, L, r, m, s, 0.0, 0.0,
                             "adagrad", "evalbench", dec, False, True, False, 1.0, device=dev,
                             neg_sampler="philox", mfma_bf16=cfg["bf16"])
    ind.compile_function()
    eng = ind.engine
    st = torch.cuda.current_stream()
    eng.sample_epoch_negatives(ind.negativeSampler, "philox", 0, 0)
    fwd_us = train_forward_us(eng, torch)
    split = eng.split
    N = split.N
    n1, n2 = eng.eval_negatives(split, ind.negativeSampler)
    ev = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(2)) for _ in range(13)]
    for a, b in ev:
        a.record(st)
        eng.queue_evaluate(split, 0, N, n1, n2)
        b.record(st)
    torch.cuda.synchronize()
    ms = float(np.median([a.elapsed_time(b) for a, b in ev[3:]]))
    res = eng.evaluate(split)
    assert np.isfinite(res.cost)
    f = float(split.indptr_np[-1]) / N
    vals = 0 if split.values is None else 4 * f
    arows = (1 + 2 * s) if dec == "sp" else (2 + 2 * s)
    bpe = 4 * (f + 1) + vals + 4 * f * m + 4 * r * arows + 4 * (2 + 2 * s) + 8 + 8 * s + 12
    eps = N / (ms * 1e-3)
    tps = L / (fwd_us * 1e-6)
    out = {"shape": name, "decoder": dec, "N": N, "relations": m, "embed": r, "neg_samples": s,
           "mean_features": f, "eval_ms": ms, "eval_ex_per_s": eps, "bytes_per_example": bpe,
           "eval_GBs": eps * bpe / 1e9, "measured_copy_GBs": copy_gbs,
           "frac_of_measured_copy": eps * bpe / 1e9 / copy_gbs,
           "train_fwd_us": fwd_us, "train_fwd_batch": L, "train_fwd_bf16": bool(cfg["bf16"]),
           "train_fwd_ex_per_s": tps, "eval_over_train_fwd": eps / tps,
           "meets_criterion": bool(eps >= tps), "objective": res.cost,
           "how": "HIP events around rae_eval_cost over the train split, 3 warm-ups, median of "
                  "10; training forward: rae_time_next on rae_step_forward, median of 10 steps"}
    if dec != "sp":
        out["mfma_tflops"] = eps * (2.0 * r * r * m + 4.0 * r * r) / 1e12
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="c2,c3,c5")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge
    ge.build()
    from rae import _lib
    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _lib.load()
    copy_gbs = copy_rate(lib, torch, dev, torch.cuda.current_stream())
    lines = []
    for name in args.shapes.split(","):
        res = run_shape(name, SHAPES[name], torch, dev, copy_gbs)
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
