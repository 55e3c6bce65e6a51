"""Record what the device-side analysis entry points refuse, and the workspace sizes
rae_feature_topk asks for.

TEST INFRASTRUCTURE ONLY.  The sibling of gen_entry_rejections.py (same method, same helpers) for
the entries that take no rae_eval_args: rae_cluster_count, rae_b3_metrics, rae_row_keys,
rae_cluster_key_count, rae_cluster_topk, rae_feature_support, rae_feature_topk and
rae_feature_topk_workspace_bytes.  Writes tests/golden/analysis_entry_rejections.json, which
tests/test_entry_rejections.py replays.

A case is {"fn", "base", "change"}: the entry's well-formed arguments (made-up aligned addresses),
`base` overriding some of them with other well-formed values, then the changes [name, op, value]
-- one per line, or two where the line pins which of two faults is reported.

Usage:  python oracle/gen_analysis_rejections.py [outfile]
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from gen_entry_rejections import INVALID, ROOT, _fake, _lib_mod, record

OUT = os.path.join(ROOT, "tests", "golden", "analysis_entry_rejections.json")
SIZER = "rae_feature_topk_workspace_bytes"
FTOPK = ("rae_feature_topk", SIZER)

# the well-formed arguments in call order (the stream, last, is always NULL); P = a made-up address
P = object()
ARGS = {
    "rae_cluster_count": dict(labels=P, gold=P, nrows=1000, relations=100, n_gold=40, form=0,
                              table=P),
    "rae_b3_metrics": dict(table=P, gold_sizes=P, n_assessable=900, relations=100, n_gold=40,
                           metrics_out=P, sizes_out=P),
    "rae_row_keys": dict(indptr=P, indices=P, values=P, key_of_feature=P, n_features=5000, row0=0,
                         nrows=1000, keys_out=P),
    "rae_cluster_key_count": dict(labels=P, keys=P, nrows=1000, relations=100, n_keys=481,
                                  accumulate=0, counts=P),
    "rae_cluster_topk": dict(counts=P, relations=100, n_keys=481, ld=481, top=5, keys_out=P,
                             counts_out=P),
    "rae_feature_support": dict(indptr=P, indices=P, values=P, n_features=5000, row0=0,
                                nrows=1000, accumulate=0, support=P),
}
ENTRIES = tuple(ARGS) + FTOPK


def ftopk_args(n_features=5000, relations=100, top=5, centre=1):
    a = _lib_mod().RaeFtopkArgs()
    _fake(a, ("W", "support", "feats_out", "scores_out", "workspace"))
    a.n_features, a.relations, a.ldw, a.top, a.centre = n_features, relations, relations, top, centre
    a.min_support = 2
    return a


def run(lib, case):
    """Make the case's call; returns (return value, rae_last_error() text)."""
    fn = case["fn"]
    if fn in FTOPK:
        a = ftopk_args()
        for k, v in case["base"].items():
            setattr(a, k, v)
        if fn == "rae_feature_topk":
            a.workspace_bytes = int(lib.rae_feature_topk_workspace_bytes(C.byref(a)))
            assert a.workspace_bytes > 0, (case, lib.rae_last_error())
        get, put = (lambda k: getattr(a, k) or 0), (lambda k, v: setattr(a, k, v))
    else:
        d = {k: 0x100000 + 0x10000 * i if v is P else v for i, (k, v) in enumerate(ARGS[fn].items())}
        d.update(case["base"])
        get, put = (lambda k: d[k] or 0), d.__setitem__
    null = False
    for name, op, value in case["change"]:
        if op == "null":                       # the argument struct itself
            null = True
        else:
            put(name, value if op == "set" else get(name) + value)
    if fn == SIZER:
        rc = int(lib.rae_feature_topk_workspace_bytes(None if null else C.byref(a)))
    elif fn == "rae_feature_topk":
        rc = int(lib.rae_feature_topk(None if null else C.byref(a), None))
    else:
        rc = int(getattr(lib, fn)(*d.values(), None))
    return rc, lib.rae_last_error().decode()


# ------------------------------------------------------------------ the cases
def _entry_cases(fn):
    """(base, changes) of one entry: every check alone, then pairs of faults."""
    out = []
    one = lambda name, op, value, **base: out.append((base, [[name, op, value]]))
    two = lambda a, b, **base: out.append((base, [list(a), list(b)]))
    rng = lambda name, *vals: [one(name, "set", v) for v in vals]
    null = lambda *names: [one(n, "set", None) for n in names]
    move = lambda by, *names: [one(n, "add", by) for n in names]
    if fn == "rae_cluster_count":
        null("labels", "gold", "table")
        rng("relations", 0, 513), rng("n_gold", -1, 4096), rng("nrows", -1), rng("form", 3, 0x103)
        move(4, "labels", "table"), move(2, "gold")
        one("form", "set", 1, relations=512, n_gold=40)        # 20992 counters
        one("form", "set", 0x101, nrows=1 << 40)
        two(("labels", "set", None), ("relations", "set", 0))
        two(("table", "set", None), ("gold", "set", None))
        two(("relations", "set", 513), ("n_gold", "set", -1))
        two(("n_gold", "set", 4096), ("table", "add", 4))
        two(("nrows", "set", -1), ("form", "set", 3))
        two(("form", "set", 3), ("labels", "add", 4))
        two(("gold", "add", 2), ("form", "set", 1), relations=512, n_gold=40)
    elif fn == "rae_b3_metrics":
        null("table", "metrics_out", "gold_sizes")
        rng("relations", 0, 513), rng("n_gold", -1, 4096), rng("n_assessable", -1)
        move(4, "table", "gold_sizes", "metrics_out", "sizes_out")
        two(("table", "set", None), ("relations", "set", 0))
        two(("metrics_out", "set", None), ("table", "set", None))
        two(("gold_sizes", "set", None), ("relations", "set", 513))
        two(("gold_sizes", "set", None), ("n_gold", "set", 4096))
        two(("gold_sizes", "set", None), ("n_assessable", "set", -1))
        two(("n_assessable", "set", -1), ("sizes_out", "add", 4))
    elif fn == "rae_row_keys":
        null("indptr", "indices", "key_of_feature", "keys_out")
        rng("n_features", -1, 1 << 31), rng("row0", -1), rng("nrows", -1, 1 << 31)
        move(2, "indptr", "indices", "values", "key_of_feature", "keys_out")
        two(("keys_out", "set", None), ("n_features", "set", -1))
        two(("indices", "set", None), ("indptr", "set", None))
        two(("n_features", "set", 1 << 31), ("row0", "set", -1))
        two(("row0", "set", -1), ("nrows", "set", 1 << 31))
        two(("nrows", "set", -1), ("values", "add", 2))
    elif fn == "rae_cluster_key_count":
        null("labels", "keys", "counts")
        rng("relations", 0, 513), rng("n_keys", 0, (1 << 22) + 1), rng("nrows", -1, 1 << 31)
        one("n_keys", "add", 1, relations=512, n_keys=1 << 18)  # 2^27 cells and one column
        move(4, "labels"), move(2, "keys", "counts")
        two(("counts", "set", None), ("relations", "set", 0))
        two(("relations", "set", 513), ("n_keys", "set", 0))
        two(("n_keys", "set", (1 << 22) + 1), ("relations", "set", 512))
        two(("n_keys", "add", 1), ("nrows", "set", -1), relations=512, n_keys=1 << 18)
        two(("nrows", "set", 1 << 31), ("labels", "add", 4))
    elif fn == "rae_cluster_topk":
        null("counts", "keys_out", "counts_out")
        rng("relations", 0, 513), rng("n_keys", 0, (1 << 22) + 1), rng("top", 0, 33)
        one("ld", "add", -1)
        move(2, "counts", "keys_out", "counts_out")
        two(("counts_out", "set", None), ("relations", "set", 513))
        two(("relations", "set", 0), ("n_keys", "set", 0))
        two(("n_keys", "set", (1 << 22) + 1), ("ld", "set", 0))
        two(("ld", "add", -1), ("top", "set", 33))
        two(("top", "set", 0), ("counts", "add", 2))
    elif fn == "rae_feature_support":
        null("indptr", "indices", "support")
        rng("n_features", -1, 1 << 31), rng("row0", -1), rng("nrows", -1, 1 << 31)
        move(2, "indptr", "indices", "values", "support")
        two(("support", "set", None), ("n_features", "set", 1 << 31))
        two(("indices", "set", None), ("indptr", "set", None))
        two(("n_features", "set", -1), ("row0", "set", -1))
        two(("row0", "set", -1), ("nrows", "set", -1))
        two(("nrows", "set", 1 << 31), ("support", "add", 2))
    else:                                                      # rae_feature_topk and its sizer
        one("a", "null", None)
        rng("relations", 0, 513), rng("n_features", -1, 1 << 31), rng("top", 0, 33)
        rng("centre", 2, -1)
        one("ldw", "add", -1)
        two(("relations", "set", 513), ("n_features", "set", -1))
        two(("n_features", "set", 1 << 31), ("ldw", "set", 0))
        two(("ldw", "add", -1), ("top", "set", 0))
        two(("top", "set", 33), ("centre", "set", 2))
        if fn == "rae_feature_topk":
            null("W", "feats_out", "workspace")
            move(2, "W", "support", "feats_out", "scores_out")
            one("workspace", "add", 128)
            one("workspace_bytes", "add", -1)
            one("workspace_bytes", "add", -1, centre=0)
            two(("centre", "set", 2), ("W", "set", None))
            two(("W", "set", None), ("feats_out", "set", None))
            two(("feats_out", "set", None), ("scores_out", "add", 2))
            two(("W", "add", 2), ("workspace", "set", None))
            two(("workspace", "add", 128), ("workspace_bytes", "add", -1))
    return out


def cases():
    return [dict(fn=fn, base=base, change=ch) for fn in ENTRIES for base, ch in _entry_cases(fn)]


# ------------------------------------------------------------------ accepted shapes' sizes
def size_case(lib, s):
    a = ftopk_args(s["n_features"], s["relations"], s["top"], s["centre"])
    return int(lib.rae_feature_topk_workspace_bytes(C.byref(a)))


def size_specs():
    return [dict(fn=SIZER, n_features=d, relations=m, top=t, centre=c)
            for d in (0, 1, 511, 512, 513, 65536, (1 << 31) - 1) for m in (1, 64, 65, 512)
            for t in (1, 32) for c in (1, 0)]


if __name__ == "__main__":
    record(sys.argv[1] if len(sys.argv) > 1 else OUT, cases(), run, size_specs(), size_case,
           lambda s, b: b > 0)
