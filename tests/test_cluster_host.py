"""Host side of the device cluster evaluation (rae_cluster_count / rae_b3_metrics,
include/rae.h): the array oracle in rae/evaluation.py (GoldIndex, contingency_table,
b3_from_table) against the reference-pinned evaluator, the argument checks (which run before
any HIP call, so they work without a GPU) and the command line flag.  No GPU needed."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from rae.evaluation import (GoldIndex, b3_from_table, construct_split_evaluator,
                            contingency_table)

with open(os.path.join(GOLDEN, "b3_cases.json")) as fh:
    CASES = json.load(fh)["cases"]

REL, ABS = 1e-12, 1e-15       # the tolerance tests/test_b3.py pins the evaluator with


def _labels_of(induced, n):
    """The label vector of a cluster id -> members mapping; -1 where an id is in no cluster."""
    lab = np.full(n, -1, dtype=np.int64)
    for cid, members in induced.items():
        for e in members:
            assert lab[e] == -1, "an example in two clusters"
            lab[e] = cid
    return lab


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_table_path_matches_reference_fixture(case):
    """b3_from_table(contingency_table(labels)) gives the executed reference's numbers.  In
    these cases every example id in range(N) is a member of exactly one induced cluster (no
    member-less ids, checked here), so the clusters are a label vector without loss."""
    gold = {int(k): v for k, v in case["gold"].items()}
    induced = {int(k): list(v) for k, v in case["induced"].items()}
    members = [e for v in induced.values() for e in v]
    n = 1 + max(members)
    lab = _labels_of(induced, n)
    assert sorted(members) == list(range(n)) and (lab >= 0).all()
    assert all(0 <= e < n for e in gold)
    m = 1 + max(induced)
    gi = GoldIndex(gold, n)
    tb = contingency_table(lab, gi, m)
    assert tb.dtype == np.int64 and tb.shape == (m, gi.n_gold + 1)
    assert int(tb.sum()) == case["number_of_elements"]
    f1, pre, rec = b3_from_table(tb, gi.sizes, gi.n_assessable)
    assert pre == pytest.approx(case["precision"], rel=REL, abs=ABS)
    assert rec == pytest.approx(case["recall"], rel=REL, abs=ABS)
    assert f1 == pytest.approx(case["f1"], rel=REL, abs=ABS)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_table_path_matches_evaluator_with_dropped_tail(seed):
    """Random labels over the first n_rows examples of a gold standard that reaches past them
    (the batch loop drops the tail, the gold standard does not): same triple as
    SingleLabelClusterEvaluation fed the cluster sets."""
    g = np.random.RandomState(seed)
    N, n_rows, m = 500, 430, 7
    names = ["R%d" % k for k in range(5)] + [""]
    gold = {int(i): [names[g.randint(len(names))], "X"] for i in np.nonzero(g.rand(N) < 0.3)[0]}
    assert max(gold) >= n_rows
    lab = g.randint(0, m - 1, n_rows)          # cluster m-1 stays empty
    clusters = {c: set() for c in range(m)}
    for i, c in enumerate(lab):
        clusters[int(c)].add(i)
    ev = construct_split_evaluator(gold, "valid")
    ev.feed_induced_clusters(clusters)
    want = ev.compute_metrics()
    gi = GoldIndex(gold, n_rows)
    tb = contingency_table(lab, gi, m)
    got = b3_from_table(tb, gi.sizes, gi.n_assessable)
    assert got == pytest.approx(want, rel=REL, abs=ABS)
    assert int(tb.sum()) == ev.numberOfElements == n_rows
    assert gi.n_assessable == len(ev.assessableElemSet)
    assert gi.sizes.tolist() == [len(v) for _, v in sorted(ev.gold_clusters.items())]


def test_gold_index_fields():
    gold = {0: ["B"], 1: ["A", "B"], 2: [""], 4: ["B"], 7: ["C"], 9: ["A"]}
    gi = GoldIndex(gold, 6)
    assert gi.names == ["A", "B", "C"] and gi.n_gold == 3
    assert gi.ids.dtype == np.int32 and gi.sizes.dtype == np.int64
    # '' first label, a missing id (3, 5) and ids beyond n_rows (7, 9) are -1 / absent
    assert gi.ids.tolist() == [1, 0, -1, -1, 1, -1]
    # ... but the examples beyond n_rows still count in the sizes and in |A|
    assert gi.sizes.tolist() == [2, 2, 1]
    assert gi.n_assessable == 5
    empty = GoldIndex({}, 4)
    assert empty.n_gold == 0 and empty.ids.tolist() == [-1] * 4 and empty.n_assessable == 0
    assert b3_from_table(contingency_table([0, 1, 1, 0], empty, 2), empty.sizes, 0) == (0, 0, 0)


def test_table_rules():
    """Out-of-range labels are skipped, out-of-range gold ids go to the last column; a cluster
    with only unlabelled members and a gold class of size 0 add nothing."""
    gi = GoldIndex({0: ["A"], 1: ["A"], 2: ["B"]}, 6)
    gi.ids[5] = 7                                     # an id no class has
    tb = contingency_table([0, 0, 1, 1, -1, 2], gi, 3)
    assert tb.tolist() == [[2, 0, 0], [0, 1, 1], [0, 0, 1]]
    f1, pre, rec = b3_from_table(tb, gi.sizes, gi.n_assessable)
    assert pre == pytest.approx(1.0) and rec == pytest.approx(1.0)
    # a gold class of size 0: its column is ignored by the recall
    assert b3_from_table(tb, [2, 0], 3)[2] == pytest.approx(2 / 3)


# ------------------------------------------------------------------------- argument checks
def _count(lib, labels=0x10000, gold=0x20000, nrows=1000, m=100, ng=40, form=0, table=0x30000):
    return lib.rae_cluster_count(labels, gold, nrows, m, ng, form, table, None)


def _b3(lib, table=0x30000, sizes=0x40000, na=10, m=100, ng=40, out=0x50000, so=0x60000):
    return lib.rae_b3_metrics(table, sizes, na, m, ng, out, so, None)


def test_cluster_calls_reject_bad_arguments(built_lib):
    """Made-up (never dereferenced) device addresses: every refusal is RAE_E_INVALID with a
    message naming the argument, before any HIP call."""
    from rae import _lib
    lib = built_lib
    bad = []

    def case(name, word, rc):
        msg = lib.rae_last_error().decode()
        if rc != -1 or word not in msg:
            bad.append((name, rc, msg))

    case("relations 0", "relations", _count(lib, m=0))
    case("relations 513", "relations", _count(lib, m=513))
    case("n_gold -1", "n_gold", _count(lib, ng=-1))
    case("n_gold 4096", "n_gold", _count(lib, ng=4096))
    case("nrows -1", "nrows", _count(lib, nrows=-1))
    case("null labels", "labels", _count(lib, labels=None))
    case("null gold", "gold", _count(lib, gold=None))
    case("null table", "table", _count(lib, table=None))
    case("form 3", "form", _count(lib, form=3))
    case("form 0x200", "form", _count(lib, form=0x200))
    # 512 x 128 counters = 256 KiB: over the LDS budget (and over gfx950's 160 KiB)
    assert 512 * 128 > _lib.RAE_CCOUNT_LDS_CELLS
    case("LDS over budget", "LDS", _count(lib, m=512, ng=127, form=_lib.RAE_CCOUNT_LDS))
    case("LDS over budget, accumulate", "LDS",
         _count(lib, m=512, ng=127, form=_lib.RAE_CCOUNT_LDS | _lib.RAE_CCOUNT_ACCUMULATE))
    # one counter past the budget: 128 x 129 = 16512 > 16384 >= 128 x 128
    assert 128 * 128 == _lib.RAE_CCOUNT_LDS_CELLS
    case("LDS one past", "LDS", _count(lib, m=128, ng=128, form=_lib.RAE_CCOUNT_LDS))
    case("b3 relations 0", "relations", _b3(lib, m=0))
    case("b3 relations 513", "relations", _b3(lib, m=513))
    case("b3 n_gold -1", "n_gold", _b3(lib, ng=-1))
    case("b3 n_gold 4096", "n_gold", _b3(lib, ng=4096))
    case("b3 null table", "table", _b3(lib, table=None))
    case("b3 null metrics", "metrics_out", _b3(lib, out=None))
    case("b3 null sizes", "gold_sizes", _b3(lib, sizes=None))
    case("b3 n_assessable -1", "n_assessable", _b3(lib, na=-1))
    assert not bad, bad


def test_binding_constants_match_header():
    import re
    from rae import _lib
    txt = open(_lib.HEADER).read()
    for name in ("RAE_CCOUNT_AUTO", "RAE_CCOUNT_LDS", "RAE_CCOUNT_GLOBAL",
                 "RAE_CCOUNT_ACCUMULATE", "RAE_CCOUNT_LDS_CELLS"):
        val = re.search(r"#define\s+%s\s+(\S+)" % name, txt).group(1)
        assert int(val, 0) == getattr(_lib, name), name
    assert {"rae_cluster_count", "rae_b3_metrics"} <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------ command line
def test_cli_cluster_eval_flag(monkeypatch):
    import torch
    from rae import cli, inducer
    base = ["synthetic:200:64:3", "--model-name", "m", "--decoder", "sp", "--epochs", "1"]
    assert cli.get_command_args(base).cluster_eval == "host"
    assert cli.get_command_args(base + ["--cluster-eval", "device"]).cluster_eval == "device"
    with pytest.raises(SystemExit):
        cli.get_command_args(base + ["--cluster-eval", "gpu"])
    # the flag reaches the inducer: main() hands it to the constructor
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop()

    monkeypatch.setattr(inducer, "ReconstructInducer", fake)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    with pytest.raises(Stop):
        cli.main(base + ["--cluster-eval", "device"])
    assert seen["cluster_eval"] == "device"
    monkeypatch.undo()
    # the constructor refuses anything else before it touches a device
    with pytest.raises(ValueError, match="cluster_eval"):
        inducer.ReconstructInducer(None, {}, None, 1, 0.1, 10, 4, 3, 2, 0.0, 0.0, "adagrad", "m",
                                   "sp", False, True, False, 1.0, cluster_eval="gpu")
    # without a GPU a device run raises where the product path raises today (there is no CPU
    # fallback): the same exception type as the host-evaluated run
    if not torch.cuda.is_available():
        errs = []
        for mode in ("host", "device"):
            with pytest.raises(Exception) as ei:
                cli.main(base + ["--cluster-eval", mode])
            errs.append(type(ei.value))
        assert errs[0] is errs[1]
