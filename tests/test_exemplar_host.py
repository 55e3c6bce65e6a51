"""Cluster exemplars without a GPU: the numpy oracles (rae.evaluation.label_stats /
cluster_exemplars / format_cluster_exemplars) against explicit Python loops and hand-written lines,
the flags, and the argument checks of rae_label_stats / rae_cluster_exemplars (include/rae.h)."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

from rae.evaluation import cluster_exemplars, format_cluster_exemplars, label_stats


# ------------------------------------------------------------------------ 1. label_stats
def _better(v, k, best, bk):
    """lbl_better (csrc/rae_label.hpp): numpy's argmax order, NaN counting as the maximum."""
    if bk is None:
        return True
    if math.isnan(best):
        return math.isnan(v) and k < bk
    if math.isnan(v):
        return True
    return v > best or (v == best and k < bk)


def _stats_loop(S):
    """(labels, margin, pmax) of the float32 logits S by explicit loops."""
    S = np.asarray(S, dtype=np.float32)
    N, m = S.shape
    labels, margin, pmax = np.zeros(N, np.int64), np.zeros(N, np.float32), np.zeros(N, np.float32)
    for i in range(N):
        best = bk = None
        for k in range(m):
            if _better(float(S[i, k]), k, best, bk):
                best, bk = float(S[i, k]), k
        sec = sk = None
        for k in range(m):
            if k != bk and _better(float(S[i, k]), k, sec, sk):
                sec, sk = float(S[i, k]), k
        labels[i] = bk
        with np.errstate(invalid="ignore", over="ignore"):
            margin[i] = np.inf if m == 1 else np.float32(best) - np.float32(sec)
            e = np.exp(S[i] - np.float32(best)).astype(np.float32)
            pmax[i] = np.exp(np.float32(best) - np.float32(best)) / e.sum(dtype=np.float32)
    return labels, margin, pmax


def _logits_as_problem(S):
    """X = I, W = 0, Wb = ... cannot carry per-row logits; use X = I (N, N) and W = S, Wb = 0."""
    S = np.asarray(S, dtype=np.float32)
    return sp.identity(S.shape[0], dtype=np.float32, format="csr"), S, np.zeros(S.shape[1], np.float32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


LOGIT_CASES = {
    "plain": [[0.5, 2.0, -1.0], [3.0, 1.0, 2.5]],
    "tie": [[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [4.0, 4.0, 4.0]],
    "nan_one": [[0.0, np.nan, 5.0], [np.nan, 1.0, 2.0]],
    "nan_two": [[np.nan, 1.0, np.nan], [1.0, np.nan, np.nan]],
    "inf": [[np.inf, np.inf, 0.0], [np.inf, 1.0, -np.inf], [-np.inf, -np.inf, -np.inf]],
    "zeros": [[0.0, -0.0, -1.0], [-0.0, 0.0, -0.0]],
    "one_relation": [[1.5], [np.nan], [-np.inf]],
}


@pytest.mark.parametrize("name", sorted(LOGIT_CASES))
def test_label_stats_oracle_against_loops(name):
    S = np.array(LOGIT_CASES[name], dtype=np.float32)
    X, W, Wb = _logits_as_problem(S)
    lab, mar, pm = label_stats(X, W, Wb)
    wl, wm, wp = _stats_loop(S)
    assert _same(lab, wl) and _same(mar, wm) and _same(pm, wp), (lab, wl, mar, wm, pm, wp)
    assert mar.dtype == np.float32 and pm.dtype == np.float32 and lab.dtype == np.int64


def test_label_stats_oracle_rules():
    X, W, Wb = _logits_as_problem(np.array(LOGIT_CASES["tie"], np.float32))
    lab, mar, _ = label_stats(X, W, Wb)
    assert lab.tolist() == [0, 1, 0] and mar.tolist() == [0.0, 0.0, 0.0]
    X, W, Wb = _logits_as_problem(np.array(LOGIT_CASES["one_relation"], np.float32))
    lab, mar, _ = label_stats(X, W, Wb)
    assert lab.tolist() == [0, 0, 0] and np.all(np.isposinf(mar))
    X, W, Wb = _logits_as_problem(np.array(LOGIT_CASES["inf"], np.float32))
    lab, mar, _ = label_stats(X, W, Wb)
    assert lab.tolist() == [0, 0, 0] and np.isnan(mar[0]) and np.isposinf(mar[1]) and np.isnan(mar[2])
    X, W, Wb = _logits_as_problem(np.array(LOGIT_CASES["nan_one"], np.float32))
    lab, mar, _ = label_stats(X, W, Wb)
    assert lab.tolist() == [1, 0] and np.all(np.isnan(mar))


def test_label_stats_oracle_on_a_sparse_problem():
    g = np.random.RandomState(3)
    N, d, m = 40, 30, 7
    X = sp.random(N, d, density=0.2, format="csr", random_state=g, dtype=np.float32)
    X.data[:] = g.randint(1, 4, X.data.shape[0])
    W = (g.randint(-64, 65, (d, m)) / 8.0).astype(np.float32)
    Wb = (g.randint(-64, 65, m) / 8.0).astype(np.float32)
    S = np.asarray(X.toarray() @ W + Wb, dtype=np.float32)       # exact: dyadic
    got = label_stats(X, W, Wb)
    want = _stats_loop(S)
    assert all(_same(a, b) for a, b in zip(got, want))
    l64, m64, p64 = label_stats(X, W, Wb, dtype=np.float64)
    assert m64.dtype == np.float64 and np.array_equal(l64, got[0])
    assert np.array_equal(m64.astype(np.float32), got[1])


# ------------------------------------------------------------------------ 2. cluster_exemplars
def _exemplars_loop(labels, scores, relations, top, largest):
    rows = np.full((relations, top), -1, np.int32)
    out = np.full((relations, top), -np.inf, np.float32)
    for c in range(relations):
        cand = []
        for i, (l, s) in enumerate(zip(labels, scores)):
            s = float(s)
            if int(l) != c or math.isnan(s):
                continue
            s = 0.0 if s == 0.0 else s
            cand.append(((-s if largest else s), i, s))
        cand.sort(key=lambda t: (t[0], t[1]))
        for j, (_, i, s) in enumerate(cand[:top]):
            rows[c, j], out[c, j] = i, s
    return rows, out


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


EX_CASES = {
    # labels, scores, relations
    "ties": ([0, 0, 0, 1, 1, 0], [1.0, 2.0, 1.0, 5.0, 5.0, 2.0], 2),
    "empty_clusters": ([2, 2, 2], [0.1, 0.3, 0.2], 4),
    "out_of_range": ([-1, 0, 3, 1, 2, 1 << 40, 0], [9.0, 1.0, 9.0, 2.0, 9.0, 9.0, 3.0], 2),
    "special": ([0] * 8, [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, np.nan, -1.0], 1),
    "zeros": ([0, 0, 1, 1], [-0.0, 0.0, 0.0, -0.0], 2),
    "all_nan": ([0, 1], [np.nan, np.nan], 2),
    "none": ([], [], 3),
}


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("top", [1, 2, 5])
@pytest.mark.parametrize("name", sorted(EX_CASES))
def test_cluster_exemplars_oracle_against_loops(name, top, largest):
    labels, scores, m = EX_CASES[name]
    labels = np.array(labels, dtype=np.int64)
    scores = np.array(scores, dtype=np.float32)
    rows, out = cluster_exemplars(labels, scores, m, top, largest)
    wr, wo = _exemplars_loop(labels, scores, m, top, largest)
    assert rows.dtype == np.int32 and out.dtype == np.float32
    assert np.array_equal(rows, wr), (rows, wr)
    assert np.array_equal(_bits(out), _bits(wo)), (out, wo)       # bitwise: -0 is returned as +0


def test_cluster_exemplars_oracle_rules():
    labels, scores, m = EX_CASES["special"]
    rows, out = cluster_exemplars(labels, scores, m, 8, True)
    assert rows[0].tolist() == [1, 5, 3, 4, 7, 2, -1, -1]
    assert np.array_equal(_bits(out[0]), _bits([np.inf, 1.0, 0.0, 0.0, -1.0, -np.inf, -np.inf, -np.inf]))
    rows, out = cluster_exemplars(labels, scores, m, 8, False)
    assert rows[0].tolist() == [2, 7, 3, 4, 5, 1, -1, -1]
    assert np.array_equal(_bits(out[0]), _bits([-np.inf, -1.0, 0.0, 0.0, 1.0, np.inf, -np.inf, -np.inf]))


# ------------------------------------------------------------------------ 3. the lines
def test_format_cluster_exemplars_lines():
    rows = np.array([[4, 0, -1], [-1, -1, -1], [2, 1, 3]], np.int32)
    scores = np.array([[2.5, 0.0, -np.inf], [-np.inf] * 3, [np.inf, 1e-3, -7.0]], np.float32)
    sizes = [2, 0, 9]
    a1 = np.array([10, 11, 12, 13, 14])
    a2 = np.array([20, 21, 22, 23, 24])
    assert format_cluster_exemplars(rows, scores, sizes, a1, a2) == [
        "relation 0 (2 rows): 4:14 | 24:2.5 0:10 | 20:0",
        "relation 1 (0 rows):",
        "relation 2 (9 rows): 2:12 | 22:inf 1:11 | 21:0.00100000005 3:13 | 23:-7",
    ]
    names = {10: "Paris", 24: "Seine", 14: None}
    keys = np.array([1, -1, 0, 0, 1], np.int32)
    assert format_cluster_exemplars(rows, scores, sizes, a1, a2, names, keys, ["flows", "in"]) == [
        "relation 0 (2 rows): 4:14 | in | Seine:2.5 0:Paris | in | 20:0",
        "relation 1 (0 rows):",
        "relation 2 (9 rows): 2:12 | flows | 22:inf 1:11 | - | 21:0.00100000005 3:13 | flows | 23:-7",
    ]
    # a key index without names prints the key ids
    assert format_cluster_exemplars(rows[:1], scores[:1], sizes, a1, a2, None, keys)[0] == \
        "relation 0 (2 rows): 4:14 | 1 | 24:2.5 0:10 | 1 | 20:0"
    for s in scores[np.isfinite(scores)]:
        assert np.float32(float("{:.9g}".format(float(s)))) == s           # round-trips


# ------------------------------------------------------------------------ 4. the flags
def test_cli_flags_and_inducer_values():
    from rae import inducer
    from rae.cli import get_command_args
    base = ["data.npz", "--model-name", "m", "--decoder", "sp"]
    a = get_command_args(base)
    assert (a.print_exemplars, a.print_exemplars_order, a.print_exemplars_by) == (0, "most", "margin")
    assert get_command_args(base + ["--print-exemplars"]).print_exemplars == 5
    a = get_command_args(base + ["--print-exemplars", "7", "--print-exemplars-order", "both",
                                 "--print-exemplars-by", "pmax"])
    assert (a.print_exemplars, a.print_exemplars_order, a.print_exemplars_by) == (7, "both", "pmax")
    for bad in (["--print-exemplars-order", "first"], ["--print-exemplars-by", "psi"]):
        with pytest.raises(SystemExit):
            get_command_args(base + bad)
    mk = lambda **kw: inducer.ReconstructInducer(
        None, {}, None, 1, 0.1, 10, 4, 3, 2, 0.0, 0.0, "adagrad", "m", "sp", False, True, False,
        1.0, **kw)
    with pytest.raises(ValueError, match="print_exemplars"):
        mk(print_exemplars=33)
    with pytest.raises(ValueError, match="print_exemplars"):
        mk(print_exemplars=-1)
    with pytest.raises(ValueError, match="print_exemplars_order"):
        mk(print_exemplars=3, print_exemplars_order="first")
    with pytest.raises(ValueError, match="print_exemplars_by"):
        mk(print_exemplars=3, print_exemplars_by="psi")


# ------------------------------------------------------------------------ 5. the rejections
# Made-up addresses: every call below is refused before the first HIP call.  If a check were ever
# lost the call would go on to launch with them, so -- like tests/test_entry_rejections.py -- the
# calls run only where no GPU is visible.
@pytest.fixture(scope="module")
def host_lib(built_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must never reach a visible GPU")
    return built_lib


def _cex_args(**kw):
    from rae import _lib
    a = _lib.RaeExemplarArgs()
    a.labels, a.scores, a.nrows = 0x100000, 0x200000, 1000
    a.relations, a.top, a.largest = 100, 5, 1
    a.rows_out, a.scores_out = 0x300000, 0x400000
    a.workspace, a.workspace_bytes = 0x800000, 1 << 30
    for k, v in kw.items():
        setattr(a, k, v)
    return a


CEX_SHAPE_REJECTIONS = [
    (dict(relations=0), "relations"),
    (dict(relations=513), "relations"),
    (dict(top=0), "top"),
    (dict(top=33), "top"),
    (dict(nrows=-1), "nrows"),
    (dict(nrows=1 << 31), "nrows"),
    (dict(largest=2), "largest"),
]
CEX_REJECTIONS = CEX_SHAPE_REJECTIONS + [
    (dict(labels=None), "labels"),
    (dict(scores=None), "scores"),
    (dict(rows_out=None), "rows_out"),
    (dict(labels=0x100004), "labels"),
    (dict(scores=0x200002), "scores"),
    (dict(workspace=None), "workspace"),
    (dict(workspace=0x800080), "workspace"),                   # not 256-byte aligned
    (dict(workspace_bytes=0), "workspace_bytes"),
]


@pytest.mark.parametrize("change,word", CEX_REJECTIONS,
                         ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in CEX_REJECTIONS])
def test_cluster_exemplars_rejections(host_lib, change, word):
    from rae import _lib
    a = _cex_args(**change)
    rc = host_lib.rae_cluster_exemplars(C.byref(a), None)
    assert rc == -1                                            # RAE_E_INVALID
    assert word in host_lib.rae_last_error().decode(), host_lib.rae_last_error()


def test_cluster_exemplars_null_struct_and_short_workspace(host_lib):
    assert host_lib.rae_cluster_exemplars(None, None) == -1
    a = _cex_args()
    need = host_lib.rae_cluster_exemplars_workspace_bytes(C.byref(a))
    assert need > 0
    a.workspace_bytes = need - 1                               # one byte short
    assert host_lib.rae_cluster_exemplars(C.byref(a), None) == -1
    assert "rae_cluster_exemplars_workspace_bytes" in host_lib.rae_last_error().decode()


def test_cluster_exemplars_workspace_bytes(built_lib):
    """Host only (no address is used): strips x relations x top keys rounded up to 256 bytes, a
    function of (nrows, relations, top) alone, at most 16 MiB; -1 on a bad argument."""
    from rae import _lib
    size = built_lib.rae_cluster_exemplars_workspace_bytes
    al = lambda x: (x + 255) & ~255
    for n in (0, 1, 4095, 4096, 4097, 20011, 1 << 20, (1 << 31) - 1):
        strips = _lib.cex_strips(n)
        assert 1 <= strips <= _lib.RAE_CX_MAXSTRIPS
        for m, top in ((1, 1), (100, 5), (512, 32)):
            for largest in (0, 1):
                a = _cex_args(nrows=n, relations=m, top=top, largest=largest, labels=None,
                              scores=None, workspace=None)
                assert size(C.byref(a)) == al(strips * m * top * 8), (n, m, top)
    assert _lib.cex_strips(20011) > 1
    assert size(C.byref(_cex_args(nrows=(1 << 31) - 1, relations=512, top=32))) == 16 << 20
    for change, word in CEX_SHAPE_REJECTIONS:
        assert size(C.byref(_cex_args(**change))) == -1, change
        assert word in built_lib.rae_last_error().decode()
    assert size(None) == -1
    # the waves of a workgroup keep its lists within 64 KiB; one wave's lists may be larger
    assert [_lib.cex_waves(*s) for s in ((100, 5), (64, 32), (128, 32), (256, 32), (512, 32))] == \
        [4, 4, 2, 1, 1]


LABEL_STATS_REJECTIONS = [
    (dict(indptr=None), "indptr"),
    (dict(indices=None), "indices"),
    (dict(W=None), "W"),
    (dict(Wb=None), "Wb"),
    (dict(labels_out=None), "labels_out"),
    (dict(relations=0), "relations"),
    (dict(relations=513), "relations"),
    (dict(relations=130), "relations"),                        # above 128: a multiple of 4
    (dict(row0=-1), "row0"),
    (dict(nrows=-1), "nrows"),
    (dict(nrows=1 << 31), "nrows"),
    (dict(W=0x400004), "W"),                                   # relations % 4 == 0: 16 bytes
    (dict(margin_out=0x700002), "margin_out"),
    (dict(labels_out=0x600004), "labels_out"),
]


@pytest.mark.parametrize("change,word", LABEL_STATS_REJECTIONS,
                         ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in LABEL_STATS_REJECTIONS])
def test_label_stats_rejections(host_lib, change, word):
    kw = dict(indptr=0x100000, indices=0x200000, values=0x300000, W=0x400000, Wb=0x500000,
              relations=100, row0=0, nrows=10, labels_out=0x600000, margin_out=0x700000,
              pmax_out=0x800000)
    kw.update(change)
    rc = host_lib.rae_label_stats(kw["indptr"], kw["indices"], kw["values"], kw["W"], kw["Wb"],
                                  kw["relations"], kw["row0"], kw["nrows"], kw["labels_out"],
                                  kw["margin_out"], kw["pmax_out"], None)
    assert rc == -1                                            # RAE_E_INVALID
    assert word in host_lib.rae_last_error().decode(), host_lib.rae_last_error()
