"""Relation feature profiles, the host side (no GPU): the numpy oracles of rae/evaluation.py
(feature_support, tree_row_sum, feature_topk, format_relation_features) against explicit Python
loops, and the argument rejections of rae_feature_support / rae_feature_topk /
rae_feature_topk_workspace_bytes through the C ABI."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

from rae.evaluation import (feature_scores, feature_support, feature_topk,
                            format_relation_features, tree_row_sum)

from _profile_sample import sample_data


# ------------------------------------------------------------------------ 1. the row sum
def _lane_tree_sum(row):
    """The definition, spelled out: 64 lanes, columns j, j + 64, ... ascending, xor tree."""
    lanes = [0.0] * 64
    for j in range(64):
        for c in range(j, len(row), 64):
            lanes[j] = lanes[j] + float(row[c])
    for o in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[j] + lanes[j ^ o] for j in range(64)]
    assert all(math.isnan(v) for v in lanes) or len(set(lanes)) == 1    # every lane holds the sum
    return lanes[0]


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 130, 512])
def test_tree_row_sum_is_the_lane_and_tree_order(m):
    g = np.random.RandomState(m)
    W = (g.standard_normal((9, m)) * np.power(10.0, g.randint(-3, 4, (9, 1)))).astype(np.float32)
    got = tree_row_sum(W)
    assert got.dtype == np.float64 and got.shape == (9,)
    for f in range(9):
        want = _lane_tree_sum(W[f])
        assert got[f] == want, (f, got[f], want)              # bit for bit
        exact = math.fsum(float(x) for x in W[f])
        bound = m * 2.0 ** -53 * float(np.abs(W[f].astype(np.float64)).sum())
        assert abs(got[f] - exact) <= bound, (f, got[f], exact, bound)


def test_tree_row_sum_order_matters_and_specials():
    # a row whose sum depends on the order: the oracle must follow the tree, not np.sum
    W = np.zeros((1, 130), np.float32)
    W[0, 0], W[0, 64], W[0, 128], W[0, 1] = 1e8, 1.0, -1e8, 3.0
    assert tree_row_sum(W)[0] == _lane_tree_sum(W[0])
    S = np.array([[np.nan, 1, 2], [np.inf, 1, 2], [np.inf, -np.inf, 0], [-0.0, -0.0, -0.0]],
                 np.float32)
    t = tree_row_sum(S)
    assert np.isnan(t[0]) and t[1] == np.inf and np.isnan(t[2]) and t[3] == 0.0


# ------------------------------------------------------------------------ 2. the support
def test_feature_support_against_a_dense_count():
    g = np.random.RandomState(3)
    n, d = 200, 37
    dense = (g.rand(n, d) < 0.2).astype(np.float32)
    X = sp.csr_matrix(dense)
    # stored zeros: present in indices, not in the count when values are used
    X.data[g.rand(X.nnz) < 0.15] = 0.0
    kept = np.zeros((n, d), np.int64)
    stored = np.zeros((n, d), np.int64)
    for i in range(n):
        for p in range(X.indptr[i], X.indptr[i + 1]):
            stored[i, X.indices[p]] += 1
            kept[i, X.indices[p]] += X.data[p] != 0
    got = feature_support(X)
    assert got.dtype == np.int32 and np.array_equal(got, kept.sum(0))
    assert np.array_equal(feature_support(X, use_values=False), stored.sum(0))
    assert (kept.sum(0) != stored.sum(0)).any()
    # columns at and past n_features are skipped
    assert np.array_equal(feature_support(X, n_features=20), kept.sum(0)[:20])
    assert feature_support(X, n_features=0).shape == (0,)


# ------------------------------------------------------------------------ 3. the top-k
def _brute(W, support, min_support, centre, top):
    d, m = W.shape
    if centre:
        s = np.empty((d, m), np.float32)
        for f in range(d):
            mean = _lane_tree_sum(W[f]) / float(m)
            for k in range(m):
                s[f, k] = np.float32(float(W[f, k]) - mean)
    else:
        s = W.copy()
    feats, scores = [], []
    for k in range(m):
        cand = [f for f in range(d) if (support is None or support[f] >= min_support)
                and not math.isnan(s[f, k])]
        cand.sort(key=lambda f: (-(float(s[f, k]) + 0.0), f))
        cand = cand[:top]
        feats.append(cand + [-1] * (top - len(cand)))
        scores.append([float(s[f, k]) + 0.0 for f in cand] + [-math.inf] * (top - len(cand)))
    return np.array(feats, np.int32), np.array(scores, np.float32)


def _same(a, b):
    """Equal feature ids and equal score bits."""
    return np.array_equal(a[0], b[0]) and a[1].dtype == b[1].dtype == np.float32 and \
        np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("centre", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (50, 4), (50, 64), (37, 65), (20, 130)])
def test_feature_topk_against_brute_force(shape, centre):
    d, m = shape
    g = np.random.RandomState(d * 131 + m)
    ties = g.randint(-2, 3, (d, m)).astype(np.float32)           # massive ties: feature ascending
    floats = g.standard_normal((d, m)).astype(np.float32)
    sup = g.randint(0, 10, d).astype(np.int32)
    for W in (ties, floats):
        for top in (1, 5, 32, d + 3 if d + 3 <= 32 else 32):
            for support, ms in ((None, 0), (sup, 5), (sup, 0), (sup, 10)):
                got = feature_topk(W, support, ms, centre, top)
                want = _brute(W, support, ms, centre, top)
                assert got[0].shape == (m, top) and _same(got, want), (top, ms)


def test_feature_topk_specials_padding_and_eligibility():
    W = np.array([[1.0, -0.0], [np.nan, 0.0], [np.inf, 2.0], [-np.inf, -3.0], [0.0, np.nan]],
                 np.float32)
    f, s = feature_topk(W, None, 0, False, 6)                    # top > d: padded
    assert f[0].tolist() == [2, 0, 4, 3, -1, -1]                 # the NaN cell is no candidate
    assert s[0].tolist()[:4] == [np.inf, 1.0, 0.0, -np.inf] and s[0, 4] == -np.inf
    assert f[1].tolist() == [2, 0, 1, 3, -1, -1]                 # -0 ties with +0: feature ascending
    assert not np.signbit(s[1, 1]) and not np.signbit(s[1, 2])   # ... and is returned as +0
    assert _same((f, s), _brute(W, None, 0, False, 6))
    # centred: a row with a NaN, or with +inf (inf - inf), has NaN in the affected cells
    fc, sc = feature_topk(W, None, 0, True, 6)
    assert _same((fc, sc), _brute(W, None, 0, True, 6))
    assert 1 not in fc[0].tolist() and 1 not in fc[1].tolist()   # the NaN row: every score NaN
    assert 2 not in fc[0].tolist() and fc[1].tolist().count(2) == 1
    # eligibility on both sides of min_support
    sup = np.array([4, 5, 6, 5, 0], np.int32)
    f5, _ = feature_topk(W, sup, 5, False, 6)
    assert sorted(x for x in f5[1].tolist() if x >= 0) == [1, 2, 3]
    f6, _ = feature_topk(W, sup, 6, False, 6)
    assert f6[1].tolist() == [2, -1, -1, -1, -1, -1]
    f7, s7 = feature_topk(W, sup, 7, False, 2)                   # nobody eligible: all padding
    assert (f7 == -1).all() and (s7 == -np.inf).all()
    # no features at all
    f0, s0 = feature_topk(np.zeros((0, 3), np.float32), None, 0, True, 4)
    assert f0.shape == (3, 4) and (f0 == -1).all() and (s0 == -np.inf).all()
    # the centred score is one rounding of the double difference
    Wc = np.array([[1.0, 1e-8, -1.0, 3.0]], np.float32)
    mean = _lane_tree_sum(Wc[0]) / 4.0
    assert feature_scores(Wc)[0].tolist() == [float(np.float32(float(x) - mean)) for x in Wc[0]]


# ------------------------------------------------------------------------ 4. the lines
def test_format_relation_features_on_the_sample():
    data, _ = sample_data()
    X = data.split["train"].xFeats
    lex = data.featureLex
    d = X.shape[1]
    sup = feature_support(X)
    # the count is the document frequency of the feature in the split
    dense_df = np.asarray((X != 0).sum(axis=0)).ravel()
    assert np.array_equal(sup, dense_df)
    g = np.random.RandomState(11)
    m, top = 6, 5
    W = g.standard_normal((d, m)).astype(np.float32)
    feats, scores = feature_topk(W, sup, 5, True, top)
    lines = format_relation_features(feats, scores, sup, lex.get_str_pruned)
    assert len(lines) == m
    strings = [lex.get_str_pruned(f) for f in range(d)]
    assert all(isinstance(s, str) and s for s in strings)
    for k, ln in enumerate(lines):
        assert ln.startswith(f"relation {k}: ")
        rest = ln[len(f"relation {k}: "):]
        # every printed name is the feature's lexicon string, every count its document frequency
        for f, s in zip(feats[k], scores[k]):
            assert f >= 0 and dense_df[f] >= 5
            item = "{}:{:.9g}({})".format(strings[f], float(s), dense_df[f])
            assert rest.startswith(item), (rest, item)
            assert np.float32(float("{:.9g}".format(float(s)))) == s           # round-trips
            rest = rest[len(item) + 1:]
        assert rest == ""
    # without a lexicon: the feature ids; padding is dropped; no support: no count
    feats2 = np.array([[3, 1, -1], [-1, -1, -1]], np.int32)
    scores2 = np.array([[0.5, -2.0, -np.inf], [-np.inf] * 3], np.float32)
    assert format_relation_features(feats2, scores2, np.arange(5)) == \
        ["relation 0: 3:0.5(3) 1:-2(1)", "relation 1:"]
    assert format_relation_features(feats2, scores2, None, {3: "a b", 1: None}) == \
        ["relation 0: a b:0.5 1:-2", "relation 1:"]


# ------------------------------------------------------------------------ 5. the flags
def test_cli_flags_and_inducer_values():
    from rae import inducer
    from rae.cli import get_command_args
    base = ["data.npz", "--model-name", "m", "--decoder", "sp"]
    a = get_command_args(base)
    assert (a.print_features, a.print_features_min_count, a.print_features_raw) == (0, 5, False)
    assert get_command_args(base + ["--print-features"]).print_features == 10
    a = get_command_args(base + ["--print-features", "7", "--print-features-min-count", "2",
                                 "--print-features-raw"])
    assert (a.print_features, a.print_features_min_count, a.print_features_raw) == (7, 2, True)
    mk = lambda **kw: inducer.ReconstructInducer(
        None, {}, None, 1, 0.1, 10, 4, 3, 2, 0.0, 0.0, "adagrad", "m", "sp", False, True, False,
        1.0, **kw)
    with pytest.raises(ValueError, match="print_features"):
        mk(print_features=33)
    with pytest.raises(ValueError, match="print_features_min_count"):
        mk(print_features=3, print_features_min_count=-1)


# ------------------------------------------------------------------------ 6. the rejections
# Made-up addresses: every call below is refused before the first HIP call.  If a check were ever
# lost the call would go on to launch with them, so -- like tests/test_entry_rejections.py -- the
# calls run only where no GPU is visible.
@pytest.fixture(scope="module")
def host_lib(built_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must never reach a visible GPU")
    return built_lib


def _ftopk_args(**kw):
    from rae import _lib
    a = _lib.RaeFtopkArgs()
    a.W, a.n_features, a.relations, a.ldw = 0x100000, 1000, 100, 100
    a.support, a.min_support, a.centre, a.top = 0x200000, 5, 1, 10
    a.feats_out, a.scores_out = 0x300000, 0x400000
    a.workspace, a.workspace_bytes = 0x800000, 1 << 30
    for k, v in kw.items():
        setattr(a, k, v)
    return a


FTOPK_REJECTIONS = [
    (dict(W=None), "W"),
    (dict(relations=0), "relations"),
    (dict(relations=513, ldw=600), "relations"),
    (dict(ldw=99), "ldw"),
    (dict(top=0), "top"),
    (dict(top=33), "top"),
    (dict(n_features=-1), "n_features"),
    (dict(n_features=1 << 31), "n_features"),
    (dict(centre=2), "centre"),
    (dict(feats_out=None), "feats_out"),
    (dict(W=0x100002), "W"),
    (dict(workspace=None), "workspace"),
    (dict(workspace=0x800080), "workspace"),                   # not 256-byte aligned
    (dict(workspace_bytes=0), "workspace_bytes"),
]


@pytest.mark.parametrize("change,word", FTOPK_REJECTIONS,
                         ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in FTOPK_REJECTIONS])
def test_feature_topk_rejections(host_lib, change, word):
    a = _ftopk_args(**change)
    rc = host_lib.rae_feature_topk(C.byref(a), None)
    assert rc == -1
    assert word in host_lib.rae_last_error().decode(), host_lib.rae_last_error()


def test_feature_topk_short_workspace_is_one_byte_short(host_lib):
    a = _ftopk_args()
    need = host_lib.rae_feature_topk_workspace_bytes(C.byref(a))
    a.workspace_bytes = need - 1
    assert host_lib.rae_feature_topk(C.byref(a), None) == -1
    assert "rae_feature_topk_workspace_bytes" in host_lib.rae_last_error().decode()


def test_feature_topk_workspace_bytes(built_lib):
    """Host only (no address is used): strips x relations x top keys, plus 8 bytes per feature in
    centred mode, each block rounded up to 256 bytes; -1 on a bad argument."""
    from rae import _lib
    size = built_lib.rae_feature_topk_workspace_bytes
    al = lambda x: (x + 255) & ~255
    for d in (0, 1, 511, 512, 513, 4097, 65536, 65537, 1 << 20, (1 << 31) - 1):
        strips = _lib.ftopk_strips(d)
        assert 1 <= strips <= _lib.RAE_FT_MAXSTRIPS
        assert strips * _lib.ftopk_strip_rows(d) >= d
        for m, top in ((1, 1), (100, 10), (512, 32)):
            for centre in (0, 1):
                a = _ftopk_args(n_features=d, relations=m, ldw=m, top=top, centre=centre)
                want = al(strips * m * top * 8) + (al(8 * d) if centre else 0)
                assert size(C.byref(a)) == want, (d, m, top, centre)
    assert _lib.ftopk_strips((1 << 31) - 1) == _lib.RAE_FT_MAXSTRIPS
    for change, word in FTOPK_REJECTIONS[1:9]:
        assert size(C.byref(_ftopk_args(**change))) == -1, change
        assert word in built_lib.rae_last_error().decode()
    assert size(None) == -1


SUPPORT_REJECTIONS = [
    (dict(indptr=None), "indptr"),
    (dict(indices=None), "indices"),
    (dict(support=None), "support"),
    (dict(n_features=-1), "n_features"),
    (dict(n_features=1 << 31), "n_features"),
    (dict(row0=-1), "row0"),
    (dict(nrows=-1), "nrows"),
    (dict(nrows=1 << 31), "nrows"),
    (dict(values=0x500002), "values"),
]


@pytest.mark.parametrize("change,word", SUPPORT_REJECTIONS,
                         ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in SUPPORT_REJECTIONS])
def test_feature_support_rejections(host_lib, change, word):
    kw = dict(indptr=0x100000, indices=0x200000, values=0x500000, n_features=1000, row0=0,
              nrows=10, accumulate=0, support=0x300000)
    kw.update(change)
    rc = host_lib.rae_feature_support(kw["indptr"], kw["indices"], kw["values"], kw["n_features"],
                                      kw["row0"], kw["nrows"], kw["accumulate"], kw["support"],
                                      None)
    assert rc == -1
    assert word in host_lib.rae_last_error().decode(), host_lib.rae_last_error()
