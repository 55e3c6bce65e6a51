"""Per-cluster profiles, host side (no GPU): rae.evaluation's KeyIndex and numpy oracles
(row_keys, key_table, topk_from_table, format_cluster_profiles) against a Python 3
transliteration of the reference's Visualizator.print_clusters (evaluation/Visuals.py:8-45) and
DatasetManager.get_example_feature (learning/OieData.py:100-106) on the preprocessed sample, and
the argument checks of rae_row_keys / rae_cluster_key_count / rae_cluster_topk."""
import ctypes as C
import operator
from collections import Counter

import numpy as np
import pytest
import scipy.sparse as sp

from _profile_sample import count_rows, sample_data


# ------------------------------------------------- the reference, transliterated line by line
def ref_get_example_feature(dm, an_id, a_split, feature):          # OieData.py:100-106
    for e in dm.split[a_split].xFeats[an_id].nonzero()[1]:
        feat = dm.featureLex.get_str_pruned(e)
        if dm.featureLex.get_str_pruned(e).find(feature) > -1:
            return feat
    return None


def ref_remove_trigger_token(trigger):                              # Visuals.py:60-64
    if trigger is None:
        return None
    return trigger.replace('trigger#', '')


def ref_print_clusters(cluster_sets, dm, split, threshold, goldstandard=None):
    """Visuals.py:22-30,44-45: per cluster id the full Counter and the printed list."""
    if goldstandard is None:
        extractor = lambda x: ref_remove_trigger_token(               # noqa: E731
            ref_get_example_feature(dm, x, split, 'trigger'))
    else:
        extractor = lambda x: goldstandard[split][x][0]               # noqa: E731
    out = {}
    for cl_id, cl_members in cluster_sets.items():
        trig_or_labels = [extractor(idx) for idx in cl_members]
        frequencies = Counter([idx for idx in trig_or_labels if idx is not None])
        _ = sorted(frequencies.items(), key=operator.itemgetter(1), reverse=True)
        out[cl_id] = (frequencies, _[:threshold])
    return out


def _assert_same_up_to_ties(ref, keys, counts, names, table, top):
    """The reference breaks ties by set / dict iteration order, which is no specification: per
    cluster the frequency sequences are equal, the entries strictly above the top-th count are
    the same set, and every other printed entry -- on either side -- really is an entry of the
    cluster with the cutoff count."""
    assert sorted(ref) == list(range(len(keys)))
    for c in range(len(keys)):
        freq, printed = ref[c]
        mine = [(names[k], int(n)) for k, n in zip(keys[c], counts[c]) if k >= 0]
        assert [n for _, n in mine] == [n for _, n in printed], c
        assert len(mine) == min(top, len(freq))
        if not mine:
            continue
        cut = mine[-1][1]
        assert {e for e in mine if e[1] > cut} == {e for e in printed if e[1] > cut}, c
        full = {names[k]: int(n) for k, n in enumerate(table[c]) if n > 0}
        assert full == dict(freq), c
        for name, n in mine + printed:
            assert freq[name] == n and (n > cut or n == cut), (c, name)


# ------------------------------------------------------------------------ 1. the sample
def test_key_index_from_lexicon_on_the_sample():
    from rae.evaluation import KeyIndex, row_keys
    dm, _ = sample_data()
    X = dm.split["train"].xFeats
    assert X.shape == (1000, 6271)
    ki = KeyIndex.from_lexicon(dm.featureLex)
    kof = ki.key_of_feature
    assert kof.dtype == np.int32 and kof.shape == (6271,)
    assert int((kof >= 0).sum()) == 481 and ki.n_keys == 481 == len(set(ki.names))
    per_row = np.asarray((X[:, np.flatnonzero(kof >= 0)] != 0).sum(axis=1)).ravel()
    assert per_row.min() == 1 and per_row.max() == 1          # exactly one trigger feature each
    keys = row_keys(X, kof)
    assert keys.dtype == np.int32 and keys.min() >= 0
    # the reference's rule, feature by feature; keys numbered by the smallest feature id
    first = {}
    for f in range(6271):
        s = dm.featureLex.get_str_pruned(f)
        assert (kof[f] >= 0) == (s.find("trigger") > -1)
        if kof[f] >= 0:
            assert ki.names[kof[f]] == s.replace("trigger#", "")
            first.setdefault(int(kof[f]), f)
    assert [first[k] for k in range(481)] == sorted(first.values())
    for i in (0, 1, 499, 999):
        assert ki.names[keys[i]] == ref_remove_trigger_token(
            ref_get_example_feature(dm, i, "train", "trigger"))


@pytest.mark.parametrize("top", [1, 5, 32])
def test_oracles_match_the_reference_print_clusters(top):
    from rae.evaluation import KeyIndex, key_table, row_keys, topk_from_table
    dm, _ = sample_data()
    X = dm.split["train"].xFeats
    ki = KeyIndex.from_lexicon(dm.featureLex)
    m = 10
    lab = np.random.RandomState(11).randint(0, m, X.shape[0])
    lab[lab == 7] = 3                                          # an empty cluster
    sets = {c: set(np.flatnonzero(lab == c).tolist()) for c in range(m)}
    ref = ref_print_clusters(sets, dm, "train", top)
    table = key_table(lab, row_keys(X, ki.key_of_feature), m, ki.n_keys)
    assert table.sum() == X.shape[0]
    keys, counts = topk_from_table(table, top)
    assert len(ref[7][1]) == 0 and (keys[7] == -1).all() and (counts[7] == 0).all()
    _assert_same_up_to_ties(ref, keys, counts, ki.names, table, top)


def test_from_gold_counts_the_empty_label():
    from rae.evaluation import KeyIndex, key_table, topk_from_table
    gold = {"valid": {0: ["b"], 1: [""], 2: ["a", "b"], 3: [""], 4: ["b"], 5: [""], 7: ["a"],
                      9: ["zz"]}}
    n = 8                                                     # row 6 has no entry, 9 is past n
    ki = KeyIndex.from_gold(gold["valid"], n)
    assert ki.key_of_feature is None
    assert ki.names == ["b", "", "a"]                         # by the smallest row carrying them
    assert ki.rows.tolist() == [0, 1, 2, 1, 0, 1, -1, 2]
    lab = np.array([0, 0, 0, 1, 1, 1, 1, 0])
    keys, counts = topk_from_table(key_table(lab, ki.rows, 2, ki.n_keys), 5)
    sets = {c: set(np.flatnonzero((lab == c) & (ki.rows >= 0)).tolist()) for c in range(2)}
    ref = ref_print_clusters(sets, None, "valid", 5, goldstandard=gold)
    table = key_table(lab, ki.rows, 2, ki.n_keys)
    _assert_same_up_to_ties(ref, keys, counts, ki.names, table, 5)
    assert ref[1][0][""] == 2                                 # '' is counted like any label
    assert KeyIndex.from_gold({}, 3).n_keys == 0 and KeyIndex.from_gold(None, 3).rows.tolist() == [-1] * 3


def test_from_mask():
    from rae.evaluation import KeyIndex
    mask = np.zeros(9, bool)
    mask[[2, 5, 6]] = True
    ki = KeyIndex.from_mask(mask)
    assert ki.key_of_feature.tolist() == [-1, -1, 0, -1, -1, 1, 2, -1, -1]
    assert ki.names == ["2", "5", "6"] and ki.rows is None
    assert KeyIndex.from_mask(mask, ["x", "y", "z"]).names == ["x", "y", "z"]
    with pytest.raises(ValueError):
        KeyIndex.from_mask(mask, ["x"])


# ------------------------------------------------------------- 2. oracles vs brute force
def _random_csr(g, n, d, lengths):
    indptr, idx, val = [0], [], []
    for i in range(n):
        k = lengths[i % len(lengths)]
        cols = np.sort(g.choice(d, size=k, replace=False))
        idx.extend(cols.tolist())
        val.extend(np.where(g.rand(k) < 0.2, 0.0, 1.0).tolist())
        indptr.append(len(idx))
    X = sp.csr_matrix((np.array(val, np.float32), np.array(idx, np.int32),
                       np.array(indptr, np.int32)), shape=(n, d))
    return X


def test_row_keys_matches_a_loop():
    from rae.evaluation import row_keys
    g = np.random.RandomState(3)
    d = 300
    X = _random_csr(g, 200, d, [0, 1, 17, 64, 65, 130])
    assert (X.data == 0).any()                                 # explicit zeros stay stored
    kof = np.where(g.rand(d) < 0.1, g.randint(0, 20, d), -1).astype(np.int32)
    for use_values in (True, False):
        want = []
        for i in range(X.shape[0]):
            k = -1
            for p in range(X.indptr[i], X.indptr[i + 1]):
                if (not use_values or X.data[p] != 0) and kof[X.indices[p]] >= 0:
                    k = kof[X.indices[p]]
                    break
            want.append(k)
        got = row_keys(X, kof, use_values=use_values)
        assert got.tolist() == want
    assert row_keys(X, kof).tolist() != row_keys(X, kof, use_values=False).tolist()
    assert row_keys(X, np.full(d, -1)).tolist() == [-1] * 200
    assert row_keys(X[:0], kof).shape == (0,)


@pytest.mark.parametrize("kind", ["uniform", "zipf", "one-cell", "one-cluster"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 1003)], ids=lambda s: f"m{s[0]}-k{s[1]}")
def test_table_and_topk_match_loops(shape, kind):
    from rae.evaluation import key_table, topk_from_table
    m, nk = shape
    lab, key = count_rows(np.random.RandomState(m + nk), 3000, m, nk, kind)
    want = np.zeros((m, nk), dtype=np.int64)
    for c, k in zip(lab.tolist(), key.tolist()):
        if 0 <= c < m and 0 <= k < nk:
            want[c, k] += 1
    table = key_table(lab, key, m, nk)
    assert table.dtype == np.int32 and np.array_equal(table, want)
    for top in (1, 5, 32):
        keys, counts = topk_from_table(table, top)
        assert keys.shape == counts.shape == (m, top) and keys.dtype == counts.dtype == np.int32
        for c in range(m):
            cells = sorted(((int(n), k) for k, n in enumerate(want[c]) if n > 0),
                           key=lambda e: (-e[0], e[1]))[:top]
            pad = top - len(cells)
            assert keys[c].tolist() == [k for _, k in cells] + [-1] * pad
            assert counts[c].tolist() == [n for n, _ in cells] + [0] * pad
    with pytest.raises(ValueError):
        key_table(lab, key[:-1], m, nk)


def test_topk_orders_large_counts():
    from rae.evaluation import topk_from_table
    t = np.array([[2 ** 30, 2 ** 31 - 1, 0, 2 ** 30]], dtype=np.int32)
    keys, counts = topk_from_table(t, 3)
    assert keys.tolist() == [[1, 0, 3]] and counts.tolist() == [[2 ** 31 - 1, 2 ** 30, 2 ** 30]]


def test_format_cluster_profiles():
    from rae.evaluation import format_cluster_profiles
    names = ["wrote", "born in", "", "it's"]
    keys = np.array([[1, 0, -1], [-1, -1, -1], [3, 2, 0]], dtype=np.int32)
    counts = np.array([[7, 2, 0], [0, 0, 0], [4, 4, 1]], dtype=np.int32)
    assert format_cluster_profiles(keys, counts, names) == [
        "0 ('born in', 7) ('wrote', 2)",
        "1 ",                                   # `print 1,` then the empty join
        "2 (\"it's\", 4) ('', 4) ('wrote', 1)",
    ]


# ---------------------------------------------------------------------- 3. inducer options
def test_print_clusters_by_trigger_needs_a_lexicon():
    """Checked at construction, before anything touches the GPU."""
    from rae.data import synthetic_dataset
    from rae.inducer import ReconstructInducer
    data, gold = synthetic_dataset(200, 100, 3, seed=1)
    args = (data, gold, np.random.RandomState(1), 1, 0.1, 50, 8, 4, 2, 0.0, 0.0, "adagrad", "x",
            "sp", False, True, False, 1.0)
    with pytest.raises(ValueError, match="feature lexicon"):
        ReconstructInducer(*args, device="cpu", print_clusters="device")
    for bad in (dict(print_clusters="on"), dict(print_clusters="host", print_by="label"),
                dict(print_clusters="host", print_by="gold", print_top=33)):
        with pytest.raises(ValueError):
            ReconstructInducer(*args, device="cpu", **bad)


def test_cli_flags():
    from rae.cli import get_command_args
    base = ["x.npz", "--model-name", "n", "--decoder", "sp"]
    a = get_command_args(base)
    assert (a.print_clusters, a.print_top, a.print_by) == ("off", 5, "trigger")
    a = get_command_args(base + ["--print-clusters", "device", "--print-top", "7",
                                 "--print-clusters-by", "gold"])
    assert (a.print_clusters, a.print_top, a.print_by) == ("device", 7, "gold")


# -------------------------------------------------------------------- 4. argument checks
INVALID = -1                                                   # RAE_E_INVALID


def _rejected(lib, rc, word):
    assert rc == INVALID
    assert word.encode() in lib.rae_last_error(), lib.rae_last_error()


def test_entry_points_check_their_arguments(built_lib):
    """Every rejection happens before the first HIP call, so it needs no GPU: the pointers are
    host addresses no kernel ever sees."""
    lib = built_lib
    buf = (C.c_int64 * 8)()
    p = C.c_void_p(C.addressof(buf))
    assert C.addressof(buf) % 8 == 0
    kc = lambda **k: lib.rae_cluster_key_count(*[k.get(a, d) for a, d in (      # noqa: E731
        ("labels", p), ("keys", p), ("nrows", 10), ("m", 4), ("nk", 5), ("acc", 0),
        ("counts", p), ("st", None))])
    _rejected(lib, kc(m=0), "relations")
    _rejected(lib, kc(m=513), "relations")
    _rejected(lib, kc(nk=0), "n_keys")
    _rejected(lib, kc(nk=(1 << 22) + 1), "n_keys")
    _rejected(lib, kc(m=512, nk=(1 << 18) + 1), "2^27")
    _rejected(lib, kc(m=33, nk=1 << 22), "2^27")
    _rejected(lib, kc(nrows=-1), "nrows")
    _rejected(lib, kc(nrows=1 << 31), "nrows")
    for name in ("labels", "keys", "counts"):
        _rejected(lib, kc(**{name: None}), name)
    tk = lambda **k: lib.rae_cluster_topk(*[k.get(a, d) for a, d in (            # noqa: E731
        ("counts", p), ("m", 4), ("nk", 5), ("ld", 5), ("top", 3), ("keys_out", p),
        ("counts_out", p), ("st", None))])
    _rejected(lib, tk(m=0), "relations")
    _rejected(lib, tk(m=513), "relations")
    _rejected(lib, tk(nk=0), "n_keys")
    _rejected(lib, tk(top=0), "top")
    _rejected(lib, tk(top=33), "top")
    _rejected(lib, tk(ld=4), "ld")
    for name in ("counts", "keys_out", "counts_out"):
        _rejected(lib, tk(**{name: None}), name)
    rk = lambda **k: lib.rae_row_keys(*[k.get(a, d) for a, d in (                # noqa: E731
        ("indptr", p), ("indices", p), ("values", None), ("key_of_feature", p), ("d", 10),
        ("row0", 0), ("nrows", 4), ("keys_out", p), ("st", None))])
    _rejected(lib, rk(nrows=-1), "nrows")
    _rejected(lib, rk(nrows=1 << 31), "nrows")
    _rejected(lib, rk(row0=-1), "row0")
    _rejected(lib, rk(d=-1), "n_features")
    for name in ("indptr", "indices", "key_of_feature", "keys_out"):
        _rejected(lib, rk(**{name: None}), name)
