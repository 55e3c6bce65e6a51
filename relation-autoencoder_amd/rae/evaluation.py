"""B^3 cluster evaluation of the induced relation assignments
(evaluation/OieEvaluation.py:5-44,90-127,215-220).

Element-level B^3 over the examples that carry a gold label (first label only):
  precision = (1/|A|) sum_{e in A} |C(e) n G(e)| / |C(e) n A|
  recall    = (1/|A|) sum_{e in A} |C(e) n G(e)| / |G(e)|
computed here from the cluster x gold contingency table (same values as the reference's
per-element set intersections, without its O(|A| * |C|) set work).

GoldIndex / contingency_table / b3_from_table are the array form of the same computation: the
gold standard as an id vector, the table by bincount, the metrics from the table.  They are the
host oracle of the device path (rae_cluster_count / rae_b3_metrics, TrainEngine.cluster_metrics).

KeyIndex / row_keys / key_table / topk_from_table / format_cluster_profiles do the same for the
per-cluster profiles (rae_row_keys / rae_cluster_key_count / rae_cluster_topk,
TrainEngine.cluster_profiles).
"""
from __future__ import annotations

import numpy as np


class SingleLabelClusterEvaluation:
    def __init__(self, split_goldstandard, split_label):
        assert split_label in ("train", "valid", "test")
        self.split_label = split_label
        self.numberOfElements = 0
        self.induced_clusters = {}
        self.gold_clusters, self.assessableElemSet = self._parse_first_relation_label(
            split_goldstandard)

    @staticmethod
    def _parse_first_relation_label(relations):
        """OieEvaluation.py:190-210."""
        gold, labeled = {}, set()
        for ex_id, labels in relations.items():
            first = labels[0]
            if first != "":
                labeled.add(ex_id)
                gold.setdefault(first, set()).add(ex_id)
        return gold, labeled

    def feed_induced_clusters(self, response):
        """OieEvaluation.py:23-34: drop empty clusters."""
        self.numberOfElements = 0
        self.induced_clusters = {}
        for cid, members in response.items():
            if len(members) > 0:
                self.numberOfElements += len(members)
                self.induced_clusters[cid] = set(members)

    def _contingency(self):
        gold_of = {}
        for gi, (_, members) in enumerate(sorted(self.gold_clusters.items())):
            for e in members:
                gold_of[e] = gi
        ng = len(self.gold_clusters)
        rows = []
        for _, members in sorted(self.induced_clusters.items()):
            row = np.zeros(ng, dtype=np.float64)
            for e in members:
                g = gold_of.get(e)
                if g is not None:
                    row[g] += 1
            rows.append(row)
        return np.array(rows).reshape(-1, ng)

    def b3_total_element_precision(self):
        n = self._contingency()
        nc = n.sum(axis=1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(nc > 0, n * n / np.where(nc > 0, nc, 1), 0.0)
        return float(t.sum()) / float(len(self.assessableElemSet))

    def b3_total_element_recall(self):
        n = self._contingency()
        sizes = np.array([len(v) for _, v in sorted(self.gold_clusters.items())],
                         dtype=np.float64)
        t = n * n / np.where(sizes > 0, sizes, 1)[None, :]
        return float(t.sum()) / float(len(self.assessableElemSet))

    def compute_metrics(self):
        """OieEvaluation.py:36-44 -> (f1, precision, recall)."""
        if not self.assessableElemSet:
            return 0.0, 0.0, 0.0
        rec = self.b3_total_element_recall()
        pre = self.b3_total_element_precision()
        if rec == 0.0 and pre == 0.0:
            return 0.0, pre, rec
        return (2 * rec * pre) / (rec + pre), pre, rec


def construct_split_evaluator(split_goldstandard, split_label):
    """OieEvaluation.py:220-230."""
    return SingleLabelClusterEvaluation(split_goldstandard or {}, split_label)


class GoldIndex:
    """A split's gold standard as arrays (first label only, as _parse_first_relation_label):
    names  the sorted first-label names (gold class g = names[g]);
    ids    int32, length n_rows: the gold class of example i, -1 when it has no entry, its first
           label is '' or it is not an example id in [0, n_rows);
    sizes  int64 |G_g| and n_assessable |A| over the WHOLE gold standard: examples labelled
           there with ids >= n_rows (the dropped tail) still count, as in the reference."""

    def __init__(self, split_goldstandard, n_rows):
        first = {ex: labels[0] for ex, labels in (split_goldstandard or {}).items()
                 if labels[0] != ""}
        self.names = sorted(set(first.values()))
        col = {name: g for g, name in enumerate(self.names)}
        self.n_rows = int(n_rows)
        self.ids = np.full(self.n_rows, -1, dtype=np.int32)
        self.sizes = np.zeros(len(self.names), dtype=np.int64)
        for ex, name in first.items():
            g = col[name]
            self.sizes[g] += 1
            if isinstance(ex, (int, np.integer)) and 0 <= ex < self.n_rows:
                self.ids[ex] = g
        self.n_assessable = len(first)

    @property
    def n_gold(self):
        return len(self.names)


def contingency_table(labels, gold_index, relations):
    """(relations, n_gold + 1) int64: cell (c, g) counts the examples i < len(labels) with
    labels[i] == c and gold id g; the last column the ones without a gold class.  Labels
    outside [0, relations) are skipped (rae_cluster_count's rule)."""
    lab = np.asarray(labels, dtype=np.int64)
    ng = gold_index.n_gold
    gid = np.asarray(gold_index.ids[:lab.shape[0]], dtype=np.int64)
    if gid.shape[0] != lab.shape[0]:
        raise ValueError(f"{lab.shape[0]} labels for a gold index of {gold_index.n_rows} rows")
    keep = (lab >= 0) & (lab < relations)
    col = np.where((gid >= 0) & (gid < ng), gid, ng)
    cell = lab[keep] * (ng + 1) + col[keep]
    return np.bincount(cell, minlength=relations * (ng + 1)).astype(np.int64).reshape(
        relations, ng + 1)


def b3_from_table(table, sizes, n_assessable):
    """(f1, precision, recall) of a contingency_table: the float64 formulas of
    SingleLabelClusterEvaluation (b3_total_element_precision / _recall, compute_metrics).  A
    cluster without labelled members and a gold class of size 0 add nothing."""
    if n_assessable == 0:
        return 0.0, 0.0, 0.0
    n = np.asarray(table)[:, :-1].astype(np.float64)
    sizes = np.asarray(sizes, dtype=np.float64)
    nc = n.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(nc > 0, n * n / np.where(nc > 0, nc, 1), 0.0)
    pre = float(t.sum()) / float(n_assessable)
    t = np.where(sizes > 0, n * n / np.where(sizes > 0, sizes, 1)[None, :], 0.0)
    rec = float(t.sum()) / float(n_assessable)
    if rec == 0.0 and pre == 0.0:
        return 0.0, pre, rec
    return (2 * rec * pre) / (rec + pre), pre, rec


# ---------------------------------------------------------------------------------------------
# argument ranking over all entities (rae_eval_rank): the numpy oracle of its summary kernel
# ---------------------------------------------------------------------------------------------
def rank_summary(greater, equal, target, lse, ks=(1, 10, 100)):
    """The 16 doubles rae_eval_rank's summary kernel writes, from its per-query outputs (each
    (nrows, 2): column t - 1 = the side whose argument is replaced).  In float64:
        rank = 1 + greater + equal / 2        logp = target - logaddexp(target, lse)
    out[8 side + j]: j = 0 sum 1/rank, 1 sum rank, 2 sum logp, 3..6 the number of rows with
    rank <= ks[j - 3] (up to four ks; a k <= 0 or a missing one counts nothing), 7 nrows."""
    ks = list(ks)
    if len(ks) > 4:
        raise ValueError("at most four hit thresholds")
    g = np.asarray(greater, dtype=np.float64).reshape(-1, 2)
    e = np.asarray(equal, dtype=np.float64).reshape(-1, 2)
    u = np.asarray(target, dtype=np.float64).reshape(-1, 2)
    l = np.asarray(lse, dtype=np.float64).reshape(-1, 2)
    rank = 1.0 + g + 0.5 * e
    with np.errstate(invalid="ignore"):
        logp = np.where(np.isneginf(l), 0.0, u - np.logaddexp(u, l))
    out = np.zeros(16, np.float64)
    for side in range(2):
        out[8 * side + 0] = (1.0 / rank[:, side]).sum()
        out[8 * side + 1] = rank[:, side].sum()
        out[8 * side + 2] = logp[:, side].sum()
        for j, k in enumerate(ks):
            if k > 0:
                out[8 * side + 3 + j] = float((rank[:, side] <= k).sum())
        out[8 * side + 7] = float(rank.shape[0])
    return out


# ---------------------------------------------------------------------------------------------
# per-cluster profiles (Visualizator.print_clusters, evaluation/Visuals.py:8-45): for every
# induced relation the most frequent triggers (or gold labels) of its members
# ---------------------------------------------------------------------------------------------
class KeyIndex:
    """What print_clusters counts, as arrays (the analogue of GoldIndex):
    key_of_feature  int32, length d: the key a feature carries, -1 for none -- an example's key
                    is that of its first keyed stored column (get_example_feature,
                    learning/OieData.py:100-106); None for an index made by from_gold;
    names           the keys' display strings (key k prints as names[k]);
    rows            None, or (from_gold) the per-row keys themselves, int32."""

    def __init__(self, key_of_feature, names, rows=None):
        self.key_of_feature = None if key_of_feature is None else \
            np.ascontiguousarray(key_of_feature, dtype=np.int32)
        self.names = list(names)
        self.rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)

    @property
    def n_keys(self):
        return len(self.names)

    @classmethod
    def from_lexicon(cls, lex, token="trigger"):
        """The reference's rule: a feature carries a key iff its pruned string s has
        s.find(token) > -1 (OieData.py:104); it displays as s.replace(token + '#', '')
        (Visuals.py:64).  Features with equal display strings share a key (the reference's
        Counter counts strings); keys are numbered by the smallest feature id carrying them."""
        d = int(lex.get_feature_space_dimensionality())
        kof = np.full(d, -1, dtype=np.int32)
        names, key_of_name = [], {}
        for f in range(d):
            s = lex.get_str_pruned(f)
            if s is None or s.find(token) < 0:
                continue
            name = s.replace(token + "#", "")
            k = key_of_name.get(name)
            if k is None:
                k = key_of_name[name] = len(names)
                names.append(name)
            kof[f] = k
        return cls(kof, names)

    @classmethod
    def from_mask(cls, mask, names=None):
        """Every feature with mask[f] set is a key of its own, numbered in feature order;
        names default to the feature ids as strings."""
        mask = np.asarray(mask, dtype=bool)
        feats = np.flatnonzero(mask)
        kof = np.full(mask.shape[0], -1, dtype=np.int32)
        kof[feats] = np.arange(feats.shape[0], dtype=np.int32)
        if names is None:
            names = [str(int(f)) for f in feats]
        if len(names) != feats.shape[0]:
            raise ValueError(f"{len(names)} names for {feats.shape[0]} keyed features")
        return cls(kof, names)

    @classmethod
    def from_gold(cls, gold_split, n_rows):
        """print_clusters(goldstandard=...) (Visuals.py:24-25,52-53): an example's key is its
        first gold label, the empty label '' included (the reference's Counter drops None
        only).  Keys are numbered by the smallest row carrying them; rows without an entry
        get -1."""
        rows = np.full(int(n_rows), -1, dtype=np.int32)
        names, key_of_name = [], {}
        for ex in sorted(e for e in (gold_split or {})
                         if isinstance(e, (int, np.integer)) and 0 <= e < n_rows):
            name = gold_split[ex][0]
            k = key_of_name.get(name)
            if k is None:
                k = key_of_name[name] = len(names)
                names.append(name)
            rows[ex] = k
        return cls(None, names, rows)


def row_keys(X, key_of_feature, use_values=True):
    """The host oracle of rae_row_keys: int32 per row of the CSR matrix X, the key of its first
    stored column (CSR order) that carries one, -1 for none.  use_values: a stored 0 is not a
    column of the row (scipy's nonzero()); False = rae_row_keys with values == NULL."""
    kof = np.asarray(key_of_feature, dtype=np.int64)
    indptr = np.asarray(X.indptr, dtype=np.int64)
    idx = np.asarray(X.indices, dtype=np.int64)
    inr = (idx >= 0) & (idx < kof.shape[0])
    k = np.full(idx.shape[0], -1, dtype=np.int64)
    k[inr] = kof[idx[inr]]
    ok = k >= 0
    if use_values:
        ok &= np.asarray(X.data) != 0
    pos = np.flatnonzero(ok)                                # positions that carry a key
    j = np.searchsorted(pos, indptr[:-1], side="left")      # the first one at or after the row
    nxt = np.append(pos, idx.shape[0])[j]                  # nnz when there is none
    hit = nxt < indptr[1:]
    out = np.full(indptr.shape[0] - 1, -1, dtype=np.int32)
    out[hit] = k[nxt[hit]]
    return out


def key_table(labels, keys, relations, n_keys):
    """(relations, n_keys) int32: cell (c, k) counts the rows with labels[i] == c and
    keys[i] == k; rows with either out of range are skipped (rae_cluster_key_count)."""
    lab = np.asarray(labels, dtype=np.int64)
    key = np.asarray(keys, dtype=np.int64)
    if lab.shape != key.shape:
        raise ValueError(f"{lab.shape[0]} labels for {key.shape[0]} keys")
    keep = (lab >= 0) & (lab < relations) & (key >= 0) & (key < n_keys)
    cell = lab[keep] * n_keys + key[keep]
    return np.bincount(cell, minlength=relations * n_keys).astype(np.int32).reshape(
        relations, n_keys)


def topk_from_table(table, top):
    """(keys, counts), both (relations, top) int32: per row the cells with count > 0 by count
    descending, then key ascending, cut to `top` and padded with (-1, 0) (rae_cluster_topk)."""
    table = np.asarray(table)
    m = table.shape[0]
    keys = np.full((m, top), -1, dtype=np.int32)
    counts = np.zeros((m, top), dtype=np.int32)
    for c in range(m):
        row = table[c].astype(np.int64)
        nz = np.flatnonzero(row > 0)
        order = nz[np.lexsort((nz, -row[nz]))][:top]
        keys[c, :order.shape[0]] = order
        counts[c, :order.shape[0]] = row[order]
    return keys, counts


def format_cluster_profiles(keys, counts, names):
    """One line per cluster id 0..m-1 (empty clusters included) as print_clusters renders it:
    `print cl_id,` then ' '.join(map(str, [(name, freq), ...])) -- the id, a space, the tuples
    joined by spaces (an empty cluster's line is the id and the space)."""
    lines = []
    for c in range(len(keys)):
        items = [(names[int(k)], int(n)) for k, n in zip(keys[c], counts[c]) if k >= 0]
        lines.append(f"{c} " + " ".join(map(str, items)))
    return lines


# ------------------------------------------------------------------ top-k entity retrieval
def topk_from_scores(g, top, skip=None):
    """(ents, scores) of rae_topk_queries from the (nq, n) score matrix g: per row the entities
    other than skip[q] (skip outside [0, n): nothing is skipped) whose score is not NaN, ordered by
    score descending, then entity ascending, cut to `top` and padded with (-1, -inf).  -0.0 is
    +0.0, in the order and in the output.  ents int32 (nq, top), scores g's dtype."""
    g = np.array(g, copy=True)
    if g.dtype.kind != "f":
        g = g.astype(np.float64)
    nq, n = g.shape
    g = np.where(g == 0, g.dtype.type(0), g)                  # -0 -> +0
    ents = np.full((nq, top), -1, dtype=np.int32)
    scores = np.full((nq, top), -np.inf, dtype=g.dtype)
    sk = None if skip is None else np.asarray(skip).astype(np.int64)
    for q in range(nq):
        row = g[q]
        keep = ~np.isnan(row)
        if sk is not None and 0 <= sk[q] < n:
            keep[sk[q]] = False
        cand = np.flatnonzero(keep)
        order = cand[np.lexsort((cand, -row[cand]))][:top]
        ents[q, :order.shape[0]] = order
        scores[q, :order.shape[0]] = row[order]
    return ents, scores


def entity_name(names, e):
    """The string of entity id e: names[e] of a mapping or sequence (DatasetManager.id2Arg), or
    the id itself when there is none."""
    e = int(e)
    if names is not None:
        try:
            s = names[e]
            if s is not None:
                return str(s)
        except (KeyError, IndexError):
            pass
    return str(e)


def _topk_pairs(ents, scores, names):
    # %.9g round-trips a float32
    return ["{}:{:.9g}".format(entity_name(names, e), float(s))
            for e, s in zip(ents, scores) if e >= 0]


def format_relation_preferences(ents, scores, names=None):
    """ents / scores (2, m, top) of TrainEngine.relation_preferences -> one line per relation and
    slot, tab-separated: 'preferences', the relation id, the slot (1 or 2), then entity:score
    pairs, best first (padding is not printed)."""
    ents, scores = np.asarray(ents), np.asarray(scores)
    lines = []
    for k in range(ents.shape[1]):
        for t in range(2):
            lines.append("\t".join(["preferences", str(k), str(t + 1)] +
                                   _topk_pairs(ents[t, k], scores[t, k], names)))
    return lines


# ------------------------------------------------------------------ relation feature profiles
def feature_support(X, use_values=True, n_features=None):
    """The host oracle of rae_feature_support: int32 per feature, the number of stored entries of
    the CSR matrix X in its column whose value is non-zero -- the feature's document frequency.
    use_values=False counts every stored entry (values == NULL).  Columns outside
    [0, n_features) (default: X's width) are skipped."""
    d = int(X.shape[1] if n_features is None else n_features)
    idx = np.asarray(X.indices, dtype=np.int64)
    keep = (idx >= 0) & (idx < d)
    if use_values:
        keep &= np.asarray(X.data) != 0
    return np.bincount(idx[keep], minlength=d).astype(np.int32)[:d]


def tree_row_sum(W):
    """The row sums of W (d, m) in float64 in the order rae_b3_metrics and rae_feature_topk use:
    lane j of 64 adds columns j, j + 64, ... in ascending order from 0.0, then the 64 lane sums
    fold by the xor tree 32, 16, ..., 1 (every lane adds its partner's value).  A function of m
    alone; bit for bit the device's."""
    W = np.asarray(W)
    if W.ndim != 2:
        raise ValueError("W must be (d, m)")
    d, m = W.shape
    lanes = np.zeros((d, 64), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, m, 64):
            w = min(64, m - c0)
            lanes[:, :w] = lanes[:, :w] + W[:, c0:c0 + w].astype(np.float64)
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, idx ^ o]
    return lanes[:, 0].copy()


def feature_scores(W, centre=True):
    """score(f, k) of rae_feature_topk, float32 (d, m): W itself, or centred
    (float)((double)W[f, k] - tree_row_sum(W)[f] / m) with one rounding to float32."""
    W = np.asarray(W, dtype=np.float32)
    if not centre:
        return W.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        mean = tree_row_sum(W) / np.float64(W.shape[1])
        return (W.astype(np.float64) - mean[:, None]).astype(np.float32)


def feature_topk(W, support=None, min_support=0, centre=True, top=10):
    """The host oracle of rae_feature_topk: (feats int32, scores float32), both (m, top).  Row k:
    the features f with support[f] >= min_support (support None: all) whose score is not NaN,
    by score descending, then feature ascending, cut to `top` and padded with (-1, -inf).
    -0.0 is +0.0, in the order and in the output."""
    W = np.asarray(W, dtype=np.float32)
    d, m = W.shape
    s = feature_scores(W, centre)
    s = np.where(s == 0, np.float32(0), s)                    # -0 -> +0
    ok = np.ones(d, dtype=bool) if support is None else \
        np.asarray(support)[:d].astype(np.int64) >= int(min_support)
    feats = np.full((m, top), -1, dtype=np.int32)
    scores = np.full((m, top), -np.inf, dtype=np.float32)
    for k in range(m):
        col = s[:, k]
        cand = np.flatnonzero(ok & ~np.isnan(col))
        order = cand[np.lexsort((cand, -col[cand]))][:top]
        feats[k, :order.shape[0]] = order
        scores[k, :order.shape[0]] = col[order]
    return feats, scores


def format_relation_features(feats, scores, support, names=None):
    """feats / scores (m, top) of TrainEngine.relation_features -> one line per relation:
    'relation k: name:score(count) ...', best first.  name is names(f) of a callable or names[f]
    of a mapping / sequence (the lexicon's pruned strings), the feature id where there is none;
    count is support[f] (support None: no count).  Padding is not printed."""
    feats, scores = np.asarray(feats), np.asarray(scores)
    lines = []
    for k in range(feats.shape[0]):
        items = []
        for f, s in zip(feats[k], scores[k]):
            if f < 0:
                continue
            name = None
            if callable(names):
                name = names(int(f))
            elif names is not None:
                name = entity_name(names, f)
            name = str(int(f)) if name is None else str(name)
            cnt = "" if support is None else "({})".format(int(support[int(f)]))
            items.append("{}:{:.9g}{}".format(name, float(s), cnt))      # %.9g round-trips a float32
        lines.append("relation {}: {}".format(k, " ".join(items)).rstrip())
    return lines


# ------------------------------------------------------------------ cluster exemplars
def label_stats(X, W, Wb, dtype=np.float32):
    """The host oracle of rae_label_stats: (labels int64, margin, pmax) of every row of the CSR
    matrix X with S = X W + Wb computed in `dtype` (float32: the device's formats; float64: the
    reference a rounding bound is measured against).
      labels  np.argmax: the first maximum, NaN counting as the maximum.
      margin  S[label] - S[second], second the argmax over the columns k != label; +inf with one
              relation; NaN whenever the subtraction is (a NaN logit, inf - inf).
      pmax    exp(S[label] - best) / sum_k exp(S[k] - best), best = S[label]."""
    W = np.asarray(W, dtype=dtype)
    Wb = np.asarray(Wb, dtype=dtype).reshape(-1)
    N, m = X.shape[0], W.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        S = np.asarray(X.astype(dtype) @ W, dtype=dtype).reshape(N, m) + Wb[None, :]
        rows = np.arange(N)
        labels = np.argmax(S, axis=1).astype(np.int64) if N else np.zeros(0, np.int64)
        best = S[rows, labels]
        if m == 1:
            margin = np.full(N, np.inf, dtype=dtype)
        else:
            own = np.zeros(S.shape, dtype=bool)
            own[rows, labels] = True
            nan = np.isnan(S)
            # the maximum over the other columns, NaN counting as the maximum
            second = np.where((nan & ~own).any(axis=1), np.nan,
                              np.where(own | nan, -np.inf, S).max(axis=1)).astype(dtype)
            margin = (best - second).astype(dtype)
        e = np.exp((S - best[:, None]).astype(dtype)).astype(dtype)
        pmax = (np.exp((best - best).astype(dtype)).astype(dtype) / e.sum(axis=1, dtype=dtype))
    return labels, margin.astype(dtype), pmax.astype(dtype)


def cluster_exemplars(labels, scores, relations, top, largest=True):
    """The host oracle of rae_cluster_exemplars: (rows int32, scores float32), both (relations,
    top).  Row c: the rows i with labels[i] == c whose score is not NaN, by score (descending for
    largest, else ascending), then row ascending, cut to `top` and padded with (-1, -inf).  -0.0 is
    +0.0, in the order and in the output; labels outside [0, relations) are skipped."""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    s = np.where(s == 0, np.float32(0), s)                    # -0 -> +0
    relations, top = int(relations), int(top)
    rows_out = np.full((relations, top), -1, dtype=np.int32)
    scores_out = np.full((relations, top), -np.inf, dtype=np.float32)
    cand = np.flatnonzero((labels >= 0) & (labels < relations) & ~np.isnan(s))
    order = cand[np.lexsort((cand, -s[cand] if largest else s[cand], labels[cand]))]
    lab = labels[order]
    start = np.searchsorted(lab, np.arange(relations), side="left")
    stop = np.searchsorted(lab, np.arange(relations), side="right")
    for c in range(relations):
        take = order[start[c]:min(stop[c], start[c] + top)]
        rows_out[c, :take.shape[0]] = take
        scores_out[c, :take.shape[0]] = s[take]
    return rows_out, scores_out


def format_cluster_exemplars(rows, scores, sizes, args1, args2, entity_names=None, row_keys=None,
                             key_names=None):
    """rows / scores (m, top) of TrainEngine.cluster_exemplars -> one line per relation:
    'relation k (n rows): row:e1 | trigger | e2:score ...', first exemplar first; n = sizes[k].
    e1 / e2 are args1[row] / args2[row] through entity_name; the trigger is key_names[row_keys[row]]
    ('-' for a row without a key) and is omitted with its bars when row_keys is None.  Padding is
    not printed."""
    rows, scores = np.asarray(rows), np.asarray(scores)
    lines = []
    for k in range(rows.shape[0]):
        items = []
        for i, s in zip(rows[k], scores[k]):
            if i < 0:
                continue
            i = int(i)
            mid = ""
            if row_keys is not None:
                key = int(row_keys[i])
                name = "-" if key < 0 else (str(key) if key_names is None else str(key_names[key]))
                mid = " {} |".format(name)
            items.append("{}:{} |{} {}:{:.9g}".format(                # %.9g round-trips a float32
                i, entity_name(entity_names, args1[i]), mid,
                entity_name(entity_names, args2[i]), float(s)))
        lines.append("relation {} ({} rows): {}".format(k, int(sizes[k]), " ".join(items)).rstrip())
    return lines


# ------------------------------------------------------------------ relation scores from the decoder
def relation_scores(params, decoder, e1, e2):
    """psi (nq, m) float64, the oracle of rae_relation_scores: the decoder's score of every
    relation k for the pairs (e1[q], e2[q]), a1 = A[e1], a2 = A[e2]:
        sp          <C1[:,k], a1> + <C2[:,k], a1>     (A[args1] twice, as the objective scores it)
        rescal      a1^T R[:,:,k] a2
        rescal+sp   a1^T C[:,:,k] a2 + <C1[:,k], a1> + <C2[:,k], a2>
    params: name -> array (A (n, r); C1, C2 (r, m); R or C (r, r, m)).  Ids out of range raise
    IndexError."""
    if decoder not in ("sp", "rescal", "rescal+sp"):
        raise ValueError(f"unknown decoder {decoder!r}")
    A = np.asarray(params["A"], dtype=np.float64)
    e1 = np.asarray(e1).astype(np.int64).reshape(-1)
    e2 = np.asarray(e2).astype(np.int64).reshape(-1)
    for e in (e1, e2):
        if e.size and (e.min() < 0 or e.max() >= A.shape[0]):
            raise IndexError(f"entity ids must be in [0, {A.shape[0]})")
    a1, a2 = A[e1], A[e2]
    if decoder == "sp":
        return a1 @ np.asarray(params["C1"], np.float64) + a1 @ np.asarray(params["C2"], np.float64)
    R = np.asarray(params["R" if decoder == "rescal" else "C"], dtype=np.float64)
    psi = np.einsum("bi,ijk,bj->bk", a1, R, a2, optimize=True)
    if decoder == "rescal+sp":
        psi = psi + a1 @ np.asarray(params["C1"], np.float64) \
            + a2 @ np.asarray(params["C2"], np.float64)
    return psi


def log_sigmoid(x):
    """log(sigmoid(x)) = -softplus(-x), float64, stable."""
    x = np.asarray(x, dtype=np.float64)
    return -(np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x))))


def joint_scores(logits, psi, Ab, e1, e2):
    """J (nrows, m) float64, the oracle of rae_eval_relations' joint output:
    J_k = logsoftmax_k(logits) + logsig(psi_k + Ab[e1]) + logsig(psi_k + Ab[e2]), the
    log-softmax as z_k - log sum exp z with z = logits - max logits."""
    S = np.asarray(logits, dtype=np.float64)
    psi = np.asarray(psi, dtype=np.float64)
    Ab = np.asarray(Ab, dtype=np.float64).reshape(-1)
    z = S - S.max(axis=1, keepdims=True)
    lsm = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    b1 = Ab[np.asarray(e1).astype(np.int64)][:, None]
    b2 = Ab[np.asarray(e2).astype(np.int64)][:, None]
    return lsm + log_sigmoid(psi + b1) + log_sigmoid(psi + b2)


def format_relation_predictions(e1, e2, enc_labels, enc_probs, psi, joint_labels, top,
                                names=None, row0=0):
    """One line per row, tab-separated: 'relations', the row, the two entities, the encoder's
    label as k:probability, the `top` relations by psi as k:psi (best first, ties by relation
    ascending), then 'joint' and the joint label."""
    psi = np.asarray(psi)
    lines = []
    for b in range(psi.shape[0]):
        row = psi[b]
        order = np.lexsort((np.arange(row.shape[0]), -row))[:int(top)]
        lines.append("\t".join(
            ["relations", str(row0 + b), entity_name(names, e1[b]), entity_name(names, e2[b]),
             "{}:{:.9g}".format(int(enc_labels[b]), float(enc_probs[b]))] +
            ["{}:{:.9g}".format(int(k), float(row[k])) for k in order] +
            ["joint", str(int(joint_labels[b]))]))
    return lines


def format_argument_predictions(ents, scores, true, names=None, row0=0):
    """ents / scores (nrows, 2, top) of TrainEngine.predict_arguments, true (nrows, 2) the rows'
    arguments -> one line per row and side, tab-separated: 'predictions', the row, the side (1 or
    2), the true argument, then entity:score pairs, best first."""
    ents, scores, true = np.asarray(ents), np.asarray(scores), np.asarray(true)
    lines = []
    for b in range(ents.shape[0]):
        for t in range(2):
            lines.append("\t".join(["predictions", str(row0 + b), str(t + 1),
                                    entity_name(names, true[b, t])] +
                                   _topk_pairs(ents[b, t], scores[b, t], names)))
    return lines
