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
