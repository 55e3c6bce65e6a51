"""Shared pieces of the tests of rae_topk_queries / rae_eval_topk (include/rae.h): the ctypes
calls and the comparison of a float32 top-k with float64 scores.

References: rae.evaluation.topk_from_scores (numpy lexsort) on the float64 product for exact
inputs; for real-valued inputs the float64 scores of tests/_rank_ref.py (pinned to the oracle by
tests/test_rank_host.py) through a band around the cut, with test_gpu_eval's tolerances in score
space as tests/_rank_ref.py uses them.
"""
import ctypes as C

import numpy as np

from _rank_ref import MAX_AMBIGUOUS, MAX_WIDTH
from test_gpu_eval import TERM_ATOL, TERM_RTOL

GUARD_ENT = -7


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------- device calls
def topk_queries(lib, dev, Q, A, top, add=None, Ab=None, skip=None, embed=None, scores=True,
                 ws=None):
    """rae_topk_queries on host arrays (Q may be wider than embed: ldq = Q.shape[1]); returns
    (ents, scores or None) as numpy arrays (nq, top).  The workspace is poisoned first and the
    outputs are allocated with a guard row behind them that must survive."""
    import torch
    from rae import _lib
    up = lambda x, dt: None if x is None else torch.as_tensor(
        np.ascontiguousarray(x, dtype=dt), device=dev)
    Q = np.asarray(Q, dtype=np.float32)
    if Q.shape[1] % 4:                    # ldq % 4 == 0: columns past embed that are never read
        Q = np.concatenate([Q, np.full((Q.shape[0], 4 - Q.shape[1] % 4), 1000.0, np.float32)],
                           axis=1)
    tQ, tA = up(Q, np.float32), up(A, np.float32)
    ta, tb, ts = up(add, np.float32), up(Ab, np.float32), up(skip, np.int32)
    nq = int(tQ.shape[0])
    a = _lib.RaeTopkArgs()
    a.Q, a.ldq, a.nq = _lib.ptr(tQ), int(tQ.shape[1]), nq
    a.add, a.skip = _lib.ptr(ta), _lib.ptr(ts)
    a.A, a.Ab = _lib.ptr(tA), _lib.ptr(tb)
    a.n_entities, a.embed = int(tA.shape[0]), int(tA.shape[1] if embed is None else embed)
    a.top = int(top)
    assert tA.shape[1] == a.embed
    need = int(lib.rae_topk_workspace_bytes(C.byref(a), None, int(top)))
    assert need > 0, lib.rae_last_error()
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ws.fill_(0xFF)
    en = torch.full((nq + 1, top), GUARD_ENT, dtype=torch.int32, device=dev)
    sc = torch.full((nq + 1, top), float("nan"), dtype=torch.float32, device=dev) if scores else None
    a.ents_out, a.scores_out = _lib.ptr(en), _lib.ptr(sc)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), int(ws.numel())
    _lib.check(lib.rae_topk_queries(C.byref(a), None), "rae_topk_queries")
    torch.cuda.synchronize()
    en = en.cpu().numpy()
    assert (en[nq] == GUARD_ENT).all()
    if scores:
        sc = sc.cpu().numpy()
        assert np.isnan(sc[nq]).all()
    return en[:nq], (sc[:nq] if scores else None)


class DeviceTopk:
    """rae_eval_topk calls on a DeviceEval's problem (tests/_entry_ref.py) with a workspace of
    its own."""

    def __init__(self, de, top_max=32):
        import torch
        self.de = de
        a = de.args(0, 0)
        need = int(de.lib.rae_topk_workspace_bytes(None, C.byref(a), top_max))
        assert need > 0, de.lib.rae_last_error()
        self.ws = torch.empty(need, dtype=torch.uint8, device=de.dev)

    def run(self, row0, nrows, top, skip_true, scores=True):
        """(ents, scores or None) numpy (nrows, 2, top)."""
        import torch
        de, L = self.de, self.de._lib
        a = de.args(row0, nrows)
        a.neg_samples, a.neg1, a.neg2, a.neg_stride = 0, None, None, 0
        a.terms_out, a.sums_out = None, None
        self.ws.fill_(0xFF)
        a.workspace, a.workspace_bytes = L.ptr(self.ws), int(self.ws.numel())
        en = torch.full((nrows + 1, 2, top), GUARD_ENT, dtype=torch.int32, device=de.dev)
        sc = torch.full((nrows + 1, 2, top), float("nan"), dtype=torch.float32,
                        device=de.dev) if scores else None
        o = L.RaeTopkOut()
        o.ents, o.scores, o.top, o.skip_true = L.ptr(en), L.ptr(sc), int(top), int(skip_true)
        L.check(de.lib.rae_eval_topk(C.byref(a), C.byref(o), None), "rae_eval_topk")
        torch.cuda.synchronize()
        en = en.cpu().numpy()
        assert (en[nrows] == GUARD_ENT).all()
        return en[:nrows], (sc.cpu().numpy()[:nrows] if scores else None)


# ----------------------------------------------------------------- float32 top-k vs float64
def _cut_and_tol(g, top, skip):
    """g (nq, n) float64 -> (gm, cut, tol): the scores with the skipped entity at -inf, the
    top-th best score per query (-inf when there are fewer candidates) and
    tol = TERM_ATOL + TERM_RTOL max(|cut|, |g|) per (query, entity)."""
    gm = np.array(g, dtype=np.float64, copy=True)
    nq, n = gm.shape
    if skip is not None:
        sk = np.asarray(skip).astype(np.int64)
        ok = (sk >= 0) & (sk < n)
        gm[np.nonzero(ok)[0], sk[ok]] = -np.inf
    srt = -np.sort(-gm, axis=1)
    cut = srt[:, top - 1] if top <= n else np.full(nq, -np.inf)
    with np.errstate(invalid="ignore"):
        big = np.maximum(np.abs(cut)[:, None], np.abs(gm))
    tol = TERM_ATOL + TERM_RTOL * np.where(np.isfinite(big), big, 0.0)
    return gm, cut, tol


def assert_band_cap(g, top, skip, what):
    """The leniency of the comparison, bounded on the float64 reference alone: at most
    MAX_AMBIGUOUS of the queries have an entity other than the cut entity in the band
    (cut - tol, cut + tol], and no band holds more than MAX_WIDTH."""
    gm, cut, tol = _cut_and_tol(g, top, skip)
    c = cut[:, None]
    fin = np.isfinite(c) & np.isfinite(gm)
    inband = fin & (gm > c - tol) & (gm <= c + tol)
    others = inband.sum(axis=1) - np.isfinite(cut)            # the cut entity is in its own band
    share = float((others > 0).mean()) if others.size else 0.0
    width = int(others.max()) if others.size else 0
    print(f"{what}: ambiguous queries {100 * share:.2f} %, widest band {width}")
    assert share <= MAX_AMBIGUOUS, (what, share)
    assert width <= MAX_WIDTH, (what, width)


def check_topk_against_float64(ents, scores, g, top, skip, what):
    """ents / scores (nq, top) of the device against g (nq, n) float64: every entity with
    g > cut + tol is returned; every returned entity has g >= cut - tol; every returned score
    is within tol of its entity's g; rows are non-increasing, without duplicates, and padded
    exactly when there are fewer than `top` candidates."""
    gm, cut, tol = _cut_and_tol(g, top, skip)
    nq, n = gm.shape
    ncand = np.isfinite(gm).sum(axis=1) if skip is not None else np.full(nq, n)
    worst = 0.0
    for q in range(nq):
        k = int(min(top, ncand[q]))
        e, s = ents[q], scores[q]
        assert (e[k:] == -1).all() and np.isneginf(s[k:]).all(), (what, q, "padding")
        e, s = e[:k].astype(np.int64), s[:k].astype(np.float64)
        assert (e >= 0).all() and (e < n).all(), (what, q)
        assert len(set(e.tolist())) == k, (what, q, "duplicate entity")
        assert (np.diff(s) <= 0).all(), (what, q, "not sorted")
        if skip is not None:
            assert int(skip[q]) not in e.tolist(), (what, q, "skipped entity returned")
        must = np.flatnonzero(gm[q] > cut[q] + tol[q])
        assert np.isin(must, e).all(), (what, q, "a clearly better entity is missing")
        assert (gm[q, e] >= cut[q] - tol[q, e]).all(), (what, q, "a clearly worse entity returned")
        err = np.abs(s - gm[q, e])
        assert (err <= tol[q, e]).all(), (what, q, err.max())
        worst = max(worst, float(err.max()) if k else 0.0)
    print(f"{what}: {nq} queries, max |score - float64| {worst:.3e}")
