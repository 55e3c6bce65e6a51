"""Shared pieces of the tests of rae_rank_queries / rae_eval_rank (include/rae.h): a float64
restatement of the query table, the interval logic that compares integer counts computed in
float32 with float64 scores, the float64 log-sum-exp, and the ctypes calls.

Reference: the table in include/rae.h (rae_eval_rank), pinned by tests/test_rank_host.py to
oracle/rae_oracle.py's train_step_grads with every entity given as a negative.  Tolerances are
test_gpu_eval's TERM_RTOL / TERM_ATOL: they bound per-example log-sigmoids of the scores, and
|d logsig / dx| <= 1, so a score within them is what those tests already ask of the kernels.
"""
import ctypes as C

import numpy as np

from test_gpu_eval import TERM_ATOL, TERM_RTOL

DEC_ID = {"sp": 0, "rescal": 1, "rescal+sp": 2}
MAX_AMBIGUOUS = 0.10          # share of a case's queries whose interval may be open
MAX_WIDTH = 4                 # widest interval


# ----------------------------------------------------------------------- float64 restatement
def queries64(dec, p, X, e1, e2):
    """q (l, 2, r), c (l, 2), u (l, 2), true (l, 2) of the rows of X in float64: side t - 1
    replaces argument t (include/rae.h, rae_eval_rank)."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    S = np.asarray(X.astype(np.float64) @ p["W"]) + p["Wb"]
    z = S - S.max(axis=1, keepdims=True)
    P = np.exp(z)
    P /= P.sum(axis=1, keepdims=True)
    A, Ab = p["A"], p["Ab"]
    a1, a2 = A[e1], A[e2]
    if dec != "rescal":
        wC1, wC2 = P @ p["C1"].T, P @ p["C2"].T
    if dec == "sp":
        q1, q2 = wC1, wC2
        c1, c2 = (wC2 * a1).sum(axis=1), (wC1 * a1).sum(axis=1)
        one = c1 + c2
    else:
        R = p["R"] if dec == "rescal" else p["C"]
        M = np.einsum("bk,ijk->bij", P, R)
        q1 = np.einsum("bij,bj->bi", M, a2)
        q2 = np.einsum("bij,bi->bj", M, a1)
        if dec == "rescal+sp":
            q1, q2 = q1 + wC1, q2 + wC2
            c1, c2 = (wC2 * a2).sum(axis=1), (wC1 * a1).sum(axis=1)
            one = (a1 * q1).sum(axis=1) + c1
        else:
            c1 = c2 = np.zeros(len(e1))
            one = (a1 * q1).sum(axis=1)
    q = np.stack([q1, q2], axis=1)
    c = np.stack([c1, c2], axis=1)
    u = np.stack([one + Ab[e1], one + Ab[e2]], axis=1)
    true = np.stack([np.asarray(e1), np.asarray(e2)], axis=1).astype(np.int64)
    return q, c, u, true


def scores64(q, c, A, Ab):
    """g[b, t, e] = <A[e], q[b, t]> + c[b, t] + Ab[e]."""
    A, Ab = np.asarray(A, np.float64), np.asarray(Ab, np.float64)
    return np.einsum("btr,er->bte", q, A) + c[:, :, None] + Ab[None, None, :]


def intervals(g, u, true):
    """(lo, hi) per query: lo = #{g > u + tol}, hi = #{g > u - tol} over the entities other than
    the true one, tol = TERM_ATOL + TERM_RTOL max(|u|, |g|).  A float32 evaluation whose scores
    are within tol of the float64 ones has lo <= greater and greater + equal <= hi."""
    uu = u[..., None]
    tol = TERM_ATOL + TERM_RTOL * np.maximum(np.abs(uu), np.abs(g))
    keep = np.ones(g.shape, bool)
    np.put_along_axis(keep, true[..., None], False, axis=-1)
    lo = ((g > uu + tol) & keep).sum(axis=-1)
    hi = ((g > uu - tol) & keep).sum(axis=-1)
    return lo, hi


def assert_cap(lo, hi, what):
    """The leniency of the interval test is bounded on the float64 reference alone."""
    share = float((hi > lo).mean()) if lo.size else 0.0
    width = int((hi - lo).max()) if lo.size else 0
    print(f"{what}: ambiguous queries {100 * share:.2f} %, widest interval {width}")
    assert share <= MAX_AMBIGUOUS, (what, share)
    assert width <= MAX_WIDTH, (what, width)


def lse64(g, true):
    """log sum over the entities other than the true one of exp g (-inf when there is none)."""
    gg = np.array(g, dtype=np.float64, copy=True)
    np.put_along_axis(gg, true[..., None], -np.inf, axis=-1)
    m = gg.max(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(np.isneginf(m), 0.0,
                     np.exp(gg - np.where(np.isneginf(m), 0.0, m)[..., None]).sum(axis=-1))
        return np.where(np.isneginf(m), -np.inf, m + np.log(s))


def counts_exact(Q, A, add, Ab, target, skip):
    """greater / equal of rae_rank_queries on small-integer-valued inputs (float64 holds every
    sum exactly)."""
    Q, A = np.asarray(Q).astype(np.float64), np.asarray(A).astype(np.float64)
    assert np.array_equal(Q, np.round(Q)) and np.array_equal(A, np.round(A))
    nq, n = Q.shape[0], A.shape[0]
    g = Q @ A.T
    if add is not None:
        g = g + np.asarray(add).astype(np.float64)[:, None]
    if Ab is not None:
        g = g + np.asarray(Ab).astype(np.float64)[None, :]
    keep = np.ones((nq, n), bool)
    if skip is not None:
        sk = np.asarray(skip).astype(np.int64)
        ok = (sk >= 0) & (sk < n)
        keep[np.nonzero(ok)[0], sk[ok]] = False
    t = np.asarray(target).astype(np.float64)[:, None]
    return ((g > t) & keep).sum(axis=1).astype(np.int32), \
        ((g == t) & keep).sum(axis=1).astype(np.int32)


# ------------------------------------------------------------------------------- device calls
def rank_queries(lib, dev, Q, A, target, add=None, Ab=None, skip=None, embed=None, lse=True,
                 ws=None):
    """rae_rank_queries on host arrays (Q may be wider than embed: ldq = Q.shape[1]); returns
    (greater, equal, lse or None) as numpy arrays."""
    import torch
    from rae import _lib
    up = lambda x, dt: None if x is None else torch.as_tensor(
        np.ascontiguousarray(x, dtype=dt), device=dev)
    Q = np.asarray(Q, dtype=np.float32)
    if Q.shape[1] % 4:                    # ldq % 4 == 0: columns past embed that are never read
        Q = np.concatenate([Q, np.full((Q.shape[0], 4 - Q.shape[1] % 4), 1000.0, np.float32)],
                           axis=1)
    tQ, tA = up(Q, np.float32), up(A, np.float32)
    tt, ta, tb, ts = up(target, np.float32), up(add, np.float32), up(Ab, np.float32), \
        up(skip, np.int32)
    nq = int(tQ.shape[0])
    a = _lib.RaeRankArgs()
    a.Q, a.ldq, a.nq = _lib.ptr(tQ), int(tQ.shape[1]), nq
    a.add, a.target, a.skip = _lib.ptr(ta), _lib.ptr(tt), _lib.ptr(ts)
    a.A, a.Ab = _lib.ptr(tA), _lib.ptr(tb)
    a.n_entities, a.embed = int(tA.shape[0]), int(tA.shape[1] if embed is None else embed)
    assert tA.shape[1] == a.embed
    need = int(lib.rae_rank_workspace_bytes(C.byref(a), None))
    assert need > 0, lib.rae_last_error()
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ws.fill_(0xFF)
    gr = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    eq = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    ls = torch.full((nq,), float("nan"), dtype=torch.float32, device=dev) if lse else None
    a.greater, a.equal, a.lse = _lib.ptr(gr), _lib.ptr(eq), _lib.ptr(ls)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), int(ws.numel())
    _lib.check(lib.rae_rank_queries(C.byref(a), None), "rae_rank_queries")
    torch.cuda.synchronize()
    return gr.cpu().numpy(), eq.cpu().numpy(), (ls.cpu().numpy() if lse else None)


class DeviceRank:
    """rae_eval_rank calls on a DeviceEval's problem (tests/_entry_ref.py), by default on the
    DeviceEval's own workspace grown to what both entries need."""

    def __init__(self, de):
        import torch
        self.de = de
        a = de.args(0, 0)
        need = int(de.lib.rae_rank_workspace_bytes(None, C.byref(a)))
        assert need > 0, de.lib.rae_last_error()
        if de.ws.numel() < need:
            de.ws = torch.empty(need, dtype=torch.uint8, device=de.dev)
        self.summary = torch.zeros(16, dtype=torch.float64, device=de.dev)

    def run(self, row0, nrows, ks=(1, 10, 100), per_query=True, summary=True, values=True):
        """(greater, equal, target, lse) numpy (nrows, 2) and the 16 summary doubles."""
        import torch
        de, L = self.de, self.de._lib
        a = de.args(row0, nrows)
        a.neg_samples, a.neg1, a.neg2, a.neg_stride = 0, None, None, 0
        if not values:
            a.values = None
        a.workspace, a.workspace_bytes = L.ptr(de.ws), int(de.ws.numel())
        mk = lambda dt, fill: torch.full((nrows, 2), fill, dtype=dt, device=de.dev)
        gr, eq = mk(torch.int32, -7), mk(torch.int32, -7)
        tg = mk(torch.float32, float("nan")) if per_query else None
        ls = mk(torch.float32, float("nan")) if per_query else None
        o = L.RaeRankOut()
        o.greater, o.equal, o.target, o.lse = L.ptr(gr), L.ptr(eq), L.ptr(tg), L.ptr(ls)
        self.summary.fill_(float("nan"))
        o.summary = L.ptr(self.summary) if summary else None
        for j in range(4):
            o.hits_k[j] = int(ks[j]) if j < len(ks) else 0
        L.check(de.lib.rae_eval_rank(C.byref(a), C.byref(o), None), "rae_eval_rank")
        torch.cuda.synchronize()
        host = lambda t: None if t is None else t.cpu().numpy()
        return host(gr), host(eq), host(tg), host(ls), self.summary.cpu().numpy().copy()
