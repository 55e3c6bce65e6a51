"""Shared pieces of the tests of rae_relation_scores / rae_eval_relations (include/rae.h): the
float64 reference (psi, log-softmax, l, J), S_abs (the sum of the absolute values of the terms of
psi_k, which the derived error bound scales with), a float32 numpy restatement (a check of the
inputs, never compared with a kernel), the problem generators shared by the host and the GPU
tests, and the ctypes calls.

Reference: the table in include/rae.h, pinned by tests/test_relations_host.py to
tests/_rank_ref.py's `one` and to oracle/rae_oracle.py's positive score.

Bounds.  psi_k is a sum of K products (K = r^2, 2r or r^2 + 2r); the kernel rounds the outer
product a1_i a2_j once and then accumulates in fp32, in some order.  Any fp32 summation order of n
rounded terms has forward error <= gamma_n sum |terms| (Higham, Accuracy and Stability of
Numerical Algorithms, section 4.2), gamma_n = n u / (1 - n u), u = 2^-24; with the rounding of
the outer product and of the final sums of the parts: gamma_{K+3} S_abs_k.  Derived, not measured.
J adds the log-softmax and l: |dl / dpsi| <= 2, so twice the psi bound, plus the tolerances the
project already holds rae_eval_cost's pos term (TERM_RTOL, TERM_ATOL: l_k is that term at a
one-hot P) and rae_label's probabilities to.  A relative error PROB_RTOL of P is an absolute
error PROB_RTOL of log P; a logarithm of magnitude above 1 is itself rounded relatively, so the
log-space form is PROB_RTOL max(1, |log P|).  PROB_ATOL has no finite counterpart in log space
at small P and is left out (the stricter choice).
"""
import ctypes as C

import numpy as np

from _entry_ref import PROB_RTOL, TERM_ATOL, TERM_RTOL

DEC_ID = {"sp": 0, "rescal": 1, "rescal+sp": 2}
DECODERS = ("sp", "rescal", "rescal+sp")
ROUND = 16384                     # pairs / rows per launch round (csrc/rae_relscore.hpp)
U32 = 2.0 ** -24


def block_examples(m):
    """examples of one workgroup (csrc/rae_relscore.hpp rel_config)"""
    return 128 if m <= 16 else 64


def contraction_length(dec, r):
    return {"sp": 2 * r, "rescal": r * r, "rescal+sp": r * r + 2 * r}[dec]


def gamma(n):
    return n * U32 / (1.0 - n * U32)


# ----------------------------------------------------------------------- float64 reference
def _bilinear(a1, a2, R, chunk=64):
    """out[b, k] = sum_ij a1[b, i] R[i, j, k] a2[b, j] without the (b, r, r) outer product."""
    r, m = R.shape[0], R.shape[2]
    R2 = R.reshape(r, r * m)
    out = np.empty((a1.shape[0], m), R.dtype)
    for b0 in range(0, a1.shape[0], chunk):
        T = (a1[b0:b0 + chunk] @ R2).reshape(-1, r, m)
        out[b0:b0 + chunk] = np.einsum("bjk,bj->bk", T, a2[b0:b0 + chunk])
    return out


def psi64(dec, p, e1, e2, absolute=False):
    """psi (nq, m) in float64 (absolute=True: S_abs, every term replaced by its magnitude)."""
    f = (lambda x: np.abs(np.asarray(x, np.float64))) if absolute else \
        (lambda x: np.asarray(x, np.float64))
    A = f(p["A"])
    a1, a2 = A[np.asarray(e1, np.int64)], A[np.asarray(e2, np.int64)]
    if dec == "sp":
        return a1 @ f(p["C1"]) + a1 @ f(p["C2"])
    out = _bilinear(a1, a2, f(p["R" if dec == "rescal" else "C"]))
    if dec == "rescal+sp":
        out = out + a1 @ f(p["C1"]) + a2 @ f(p["C2"])
    return out


def psi_bound(dec, p, e1, e2):
    """gamma_{K+3} S_abs_k, (nq, m)."""
    r = np.asarray(p["A"]).shape[1]
    return gamma(contraction_length(dec, r) + 3) * psi64(dec, p, e1, e2, absolute=True)


def logits64(p, X):
    return np.asarray(X.astype(np.float64) @ np.asarray(p["W"], np.float64)) + \
        np.asarray(p["Wb"], np.float64)


def logsoftmax64(S):
    z = S - S.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def logsig64(x):
    x = np.asarray(x, np.float64)
    return -(np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x))))


def ell64(psi, Ab, e1, e2):
    Ab = np.asarray(Ab, np.float64)
    return logsig64(psi + Ab[e1][:, None]) + logsig64(psi + Ab[e2][:, None])


def joint64(dec, p, X, e1, e2):
    """(psi, logsoftmax, l, J) of the rows of X in float64."""
    psi = psi64(dec, p, e1, e2)
    lsm = logsoftmax64(logits64(p, X))
    ell = ell64(psi, p["Ab"], e1, e2)
    return psi, lsm, ell, lsm + ell


def joint_bound(dec, p, X, e1, e2):
    """The bound of |J^ - J| (module docstring), (nrows, m)."""
    _, lsm, ell, _ = joint64(dec, p, X, e1, e2)
    return 2.0 * psi_bound(dec, p, e1, e2) + TERM_ATOL + TERM_RTOL * np.abs(ell) + \
        PROB_RTOL * np.maximum(1.0, np.abs(lsm))


# ------------------------------------------------------- float32 restatement (input check only)
def psi32(dec, p, e1, e2):
    f = lambda x: np.asarray(x, np.float32)
    A = f(p["A"])
    a1, a2 = A[np.asarray(e1, np.int64)], A[np.asarray(e2, np.int64)]
    if dec == "sp":
        out = a1 @ f(p["C1"]) + a1 @ f(p["C2"])
    else:
        out = _bilinear(a1, a2, f(p["R" if dec == "rescal" else "C"]))
        if dec == "rescal+sp":
            out = out + a1 @ f(p["C1"]) + a2 @ f(p["C2"])
    assert out.dtype == np.float32
    return out


def joint32(dec, p, X, e1, e2):
    from _entry_ref import _f32_logsig, f32_encoder
    psi = psi32(dec, p, e1, e2)
    _, _, logP = f32_encoder(X, p["W"], p["Wb"])
    Ab = np.asarray(p["Ab"], np.float32)
    J = logP + _f32_logsig(psi + Ab[e1][:, None]) + _f32_logsig(psi + Ab[e2][:, None])
    assert J.dtype == np.float32
    return psi, J


# --------------------------------------------------------------------------- problem generators
def int_params(seed, dec, n, r, m):
    """Parameters with small-integer values: {-2..2}, {-1, 0, 1} at r = 1024 -- every order of
    summation gives the same float."""
    g = np.random.RandomState(seed)
    lo, hi = (-1, 2) if r >= 1024 else (-2, 3)
    f = lambda *shape: g.randint(lo, hi, size=shape).astype(np.float32)
    p = {"A": f(n, r)}
    if dec != "rescal":
        p["C1"], p["C2"] = f(r, m), f(r, m)
    if dec != "sp":
        p["R" if dec == "rescal" else "C"] = f(r, r, m)
    return p


def int_pairs(seed, n, nq):
    g = np.random.RandomState(seed + 1)
    return g.randint(0, n, nq).astype(np.int32), g.randint(0, n, nq).astype(np.int32)


def max_partial_magnitude(dec, p):
    """An upper bound of every partial sum of every psi_k of every pair: max over k of the sum of
    the largest possible magnitudes of the terms."""
    A = np.abs(np.asarray(p["A"], np.float64))
    amax = A.max(axis=0)                                     # (r,)
    tot = 0.0
    if dec != "sp":
        R = np.abs(np.asarray(p["R" if dec == "rescal" else "C"], np.float64))
        tot = np.einsum("i,ijk,j->k", amax, R, amax)
    if dec != "rescal":
        tot = tot + amax @ np.abs(np.asarray(p["C1"], np.float64)) + \
            amax @ np.abs(np.asarray(p["C2"], np.float64))
    return float(np.max(tot))


def float_params(seed, dec, n, r, m):
    """_entry_ref.eval_params' scales without the encoder."""
    from _entry_ref import eval_params
    p = eval_params(np.random.RandomState(seed), dec, 8, m, n, r)
    return {k: v for k, v in p.items() if k not in ("W", "Wb", "Ab")}


# shapes of the float tests (the issue's) and of the eval-relations problems
FLOAT_SHAPES = ((200, 100), (33, 17))
# (decoder, m, r, rows): rows cross a workgroup's example block; the last row lengths are the edge
# cases of the encoder's gather
EVAL_CASES = tuple((dec, m, r, 150) for dec in DECODERS for (r, m) in ((33, 17), (40, 100)))


def eval_problem(dec, m, r, rows, seed=3):
    from _entry_ref import EDGE_NNZ, EvalProblem
    g = np.random.RandomState(seed)
    lens = list(g.randint(1, 40, size=rows - len(EDGE_NNZ))) + EDGE_NNZ
    return EvalProblem(dec, m, r, 1, lens, n=30, d=400, seed=seed)


# ------------------------------------------------------------------------------- device calls
class DeviceRel:
    """Parameters in device memory and rae_relation_scores calls on them."""

    def __init__(self, lib, dev, dec, p):
        import torch
        from rae import _lib
        self.lib, self.dev, self.dec, self._lib = lib, dev, dec, _lib
        self.t = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32), device=dev)
                  for k, v in p.items() if k in ("A", "C1", "C2", "R", "C")}
        self.n, self.r = (int(x) for x in self.t["A"].shape)
        mat = self.t.get("C1", self.t.get("R", self.t.get("C")))
        self.m = int(mat.shape[-1])

    def args(self, e1, e2, nq, psi, ldp):
        q, t = self._lib.ptr, self.t
        a = self._lib.RaeRelscoreArgs()
        a.decoder, a.relations, a.embed, a.n_entities = DEC_ID[self.dec], self.m, self.r, self.n
        a.A, a.C1, a.C2, a.R3 = q(t["A"]), q(t.get("C1")), q(t.get("C2")), \
            q(t.get("R", t.get("C")))
        a.e1, a.e2, a.nq = q(e1), q(e2), nq
        a.psi_out, a.ldp = q(psi), ldp
        return a

    def run(self, e1, e2, ldp=None, sentinel=-77.0):
        """psi (nq, ldp) as numpy; the output buffer is filled with `sentinel` first."""
        import torch
        ldp = self.m if ldp is None else ldp
        nq = len(e1)
        up = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=self.dev)
        t1, t2 = up(e1), up(e2)
        psi = torch.full((max(nq, 1), ldp), sentinel, dtype=torch.float32, device=self.dev)
        a = self.args(t1 if nq else None, t2 if nq else None, nq, psi, ldp)
        self._lib.check(self.lib.rae_relation_scores(C.byref(a), None), "rae_relation_scores")
        torch.cuda.synchronize()
        return psi.cpu().numpy()[:nq]


class DeviceRelEval:
    """rae_eval_relations calls on a DeviceEval's problem (tests/_entry_ref.py)."""

    def __init__(self, de):
        import torch
        self.de = de
        need = int(de.lib.rae_relscore_workspace_bytes(None, C.byref(de.args(0, 0))))
        assert need > 0, de.lib.rae_last_error()
        self.ws = torch.empty(need, dtype=torch.uint8, device=de.dev)

    def run(self, row0, nrows, want=("psi", "joint", "labels_dec", "labels_joint")):
        import torch
        de, L = self.de, self.de._lib
        a = de.args(row0, nrows)
        a.neg_samples, a.neg1, a.neg2, a.neg_stride = 0, None, None, 0
        self.ws.fill_(0xFF)
        a.workspace, a.workspace_bytes = L.ptr(self.ws), int(self.ws.numel())
        m = de.prob.m
        bufs = {"psi": torch.full((max(nrows, 1), m), float("nan"), device=de.dev),
                "joint": torch.full((max(nrows, 1), m), float("nan"), device=de.dev),
                "labels_dec": torch.full((max(nrows, 1),), -7, dtype=torch.int64, device=de.dev),
                "labels_joint": torch.full((max(nrows, 1),), -7, dtype=torch.int64, device=de.dev)}
        o = L.RaeRelOut()
        for k in want:
            setattr(o, k, bufs[k].data_ptr())
        L.check(de.lib.rae_eval_relations(C.byref(a), C.byref(o), None), "rae_eval_relations")
        torch.cuda.synchronize()
        return {k: bufs[k].cpu().numpy()[:nrows] for k in want}


def np_argmax_first(x):
    """numpy's argmax: the first maximum, a NaN counting as the maximum."""
    return np.argmax(x, axis=1).astype(np.int64)
