"""Shared pieces of the tests of the three plan-free entry points of include/rae.h
(rae_eval_cost, rae_label, rae_neg_sample_philox): the inputs, the float64 reference in row
blocks, a float32 numpy restatement of the same forward formulas (the check of the inputs, never
compared with a kernel), a numpy Philox4x32-10, and the ctypes calls.

Reference: oracle/rae_oracle.py in float64 (train_step_grads(...).scores regrouped per example
as test_gpu_eval._group does, and label).  Tolerances are the project's own (test_gpu_eval,
test_label_pass_matches_oracle) and are not re-tuned here.
"""
import ctypes as C
import math

import numpy as np
import scipy.sparse as sp

import rae_oracle as O
from test_gpu_eval import COST_RTOL, TERM_ATOL, TERM_RTOL, _group as group

PROB_RTOL, PROB_ATOL = 1e-4, 1e-6
MARGIN = 1e-4                       # labels compared where the oracle's top-2 margin exceeds it
LABEL_MARGIN = 1e-5                 # ... test_gpu_fullscale.check_labels' margin (the trained split)

DEC_ID = {"sp": 0, "rescal": 1, "rescal+sp": 2}
EDGE_NNZ = [0, 1, 17, 64, 65, 130]
# launch rounds of rae_eval_cost (csrc/rae_eval.hpp RAE_EV_CHUNK_BIL / RAE_EV_CHUNK_SP)
CHUNK = {"sp": 65536, "rescal": 2048, "rescal+sp": 2048}
LDS_BYTES = 160 * 1024              # per 16-example tile (include/rae.h)


# ------------------------------------------------------------------------------------ inputs
def csr_of_lengths(g, lens, d):
    """CSR with the given row lengths, distinct columns per row, values in [0.25, 1.75]."""
    lens = np.asarray(lens, dtype=np.int64)
    rows = np.repeat(np.arange(len(lens)), lens)
    cols = np.concatenate([g.choice(d, size=k, replace=False) for k in lens] +
                          [np.zeros(0, np.int64)]).astype(np.int64)
    vals = g.uniform(0.25, 1.75, size=rows.shape[0]).astype(np.float32)
    X = sp.csr_matrix((vals, (rows, cols)), shape=(len(lens), d))
    X.sort_indices()
    assert np.array_equal(np.diff(X.indptr), lens)
    return X


def eval_params(g, dec, d, m, n, r):
    """float32 parameters away from the uniform-P point, at test_gpu_eval._randomize's scales;
    for long dot products A is scaled by 1 / sqrt(r / 16) so that the scores stay of order 1."""
    sa = 0.5 / math.sqrt(r / 16.0) if r >= 256 else 0.5
    f = lambda scale, *shape: (g.standard_normal(shape) * scale).astype(np.float32)
    p = {"W": f(0.4, d, m), "Wb": f(0.5, m), "A": f(sa, n, r), "Ab": f(0.5, n)}
    if dec != "rescal":
        p["C1"], p["C2"] = f(0.3, r, m), f(0.3, r, m)
    if dec != "sp":
        p["R" if dec == "rescal" else "C"] = f(0.3, r, r, m)
    return p


class EvalProblem:
    """One split (CSR, entity ids, negatives with neg_stride = N + 7) and one parameter set."""

    def __init__(self, dec, m, r, s, lens, n=30, d=400, seed=0, alpha=1.0):
        g = np.random.RandomState(seed)
        self.dec, self.m, self.r, self.s, self.n, self.d, self.alpha = dec, m, r, s, n, d, alpha
        self.X = csr_of_lengths(g, lens, d)
        N = self.N = self.X.shape[0]
        self.a1 = g.randint(0, n, N).astype(np.int32)
        self.a2 = g.randint(0, n, N).astype(np.int32)
        same = g.choice(N, size=max(1, N // 16), replace=False)
        self.a2[same] = self.a1[same]                           # some rows with e1 == e2
        self.stride = N + 7
        self.n1 = g.randint(0, n, size=(s, self.stride)).astype(np.int32)
        self.n2 = g.randint(0, n, size=(s, self.stride)).astype(np.int32)
        self.p32 = eval_params(g, dec, d, m, n, r)
        self.p64 = {k: v.astype(np.float64) for k, v in self.p32.items()}

    def oracle_terms(self, row0=0, nrows=None, block=4096):
        """float64 (nrows, 3) terms of rows [row0, row0 + nrows), the oracle called in row
        blocks (terms are per example, so the blocking changes nothing)."""
        nrows = self.N - row0 if nrows is None else nrows
        out = np.empty((nrows, 3), np.float64)
        for b0 in range(0, nrows, block):
            lo, hi = row0 + b0, row0 + min(nrows, b0 + block)
            res = O.train_step_grads(self.dec, self.p64, self.X[lo:hi], self.a1[lo:hi],
                                     self.a2[lo:hi], self.n1[:, lo:hi], self.n2[:, lo:hi],
                                     alpha=self.alpha)
            out[lo - row0:hi - row0] = group(self.dec, res.scores, hi - lo, self.s)
        return out

    def f32_terms(self, row0=0, nrows=None):
        nrows = self.N - row0 if nrows is None else nrows
        lo, hi = row0, row0 + nrows
        return f32_terms(self.dec, self.p32, self.X[lo:hi], self.a1[lo:hi], self.a2[lo:hi],
                         self.n1[:, lo:hi], self.n2[:, lo:hi], self.alpha)


def cost_of_terms(terms, s):
    """-(S_pos + 2 S_H + S_neg) / (nrows (4 + 2s)) (include/rae.h), in float64 / exact sums."""
    S = [math.fsum(float(x) for x in terms[:, c]) for c in range(3)]
    return -(S[0] + 2.0 * S[1] + S[2]) / (terms.shape[0] * (4 + 2 * s)), S


# ------------------------------------------------------- float32 restatement (input check only)
def _f32_logsig(x):
    x = x.astype(np.float32)
    return -(np.maximum(-x, np.float32(0)) + np.log1p(np.exp(-np.abs(x)))).astype(np.float32)


def f32_encoder(X, W, Wb):
    """S = X.W + Wb, log-softmax, P, all in float32."""
    S = (np.asarray(X.astype(np.float32) @ W.astype(np.float32)) + Wb).astype(np.float32)
    z = S - S.max(axis=1, keepdims=True)
    logP = z - np.log(np.exp(z).sum(axis=1, keepdims=True, dtype=np.float32))
    return S, np.exp(logP).astype(np.float32), logP.astype(np.float32)


def f32_terms(dec, p, X, e1, e2, n1, n2, alpha=1.0):
    """The forward formulas of the three decoders (oracle/rae_oracle.py
    _decoder_forward_backward, forward half) in float32 numpy: (l, 3) terms."""
    ein = lambda spec, *ops: np.einsum(spec, *ops, dtype=np.float32)
    _, P, logP = f32_encoder(X, p["W"], p["Wb"])
    H = np.float32(alpha) * -(P * logP).sum(axis=1, dtype=np.float32)
    A, Ab = p["A"], p["Ab"]
    a1, a2 = A[e1], A[e2]
    N1, N2 = A[n1], A[n2]                                    # (s, l, r)
    if dec == "sp":
        wC1, wC2 = P @ p["C1"].T, P @ p["C2"].T
        left, right = ein("br,br->b", wC1, a1), ein("br,br->b", wC2, a1)
        one = left + right
        gL = ein("br,tbr->tb", wC1, N1) + right[None] + Ab[n1]
        gR = ein("br,tbr->tb", wC2, N2) + left[None] + Ab[n2]
    else:
        R = p["R"] if dec == "rescal" else p["C"]
        r = R.shape[0]
        M = (P @ R.reshape(r * r, -1).T).reshape(-1, r, r)
        Ma2, MTa1 = ein("bij,bj->bi", M, a2), ein("bij,bi->bj", M, a1)
        addL = addR = np.float32(0)
        if dec == "rescal+sp":
            wC1, wC2 = P @ p["C1"].T, P @ p["C2"].T
            sp1, sp2 = ein("br,br->b", wC1, a1), ein("br,br->b", wC2, a2)
            Ma2, MTa1 = Ma2 + wC1, MTa1 + wC2
            addL, addR = sp2[None], sp1[None]
            one = ein("bi,bi->b", a1, Ma2) + sp2
        else:
            one = ein("bi,bi->b", a1, Ma2)
        gL = ein("tbi,bi->tb", N1, Ma2) + addL + Ab[n1]
        gR = ein("bj,tbj->tb", MTa1, N2) + addR + Ab[n2]
    pos = _f32_logsig(one + Ab[e1]) + _f32_logsig(one + Ab[e2])
    neg = _f32_logsig(-gL).sum(axis=0, dtype=np.float32) + \
        _f32_logsig(-gR).sum(axis=0, dtype=np.float32)
    out = np.stack([pos, H, neg], axis=1)
    assert out.dtype == np.float32
    return out


def check_inputs_f32(prob, row0, nrows, what):
    """The float32 restatement agrees with the float64 oracle within HALF of the tolerances the
    kernels are held to: the inputs leave a float32 evaluation that much room."""
    want = prob.oracle_terms(row0, nrows)
    got = prob.f32_terms(row0, nrows).astype(np.float64)
    err = np.abs(got - want)
    c_want, _ = cost_of_terms(want, prob.s)
    c_got, _ = cost_of_terms(got, prob.s)
    print(f"{what}: float32 restatement max |dterm| {err.max():.3e} "
          f"(|term| max {np.abs(want).max():.3e}) |dc| {abs(c_got - c_want):.3e}")
    np.testing.assert_allclose(got, want, rtol=TERM_RTOL / 2, atol=TERM_ATOL / 2, err_msg=what)
    assert abs(c_got - c_want) <= COST_RTOL / 2 * max(1.0, abs(c_want)), what


# ------------------------------------------------------------------------------ Philox4x32-10
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11):
    ctr = four uint32 arrays, key = two Python ints; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint32) for c in ctr)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0.astype(np.uint64), _M1 * c2.astype(np.uint64)
        h0, l0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & _LO).astype(np.uint32)
        h1, l1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & _LO).astype(np.uint32)
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint32(k0), l1, h0 ^ c3 ^ np.uint32(k1), l0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_uniforms(seed, offset, count):
    """U_i of include/rae.h: counter (lo32(idx), hi32(idx), 0, 0), idx = offset + i (mod 2^64),
    key (lo32(seed), hi32(seed)); u = ((c0 >> 5) 2^26 + (c1 >> 6)) / 2^53."""
    idx = (int(offset) + np.arange(count, dtype=object)) % (1 << 64)
    idx = np.array(idx, dtype=np.uint64)
    z = np.zeros(count, np.uint32)
    c0, c1, _, _ = philox4x32_10(((idx & _LO).astype(np.uint32),
                                  (idx >> np.uint64(32)).astype(np.uint32), z, z),
                                 (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    a, b = (c0 >> np.uint32(5)).astype(np.uint64), (c1 >> np.uint32(6)).astype(np.uint64)
    return (a * np.uint64(1 << 26) + b).astype(np.float64) * (1.0 / 9007199254740992.0)


def philox_draws(cum, seed, offset, count):
    cum = np.asarray(cum, dtype=np.float64)
    return cum.searchsorted(philox_uniforms(seed, offset, count) * cum[-1]).astype(np.int32)


# ------------------------------------------------------------------------------- device calls
class DeviceEval:
    """An EvalProblem in device memory and rae_eval_cost calls on it through the C ABI."""

    def __init__(self, lib, prob, dev):
        import torch
        from rae import _lib
        self.lib, self.prob, self.dev, self._lib = lib, prob, dev, _lib
        up = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
        self.t = {k: up(v) for k, v in prob.p32.items()}
        X = prob.X
        self.t.update(indptr=up(X.indptr.astype(np.int32)), indices=up(X.indices.astype(np.int32)),
                      values=up(X.data.astype(np.float32)), args1=up(prob.a1), args2=up(prob.a2),
                      neg1=up(prob.n1), neg2=up(prob.n2))
        need = int(lib.rae_eval_workspace_bytes(C.byref(self.args(0, 0))))
        assert need > 0, lib.rae_last_error()
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.sums = torch.zeros(3, dtype=torch.float64, device=dev)

    def args(self, row0, nrows):
        p, t, q = self.prob, self.t, self._lib.ptr
        a = self._lib.RaeEvalArgs()
        a.decoder, a.relations, a.embed, a.neg_samples = DEC_ID[p.dec], p.m, p.r, p.s
        a.n_entities, a.alpha = p.n, p.alpha
        a.W, a.Wb, a.A, a.Ab = q(t["W"]), q(t["Wb"]), q(t["A"]), q(t["Ab"])
        a.C1, a.C2, a.R3 = q(t.get("C1")), q(t.get("C2")), q(t.get("R", t.get("C")))
        a.indptr, a.indices, a.values = q(t["indptr"]), q(t["indices"]), q(t["values"])
        a.args1, a.args2 = q(t["args1"]), q(t["args2"])
        a.neg1, a.neg2, a.neg_stride = q(t["neg1"]), q(t["neg2"]), p.stride
        a.row0, a.nrows = int(row0), int(nrows)
        return a

    def poison(self):
        """Every workspace byte 0xFF: NaN read as float or double."""
        self.ws.fill_(0xFF)

    def run(self, row0, nrows, terms=True, sums=None):
        """(terms tensor (nrows, 3) or None, the three sums as Python floats)."""
        import torch
        a = self.args(row0, nrows)
        out = torch.full((nrows, 3), float("nan"), dtype=torch.float32,
                         device=self.dev) if terms else None
        sums = self.sums if sums is None else sums
        a.terms_out, a.sums_out = self._lib.ptr(out), self._lib.ptr(sums)
        a.workspace, a.workspace_bytes = self._lib.ptr(self.ws), int(self.ws.numel())
        self._lib.check(self.lib.rae_eval_cost(C.byref(a), None), "rae_eval_cost")
        torch.cuda.synchronize()
        return out, tuple(float(x) for x in sums.cpu().numpy())


def check_eval(out, sums, want_terms, s, what):
    """Terms and cost of one call against the oracle's terms; prints the maxima (as
    test_gpu_eval._check does) before it asserts."""
    got = out.cpu().double().numpy()
    nrows = want_terms.shape[0]
    want_cost, _ = cost_of_terms(want_terms, s)
    cost = -(sums[0] + 2.0 * sums[1] + sums[2]) / (nrows * (4 + 2 * s))
    err = np.abs(got - want_terms)
    print(f"{what}: max |dterm| {err.max():.3e} (|term| max {np.abs(want_terms).max():.3e}), "
          f"cost {cost:.9f} oracle {want_cost:.9f} |dc| {abs(cost - want_cost):.3e}")
    np.testing.assert_allclose(got, want_terms, rtol=TERM_RTOL, atol=TERM_ATOL, err_msg=what)
    assert abs(cost - want_cost) <= COST_RTOL * max(1.0, abs(want_cost)), (what, cost, want_cost)
    return cost, want_cost
