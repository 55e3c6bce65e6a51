"""rae_eval_cost and rae_label on an MI355X at the lane-mapping switch points and at the shape
limits include/rae.h states, against the float64 oracle (oracle/rae_oracle.py).

The encoder gather (k_label and its copy eval_encode) has three lane mappings (16 / 32 / 64
lanes per W row, from mv = m / VW), two column chunks per lane above mv = 64, a scalar path
(m % 4 != 0, m <= 128) and a float4 path; eval_dot has a scalar and a float4 form and a second
pass from r = 17 / r = 68; eval_project has scalar and float4 k-tails and more jobs than waves
from r = 33; the negative loop takes 8 tasks per round.  Every case below names the edge it is
there for.  tests/test_entry_inputs.py checks the inputs of every case on the CPU.

The saturated parameters of tests/_grad_ref.py (W, Wb x 8 or x 3, A, Ab x 2: P one-hot, shifted
logits down to -190) go through both entries as well, at the shapes S1, S3, B2 and H1.

Tolerances are the project's own (test_gpu_eval, test_label_pass_matches_oracle): cost
2e-5 max(1, |c|); terms rtol 1e-4, atol 1e-5; label probabilities rtol 1e-4, atol 1e-6; labels
equal where the oracle's top-2 margin exceeds 1e-4.
"""
import ctypes as C

import numpy as np
import pytest

import _entry_ref as E

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------- B. rae_eval_cost shapes
ROW0, NROWS = 3, 50                     # three full 16-example tiles and a tail of 2


def hybrid_max_r(m):
    """Largest r of 'rescal+sp' whose tile fits: 16 (mS + 4 r4) 4 bytes <= 160 KiB."""
    mS = (m + 3) & ~3
    return max(r for r in range(1, 1025) if 16 * (mS + 4 * ((r + 3) & ~3)) * 4 <= E.LDS_BYTES)


#        id: (decoder, m, r, s)   edge
EVAL_SHAPES = {
    # SP, scalar encoder (m % 4 != 0); eval_project's scalar k-tail m % 4 = 1, 3
    "sp-m1-r1-s1": ("sp", 1, 1, 1),           # LPR 16, mv = 1; scalar eval_dot r = 1; 2s = 2
    "sp-m3-r3-s2": ("sp", 3, 3, 2),           # m % 4 = 3; r = 3; 2s = 4
    "sp-m17-r15-s4": ("sp", 17, 15, 4),       # mv = 17: LPR 32 scalar; r = 15; 2s = 8 exactly
    "sp-m33-r17-s5": ("sp", 33, 17, 5),       # mv = 33: LPR 64 scalar; scalar second pass; 2s = 10
    "sp-m65-r40-s3": ("sp", 65, 40, 3),       # mv = 65: NQ = 2 scalar; 6 jobs over 4 waves
    "sp-m127-r13-s3": ("sp", 127, 13, 3),     # the largest scalar m, NQ = 2
    "sp-m127-r125-s3": ("sp", 127, 125, 3),   # ... with the largest scalar r: two per lane in both
    "sp-m16-r3-s1": ("sp", 16, 3, 1),         # mv = 4 float4 next to the scalar r
    # SP, float4 encoder: mv = 1, 16 | 17, 32 | 33, 64 | 65, 128
    "sp-m4-r4-s1": ("sp", 4, 4, 1),           # mv = 1; float4 eval_dot rv = 1; float4 k-tail
    "sp-m64-r64-s2": ("sp", 64, 64, 2),       # mv = 16: last LPR 16; rv = 16 exactly
    "sp-m68-r68-s4": ("sp", 68, 68, 4),       # mv = 17: first LPR 32; float4 second pass; k-tail
    "sp-m128-r40-s5": ("sp", 128, 40, 5),     # mv = 32: last LPR 32; r % 16 != 0
    "sp-m132-r20-s3": ("sp", 132, 20, 3),     # mv = 33: first LPR 64; k-tail
    "sp-m256-r16-s2": ("sp", 256, 16, 2),     # mv = 64: last NQ = 1
    "sp-m260-r300-s3": ("sp", 260, 300, 3),   # mv = 65: first NQ = 2; k-tail; long r
    "sp-m512-r1024-s3": ("sp", 512, 1024, 3),             # limit: mv = 128, a 160 KiB tile
    # RESCAL / hybrid
    "rescal-m320-r24-s2": ("rescal", 320, 24, 2),         # limit: 160 KiB of k_eval_mt LDS; r % 16 = 8
    "rescal-m127-r17-s3": ("rescal", 127, 17, 3),         # scalar staging; r one past a block edge
    "rescal-m8-r8-s3": ("rescal", 8, 8, 3),               # exact block edge (8 x 16 blocks)
    "rescal-m8-r16-s3": ("rescal", 8, 16, 3),             # exact block edge
    "hybrid-m30-r17-s5": ("rescal+sp", 30, 17, 5),        # scalar LPR 32 through k_eval_enc; 2s = 10
    "hybrid-m4-rmax-s2": ("rescal+sp", 4, hybrid_max_r(4), 2),   # limit: r = 636, a 160 KiB tile
}


# shapes added after the seeds were given out (a shape's seed is its rank among the others)
EVAL_ADDED = ["sp-m127-r125-s3"]
_EVAL_SEEDS = sorted(k for k in EVAL_SHAPES if k not in EVAL_ADDED) + EVAL_ADDED


def eval_problem(name):
    dec, m, r, s = EVAL_SHAPES[name]
    g = np.random.RandomState(7)
    lens = np.concatenate([g.randint(0, 12, ROW0 + 2), E.EDGE_NNZ,
                           g.randint(0, 12, NROWS - 2 - len(E.EDGE_NNZ))])
    assert len(lens) == ROW0 + NROWS
    return E.EvalProblem(dec, m, r, s, lens, n=30, d=400, seed=_EVAL_SEEDS.index(name))


@pytest.mark.parametrize("name", list(EVAL_SHAPES))
def test_eval_cost_shape(built_lib, cuda_dev, name):
    prob = eval_problem(name)
    if name == "hybrid-m4-rmax-s2":
        assert prob.r == 636
    dev = E.DeviceEval(built_lib, prob, cuda_dev)
    want = prob.oracle_terms(ROW0, NROWS)
    out, sums = dev.run(ROW0, NROWS, terms=True)
    E.check_eval(out, sums, want, prob.s, name)


# ----------------------------------------------------------------- C. rae_label lane-map matrix
LABEL_M = [1, 3, 17, 30, 33, 65, 127, 4, 64, 68, 128, 132, 256, 260, 512]
LABEL_D, LABEL_ROW0 = 4000, 5
MAX_UNCLEAR = 0.02                      # share of rows the margin filter may leave out


def label_problem(m):
    """Row lengths 0..130, three rows of each, non-binary values; W / Wb at _randomize's scales."""
    g = np.random.RandomState(1000 + m)
    X = E.csr_of_lengths(g, np.repeat(np.arange(131), 3), LABEL_D)
    W = (g.standard_normal((LABEL_D, m)) * 0.4).astype(np.float32)
    Wb = (g.standard_normal(m) * 0.5).astype(np.float32)
    return X, W, Wb


def label_oracle(X, W, Wb):
    """Oracle labels and probabilities, and the rows whose top-2 margin is clear."""
    lab, P = E.O.label(X, W.astype(np.float64), Wb.astype(np.float64))
    if W.shape[1] == 1:
        return lab, P, np.ones(X.shape[0], bool)
    S = np.asarray(X.astype(np.float64) @ W.astype(np.float64)) + Wb.astype(np.float64)
    srt = np.sort(S, axis=1)
    return lab, P, (srt[:, -1] - srt[:, -2]) > E.MARGIN


def _device_labels(built_lib, cuda_dev, X, W, Wb, row0, nrows):
    """rae_label on rows [row0, row0 + nrows), with and without probabilities: (labels, the
    labels of the call without probabilities, probabilities) as numpy arrays."""
    import torch
    from rae import _lib
    n, m = X.shape[0], W.shape[1]
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=cuda_dev)
    indptr, indices = up(X.indptr.astype(np.int32)), up(X.indices.astype(np.int32))
    values, Wt, Wbt = up(X.data.astype(np.float32)), up(W), up(Wb)
    # outputs one full split long: entries past nrows must stay as they are (labels[e] and
    # probs + e m are indexed by e = row - row0, not by the row)
    lab = torch.full((n,), -7, dtype=torch.int64, device=cuda_dev)
    lab2 = torch.full((n,), -7, dtype=torch.int64, device=cuda_dev)
    pr = torch.full((n, m), -7.0, dtype=torch.float32, device=cuda_dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(built_lib.rae_label(p(indptr), p(indices), p(values), p(Wt), p(Wbt), m, row0,
                                   nrows, p(lab), p(pr), None))
    _lib.check(built_lib.rae_label(p(indptr), p(indices), p(values), p(Wt), p(Wbt), m, row0,
                                   nrows, p(lab2), None, None))
    torch.cuda.synchronize()
    return lab.cpu().numpy(), lab2.cpu().numpy(), pr.cpu().numpy()


@pytest.mark.parametrize("m", LABEL_M)
def test_label_lane_maps(built_lib, cuda_dev, m):
    X, W, Wb = label_problem(m)
    n = X.shape[0]
    row0, nrows = LABEL_ROW0, n - LABEL_ROW0
    want_lab, want_p, clear = label_oracle(X, W, Wb)
    assert (~clear).mean() <= MAX_UNCLEAR
    lab, lab2, pr = _device_labels(built_lib, cuda_dev, X, W, Wb, row0, nrows)
    assert (lab[nrows:] == -7).all() and (pr[nrows:] == -7.0).all()
    assert np.array_equal(lab, lab2)
    err = np.abs(pr[:nrows] - want_p[row0:])
    print(f"label m={m}: max |dprob| {err.max():.3e}, rows left out {(~clear).sum()} of {n}")
    np.testing.assert_allclose(pr[:nrows], want_p[row0:], rtol=E.PROB_RTOL, atol=E.PROB_ATOL)
    ok = clear[row0:]
    assert lab[:nrows].min() >= 0 and lab[:nrows].max() < m
    assert np.array_equal(lab[:nrows][ok], want_lab[row0:][ok])


# ------------------------------------------- D. the forward-only entries on saturated parameters
SAT_ENTRY_SHAPES = ["S1", "S3", "B2", "H1"]
# the variant with saturated scores (A, Ab x 32) where a float32 evaluation of the inputs keeps
# half the tolerances (tests/test_entry_inputs.py); at H1 it does not: one term of 1.8e4, a sum of
# cancelling bilinear and SP parts, is 8.7e-5 off in float32 numpy
SAT_ENTRY_CASES = [(s, False) for s in SAT_ENTRY_SHAPES] + [(s, True) for s in ("S1", "S3", "B2")]


def sat_problem(shape, scores=False):
    """The train split of tests/_grad_ref.py's case (shape, O3) -- three batches, non-binary
    feature values -- with its saturated parameters (W, Wb x 8 or x 3, A, Ab x 2: P one-hot to
    1e-4, shifted logits down to -100 ... -190), as an EvalProblem.  scores: A, Ab x 32, the
    variant whose decoder scores pass +-87."""
    import _grad_ref as G
    c = G.case_config(shape, "O3", regime="saturated-scores" if scores else "saturated")
    data, neg1, neg2 = G.case_dataset(c)
    xs = data.split["train"]
    prob = E.EvalProblem.__new__(E.EvalProblem)
    prob.dec, prob.m, prob.r, prob.s = c["dec"], c["m"], c["r"], c["s"]
    prob.n, prob.d, prob.alpha = c["n"], c["d"], c["alpha"]
    prob.X = xs.xFeats.astype(np.float32).tocsr()
    prob.N = prob.stride = prob.X.shape[0]
    prob.a1, prob.a2 = xs.args1.astype(np.int32), xs.args2.astype(np.int32)
    prob.n1, prob.n2 = np.ascontiguousarray(neg1, np.int32), np.ascontiguousarray(neg2, np.int32)
    prob.p32 = dict(G.generic_params(c))
    prob.p64 = {k: v.astype(np.float64) for k, v in prob.p32.items()}
    return prob


@pytest.mark.parametrize("shape,scores", SAT_ENTRY_CASES,
                         ids=[s + ("-scores" if v else "") for s, v in SAT_ENTRY_CASES])
def test_eval_cost_saturated(built_lib, cuda_dev, shape, scores):
    """rae_eval_cost over the whole split at the saturated parameters: per-example terms and the
    cost against float64 at this module's tolerances.  "scores": A, Ab x 32, decoder scores
    beyond +-87 (the log sigmoids are then the scores themselves, or 0)."""
    prob = sat_problem(shape, scores)
    dev = E.DeviceEval(built_lib, prob, cuda_dev)
    want = prob.oracle_terms(0, prob.N)
    out, sums = dev.run(0, prob.N, terms=True)
    assert np.isfinite(out.cpu().numpy()).all() and np.isfinite(sums).all()
    E.check_eval(out, sums, want, prob.s, f"saturated {shape}")


@pytest.mark.parametrize("shape", SAT_ENTRY_SHAPES)
def test_label_saturated(built_lib, cuda_dev, shape):
    """rae_label at the saturated parameters: labels by check_labels' margin rule (equal to the
    oracle's wherever its top-2 margin exceeds LABEL_MARGIN, at least 90 % of the rows
    decisive), probabilities at this module's tolerances -- the oracle's underflow to exactly 0
    where the device's __expf does, within PROB_ATOL."""
    from types import SimpleNamespace
    from test_gpu_fullscale import check_labels
    prob = sat_problem(shape)
    W, Wb = prob.p32["W"], prob.p32["Wb"]
    lab, lab2, pr = _device_labels(built_lib, cuda_dev, prob.X, W, Wb, 0, prob.N)
    assert np.array_equal(lab, lab2) and lab.min() >= 0 and lab.max() < prob.m
    check_labels(lab, SimpleNamespace(xFeats=prob.X), W.astype(np.float64), Wb.astype(np.float64),
                 what=f"saturated {shape}")
    _, want_p = E.O.label(prob.X, W.astype(np.float64), Wb.astype(np.float64))
    assert np.isfinite(pr).all()
    print(f"saturated {shape}: max |dprob| {np.abs(pr - want_p).max():.3e}")
    np.testing.assert_allclose(pr, want_p, rtol=E.PROB_RTOL, atol=E.PROB_ATOL)
