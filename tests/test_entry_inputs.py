"""The inputs of the GPU tests of rae_eval_cost and rae_label (test_gpu_entry_shapes,
test_gpu_eval_ranges), checked on the CPU: a float32 numpy restatement of the forward formulas
(tests/_entry_ref.py) must agree with the float64 oracle within HALF of the tolerances the
kernels are held to, at every shape of the matrices -- so a plain float32 evaluation of these
inputs has room to spare and a kernel that misses a tolerance is wrong, not unlucky.  The share
of label rows the top-2 margin filter leaves out is bounded here as well.  The saturated parameters of tests/_grad_ref.py get the same check.  No GPU
needed."""
import numpy as np
import pytest

import _entry_ref as E
import test_gpu_entry_shapes as S
import test_gpu_eval_ranges as R


@pytest.mark.parametrize("name", list(S.EVAL_SHAPES))
def test_eval_shape_inputs(name):
    prob = S.eval_problem(name)
    assert list(np.diff(prob.X.indptr)[S.ROW0 + 2:S.ROW0 + 8]) == E.EDGE_NNZ
    E.check_inputs_f32(prob, S.ROW0, S.NROWS, name)
    big = np.abs(prob.oracle_terms(S.ROW0, S.NROWS)).max()
    assert np.isfinite(big) and big < 200.0, big


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_eval_range_inputs(name):
    """The long ranges: the first and the last 2500 rows (the row-length edges are there)."""
    prob = R.problem(name)
    lens = np.diff(prob.X.indptr)
    C = E.CHUNK[prob.dec]
    assert prob.N == R.n_rows(prob.dec) and lens.max() == 130
    assert {0, 1, 17} <= set(lens[:C]) and {64, 65, 130} <= set(lens[prob.N - R.TAIL:])
    assert (prob.a1 == prob.a2).sum() >= prob.N // 16
    E.check_inputs_f32(prob, 0, 2500, name + " head")
    E.check_inputs_f32(prob, prob.N - 2500, 2500, name + " tail")


@pytest.mark.parametrize("m", S.LABEL_M)
def test_label_inputs(m):
    X, W, Wb = S.label_problem(m)
    assert list(np.diff(X.indptr)) == list(np.repeat(np.arange(131), 3))
    assert X.data.min() >= 0.25 and X.data.max() <= 1.75 and len(np.unique(X.data)) > 100
    _, want_p, clear = S.label_oracle(X, W, Wb)
    _, P, _ = E.f32_encoder(X, W, Wb)
    err = np.abs(P.astype(np.float64) - want_p)
    print(f"label m={m}: float32 restatement max |dprob| {err.max():.3e}, "
          f"rows left out {(~clear).sum()} of {len(clear)}")
    np.testing.assert_allclose(P.astype(np.float64), want_p, rtol=E.PROB_RTOL / 2,
                               atol=E.PROB_ATOL / 2)
    assert (~clear).mean() <= S.MAX_UNCLEAR


@pytest.mark.parametrize("shape", S.SAT_ENTRY_SHAPES)
def test_saturated_entry_inputs(shape):
    """The saturated parameters through the forward-only entries: the float32 restatement holds
    half the kernels' tolerances on terms, cost and probabilities, the terms are finite, some
    shifted logit is below -87.3 at the x 8 shapes, and at least 90 % of the rows have a
    decisive label (check_labels' margin)."""
    prob = S.sat_problem(shape)
    E.check_inputs_f32(prob, 0, prob.N, f"saturated {shape}")
    assert np.isfinite(prob.oracle_terms(0, prob.N)).all()
    W, Wb = prob.p32["W"], prob.p32["Wb"]
    Sc, P32, _ = E.f32_encoder(prob.X, W, Wb)
    _, want_p = E.O.label(prob.X, W.astype(np.float64), Wb.astype(np.float64))
    np.testing.assert_allclose(P32.astype(np.float64), want_p, rtol=E.PROB_RTOL / 2,
                               atol=E.PROB_ATOL / 2)
    S64 = np.asarray(prob.X.astype(np.float64) @ W.astype(np.float64)) + Wb
    srt = np.sort(S64, axis=1)
    assert ((srt[:, -1] - srt[:, -2]) > E.LABEL_MARGIN).mean() >= 0.9
    if shape != "S1":
        assert (S64 - srt[:, -1:] < -87.3).any()


@pytest.mark.parametrize("shape", [s for s, scores in S.SAT_ENTRY_CASES if scores])
def test_saturated_scores_entry_inputs(shape):
    """... and the variant whose decoder scores saturate (A, Ab x 32): the float32 restatement
    holds half the kernels' tolerances, the terms are finite, and some per-example term is
    beyond -87 (a score past the point where fp32 sigmoid is exactly 0)."""
    prob = S.sat_problem(shape, scores=True)
    E.check_inputs_f32(prob, 0, prob.N, f"saturated-scores {shape}")
    terms = prob.oracle_terms(0, prob.N)
    assert np.isfinite(terms).all() and terms[:, [0, 2]].min() < -87.0
