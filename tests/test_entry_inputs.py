"""The inputs of the GPU tests of rae_eval_cost and rae_label (test_gpu_entry_shapes,
test_gpu_eval_ranges), checked on the CPU: a float32 numpy restatement of the forward formulas
(tests/_entry_ref.py) must agree with the float64 oracle within HALF of the tolerances the
kernels are held to, at every shape of the matrices -- so a plain float32 evaluation of these
inputs has room to spare and a kernel that misses a tolerance is wrong, not unlucky.  The share
of label rows the top-2 margin filter leaves out is bounded here as well.  No GPU needed."""
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
