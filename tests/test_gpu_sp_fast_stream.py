"""The compile-time-shape SP forward (rae_sp.hpp sp_example_fast: C3's m=100 r=200 s=20 and C2's
m=30 r=100 s=10, the only shapes that reach it) with its decoder matrices streamed in two
tranches -- waves 4-7 issue theirs at kernel entry, before the row's feature count is known --
on rows chosen to take every exit of that path with loads in flight:

  row lengths 0, 1, 2, 29, 30 (the most the C3 W-row registers hold), 31 (the first C3 row to
  leave for the general path), one row above the descriptor capacity (dcap = min(longest row,
  256): 300 features), and one batch in which EVERY row leaves for the general path at both
  shapes (C2's registers hold 51: lengths 52..300).

8 examples per batch, 3 batches, 40 entities, so rows and entities collide within and across
batches, and e1 appears among its own negatives.  The rows up to 64 features draw from feature
ids 0..63 so the W rows collide too; a row above dcap needs at least 257 distinct features (rows
have no duplicate ids: rae/preprocess.py collapses them), so the feature space is 320 wide and
only the rows longer than 64 reach past id 63.

Each case (shape x binary / non-binary features) runs three times from the same start: twice
under graph replay and once as eager rae_step_forward / rae_step_update launches.  Costs and
parameters agree with the float64 oracle trajectory within tests/test_gpu_train.py's
tolerances, the two graph runs are bitwise equal, and graph replay is bitwise equal to eager.
The inputs themselves are checked without a GPU (the oracle alone): every step's cost is
finite and every listed row length occurs in a batch that runs."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import rae_oracle as O

COST_RTOL = 2e-5                     # tests/test_gpu_train.py
L, NB, N_ENT, D_FEAT, D_HOT = 8, 3, 40, 320, 64
SHAPES = {"c3": (100, 200, 20), "c2": (30, 100, 10)}       # m, r, s
LENS = [0, 1, 2, 29, 30, 31, 5, 12,                         # 31: C3's first general row
        300, 30, 1, 0, 29, 17, 2, 30,                       # 300 > dcap = 256
        52, 300, 64, 53, 270, 58, 52, 61]                   # every row general at both shapes
LISTED = (0, 1, 2, 29, 30, 31, 300)


def _assert_params_close(got, want, what):                  # tests/test_gpu_train.py
    for k in want:
        err = np.abs(got[k] - want[k])
        tol = 2e-4 + 2e-3 * np.abs(want[k])
        assert np.all(err <= tol), f"{what} {k}: max err {err.max():.3e}"


@functools.lru_cache(maxsize=None)
def _inputs(values):
    g = np.random.RandomState(31)
    N = L * NB
    lens = np.array(LENS)
    assert len(lens) == N
    rows = np.repeat(np.arange(N), lens)
    cols = np.concatenate([g.choice(D_HOT if k <= D_HOT else D_FEAT, size=k, replace=False)
                           for k in lens])
    a1 = g.randint(0, N_ENT, N).astype(np.int32)             # the same for both feature kinds
    a2 = g.randint(0, N_ENT, N).astype(np.int32)
    a2[::5] = a1[::5]                                        # e1 == e2
    a1[L:L + 3] = a1[0]                                      # one entity across batches
    x = g.uniform(0.5, 2.0, size=len(rows)) if values else np.ones(len(rows))
    X = sp.csr_matrix((x.astype(np.float32), (rows, cols)), shape=(N, D_FEAT))
    return X, a1, a2


@functools.lru_cache(maxsize=None)
def _negatives(s):
    _, a1, _ = _inputs(False)
    g = np.random.RandomState(32)
    N = L * NB
    n1 = g.randint(0, N_ENT, size=(s, N)).astype(np.int32)
    n2 = g.randint(0, N_ENT, size=(s, N)).astype(np.int32)
    n1[0, ::2] = a1[::2]                                     # e1 among its own negatives
    n2[1, ::3] = a1[::3]
    n1[2, :] = n1[3, :]                                      # a negative drawn twice
    return n1, n2


def _oracle_run(shape, values, p0):
    """Float64 trajectory of the NB batches from parameters p0: (costs, parameters)."""
    m, r, s = SHAPES[shape]
    X, a1, a2 = _inputs(values)
    n1, n2 = _negatives(s)
    p = {k: np.array(v, dtype=np.float64) for k, v in p0.items()}
    acc = {k: np.zeros_like(v) for k, v in p.items()}
    costs = []
    for b in range(NB):
        rows = O.batch_rows(b, L)
        res = O.train_step_grads("sp", p, X[rows], a1[rows], a2[rows], n1[:, rows], n2[:, rows],
                                 alpha=1.0)
        O.adagrad_apply(p, acc, res.grads, 0.1)
        costs.append(res.cost)
    return np.array(costs), p


@pytest.mark.parametrize("values", [False, True])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_inputs_cover_every_exit_and_stay_finite(shape, values):
    """No GPU: the row lengths the module lists occur in batches that run, every row of the
    last batch is longer than either shape's W-row registers hold, and no step of the oracle
    trajectory sees a non-finite cost."""
    m, r, s = SHAPES[shape]
    X, a1, a2 = _inputs(values)
    nf = np.diff(X.indptr)
    assert np.array_equal(nf, LENS) and len(nf) == L * NB    # all NB batches run, no tail
    for k in LISTED:
        assert (nf == k).any(), k
    assert nf.max() > 256                                    # above dcap = min(longest, 256)
    assert nf[2 * L:].min() > 51                             # C2: 17 slots x 3 registers
    assert nf[:L].max() == 31 and (nf[:L] <= 30).sum() == L - 1
    assert values == bool(np.any(X.data != 1.0))
    n1, n2 = _negatives(s)
    assert (n1[0, ::2] == a1[::2]).all() and (n2[1, ::3] == a1[::3]).all()
    assert len(np.unique(a1)) < len(a1)                      # entities collide
    hot = X[:, :D_HOT]
    assert (np.asarray((hot != 0).sum(axis=0)).ravel() > 1).any()   # W rows collide
    p0 = O.init_params(np.random.RandomState(2), "sp", D_FEAT, m, N_ENT, r)
    p0["Ab"] = np.zeros(N_ENT)
    costs, p = _oracle_run(shape, values, p0)
    assert np.all(np.isfinite(costs)), costs
    assert all(np.all(np.isfinite(v)) for v in p.values())


def _device_run(shape, values, dev, graph):
    from rae.data import DatasetManager
    from rae.inducer import ReconstructInducer
    import torch
    m, r, s = SHAPES[shape]
    X, a1, a2 = _inputs(values)
    n1, n2 = _negatives(s)
    data = DatasetManager.from_arrays(X.copy(), a1, a2, n_entities=N_ENT)
    ind = ReconstructInducer(data, {"train": {}}, np.random.RandomState(2), 1, 0.1, L, r, m, s,
                             0.0, 0.0, "adagrad", "stream", "sp", False, True, False, 1.0,
                             device=dev, graph_chunk=2)
    ind.compile_function()
    eng = ind.engine
    p0 = {k: v.detach().cpu().double().numpy() for k, v in ind.modelFunc.named_params().items()}
    eng.set_epoch_negatives(n1, n2)
    eng.run(0, NB, graph=graph)
    torch.cuda.synchronize()
    eng.check()
    costs = eng.costs[:NB].detach().cpu().numpy().copy()
    p = {k: v.detach().cpu().numpy().copy() for k, v in ind.modelFunc.named_params().items()}
    eng.close()
    return p0, costs, p


@pytest.mark.gpu
@pytest.mark.parametrize("values", [False, True])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fast_stream_vs_oracle_graph_and_eager(built_lib, cuda_dev, shape, values):
    p0, costs, p = _device_run(shape, values, cuda_dev, graph=True)
    want_costs, want = _oracle_run(shape, values, p0)
    print(f"{shape} values={values}: costs {costs} oracle {want_costs}")
    assert np.all(np.isfinite(costs))
    np.testing.assert_allclose(costs.astype(np.float64), want_costs, rtol=COST_RTOL, atol=COST_RTOL)
    _assert_params_close({k: v.astype(np.float64) for k, v in p.items()}, want, f"{shape} stream")
    _, costs2, p2 = _device_run(shape, values, cuda_dev, graph=True)
    assert np.array_equal(costs, costs2), "two graph runs differ"
    for k in p:
        assert np.array_equal(p[k], p2[k]), f"two graph runs differ in {k}"
    _, costs3, p3 = _device_run(shape, values, cuda_dev, graph=False)
    assert np.array_equal(costs, costs3), "graph replay and eager launches differ"
    for k in p:
        assert np.array_equal(p[k], p3[k]), f"graph replay and eager launches differ in {k}"
